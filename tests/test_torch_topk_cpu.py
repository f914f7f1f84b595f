"""The torch-order key types of vrs_topk_segments (VRS_TOPK_DTYPE(d), VRS_TOPK_RANK64) and vkradixsort_amd.torch_topk without a device:
the library builds with the frozen ABI, the key-type and flag checks, the scratch sizes (unchanged without the new flag, never smaller
with it), the wrapper's refusals and their order on CPU tensors, and the rules of the kernels (csrc/vrs_topk_order.hpp, select_rank,
select_level, sort_unrank) run on the host under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi
from vkradixsort_amd.capi import VrsError

ROOT = Path(__file__).resolve().parent.parent
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
DTYPES = [capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8, capi.VRS_SORT_INT16, capi.VRS_SORT_INT32, capi.VRS_SORT_INT64, capi.VRS_SORT_FLOAT16,
          capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64]
WIDE = (capi.VRS_SORT_INT64, capi.VRS_SORT_FLOAT64)
RANK64 = capi.VRS_TOPK_RANK64


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def scratch(lib, n, S, k, flags):
    out = ctypes.c_uint64(12345)
    return lib.vrs_topk_scratch_bytes(n, S, k, flags, ctypes.byref(out)), out.value


def call(lib, key_type, flags, S=1, k=1):
    """a NULL context and NULL handles: refused for the NULL once the key type, the flags and the shape have passed their checks"""
    rc = lib.vrs_topk_segments(None, None, 10, None, S, k, key_type, flags, None, None, None)
    return rc, lib.vrs_last_error(None)


def test_the_library_builds_and_the_abi_is_what_it_was():
    import vkradixsort_amd as vrs

    assert build.build_library() == capi.LIB_PATH and capi.LIB_PATH.exists()
    assert vrs.torch_topk is importlib.import_module("vkradixsort_amd.topk").torch_topk and "torch_topk" in vrs.__doc__
    names = (ROOT / "tests" / "golden" / "c_abi_symbols.txt").read_text().split()
    assert len(names) == 146 and sorted(capi.EXPORTED_SYMBOLS) == names
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True, check=True, timeout=60).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip() and "vrs" in line.split()[-1]) == names


def test_constants_match_the_header():
    text = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    base = int(re.search(r"#define\s+VRS_TOPK_DTYPE\(d\)\s+\((0x[0-9a-fA-F]+)\s*\|\s*\(d\)\)", text).group(1), 16)
    assert base == capi.VRS_TOPK_DTYPE_BASE == 0x100 and capi.VRS_TOPK_DTYPE(capi.VRS_SORT_FLOAT64) == 0x108
    assert int(re.search(r"\bVRS_TOPK_RANK64\s*=\s*(\d+)", text).group(1)) == RANK64 == 16
    hpp = (build.CSRC / "vrs_topk.hpp").read_text()
    assert int(re.search(r"\bkTopkRank64\s*=\s*(\d+)", hpp).group(1)) == RANK64
    assert int(re.search(r"\bkTopkDtypeBase\s*=\s*(0x[0-9a-fA-F]+)", hpp).group(1), 16) == base
    assert int(re.search(r"\bkTopkLdsBytes\s*=\s*(\d+)u", hpp).group(1)) == capi.SELECT_LDS_BYTES
    block = " ".join(re.sub(r"^\s*\*\s?", "", line).strip() for line in text.splitlines())
    for phrase in ("TORCH'S ORDER: key_type VRS_TOPK_DTYPE(d)", "OWN BITS", "vrs_select_tier_for(begin, end, num_elements, d, VRS_TUNE_TOPK_GRID_MIN_KEYS)",
                   "vrs_sort_segments_pairs_u64", "4 n + 24 S k + 1 MiB"):
        assert phrase in block, phrase


def test_key_types(lib):
    """VRS_TOPK_DTYPE(d) passes the key-type check for the nine d (the call then fails for its NULL context), and no other d does"""
    for d in DTYPES:
        rc, message = call(lib, capi.VRS_TOPK_DTYPE(d), capi.VRS_TOPK_SORTED | (RANK64 if d in WIDE else 0))
        assert rc == BAD and b"NULL" in message and b"key_type" not in message, (d, message)
    for kt in (capi.VRS_TOPK_DTYPE(9), capi.VRS_TOPK_DTYPE(255), 0x200, 0x200 | capi.VRS_SORT_INT32, 0x300, 0x1100, 0x10100, -1, 3, 99, 0x100 | 0x1000):
        rc, message = call(lib, kt, capi.VRS_TOPK_SORTED)
        assert rc == BAD and b"key_type" in message, (kt, message)
    for kt in (capi.VRS_TOPK_U32, capi.VRS_TOPK_I32, capi.VRS_TOPK_F32):  # as before
        rc, message = call(lib, kt, capi.VRS_TOPK_SORTED)
        assert rc == BAD and b"NULL" in message


def test_rank64_goes_with_the_two_8_byte_dtypes_and_no_other_key_type(lib):
    for d in DTYPES:
        for base in (0, capi.VRS_TOPK_LARGEST, capi.VRS_TOPK_SORTED | capi.VRS_TOPK_LARGEST):
            good, bad = (base | RANK64, base) if d in WIDE else (base, base | RANK64)
            rc, message = call(lib, capi.VRS_TOPK_DTYPE(d), good)
            assert rc == BAD and b"NULL" in message and b"RANK64" not in message, (d, good, message)
            rc, message = call(lib, capi.VRS_TOPK_DTYPE(d), bad)
            assert rc == BAD and b"RANK64" in message and b"NULL" not in message, (d, bad, message)
    for kt in (capi.VRS_TOPK_U32, capi.VRS_TOPK_I32, capi.VRS_TOPK_F32):
        rc, message = call(lib, kt, capi.VRS_TOPK_SORTED | RANK64)
        assert rc == BAD and b"RANK64" in message
    # the other bits stay unknown, with and without the new one; the shape check still comes before the context
    for fl in (4, 8, 32, 1 << 30, 4 | RANK64, -1):
        rc, message = call(lib, capi.VRS_TOPK_DTYPE(capi.VRS_SORT_INT64), fl)
        assert rc == BAD and b"flag" in message, (fl, message)
        assert scratch(lib, 100, 4, 8, fl)[0] == BAD
    rc, message = call(lib, capi.VRS_TOPK_DTYPE(capi.VRS_SORT_FLOAT64), RANK64, S=1 << 16, k=1 << 16)
    assert rc == BAD and b"2^32" in message


# vrs_topk_scratch_bytes of the commit before the new key types, for (n, S, k): without and with VRS_TOPK_SORTED (VRS_TOPK_LARGEST changes
# neither), taken from that commit's build
BEFORE = {
    (1, 1, 1): (512, 512), (8192, 1, 8): (512, 512), (8193, 1, 8): (9216, 9216), (100000, 7, 64): (58624, 58624),
    (1000000, 3, 4096): (25856, 25856), (1000000, 3, 4097): (25856, 222256), (100000000, 1, 1024): (57856, 57856),
    (8388608, 64, 5000): (533504, 5653248), (4294967295, 1, 1): (2106112, 2106112), (4294967295, 65536, 1000): (36208896, 36208896),
    (20000, 2, 9000): (17408, 305152), (100000000, 100000, 256): (34298624, 34298624),
}


def test_scratch_sizes_without_the_flag_are_what_they_were(lib):
    for (n, S, k), (plain, in_order) in BEFORE.items():
        for largest in (0, capi.VRS_TOPK_LARGEST):
            assert scratch(lib, n, S, k, largest) == (capi.VRS_OK, plain), (n, S, k)
            assert scratch(lib, n, S, k, largest | capi.VRS_TOPK_SORTED) == (capi.VRS_OK, in_order), (n, S, k)


def test_scratch_with_rank64_is_never_smaller_and_never_shrinks(lib):
    ns = [0, 1, 1000, 4096, 4097, 8192, 8193, 16384, 100000, 1 << 20, 10 ** 8, (1 << 32) - 1]
    Ss = [1, 2, 64, 4096, 100000, 1 << 20]
    ks = [1, 10, 64, 1024, 4096, 4097, 65536]
    for base in (0, capi.VRS_TOPK_SORTED, capi.VRS_TOPK_SORTED | capi.VRS_TOPK_LARGEST):
        size = {}
        for n in ns:
            for S in Ss:
                for k in ks:
                    if S * k >= 1 << 32:
                        continue
                    rc, wide = scratch(lib, n, S, k, base | RANK64)
                    assert rc == capi.VRS_OK
                    narrow = scratch(lib, n, S, k, base)[1]
                    assert narrow <= wide <= 4 * n + 24 * S * k + (1 << 20), (n, S, k, base)
                    # the sort area: ranks and their tmp of 8 bytes, positions and their tmp of 4 -- and only where the pair sort runs
                    big = bool(base & capi.VRS_TOPK_SORTED) and k > capi.TOPK_SORT_IN_LDS_MAX_K
                    assert wide - narrow == (8 * S * k if big else 0), (n, S, k, base)
                    size[n, S, k] = wide
        for (n, S, k), b in size.items():
            for axis, values in ((0, ns), (1, Ss), (2, ks)):
                at = values.index((n, S, k)[axis])
                if at + 1 < len(values):
                    bigger = list((n, S, k))
                    bigger[axis] = values[at + 1]
                    if tuple(bigger) in size:
                        assert size[tuple(bigger)] >= b, ((n, S, k), bigger)
    assert scratch(lib, 100, 0, 8, RANK64) == (capi.VRS_OK, 0) and scratch(lib, 100, 4, 0, RANK64) == (capi.VRS_OK, 0)


def test_wrapper_refusals_and_their_order_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    from vkradixsort_amd import torch_topk
    from vkradixsort_amd.sort import _dtype_code

    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    with pytest.raises(VrsError, match="takes a tensor"):
        torch_topk([1, 2, 3], 1)
    # the dtype first, with the text sort gives (the name aside)
    for dt in (torch.bool, torch.complex64):
        with pytest.raises(VrsError) as ours:
            torch_topk(torch.zeros(4, dtype=dt), 9, dim=7)
        with pytest.raises(VrsError) as theirs:
            _dtype_code(torch, dt, "topk")
        assert ours.value.code == BAD and str(ours.value) == str(theirs.value) and f"not {dt}" in str(ours.value)
    # then the dim, as IndexError with torch's text -- before k and before the device
    for t, dim in ((x, 2), (x, -3), (x[0], 1), (torch.tensor(3.0), 1), (torch.tensor(3.0), -2)):
        with pytest.raises(IndexError) as ours:
            torch_topk(t, 99, dim=dim)
        with pytest.raises(IndexError) as ref:
            torch.topk(t, 1, dim=dim)
        assert str(ours.value) == str(ref.value) and not isinstance(ours.value, VrsError)
    # then k, with torch's wording -- before the device
    for t, k, dim in ((x, 5, 1), (x, 4, 0), (x, -1, 1), (torch.tensor(3.0), 2, 0), (torch.zeros(3, 0), 1, 1)):
        with pytest.raises(VrsError, match="selected index k out of range") as ours:
            torch_topk(t, k, dim=dim)
        with pytest.raises(RuntimeError, match="selected index k out of range"):
            torch.topk(t, k, dim=dim)
        assert ours.value.code == BAD
    # then the device: every dtype of sort is known, and a valid call on a CPU tensor is refused for where it lives
    for dt in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64):
        for t, k, dim in ((torch.zeros((3, 4), dtype=dt), 2, 0), (torch.zeros((3, 4), dtype=dt), 0, 1), (torch.zeros((), dtype=dt), 1, 0),
                          (torch.zeros((), dtype=dt), 0, -1), (torch.zeros((3, 0), dtype=dt), 0, 1)):
            with pytest.raises(VrsError, match="GPU"):
                torch_topk(t, k, dim=dim)


def test_topk_itself_is_as_it_was():
    torch = pytest.importorskip("torch")
    from vkradixsort_amd import topk

    assert "torch_topk" in topk.__doc__
    for args in [(torch.zeros(8, dtype=torch.float64), 2), (torch.zeros(8, dtype=torch.float16), 2), (torch.zeros(4, 8), 2, 0), (torch.zeros(4, 8), 9)]:
        with pytest.raises(VrsError):
            topk(*args)


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="needs the ROCm toolchain")
def test_the_rules_on_the_host_under_sanitizers(tmp_path):
    """Every bit pattern of the 8- and 16-bit dtypes and a few thousand chosen 32- and 64-bit ones: the ranks' order against torch's
    comparator, the complement, the levels' digits, sort_unrank's exact flag, and a serial 'select, then emit in index order' with the
    kernels' rules against std::stable_sort cut at k = 1, 2, L/2, L-1, L."""
    src = build.HOST / "test" / "topk_rank_host.cpp"
    exe = tmp_path / "topk_rank_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(src), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "topk_rank_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
