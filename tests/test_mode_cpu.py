"""The mode form of vrs_sort_restore (VRS_SORT_MODE, vrs.mode) without a device: the constant against the header and what the header
says about the scratch, the export, the flag checks of both calls behind a NULL context (made before the context is looked at), the
refusals of vrs.mode that the arguments alone decide, and the rules of the kernels (csrc/vrs_sort_mode_order.hpp) run on the host under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program against a brute-force count."""
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi

ROOT = Path(__file__).resolve().parent.parent
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
MODE = 2


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def restore(lib, flags, n=16, row_len=4, dtype=capi.VRS_SORT_INT32):
    return lib.vrs_sort_restore(None, None, None, None, n, row_len, dtype, flags, None, None)


def rank_keys(lib, flags, n=16, row_len=4, dtype=capi.VRS_SORT_INT32):
    return lib.vrs_sort_rank_keys(None, None, n, row_len, dtype, flags, None, None)


def test_constants_equal_the_headers():
    assert capi.VRS_SORT_MODE == MODE and capi.VRS_SORT_DESCENDING == 1
    text = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    assert int(re.search(r"\bVRS_SORT_MODE\s*=\s*(\d+)", text).group(1)) == MODE
    assert int(re.search(r"\bVRS_SORT_DESCENDING\s*=\s*(\d+)", text).group(1)) == 1
    start = text.index("torch.sort drop-in (build extension")
    lines = text[start:text.index("typedef enum vrs_sort_dtype", start)].splitlines()
    block = " ".join(re.sub(r"^\s*\*\s?", "", line).strip() for line in lines)  # (the comment's own stars, not the one in 8 * num_rows)
    for phrase in ("8 * num_rows", "8-byte boundary", "last occurrence", "tiles of 4096", "THE CALL'S SCRATCH", "VRS_SORT_MODE | VRS_SORT_DESCENDING",
                   "never waits for the device"):
        assert phrase in block, phrase
    order = (ROOT / "vkradixsort_amd" / "csrc" / "vrs_sort_mode_order.hpp").read_text()
    assert int(re.search(r"\bkModeTile\s*=\s*(\d+)u?\b", order).group(1)) == 4096
    assert int(re.search(r"\bkSortMode\s*=\s*(\d+)", order).group(1)) == MODE


def test_exported_from_the_package_and_the_abi_is_what_it_was():
    import vkradixsort_amd as vrs

    assert vrs.mode is importlib.import_module("vkradixsort_amd.mode").mode  # (the package's `mode` is the function)
    assert "mode " in vrs.__doc__ and "torch.mode" in vrs.__doc__
    names = (ROOT / "tests" / "golden" / "c_abi_symbols.txt").read_text().split()
    assert len(names) == 146 and sorted(capi.EXPORTED_SYMBOLS) == names
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True, check=True, timeout=60).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip() and "vrs" in line.split()[-1]) == names
    assert (build.CSRC / "vrs_sort_mode.hip") in build.HIP_SOURCES


def test_the_flag_checks_come_before_the_context(lib):
    """a NULL context and NULL handles: a call with known flags is refused for the NULL, every other for its flags"""
    assert restore(lib, MODE) == BAD
    message = lib.vrs_last_error(None)
    assert b"NULL" in message and b"flag" not in message, message
    assert restore(lib, MODE | capi.VRS_SORT_DESCENDING) == BAD
    message = lib.vrs_last_error(None)
    assert b"VRS_SORT_MODE" in message and b"VRS_SORT_DESCENDING" in message and b"NULL" not in message, message  # the combination
    for flags in (4, 6, 8, 4 | 1, -1):
        assert restore(lib, flags) == BAD
        message = lib.vrs_last_error(None)
        assert b"unknown flag bits" in message and b"NULL" not in message, (flags, message)
    for flags in (MODE, MODE | 1, 4, 6):  # the rank map takes no VRS_SORT_MODE
        assert rank_keys(lib, flags) == BAD
        message = lib.vrs_last_error(None)
        assert b"unknown flag bits" in message and b"NULL" not in message, (flags, message)
    for flags in (0, capi.VRS_SORT_DESCENDING):  # as before
        for call in (restore, rank_keys):
            assert call(lib, flags) == BAD
            message = lib.vrs_last_error(None)
            assert b"NULL" in message and b"flag" not in message, (flags, message)


def test_mode_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    x = torch.tensor([[1.0, 2.0, 2.0], [3.0, 3.0, 1.0]])
    for thunk in (lambda: vrs.mode(x), lambda: vrs.mode(x, 0, True), lambda: vrs.mode(torch.tensor(3)), lambda: vrs.mode([1, 2, 2])):
        with pytest.raises(vrs.VrsError, match="takes a tensor on a GPU") as e:  # CPU tensors: no fallback
            thunk()
        assert e.value.code == BAD
    for bad in (x.bool(), x.to(torch.complex64), x.to(torch.complex128)):
        with pytest.raises(vrs.VrsError, match=r"mode takes int8, .* or float64, not torch\.") as e:
            vrs.mode(bad)
        assert e.value.code == BAD
    for name in ("uint16", "uint32", "uint64"):
        if hasattr(torch, name):
            with pytest.raises(vrs.VrsError, match="mode takes int8"):
                vrs.mode(torch.zeros(3, dtype=getattr(torch, name)))
    for t, dim in ((x, 2), (x, -3), (torch.tensor(1.0), 1), (torch.tensor(1.0), -2)):
        with pytest.raises(IndexError, match="Dimension out of range") as e:
            vrs.mode(t, dim)
        with pytest.raises(type(e.value)):
            torch.mode(t, dim)
    # an empty reduced dim: the exception type torch's own mode raises for the same CPU tensor
    for shape, dim in (((3, 0), 1), ((0, 5), 0), ((0,), 0), ((2, 0, 4), -2)):
        empty = torch.empty(shape)
        with pytest.raises(Exception) as theirs:
            torch.mode(empty, dim)
        with pytest.raises(type(theirs.value)) as ours:
            vrs.mode(empty, dim)
        assert not isinstance(ours.value, vrs.VrsError) and str(ours.value) == str(theirs.value)


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="needs the ROCm toolchain")
def test_the_rules_on_the_host_under_sanitizers(tmp_path):
    """The order header's host evaluation of every tile (mode_tile_host: the head rule, the word, the better of two, the tile that owns a
    run, the search for the end of a tile's last run) merged per row as the kernel's atomicMax merges, against a brute-force count:
    row lengths 1, 2, 4095, 4096, 4097 and 12289, rows whose equal values touch, 32- and 64-bit ranks, runs that end at, before and
    behind tile boundaries, every run emitted by exactly one tile; and the tile and row arithmetic at 2^32 - 1 elements with row_len
    1, 3, 2^31 and 2^32 - 1 on ranks given by a rule."""
    src = build.HOST / "test" / "sort_mode_host.cpp"
    exe = tmp_path / "sort_mode_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(src), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "sort_mode_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
