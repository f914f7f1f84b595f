"""The membership form of the sorted search (VRS_SEARCH_MEMBER, vrs.isin) without a device: the two flag constants against the header,
what the flag check accepts and refuses, the plan functions that take no flags and so answer as before, the refusals of vrs.isin on CPU
tensors, and the decision function of the kernels (csrc/vrs_search.hpp: search_member) run on the host under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program against IEEE ==."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi

ROOT = Path(__file__).resolve().parent.parent
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
MEMBER, INVERT = 16, 32


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def call(lib, flags, nb=10, m=10, nq=10, q_len=10, dtype=capi.VRS_SORT_FLOAT32):
    return lib.vrs_search_sorted(None, None, nb, m, None, nq, q_len, dtype, flags, None, None, None)


def test_constants_equal_the_header_and_the_gap_is_stated():
    assert (capi.VRS_SEARCH_MEMBER, capi.VRS_SEARCH_MEMBER_INVERT) == (MEMBER, INVERT)
    text = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    assert int(re.search(r"\bVRS_SEARCH_MEMBER\s*=\s*(\d+)", text).group(1)) == MEMBER
    assert int(re.search(r"\bVRS_SEARCH_MEMBER_INVERT\s*=\s*(\d+)", text).group(1)) == INVERT
    enum = text[text.index("enum { VRS_SEARCH_RIGHT"):text.index("typedef enum vrs_search_tier")]
    assert "bits 4 and 8" in enum and "refused" in enum
    start = text.index("Sorted-sequence search (build extension")
    block = " ".join(t for t in text[start:text.index("enum { VRS_SEARCH_RIGHT", start)].split() if t != "*")
    for phrase in ("ONE BYTE per query", "-0.0 is a member of a row that holds +0.0", "a NaN is a member of nothing", "numpy.isin",
                   "never when c == boundary_row_len", "VRS_SEARCH_MEMBER_INVERT without VRS_SEARCH_MEMBER"):
        assert phrase in block, phrase


def test_exported_from_the_package():
    import vkradixsort_amd as vrs
    from vkradixsort_amd import search

    assert vrs.isin is search.isin


def test_the_flag_check_accepts_the_new_flags(lib):
    """a NULL context and NULL handles: the call is refused for the NULL, not for its flags"""
    for flags in (MEMBER, MEMBER | INVERT):
        assert call(lib, flags) == BAD
        message = lib.vrs_last_error(None)
        assert b"NULL" in message and b"flag" not in message, message
    for flags in (4, 8, 4 | MEMBER, 8 | MEMBER | INVERT, 64, 64 | MEMBER):
        assert call(lib, flags) == BAD
        assert b"flag" in lib.vrs_last_error(None), flags


def test_combinations_the_membership_form_refuses(lib):
    for flags, word in ((MEMBER | capi.VRS_SEARCH_RIGHT, b"VRS_SEARCH_RIGHT"), (MEMBER | capi.VRS_SEARCH_OUT_INT64, b"VRS_SEARCH_OUT_INT64"),
                        (MEMBER | INVERT | capi.VRS_SEARCH_RIGHT, b"VRS_SEARCH_RIGHT"), (INVERT, b"VRS_SEARCH_MEMBER_INVERT"),
                        (INVERT | capi.VRS_SEARCH_RIGHT, b"VRS_SEARCH_MEMBER_INVERT")):
        assert call(lib, flags) == BAD
        message = lib.vrs_last_error(None)
        assert word in message and b"NULL" not in message, (flags, message)  # (refused for the combination, before the context is looked at)
    # the counting form's flags are what they were
    for flags in (0, 1, 2, 3):
        assert call(lib, flags) == BAD and b"NULL" in lib.vrs_last_error(None)


def test_tier_and_scratch_take_no_flags_and_answer_as_before(lib):
    """pinned shapes: the values the counting call has always been given (tests/test_searchsorted_cpu.py derives the same ones)"""
    f32, i64, bf16, u8 = capi.VRS_SORT_FLOAT32, capi.VRS_SORT_INT64, capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_UINT8
    lds, table, direct, indexed = capi.VRS_SEARCH_LDS, capi.VRS_SEARCH_TABLE, capi.VRS_SEARCH_DIRECT, capi.VRS_SEARCH_INDEXED

    def tier(nb, m, nq, q_len, dtype):
        t = ctypes.c_int(-1)
        assert lib.vrs_search_tier_for(nb, m, nq, q_len, dtype, 65536, 65536, 65536, ctypes.byref(t)) == capi.VRS_OK
        return t.value

    def scratch(nb, m, dtype, sorter, t):
        b = ctypes.c_uint64(12345)
        assert lib.vrs_search_scratch_bytes(nb, m, dtype, sorter, t, ctypes.byref(b)) == capi.VRS_OK
        return b.value

    assert tier(16384, 16384, 10, 10, f32) == lds and tier(16385, 16385, 10, 10, f32) == direct
    assert tier(16385, 16385, 65536, 65536, f32) == indexed and tier(8193, 8193, 65535, 65535, i64) == direct
    assert tier(50, 50, 65536, 65536, bf16) == table and tier(50, 50, 65535, 65535, bf16) == lds
    assert tier(50, 50, 256, 256, u8) == table and tier(0, 0, 10 ** 8, 10 ** 8, u8) == lds
    assert tier(15, 5, 21, 7, f32) == lds
    assert scratch(10 ** 6, 10 ** 6, f32, 0, lds) == 0 and scratch(10 ** 6, 10 ** 6, f32, 1, direct) == 0
    assert scratch(1000, 1000, u8, 0, table) == 1024 and scratch(1000, 1000, bf16, 0, table) == 262144  # 4-byte entries hold the 0 / 1
    # the index: one 4-byte rank per 32 float32 boundaries, every 32nd again, each area rounded up to 256 bytes
    assert scratch(10 ** 6, 10 ** 6, f32, 0, indexed) == 125184 + 4096
    assert scratch(10 ** 6, 10 ** 6, f32, 1, indexed) == 125184 + 4096 + 4000000


def test_isin_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    x, t = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([2.0])
    for thunk in (lambda: vrs.isin(x, t), lambda: vrs.isin(x, 2.0), lambda: vrs.isin(2.0, t), lambda: vrs.isin(x, t, invert=True)):
        with pytest.raises(vrs.VrsError, match="GPU") as e:  # CPU tensors: no fallback
            thunk()
        assert e.value.code == BAD
    # torch's own refusal of bool, in torch's words
    for thunk in (lambda: vrs.isin(x.bool(), t.bool()), lambda: vrs.isin(x.bool(), True)):
        with pytest.raises(RuntimeError, match=r"Unsupported input type encountered for isin\(\): Bool") as e:
            thunk()
        assert not isinstance(e.value, vrs.VrsError)
    with pytest.raises(RuntimeError, match=r"Unsupported input type encountered for isin\(\): Bool"):
        torch.isin(x.bool(), t.bool())
    refused = [lambda: vrs.isin(1.0, 2.0), lambda: vrs.isin(1, 2),                    # two Python numbers
               lambda: vrs.isin(x, torch.zeros(2, dtype=torch.complex64)),            # promoted outside the nine
               lambda: vrs.isin(x.to(torch.complex128), t),
               lambda: vrs.isin(x, [2.0]), lambda: vrs.isin(x, "2")]
    for dtype in ("uint16", "uint32", "uint64"):
        if hasattr(torch, dtype):
            refused.append(lambda dtype=dtype: vrs.isin(torch.zeros(3, dtype=getattr(torch, dtype)), torch.zeros(2, dtype=getattr(torch, dtype))))
    for i, thunk in enumerate(refused):
        with pytest.raises(vrs.VrsError):
            thunk()
            pytest.fail(f"case {i} was not refused")


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="needs the ROCm toolchain")
def test_decision_function_on_the_host_under_sanitizers(tmp_path):
    """The same search_member the kernels run, behind a left count over a heap array of exact size and the kernels' guard, against
    IEEE == for float16 / bfloat16 / float32 / float64 and == for int8 / uint8 / int16 / int32 / int64: +-0.0 both ways, NaNs of both
    signs and with payloads in the queries, the boundaries and both, +-inf, subnormals, queries below and above every boundary (the
    count == m guard: the function is handed the query's own rank there and must not believe it), duplicates, all queries equal, a
    query row identical to the boundaries, empty rows, and the integers' largest rank, which is no NaN."""
    src = build.HOST / "test" / "search_member_host.cpp"
    exe = tmp_path / "search_member_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(src), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "search_member_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
