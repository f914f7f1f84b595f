"""The row form of vrs_unique / vrs_run_length_encode (VRS_UNIQUE_COLUMNS(C) in key_type / key_bytes; unique(dim=d)) without a device:
the scratch functions for the encoded values against the header's bounds, the refusals made before anything is enqueued, the constants
against the header, the frozen ABI, the torch wrappers' errors on CPU tensors, and the rules of the kernels
(csrc/vrs_unique_rows_order.hpp) run on the host under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi
from vkradixsort_amd.capi import VrsError

uq = importlib.import_module("vkradixsort_amd.unique")

ROOT = Path(__file__).resolve().parent.parent
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
COLS = capi.VRS_UNIQUE_COLUMNS
KEY_TYPES = [capi.VRS_UNIQUE_U32, capi.VRS_UNIQUE_I32, capi.VRS_UNIQUE_F32, capi.VRS_UNIQUE_U64, capi.VRS_UNIQUE_I64, capi.VRS_UNIQUE_F64]
SIZES = [0, 1, 2, capi.RLE_TILE - 1, capi.RLE_TILE, capi.RLE_TILE + 1, 10 ** 6 + 3, (1 << 24) + 5, 10 ** 8, (1 << 31) - 1]
UNIQUE_FLAGS = [0, capi.VRS_UNIQUE_INVERSE, capi.VRS_UNIQUE_COUNTS, capi.VRS_UNIQUE_INVERSE | capi.VRS_UNIQUE_COUNTS]


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def rle_bytes(lib, n, key_bytes, flags=0):
    out = ctypes.c_uint64(12345)
    return lib.vrs_run_length_encode_scratch_bytes(n, key_bytes, flags, ctypes.byref(out)), out.value


def unique_bytes(lib, n, key_type, flags=0):
    out = ctypes.c_uint64(12345)
    return lib.vrs_unique_scratch_bytes(n, key_type, flags, ctypes.byref(out)), out.value


@pytest.mark.parametrize("cols", [2, 3, 5, 128])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_unique_row_scratch_is_bounded_monotone_and_the_same_for_every_column_count(lib, key_type, cols):
    prev = -1
    for n in SIZES:
        if n * cols >= 1 << 32:
            continue
        sizes = set()
        for flags in UNIQUE_FLAGS:
            rc, b = unique_bytes(lib, n, key_type | COLS(cols), flags)
            assert rc == capi.VRS_OK, (n, cols, flags)
            sizes.add(b)
        assert len(sizes) == 1  # the positions and the offsets serve the rows whichever outputs are given
        b = sizes.pop()
        assert b == unique_bytes(lib, n, capi.VRS_UNIQUE_U32 | COLS(2))[1]  # "whatever C is"
        assert (b == 0) == (n == 0)
        assert b >= prev, n
        prev = b
        # the header's bound; and room for what it names: two key buffers of 8 bytes, two position buffers, the offsets
        assert b <= 28 * n + n // 256 + 4096, (n, b)
        if n:
            assert b >= 28 * n + 4 + 8 * (-(-n // capi.RLE_TILE))


@pytest.mark.parametrize("cols", [2, 3, 5, 128])
@pytest.mark.parametrize("width", [4, 8])
def test_encode_row_scratch_is_bounded_and_monotone(lib, width, cols):
    prev = -1
    for n in SIZES:
        if n * cols >= 1 << 32:
            continue
        rc, b = rle_bytes(lib, n, width | COLS(cols), 0)
        assert rc == capi.VRS_OK
        assert b == rle_bytes(lib, n, width | COLS(cols), capi.VRS_RLE_COUNTS)[1]  # always with the offsets
        assert (b == 0) == (n == 0)
        assert b >= prev, n
        prev = b
        assert b <= 4 * n + n // 256 + 2048, (n, b)
        if n:
            assert b >= 4 * (n + 1) + 8 * (-(-n // capi.RLE_TILE))


def test_zero_and_one_column_are_the_word_form(lib):
    for n in SIZES + [(1 << 32) - 1]:
        for c in (0, 1):
            for kt in KEY_TYPES:
                for flags in UNIQUE_FLAGS:
                    assert unique_bytes(lib, n, kt | COLS(c), flags) == unique_bytes(lib, n, kt, flags)
            for width in (4, 8):
                for flags in (0, capi.VRS_RLE_COUNTS):
                    assert rle_bytes(lib, n, width | COLS(c), flags) == rle_bytes(lib, n, width, flags)


def test_refusals_without_a_device(lib):
    n = 1000
    for low in (6, 7, 100, 255):  # an unknown low byte with columns set
        assert unique_bytes(lib, n, low | COLS(3))[0] == BAD
    for low in (0, 1, 2, 3, 5, 7, 16, 255):
        assert rle_bytes(lib, n, low | COLS(3))[0] == BAD
    for value in (-1, -4, -256, -(1 << 8) | 4, -(1 << 31)):  # negative values
        assert unique_bytes(lib, n, value)[0] == BAD
        assert rle_bytes(lib, n, value)[0] == BAD
    # n x C >= 2^32
    for n_, c in ((1 << 31, 2), ((1 << 32) - 1, 2), (1 << 30, 4), (1 << 16, 1 << 16), (3, (1 << 23) - 1 << 0)):
        expect = BAD if n_ * c >= 1 << 32 else capi.VRS_OK
        assert unique_bytes(lib, n_, capi.VRS_UNIQUE_I64 | COLS(c))[0] == expect, (n_, c)
        assert rle_bytes(lib, n_, 8 | COLS(c))[0] == expect, (n_, c)
    assert unique_bytes(lib, (1 << 31) - 1, capi.VRS_UNIQUE_I32 | COLS(2))[0] == capi.VRS_OK
    for flags in (4, 8, 1 << 30, -1):  # the flag bits, as in the word form
        assert unique_bytes(lib, n, capi.VRS_UNIQUE_U32 | COLS(2), flags)[0] == BAD
    for flags in (2, 4, 1 << 30, -1):
        assert rle_bytes(lib, n, 4 | COLS(2), flags)[0] == BAD
    assert lib.vrs_unique_scratch_bytes(n, capi.VRS_UNIQUE_U32 | COLS(2), 0, None) == BAD
    assert lib.vrs_run_length_encode_scratch_bytes(n, 4 | COLS(2), 0, None) == BAD
    # the calls themselves: the context check comes first, the encoded value is decoded behind it
    fake = ctypes.c_void_p(1)
    assert lib.vrs_unique(None, fake, 10, capi.VRS_UNIQUE_U32 | COLS(2), fake, None, None, fake, fake) == BAD
    assert lib.vrs_run_length_encode(None, fake, 10, 4 | COLS(2), None, None, None, None, fake, fake) == BAD
    assert b"context" in lib.vrs_last_error(None)


def test_python_helpers_equal_the_library(lib):
    n = 123457
    for cols in (2, 3, 9):
        assert uq.unique_scratch_bytes(n, "f64", inverse=True, counts=True, columns=cols) == \
            unique_bytes(lib, n, capi.VRS_UNIQUE_F64 | COLS(cols), capi.VRS_UNIQUE_INVERSE | capi.VRS_UNIQUE_COUNTS)[1]
        assert uq.rle_scratch_bytes(n, 8, counts=True, columns=cols) == rle_bytes(lib, n, 8 | COLS(cols), capi.VRS_RLE_COUNTS)[1]
        assert uq.rle_scratch_bytes(n, 4, columns=cols) == rle_bytes(lib, n, 4 | COLS(cols), 0)[1]
    assert uq.unique_scratch_bytes(n, "i32", columns=1) == uq.unique_scratch_bytes(n, "i32")
    with pytest.raises(VrsError):
        uq.unique_scratch_bytes(1 << 31, "i32", columns=2)
    with pytest.raises(VrsError):
        uq.rle_scratch_bytes(n, 4, columns=-1)
    with pytest.raises(VrsError):
        uq.unique_scratch_bytes(n, "i32", columns=1 << 23)


def test_constants_equal_the_header_and_the_abi_is_what_it_was():
    text = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    shift = int(re.search(r"#define\s+VRS_UNIQUE_COLUMNS\(c\)\s+\(\(int\)\(c\)\s*<<\s*(\d+)\)", text).group(1))
    assert shift == capi.VRS_UNIQUE_COLUMNS_SHIFT == 8
    assert COLS(0) == 0 and COLS(1) == 256 and COLS(5) | capi.VRS_UNIQUE_F64 == 5 * 256 + 5
    order = (build.CSRC / "vrs_unique_rows_order.hpp").read_text()
    assert int(re.search(r"\bkRowsColumnsShift\s*=\s*(\d+)u?\b", order).group(1)) == shift
    block = " ".join(re.sub(r"^\s*\*\s?", "", line).strip() for line in text.splitlines())
    assert block.count("THE ROW FORM: key_") == 2  # one paragraph in each of the two comments
    for phrase in ("28 n + n / 256 + 4096", "4 n + n / 256 + 2048", "n x C >= 2^32", "C of 0 or 1 is the form above, bit for bit"):
        assert phrase in block, phrase
    names = (ROOT / "tests" / "golden" / "c_abi_symbols.txt").read_text().split()
    assert len(names) == 146 and sorted(capi.EXPORTED_SYMBOLS) == names
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True, check=True, timeout=60).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip() and "vrs" in line.split()[-1]) == names
    assert (build.CSRC / "vrs_unique_rows.hip") in build.HIP_SOURCES


def test_wrapper_errors_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    x = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    for fn, theirs in ((uq.unique, torch.unique), (uq.unique_consecutive, torch.unique_consecutive)):
        for t, dim in ((x, 2), (x, -3), (x[0], 1), (torch.tensor(3), 0), (torch.tensor(3), -2)):
            with pytest.raises(IndexError) as ours:
                fn(t, dim=dim)
            with pytest.raises(IndexError) as ref:
                theirs(t, dim=dim)
            assert str(ours.value) == str(ref.value)
        for dim, named in ((0, 0), (1, 1), (-1, 1), (-2, 0)):  # no fallback: the refusal names the dim
            with pytest.raises(VrsError, match=rf"\(dim={named}\) takes a tensor on a GPU") as e:
                fn(x, dim=dim)
            assert e.value.code == BAD
        with pytest.raises(VrsError, match="dim"):
            fn(x, dim=(0, 1))
        with pytest.raises(VrsError, match="GPU"):  # dim=None: as before
            fn(x)


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="needs the ROCm toolchain")
def test_the_rules_on_the_host_under_sanitizers(tmp_path):
    """The order header's plan, pack and head rule on seeded matrices of all six key types, C = 1 .. 9: the LSD rounds with
    std::stable_sort on the packed keys against one stable sort with a lexicographic comparator on the ranks; heads, run ids, starts
    and counts from the head rule against memcmp of adjacent rows."""
    src = build.HOST / "test" / "unique_rows_host.cpp"
    exe = tmp_path / "unique_rows_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(src), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "unique_rows_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
