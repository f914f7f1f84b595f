"""Run-length encoding and unique without a device: the scratch sizes (vrs_run_length_encode_scratch_bytes, vrs_unique_scratch_bytes),
the argument checks that fail before anything is enqueued, and the torch wrappers' refusals."""
import ctypes
import importlib

import pytest

from vkradixsort_amd import capi
from vkradixsort_amd.capi import VrsError

uq = importlib.import_module("vkradixsort_amd.unique")  # (the package's `unique` is the function of that name)

KEY_TYPES = [capi.VRS_UNIQUE_U32, capi.VRS_UNIQUE_I32, capi.VRS_UNIQUE_F32, capi.VRS_UNIQUE_U64, capi.VRS_UNIQUE_I64, capi.VRS_UNIQUE_F64]
SIZES = [0, 1, 2, capi.RLE_TILE - 1, capi.RLE_TILE, capi.RLE_TILE + 1, 10 ** 6 + 3, (1 << 24) + 5, 10 ** 8, (1 << 32) - 1]


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def rle_bytes(lib, n, key_bytes=4, flags=0):
    out = ctypes.c_uint64(12345)
    rc = lib.vrs_run_length_encode_scratch_bytes(n, key_bytes, flags, ctypes.byref(out))
    return rc, out.value


def unique_bytes(lib, n, key_type, flags=0):
    out = ctypes.c_uint64(12345)
    rc = lib.vrs_unique_scratch_bytes(n, key_type, flags, ctypes.byref(out))
    return rc, out.value


@pytest.mark.parametrize("key_bytes", [4, 8])
@pytest.mark.parametrize("flags", [0, capi.VRS_RLE_COUNTS])
def test_rle_scratch_is_zero_for_nothing_monotone_and_bounded(lib, key_bytes, flags):
    prev = -1
    for n in SIZES:
        rc, b = rle_bytes(lib, n, key_bytes, flags)
        assert rc == capi.VRS_OK
        if n == 0:
            assert b == 0
        assert b >= prev, n
        prev = b
        # the header's bound: (VRS_RLE_COUNTS ? 4 n : 0) + n / 256 + 1024
        assert b <= (4 * n if flags else 0) + n // 256 + 1024, (n, b)
        if n:
            assert b >= 8 * (-(-n // capi.RLE_TILE)) + (4 * (n + 1) if flags else 0)  # a status word per tile (+ the offsets)


@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("flags", [0, capi.VRS_UNIQUE_INVERSE, capi.VRS_UNIQUE_COUNTS, capi.VRS_UNIQUE_INVERSE | capi.VRS_UNIQUE_COUNTS])
def test_unique_scratch_is_zero_for_nothing_monotone_and_bounded(lib, key_type, flags):
    kb = 8 if key_type >= capi.VRS_UNIQUE_U64 else 4
    per_key = 2 * kb + (8 if flags & capi.VRS_UNIQUE_INVERSE else 0) + (4 if flags & capi.VRS_UNIQUE_COUNTS else 0)
    prev = -1
    for n in SIZES:
        rc, b = unique_bytes(lib, n, key_type, flags)
        assert rc == capi.VRS_OK
        if n == 0:
            assert b == 0
        assert b >= prev, n
        prev = b
        assert per_key * n <= b <= per_key * n + n // 256 + 2048, (n, b)


def test_scratch_sizes_refuse_unknown_arguments(lib):
    out = ctypes.c_uint64()
    for kb in (0, 1, 2, 3, 5, 7, 16, -4):
        assert rle_bytes(lib, 100, kb)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    for flags in (2, 4, 1 << 30, -1):
        assert rle_bytes(lib, 100, 4, flags)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    for kt in (-1, 6, 7, 100):
        assert unique_bytes(lib, 100, kt)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    for flags in (4, 8, 1 << 30, -1):
        assert unique_bytes(lib, 100, capi.VRS_UNIQUE_U32, flags)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_run_length_encode_scratch_bytes(100, 4, 0, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_unique_scratch_bytes(100, capi.VRS_UNIQUE_U32, 0, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_unique_scratch_bytes(100, capi.VRS_UNIQUE_U32, 0, ctypes.byref(out)) == capi.VRS_OK


def test_null_context_and_buffers_fail_before_anything_is_enqueued(lib):
    fake = ctypes.c_void_p(1)  # never dereferenced: the context check comes first
    assert lib.vrs_run_length_encode(None, fake, 10, 4, None, None, None, None, fake, fake) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_run_length_encode(None, None, 0, 4, None, None, None, None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_unique(None, fake, 10, capi.VRS_UNIQUE_U32, fake, None, None, fake, fake) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_unique(None, None, 0, capi.VRS_UNIQUE_U32, None, None, None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"context" in lib.vrs_last_error(None)


def test_python_scratch_helpers_match_the_library(lib):
    n = 123457
    assert uq.rle_scratch_bytes(n, 8, counts=True) == rle_bytes(lib, n, 8, capi.VRS_RLE_COUNTS)[1]
    assert uq.unique_scratch_bytes(n, "f64", inverse=True, counts=True) == \
        unique_bytes(lib, n, capi.VRS_UNIQUE_F64, capi.VRS_UNIQUE_INVERSE | capi.VRS_UNIQUE_COUNTS)[1]
    with pytest.raises(VrsError):
        uq.unique_scratch_bytes(n, "f16")
    with pytest.raises(VrsError):
        uq.rle_scratch_bytes(n, 2)


def test_torch_wrappers_refuse_what_they_do_not_take():
    torch = pytest.importorskip("torch")
    x = torch.arange(10, dtype=torch.int32)
    for fn in (uq.unique, uq.unique_consecutive):
        with pytest.raises(VrsError, match="GPU"):
            fn(x)  # a CPU tensor
        with pytest.raises(VrsError, match="dim"):
            fn(x, dim=0)
    if torch.cuda.is_available():
        for dtype in (torch.int16, torch.uint8, torch.float16, torch.bfloat16, torch.bool):
            for fn in (uq.unique, uq.unique_consecutive):
                with pytest.raises(VrsError, match="int32"):
                    fn(torch.zeros(4, dtype=dtype, device="cuda"))
