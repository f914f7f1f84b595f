"""The one-rank selection's pure entry points (vrs_select_tier_for, vrs_select_target_for, vrs_select_scratch_bytes), its argument checks
and the torch wrappers' refusals: no device."""
import ctypes
import re
from pathlib import Path

import pytest

from vkradixsort_amd import capi

MIB = 1 << 20
NEW_SYMBOLS = ["vrs_select_segments", "vrs_select_scratch_bytes", "vrs_select_tier_for", "vrs_select_target_for", "vrs_select_stats"]
DTYPES = list(range(9))
WIDE = (capi.VRS_SORT_INT64, capi.VRS_SORT_FLOAT64)
KTH, MEDIAN, NANMEDIAN = capi.VRS_SELECT_KTH, capi.VRS_SELECT_MEDIAN, capi.VRS_SELECT_NANMEDIAN


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def rank_bytes(dtype):
    return 8 if dtype in WIDE else 4


def test_new_symbols_are_bound_and_exported(lib):
    header = "".join(h.read_text() for h in capi.HEADERS)
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes


def test_tune_keys_and_defaults():
    assert (capi.VRS_TUNE_SELECT_GRID_MIN_KEYS, capi.VRS_TUNE_SELECT_COMPACT_DIVISOR) == (33, 34)
    assert (capi.SELECT_GRID_MIN_KEYS_DEFAULT, capi.SELECT_COMPACT_DIVISOR_DEFAULT) == (1 << 17, 16)
    header = (Path(__file__).resolve().parents[1] / "include" / "vkradixsort_amd_tune.h").read_text()
    assert re.search(r"VRS_TUNE_SELECT_GRID_MIN_KEYS\s*=\s*33\b", header)
    assert re.search(r"VRS_TUNE_SELECT_COMPACT_DIVISOR\s*=\s*34\b", header)
    assert re.search(r"VRS_KERNEL_COUNT\s*=\s*10\b", header) and capi.VRS_KERNEL_COUNT == 10
    src = (Path(__file__).resolve().parents[1] / "vkradixsort_amd" / "csrc" / "vrs_select.hpp").read_text()
    assert re.search(r"kSelDefaultGridMinKeys\s*=\s*1u\s*<<\s*17", src) and re.search(r"kSelDefaultCompactDivisor\s*=\s*16u", src)


def tier_for(lib, b, e, n, dtype, grid_min):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_select_tier_for(b, e, n, dtype, grid_min, ctypes.byref(cb), ctypes.byref(ce), ctypes.byref(t)) == capi.VRS_OK
    return t.value, cb.value, ce.value


def tier_restated(b, e, n, dtype, grid_min):
    cb = min(b, n)
    ce = min(max(b, e), n)
    length = ce - cb
    if length <= capi.SELECT_LDS_BYTES // rank_bytes(dtype):
        t = capi.VRS_SELECT_LDS
    elif grid_min != 0 and length >= grid_min:
        t = capi.VRS_SELECT_GRID
    else:
        t = capi.VRS_SELECT_BLOCK
    return t, cb, ce


def test_tier_for_against_restatement(lib):
    n = 1 << 20
    lengths = [0, 1, 4096, 4097, 8192, 8193, (1 << 17) - 1, 1 << 17]
    for dtype in DTYPES:
        for grid_min in (capi.SELECT_GRID_MIN_KEYS_DEFAULT, 0, 4097, 8193, 20000):
            for length in lengths:
                for b in (0, 3, 12345):
                    assert tier_for(lib, b, b + length, n, dtype, grid_min) == tier_restated(b, b + length, n, dtype, grid_min), (dtype, length, b)
            # clamped and overlapping bounds
            for b, e in [(5, 3), (n - 2, n + 10), (n + 7, n + 20), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (40000, 40000), (n - 4097, n + 5),
                         (n - 8193, 0xFFFFFFFF), (n, n), (0, n), (n + 1, 5), (100, 100 + (1 << 17)), (50, 1 << 17)]:
                got = tier_for(lib, b, e, n, dtype, grid_min)
                assert got == tier_restated(b, e, n, dtype, grid_min), (dtype, b, e)
                assert got[1] <= got[2] <= n
    # both rank widths at the caps themselves
    assert tier_for(lib, 0, 8192, n, capi.VRS_SORT_FLOAT32, 1 << 17)[0] == capi.VRS_SELECT_LDS
    assert tier_for(lib, 0, 8193, n, capi.VRS_SORT_INT8, 1 << 17)[0] == capi.VRS_SELECT_BLOCK
    assert tier_for(lib, 0, 4096, n, capi.VRS_SORT_FLOAT64, 1 << 17)[0] == capi.VRS_SELECT_LDS
    assert tier_for(lib, 0, 4097, n, capi.VRS_SORT_INT64, 1 << 17)[0] == capi.VRS_SELECT_BLOCK
    assert tier_for(lib, 0, 4097, n, capi.VRS_SORT_INT64, 4097)[0] == capi.VRS_SELECT_GRID
    assert tier_for(lib, 0, 1 << 17, n, capi.VRS_SORT_INT16, 1 << 17)[0] == capi.VRS_SELECT_GRID


def test_tier_for_refusals(lib):
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_select_tier_for(0, 1, 1, 0, 0, None, ctypes.byref(ce), ctypes.byref(t)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_select_tier_for(0, 1, 1, 0, 0, ctypes.byref(cb), ctypes.byref(ce), None) == capi.VRS_ERROR_INVALID_ARGUMENT
    for dtype in (-1, 9, 99):
        assert lib.vrs_select_tier_for(0, 1, 1, dtype, 0, ctypes.byref(cb), ctypes.byref(ce), ctypes.byref(t)) == capi.VRS_ERROR_INVALID_ARGUMENT


def target_restated(mode, k, length, nans, descending):
    """(j, valid) by the header's rule."""
    if length == 0:
        return 0, 0
    if mode == KTH:
        return (k - 1, 1) if 1 <= k <= length else (0, 0)
    first_nan = 0 if descending else length - nans
    if mode == MEDIAN:
        return ((length - 1) // 2 if nans == 0 else first_nan), 1
    if nans == length:
        return first_nan, 1
    return (nans if descending else 0) + (length - nans - 1) // 2, 1


def test_target_for_against_restatement(lib):
    j, valid = ctypes.c_uint32(), ctypes.c_int()
    seen = 0
    for mode in (KTH, MEDIAN, NANMEDIAN):
        for descending in (0, 1):
            for length in range(10):
                for nans in range(length + 1):
                    for k in range(length + 2):
                        assert lib.vrs_select_target_for(mode, k, length, nans, descending, ctypes.byref(j), ctypes.byref(valid)) == capi.VRS_OK
                        assert (j.value, valid.value) == target_restated(mode, k, length, nans, descending), (mode, descending, length, nans, k)
                        if valid.value:
                            assert j.value < length
                        seen += 1
    assert seen == 3 * 2 * sum((L + 1) * (L + 2) for L in range(10))


def test_target_is_the_stable_orders_entry():
    """The rule against a sort: the median of a row with NaNs is its first NaN, the nanmedian the lower median of the others."""
    np = pytest.importorskip("numpy")
    rng = np.random.default_rng(5)
    for length in (1, 2, 5, 8, 9):
        for nans in range(length + 1):
            x = rng.standard_normal(length)
            x[rng.permutation(length)[:nans]] = np.nan
            order = np.argsort(x, kind="stable")  # (numpy sorts NaN last, as torch)
            j, _ = target_restated(MEDIAN, 0, length, nans, False)
            assert np.isnan(x[order[j]]) == (nans > 0)
            if nans:
                assert order[j] == np.nonzero(np.isnan(x))[0][0]
            else:
                assert x[order[j]] == np.sort(x)[(length - 1) // 2]
            j, _ = target_restated(NANMEDIAN, 0, length, nans, False)
            if nans < length:
                assert x[order[j]] == np.sort(x[~np.isnan(x)])[(length - nans - 1) // 2]
            else:
                assert order[j] == 0


def test_target_for_refusals(lib):
    j, valid = ctypes.c_uint32(), ctypes.c_int()
    for mode in (-1, 3, 99):
        assert lib.vrs_select_target_for(mode, 1, 4, 0, 0, ctypes.byref(j), ctypes.byref(valid)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_select_target_for(MEDIAN, 0, 4, 5, 0, ctypes.byref(j), ctypes.byref(valid)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_select_target_for(MEDIAN, 0, 4, 0, 0, None, ctypes.byref(valid)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_select_target_for(MEDIAN, 0, 4, 0, 0, ctypes.byref(j), None) == capi.VRS_ERROR_INVALID_ARGUMENT


def scratch(lib, n, S, dtype):
    out = ctypes.c_uint64(12345)
    rc = lib.vrs_select_scratch_bytes(n, S, dtype, ctypes.byref(out))
    return rc, out.value


def test_scratch_bytes_monotone_and_bounded(lib):
    """The header's bound: n * rank_bytes / 16 + 4 n + 4 S + 1 MiB; 0 for no segments; never shrinks as n grows."""
    ns = [0, 1, 1000, 4096, 4097, 8192, 8193, 16384, 16385, 100000, 1 << 17, 1 << 20, 10 ** 8, (1 << 32) - 1]
    for dtype in DTYPES:
        w = rank_bytes(dtype)
        for n in ns:
            assert scratch(lib, n, 0, dtype) == (capi.VRS_OK, 0)
        for S in (1, 2, 64, 4096, 4097, 100000, 1 << 20, (1 << 32) - 1):
            prev = -1
            for n in ns:
                rc, b = scratch(lib, n, S, dtype)
                assert rc == capi.VRS_OK
                assert b <= n * w // 16 + 4 * n + 4 * S + MIB, (dtype, n, S, b)
                assert b >= prev, (dtype, n, S)
                prev = b
        for n in (1000, 10 ** 6, 10 ** 8):
            prev = -1
            for S in (1, 2, 64, 4096, 100000, 1 << 20):
                b = scratch(lib, n, S, dtype)[1]
                assert b >= prev
                prev = b
    # the wide ranks' area is twice the narrow ones'
    assert scratch(lib, 10 ** 8, 1, capi.VRS_SORT_FLOAT64)[1] > scratch(lib, 10 ** 8, 1, capi.VRS_SORT_FLOAT32)[1]


def test_scratch_bytes_refusals(lib):
    assert lib.vrs_select_scratch_bytes(1, 1, 0, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    for dtype in (-1, 9, 99):
        assert scratch(lib, 100, 1, dtype)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"dtype" in lib.vrs_last_error(None)


def call(lib, ctx=None, dtype=capi.VRS_SORT_FLOAT32, mode=KTH, k=1, flags=0, S=1, src=None, offsets=None, out_values=None, scratch_buf=None):
    return lib.vrs_select_segments(ctx, src, 10, offsets, S, dtype, mode, k, flags, out_values, None, scratch_buf)


def test_invalid_arguments(lib):
    """Every refusal that needs no device: they come before the context is looked at."""
    fake = ctypes.c_void_p(0x1000)  # a handle that is never dereferenced: the checks below fail first
    for dtype in (-1, 9, 99):
        assert call(lib, dtype=dtype) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"dtype" in lib.vrs_last_error(None)
    for mode in (-1, 3, 99):
        assert call(lib, mode=mode) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"mode" in lib.vrs_last_error(None)
    for fl in (2, 4, -1, 1 << 30):
        assert call(lib, flags=fl) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"flag" in lib.vrs_last_error(None)
    assert call(lib, mode=KTH, k=0) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"k starts at 1" in lib.vrs_last_error(None)
    assert call(lib, mode=MEDIAN, k=0) == capi.VRS_ERROR_INVALID_ARGUMENT  # (k is not looked at; the context is NULL)
    assert b"context is NULL" in lib.vrs_last_error(None)
    assert call(lib, src=fake, offsets=fake, out_values=fake, scratch_buf=fake) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"context is NULL" in lib.vrs_last_error(None)
    s = ctypes.c_uint64()
    assert lib.vrs_select_stats(None, ctypes.byref(s), None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_torch_level_refusals_without_device():
    """dtype, dim, an empty reduction dim and k are refused before any device work, with torch's exception types; then a CPU tensor."""
    torch = pytest.importorskip("torch")
    from vkradixsort_amd import VrsError, kthvalue, median, nanmedian

    x = torch.zeros(3, 4)
    for fn in (median, nanmedian):
        with pytest.raises(VrsError, match="GPU"):
            fn(x, 1)
        with pytest.raises(VrsError, match="GPU"):
            fn(x)
        with pytest.raises(IndexError):
            fn(x, 2)
        with pytest.raises(IndexError):
            fn(x, -3)
        with pytest.raises(IndexError, match="non-zero size"):
            fn(torch.zeros(3, 0), 1)
        with pytest.raises(VrsError, match="bool"):
            fn(torch.zeros(3, dtype=torch.bool), 0)
        assert torch.isnan(fn(torch.zeros(0)))  # (as torch; nothing to run)
        assert fn(torch.zeros(0, dtype=torch.float16)).dtype == torch.float16
        with pytest.raises(VrsError):
            fn(torch.zeros(0, dtype=torch.int32))
    with pytest.raises(VrsError, match="GPU"):
        kthvalue(x, 1)
    with pytest.raises(IndexError):
        kthvalue(x, 1, 2)
    with pytest.raises(IndexError, match="non-zero size"):
        kthvalue(torch.zeros(3, 0), 1, 1)
    for k in (0, 5, -1):
        with pytest.raises(RuntimeError, match="out of range"):
            kthvalue(x, k)
    with pytest.raises(RuntimeError, match="out of range"):
        kthvalue(torch.tensor(5.0), 2)
    with pytest.raises(VrsError, match="complex"):
        kthvalue(torch.zeros(3, dtype=torch.complex64), 1)
    with pytest.raises(VrsError):
        kthvalue([1.0, 2.0], 1)
