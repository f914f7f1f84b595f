"""The counting entry points without a device: the tier decision (vrs_bin_count_tier_for), the scratch sizes
(vrs_bin_count_scratch_bytes), the argument checks of vrs_bin_count, the linear rule as the library's host function evaluates it
(vrs_bin_linear_host) against a numpy restatement, and the torch-level refusals of bincount / histc / histogram."""
import ctypes
import re

import numpy as np
import pytest

from vkradixsort_amd import capi

LDS = capi.BINCOUNT_LDS_BYTES_DEFAULT
T_LDS, T_GLOBAL = capi.VRS_BINCOUNT_LDS, capi.VRS_BINCOUNT_GLOBAL
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
NONE = capi.VRS_BIN_NO_WEIGHTS
I8, U8, I16, I32, I64 = capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8, capi.VRS_SORT_INT16, capi.VRS_SORT_INT32, capi.VRS_SORT_INT64
F16, BF16, F32, F64 = capi.VRS_SORT_FLOAT16, capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def tier_for(lib, num_bins, counter_bytes=4, lds=LDS):
    t = ctypes.c_int(-1)
    rc = lib.vrs_bin_count_tier_for(num_bins, counter_bytes, lds, ctypes.byref(t))
    return rc, t.value


def scratch(lib, num_bins, weight_dtype, out_dtype):
    out = ctypes.c_uint64(12345)
    return lib.vrs_bin_count_scratch_bytes(num_bins, weight_dtype, out_dtype, ctypes.byref(out)), out.value


def test_new_symbols_are_bound_and_exported():
    for name in ("vrs_bin_count", "vrs_bin_count_tier_for", "vrs_bin_count_scratch_bytes", "vrs_bin_count_plan", "vrs_bin_count_stats",
                 "vrs_bin_linear_host"):
        assert name in capi.EXPORTED_SYMBOLS
    import vkradixsort_amd as vrs
    assert all(callable(f) for f in (vrs.bincount, vrs.histc, vrs.histogram, vrs.bincount_stats))
    assert capi.VRS_TUNE_BINCOUNT_LDS_BYTES == 32 and capi.BINCOUNT_LDS_BYTES_DEFAULT == 65536
    assert (capi.VRS_BINCOUNT_LDS, capi.VRS_BINCOUNT_GLOBAL, capi.VRS_BIN_INDEX, capi.VRS_BIN_LINEAR) == (0, 1, 0, 1)


def test_tier_at_every_boundary(lib):
    # 4-byte counters (counts, float32 weights) and the default: 16384 bins are 65536 bytes
    assert tier_for(lib, 16383) == (0, T_LDS) and tier_for(lib, 16384) == (0, T_LDS) and tier_for(lib, 16385) == (0, T_GLOBAL)
    # 8-byte counters (float64 weights)
    assert tier_for(lib, 8191, 8) == (0, T_LDS) and tier_for(lib, 8192, 8) == (0, T_LDS) and tier_for(lib, 8193, 8) == (0, T_GLOBAL)
    assert tier_for(lib, 1) == (0, T_LDS) and tier_for(lib, 2 ** 32 - 1) == (0, T_GLOBAL) and tier_for(lib, 2 ** 32 - 1, 8) == (0, T_GLOBAL)
    # lds_bytes = 0: never the LDS tier
    for bins in (1, 2, 256, 16384):
        assert tier_for(lib, bins, 4, 0) == (0, T_GLOBAL) and tier_for(lib, bins, 8, 0) == (0, T_GLOBAL)
    # all a workgroup can claim, and a setting beyond it is clamped to that
    for lds in (163840, 1 << 20):
        assert tier_for(lib, 40960, 4, lds) == (0, T_LDS) and tier_for(lib, 40961, 4, lds) == (0, T_GLOBAL)
        assert tier_for(lib, 20480, 8, lds) == (0, T_LDS) and tier_for(lib, 20481, 8, lds) == (0, T_GLOBAL)
    for lds in (4, 1024, 4096):
        assert tier_for(lib, lds // 4, 4, lds) == (0, T_LDS) and tier_for(lib, lds // 4 + 1, 4, lds) == (0, T_GLOBAL)


def test_tier_for_refuses(lib):
    assert tier_for(lib, 0)[0] == BAD and b"num_bins" in lib.vrs_last_error(None)
    for cb in (0, 2, 3, 16):
        assert tier_for(lib, 10, cb)[0] == BAD and b"counter_bytes" in lib.vrs_last_error(None)
    assert lib.vrs_bin_count_tier_for(10, 4, LDS, None) == BAD and b"tier" in lib.vrs_last_error(None)


def test_scratch_bytes_for_every_output_dtype(lib):
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for bins in (1, 2, 63, 64, 65, 16384, 16385, 10 ** 6, 2 ** 26, 2 ** 32 - 1):
        # int64 counts and weighted sums are accumulated in `out`: the two skip counters only
        assert scratch(lib, bins, NONE, I64) == (0, 256)
        assert scratch(lib, bins, F32, F32) == (0, 256) and scratch(lib, bins, F64, F64) == (0, 256)
        # float counts: 32-bit counters behind them
        for out in (F16, BF16, F32, F64):
            assert scratch(lib, bins, NONE, out) == (0, 256 + up(4 * bins)), (bins, out)


def test_scratch_bytes_refuses(lib):
    assert scratch(lib, 0, NONE, I64)[0] == BAD and b"num_bins" in lib.vrs_last_error(None)
    for out in (I8, U8, I16, I32, -1, 9):
        assert scratch(lib, 10, NONE, out)[0] == BAD and b"out dtype" in lib.vrs_last_error(None)
    for w in (F16, BF16, I32, I64, -2, 9):
        assert scratch(lib, 10, w, F32)[0] == BAD and b"weight dtype" in lib.vrs_last_error(None)
    assert scratch(lib, 10, F32, F64)[0] == BAD and scratch(lib, 10, F64, I64)[0] == BAD and b"out dtype" in lib.vrs_last_error(None)
    assert lib.vrs_bin_count_scratch_bytes(10, NONE, I64, None) == BAD and b"bytes" in lib.vrs_last_error(None)


def call(lib, dtype=I32, mode=capi.VRS_BIN_INDEX, lo=0.0, hi=0.0, bins=10, w=NONE, out=I64, n=10):
    return lib.vrs_bin_count(None, None, n, dtype, mode, lo, hi, bins, None, w, out, None, None, None)


def test_bin_count_refuses_before_any_device_work(lib):
    lin = capi.VRS_BIN_LINEAR
    assert call(lib) == BAD and b"NULL" in lib.vrs_last_error(None)                       # null handles
    assert call(lib, n=0) == BAD and b"NULL" in lib.vrs_last_error(None)
    for dtype in (F16, BF16, F32, F64, -1, 9):                                            # a dtype outside the mode's list
        assert call(lib, dtype=dtype) == BAD and b"index mode" in lib.vrs_last_error(None)
    for dtype in (I8, U8, I16, I32, I64, -1, 9):
        assert call(lib, dtype=dtype, mode=lin, lo=0.0, hi=1.0, out=F32) == BAD and b"linear mode" in lib.vrs_last_error(None)
    for mode in (-1, 2, 100):
        assert call(lib, mode=mode) == BAD and b"mode" in lib.vrs_last_error(None)
    assert call(lib, bins=0) == BAD and b"num_bins" in lib.vrs_last_error(None)           # num_bins == 0
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, -0.0)):                                  # lo >= hi
        for dtype in (F16, BF16, F32, F64):
            assert call(lib, dtype=dtype, mode=lin, lo=lo, hi=hi, out=dtype) == BAD and b"lo < hi" in lib.vrs_last_error(None)
    inf, nan = float("inf"), float("nan")
    for lo, hi in ((-inf, 1.0), (0.0, inf), (nan, 1.0), (0.0, nan), (-inf, inf)):         # a range that is not finite
        for dtype in (F16, BF16, F32, F64):
            assert call(lib, dtype=dtype, mode=lin, lo=lo, hi=hi, out=dtype) == BAD and b"finite" in lib.vrs_last_error(None)
    # a range that is finite and ascending in float64 only: the kernels of the narrower dtypes see float32
    assert call(lib, dtype=F32, mode=lin, lo=0.0, hi=1e300, out=F32) == BAD and b"finite" in lib.vrs_last_error(None)
    assert call(lib, dtype=F32, mode=lin, lo=1.0, hi=1.0 + 1e-12, out=F32) == BAD and b"lo < hi" in lib.vrs_last_error(None)
    assert call(lib, dtype=F64, mode=lin, lo=1.0, hi=1.0 + 1e-12, out=F64) == BAD and b"NULL" in lib.vrs_last_error(None)
    # a finite range whose width is not: the rule divides by hi - lo in float32 (float64 for float64)
    for dtype in (F16, BF16, F32):
        assert call(lib, dtype=dtype, mode=lin, lo=-3e38, hi=3e38, out=dtype) == BAD and b"width" in lib.vrs_last_error(None)
        assert call(lib, dtype=dtype, mode=lin, lo=-1.7e38, hi=1.7e38, out=dtype) == BAD and b"NULL" in lib.vrs_last_error(None)  # (3.4e38 is finite)
    assert call(lib, dtype=F64, mode=lin, lo=-3e38, hi=3e38, out=F64) == BAD and b"NULL" in lib.vrs_last_error(None)
    assert call(lib, dtype=F64, mode=lin, lo=-1e308, hi=1e308, out=F64) == BAD and b"width" in lib.vrs_last_error(None)
    for w in (F16, BF16, I32, I64, 9):                                                    # a weight dtype that is not float32 / float64
        assert call(lib, w=w, out=F32) == BAD and b"weight dtype" in lib.vrs_last_error(None)
    assert call(lib, w=F32, out=F64) == BAD and b"out dtype" in lib.vrs_last_error(None)
    assert call(lib, out=I32) == BAD and b"out dtype" in lib.vrs_last_error(None)
    t, b = ctypes.c_int(), ctypes.c_uint64()
    assert lib.vrs_bin_count_plan(None, 10, NONE, I64, ctypes.byref(t), ctypes.byref(b)) == BAD
    assert lib.vrs_bin_count_stats(None, ctypes.byref(b), None) == BAD


# ---------------------------------------------------------------------------------------------- the linear rule

def numpy_linear_bins(x, lo, hi, bins, wide):
    """The rule restated with numpy: three separately rounded operations in float32 (float64: wide), the last bin closed, -1 outside."""
    F = np.float64 if wide else np.float32
    v, lo, hi = x.astype(F), F(lo), F(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = v - lo
        scaled = moved * F(bins)
        q = scaled / (hi - lo)
        inside = (v >= lo) & (v <= hi)
        b = np.where(inside, q, F(0)).astype(np.int64)
    b = np.minimum(b, bins - 1)
    return np.where(inside, b, -1)


def to_bits(x32, dtype):
    """float32 values as the 16-bit patterns of float16 / bfloat16 (bfloat16: truncated, which is all a test value needs)"""
    if dtype == F16:
        return x32.astype(np.float16).view(np.uint16)
    return (x32.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(bits, dtype):
    if dtype == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def host_bins(lib, raw, dtype, lo, hi, bins):
    out = np.full(raw.size, -7, dtype=np.int64)
    rc = lib.vrs_bin_linear_host(raw.ctypes.data_as(ctypes.c_void_p), raw.size, dtype, lo, hi, bins, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, lib.vrs_last_error(None)
    return out


@pytest.mark.parametrize("dtype", [F16, BF16, F32, F64])
def test_linear_rule_on_the_host_matches_numpy(lib, dtype):
    rng = np.random.default_rng(100 + dtype)
    n = 10 ** 5
    for lo, hi, bins in ((0.0, 1.0, 100), (-3.0, 5.0, 7), (0.1, 0.7, 10 ** 4), (-1000.0, 1000.0, 1), (0.0, 64.0, 64), (1.0, 3.0, 3 * 2 ** 20)):
        F = np.float64 if dtype == F64 else np.float32
        flo, fhi = F(lo), F(hi)
        x = (rng.random(n) * (hi - lo) * 1.2 + (lo - 0.1 * (hi - lo))).astype(np.float64)   # a tenth of the range beyond either end
        edges = (flo + (fhi - flo) * (np.arange(bins + 1, dtype=np.float64)[rng.integers(0, bins + 1, 2000)] / bins)).astype(np.float64)
        special = np.array([lo, hi, np.nextafter(flo, F(-np.inf)), np.nextafter(fhi, F(np.inf)), np.nextafter(flo, F(np.inf)),
                            np.nextafter(fhi, F(-np.inf)), np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float64)
        x[:2000] = edges          # values exactly on interior edges (as nearly as the type holds them), and on lo and hi
        x[2000:2000 + special.size] = special
        if dtype == F64:
            raw, seen = x, x
        elif dtype == F32:
            raw = x.astype(np.float32)
            seen = raw
        else:
            raw = to_bits(x.astype(np.float32), dtype)
            seen = from_bits(raw, dtype)
        want = numpy_linear_bins(seen, lo, hi, bins, dtype == F64)
        got = host_bins(lib, raw, dtype, lo, hi, bins)
        assert np.array_equal(got, want), (dtype, lo, hi, bins, np.nonzero(got != want)[0][:5])
        assert (got >= -1).all() and (got < bins).all() and (got >= 0).sum() > n // 2
        on_lo, on_hi = np.nonzero(seen == F(lo))[0], np.nonzero(seen == F(hi))[0]
        if dtype in (F32, F64) or lo != 0.1:  # (0.1 and 0.7 are no float16 / bfloat16 values: nothing sits on those ends)
            assert on_lo.size and on_hi.size
        assert (got[on_lo] == 0).all() and (got[on_hi] == bins - 1).all()


def test_linear_host_refuses(lib):
    x = np.zeros(4, dtype=np.float32)
    out = np.zeros(4, dtype=np.int64)
    px, po = x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert lib.vrs_bin_linear_host(px, 4, I32, 0.0, 1.0, 10, po) == BAD and b"linear mode" in lib.vrs_last_error(None)
    assert lib.vrs_bin_linear_host(px, 4, F32, 1.0, 1.0, 10, po) == BAD and b"lo < hi" in lib.vrs_last_error(None)
    assert lib.vrs_bin_linear_host(px, 4, F32, -3e38, 3e38, 10, po) == BAD and b"width" in lib.vrs_last_error(None)
    assert lib.vrs_bin_linear_host(px, 4, F32, 0.0, 1.0, 0, po) == BAD and b"num_bins" in lib.vrs_last_error(None)
    assert lib.vrs_bin_linear_host(None, 4, F32, 0.0, 1.0, 10, po) == BAD and b"NULL" in lib.vrs_last_error(None)
    assert lib.vrs_bin_linear_host(None, 0, F32, 0.0, 1.0, 10, None) == 0


# ---------------------------------------------------------------------------------------------- the wrappers

def test_torch_level_refusals_on_cpu_tensors():
    """every refusal by its own message: the argument checks come before the check that the tensors are on a GPU, so CPU tensors reach them"""
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    idx, x = torch.arange(10), torch.rand(10)
    refused = [
        (lambda: vrs.bincount(idx), "bincount takes tensors on a GPU"),     # CPU tensors: no fallback
        (lambda: vrs.bincount(idx, weights=torch.rand(10)), "bincount takes tensors on a GPU"),
        (lambda: vrs.histc(x), "histc takes tensors on a GPU"),
        (lambda: vrs.histogram(x, 4), "histogram takes tensors on a GPU"),
        (lambda: vrs.histogram(x, torch.linspace(0, 1, 5)), "histogram takes tensors on a GPU"),
        (lambda: vrs.bincount(x), "not torch.float32"),                     # wrong dtypes
        (lambda: vrs.bincount(idx.bool()), "not torch.bool"),
        (lambda: vrs.histc(idx), "histc takes float16, bfloat16, float32 or float64, not torch.int64"),
        (lambda: vrs.histogram(idx, 4), "histogram takes float32 or float64, not torch.int64"),
        (lambda: vrs.histogram(x.half(), 4), "histogram takes float32 or float64, not torch.float16"),
        (lambda: vrs.histogram(x, torch.linspace(0, 1, 5, dtype=torch.float64)), "edges of the input's dtype"),
        (lambda: vrs.bincount(idx.view(2, 5)), "1-d non-negative"),         # a 2-D bincount input
        (lambda: vrs.bincount(torch.tensor(3)), "1-d non-negative"),
        (lambda: vrs.histc(x, bins=0), "bins must be > 0"),                 # bins <= 0
        (lambda: vrs.histc(x, bins=-3), "bins must be > 0"),
        (lambda: vrs.histc(x, bins=2.5), "bins must be > 0"),
        (lambda: vrs.histogram(x, 0), "bins must be > 0"),
        (lambda: vrs.histogram(x, -1), "bins must be > 0"),
        (lambda: vrs.bincount(idx, weights=torch.rand(9)), "same length"),  # unequal weight length
        (lambda: vrs.bincount(idx, weights=torch.rand(2, 5)), "same length"),
        (lambda: vrs.histogram(x, 4, weight=torch.rand(9)), "weight must have the input's shape and dtype"),
        (lambda: vrs.histogram(x, 4, weight=torch.rand(10, dtype=torch.float64)), "weight must have the input's shape and dtype"),
        (lambda: vrs.bincount(idx, minlength=-1), "minlength should be >= 0"),
        (lambda: vrs.histc(x, min=2, max=1), "max must be larger than min"),
        (lambda: vrs.histc(x, min=0, max=float("inf")), "is not finite"),
        (lambda: vrs.histc(x, min=float("nan"), max=1), "is not finite"),
        (lambda: vrs.histogram(x, 4, range=(0.0, float("nan"))), "is not finite"),
        (lambda: vrs.histogram(x, 4, range=(2.0, 1.0)), "max must be larger than min"),
        (lambda: vrs.histogram(x, torch.linspace(0, 1, 5), range=(0.0, 1.0)), "range goes with an int bins only"),
        (lambda: vrs.histogram(x, torch.rand(2, 3)), "1-D tensor of two or more edges"),
        (lambda: vrs.histogram(x, torch.rand(1)), "1-D tensor of two or more edges"),
        (lambda: vrs.bincount([1, 2, 3]), "bincount takes tensors"),
        (lambda: vrs.histc([0.5]), "histc takes a tensor"),
        (lambda: vrs.histogram([0.5], 4), "histogram takes tensors"),
    ]
    for i, (thunk, message) in enumerate(refused):
        with pytest.raises(vrs.VrsError, match=re.escape(message)) as e:
            thunk()
        assert e.value.code == BAD, i
