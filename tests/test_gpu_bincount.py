"""vrs.bincount / vrs.histc / vrs.histogram and the C-ABI call under them on the device, count for count: against numpy.bincount, the
numpy restatement of the linear rule (tests/test_bincount_cpu.py) and numpy.searchsorted, and against torch where torch is exact;
both tiers natural and forced (asserted through bincount_stats), every element dtype, the whole-wave shortcut and its near misses,
the skip counters, views, streams, and the scratch of two calls in a row."""
import ctypes
import time

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for
from vkradixsort_amd.sort import _dtype_code

from .test_bincount_cpu import numpy_linear_bins

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INDEX_DTYPES = ["uint8", "int8", "int16", "int32", "int64"]
LINEAR_DTYPES = ["float16", "bfloat16", "float32", "float64"]
NS = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
KNOB, DEFAULT, MAX = capi.VRS_TUNE_BINCOUNT_LDS_BYTES, capi.BINCOUNT_LDS_BYTES_DEFAULT, capi.BINCOUNT_LDS_BYTES_MAX
FORCE = {"lds": MAX, "global": 0}
TIER_OF = {capi.VRS_BINCOUNT_LDS: "lds", capi.VRS_BINCOUNT_GLOBAL: "global"}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    yield c
    c.setTuning(KNOB, DEFAULT)


def count(c, values, bins, *, mode=capi.VRS_BIN_INDEX, lo=0.0, hi=0.0, weights=None, out_dtype=None, want_skipped=True):
    """vrs_bin_count itself: (out, the two skip counters as a list or None, the planned tier's name).  `out`, `skipped` and the scratch
    hold garbage on entry: the library clears what it accumulates into."""
    out_dtype = out_dtype or (weights.dtype if weights is not None else torch.int64)
    d = values.device
    out = torch.full((bins,), 77, dtype=out_dtype, device=d)
    skipped = torch.full((2,), -5, dtype=torch.int64, device=d) if want_skipped else None
    w_code = capi.VRS_BIN_NO_WEIGHTS if weights is None else _dtype_code(torch, weights.dtype)
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    c.check(c.lib.vrs_bin_count_plan(c.handle, bins, w_code, _dtype_code(torch, out_dtype), ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.full((need.value,), 0xAB, dtype=torch.uint8, device=d)
    with buffers(c, values, weights, out, skipped, scratch) as (v, w, o, s, scr):
        c.check(c.lib.vrs_bin_count(c.handle, v, values.numel(), _dtype_code(torch, values.dtype), mode, lo, hi, bins, w, w_code,
                                    _dtype_code(torch, out_dtype), o, s, scr))
    return out, (skipped.tolist() if want_skipped else None), TIER_OF[tier.value]


def as_out(counts, dtype):
    """integer counts (numpy) as a CPU tensor of the output dtype, each the correctly rounded count"""
    counts = np.asarray(counts, dtype=np.int64)
    if dtype == torch.int64:
        return torch.from_numpy(counts)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):  # (beyond float16's range: inf)
            return torch.from_numpy(counts.astype(np.float64).astype(np.float16))  # (exact in float64, then one rounding)
    if dtype == torch.bfloat16:
        assert counts.max(initial=0) < 1 << 24  # (exact in float32, then one rounding)
        return torch.from_numpy(counts.astype(np.float32)).to(torch.bfloat16)
    return torch.from_numpy(counts.astype(np.float32 if dtype == torch.float32 else np.float64))


def ref_index(x, bins, w=None):
    """numpy.bincount of the elements in [0, bins) and the two skip counts"""
    x = x.astype(np.int64)
    ok = (x >= 0) & (x < bins)
    counts = np.bincount(x[ok], weights=None if w is None else w[ok].astype(np.float64), minlength=bins)
    return counts, [int((x < 0).sum()), int((x >= bins).sum())]


def make(name, n, bins, rng, dtype):
    """n elements of a distribution over `bins` bins as int64 (numpy), within the dtype's range"""
    info = np.iinfo(dtype)
    items = 16 // np.dtype(dtype).itemsize  # elements a lane holds of one tile: lane l of a wave has elements [l * items, (l + 1) * items)
    i = np.arange(n, dtype=np.int64)
    below, beyond = (-1 if info.min < 0 else 0), min(bins, info.max)
    if name == "constant":
        x = np.full(n, bins // 2, dtype=np.int64)
    elif name == "one_lane":  # constant except lane 17 of every wave: every wave misses the shortcut by one lane
        x = np.where((i // items) % 64 == 17, bins - 1 if bins > 1 else beyond, 0)
    elif name == "one_lane_skipped":  # ... that lane's elements have no bin: the shortcut holds with one lane left out
        x = np.where((i // items) % 64 == 17, beyond, bins // 2)
    elif name == "alternating":
        x = np.where(i % 2 == 0, 0, bins - 1)
    elif name == "uniform":
        x = rng.integers(0, bins, n)
    elif name == "ramp":
        x = i % bins
    elif name == "out_of_range":
        x = np.where(i % 3 == 0, below if below < 0 else beyond, beyond)
    else:  # mix: in range, negative, and at or beyond the end
        x = rng.integers(max(info.min, -bins // 2 - 1), min(info.max, 2 * bins) + 1, n)
    return np.asarray(x, dtype=np.int64)


def stats_delta(c, before):
    now = vrs.bincount_stats(c)
    return {k: now[k] - before[k] for k in now}


def check_index(c, x, bins, dtype, tier, outs=(torch.int64, torch.float32), weights=(None,)):
    """the call on x (int64 numpy, cast to dtype) in the forced `tier`, for every output dtype and weight dtype given"""
    d = torch.device("cuda", 0)
    xd = torch.from_numpy(x.astype(dtype)).to(d)
    for wd in weights:
        w = None if wd is None else ((np.arange(x.size) % 7) - 2).astype(wd)  # small integers: every order of summation gives the same float
        counts, skips = ref_index(x, bins, w)
        for out_dtype in (outs if wd is None else (None,)):
            before = vrs.bincount_stats(c)
            got, skipped, planned = count(c, xd, bins, weights=None if w is None else torch.from_numpy(w).to(d), out_dtype=out_dtype)
            want = as_out(counts, out_dtype) if wd is None else torch.from_numpy(counts.astype(wd))
            assert got.dtype == want.dtype and torch.equal(got.cpu(), want), (dtype, x.size, bins, tier, out_dtype, wd)
            assert skipped == skips, (dtype, x.size, bins, tier, skipped, skips)
            delta = stats_delta(c, before)
            assert planned == tier and delta == {"lds": int(tier == "lds" and x.size > 0), "global": int(tier == "global" and x.size > 0)}, (delta, tier)


@pytest.mark.parametrize("tier", ["lds", "global"])
@pytest.mark.parametrize("dtype", INDEX_DTYPES)
def test_every_dtype_in_both_tiers(ctx, dtype, tier):
    rng = np.random.default_rng(INDEX_DTYPES.index(dtype))
    bins = {"uint8": 200, "int8": 100, "int16": 257, "int32": 4097, "int64": 257}[dtype]
    ctx.setTuning(KNOB, FORCE[tier])
    for n in NS:
        check_index(ctx, make("mix", n, bins, rng, dtype), bins, dtype, tier, weights=(None, np.float32) if n in (65, 4097) else (None,))
    # more tiles than the grid has workgroups, plus one element: the grid-stride loop and the tail both run
    cus = ctx.deviceInfo()[1]
    n = (capi.BINCOUNT_TILE_BYTES // np.dtype(dtype).itemsize) * cus * capi.BINCOUNT_WORKGROUPS_PER_CU + 1
    all_outs = (torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64)
    check_index(ctx, make("mix", n, bins, rng, dtype), bins, dtype, tier, outs=all_outs, weights=(None, np.float32, np.float64))
    # ... and of one value: counts beyond what float16 / bfloat16 hold exactly (float16: beyond its range), each rounded once
    check_index(ctx, make("constant", n, bins, rng, dtype), bins, dtype, tier, outs=all_outs)


@pytest.mark.parametrize("bins", [1, 2, 255, 256, 257, 16383, 16384, 16385, 1 << 20])
def test_num_bins_natural_and_forced(ctx, dev, bins):
    rng = np.random.default_rng(bins)
    x = make("mix", 50001, bins, rng, "int32")
    natural = "lds" if bins * 4 <= DEFAULT else "global"
    check_index(ctx, x, bins, "int32", natural, weights=(None, np.float32))
    # float64 weights: 8-byte counters, half as many fit
    check_index(ctx, x, bins, "int32", "lds" if bins * 8 <= DEFAULT else "global", outs=(), weights=(np.float64,))
    for tier in ("lds", "global"):
        if tier == "lds" and bins * 8 > MAX:
            continue
        ctx.setTuning(KNOB, FORCE[tier])
        check_index(ctx, x, bins, "int32", tier, weights=(None, np.float32, np.float64))
    ctx.setTuning(KNOB, DEFAULT)
    # the drop-in on the same data (its size comes from the data: the elements in range only)
    inside = torch.from_numpy(x[(x >= 0) & (x < bins)].astype(np.int32)).to(dev)
    assert torch.equal(vrs.bincount(inside, minlength=bins), torch.bincount(inside, minlength=bins))


@pytest.mark.parametrize("tier", ["lds", "global"])
@pytest.mark.parametrize("name", ["constant", "one_lane", "one_lane_skipped", "alternating", "uniform", "ramp", "out_of_range", "mix"])
def test_distributions(ctx, name, tier):
    rng = np.random.default_rng(7)
    ctx.setTuning(KNOB, FORCE[tier])
    for dtype, bins, n in (("int32", 1000, 64 * 1024 + 37), ("int8", 100, 256 * 1024 + 5), ("int64", 1, 20001), ("int16", 2, 20001)):
        check_index(ctx, make(name, n, bins, rng, dtype), bins, dtype, tier, weights=(None, np.float32, np.float64))


# ---------------------------------------------------------------------------------------------- bincount

@pytest.mark.parametrize("dtype", INDEX_DTYPES)
def test_bincount_equals_torch_bit_for_bit(dev, dtype):
    rng = np.random.default_rng(11)
    top = 100 if dtype in ("int8", "uint8") else 3000
    x = torch.from_numpy(rng.integers(0, top + 1, 30011).astype(dtype)).to(dev)
    x[5] = top
    for minlength in (0, top - 10, top + 1, top + 50):
        got = vrs.bincount(x, minlength=minlength)
        assert got.dtype == torch.int64 and torch.equal(got, torch.bincount(x, minlength=minlength)), (dtype, minlength)
    for wdtype in (torch.float32, torch.float64, torch.int32, torch.float16):  # (int32 and float16 weights: float64, as torch)
        w = torch.from_numpy(rng.integers(-3, 9, x.numel())).to(wdtype).to(dev)
        got, want = vrs.bincount(x, weights=w, minlength=top + 7), torch.bincount(x, weights=w, minlength=top + 7)
        assert got.dtype == want.dtype and torch.equal(got, want), (dtype, wdtype)


def test_bincount_negative_empty_and_views(dev):
    x = torch.tensor([3, 1, -2, 5], device=dev)
    with pytest.raises(vrs.VrsError, match="bincount only supports 1-d non-negative integral inputs"):  # (torch's message)
        vrs.bincount(x)
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    for minlength in (0, 5):
        assert torch.equal(vrs.bincount(empty, minlength=minlength), torch.bincount(empty, minlength=minlength))
        got = vrs.bincount(empty, weights=torch.empty(0, dtype=torch.float32, device=dev), minlength=minlength)
        assert got.dtype == torch.float32 and got.numel() == minlength and not got.any()
    rng = np.random.default_rng(13)
    # views that start 1 to 3 bytes into a 4-byte word (int32: 4 to 12 bytes into a 16-byte vector); non-contiguous inputs
    for dtype in ("uint8", "int8", "int16", "int32"):
        base = torch.from_numpy(rng.integers(0, 90, 10007).astype(dtype)).to(dev)
        w = torch.from_numpy(rng.integers(0, 5, 10007).astype(np.float32)).to(dev)
        for view, wv in ((base[1:], w[1:]), (base[3:], w[3:]), (base[::2], w[::2]), (base[1::3], w[1::3])):
            assert torch.equal(vrs.bincount(view), torch.bincount(view)), dtype
            assert torch.equal(vrs.bincount(view, weights=wv), torch.bincount(view, weights=wv)), dtype


# ---------------------------------------------------------------------------------------------- histc

def linear_values(dtype, n, lo, hi, bins, rng, specials=True):
    """n values around [lo, hi] as a CPU tensor of the dtype: some exactly on lo, on hi and on interior edges, NaN and both infinities"""
    x = rng.random(n) * (hi - lo) * 1.2 + (lo - 0.1 * (hi - lo))
    k = n // 10
    x[:k] = lo + (hi - lo) * rng.integers(0, bins + 1, k) / bins
    x[k:k + 8] = [lo, hi, lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), lo, hi]
    if specials:
        x[k + 8:k + 14] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    return torch.from_numpy(x).to(getattr(torch, dtype))


def ref_histc(x_cpu, lo, hi, bins):
    """counts by the numpy restatement of the rule, on the values as float32 (float64 for float64)"""
    wide = x_cpu.dtype == torch.float64
    seen = x_cpu.numpy() if wide else x_cpu.float().numpy()
    at = numpy_linear_bins(seen, lo, hi, bins, wide)
    return np.bincount(at[at >= 0], minlength=bins)


@pytest.mark.parametrize("dtype", LINEAR_DTYPES)
def test_histc_equals_the_restated_rule(ctx, dev, dtype):
    rng = np.random.default_rng(17 + LINEAR_DTYPES.index(dtype))
    dt = getattr(torch, dtype)
    for tier in ("lds", "global"):
        ctx.setTuning(KNOB, FORCE[tier])
        for lo, hi, bins, n in ((0.0, 1.0, 100, 20011), (-3.0, 5.0, 7, 4097), (0.0, 64.0, 64, 65), (-2.0, 2.0, 10 ** 4, 30001), (1.0, 3.0, 1, 257)):
            x = linear_values(dtype, n, lo, hi, bins, rng)
            before = vrs.bincount_stats(ctx)
            got = vrs.histc(x.to(dev), bins=bins, min=lo, max=hi)
            assert got.dtype == dt and got.shape == (bins,)
            assert torch.equal(got.cpu(), as_out(ref_histc(x, lo, hi, bins), dt)), (dtype, tier, lo, hi, bins)
            assert stats_delta(ctx, before)[tier] == 1
    ctx.setTuning(KNOB, DEFAULT)
    # the range from the data (no NaN or infinities in it: those raise, below); a 2-D non-contiguous input
    x = linear_values(dtype, 20011, -1.0, 7.0, 50, rng, specials=False)
    lo, hi = x.min().item(), x.max().item()
    assert torch.equal(vrs.histc(x.to(dev), bins=50).cpu(), as_out(ref_histc(x, lo, hi, 50), dt))
    x2 = x[:20000].view(100, 200).t()
    lo, hi = x2.min().item(), x2.max().item()
    assert torch.equal(vrs.histc(x2.to(dev), bins=33).cpu(), as_out(ref_histc(x2.contiguous().view(-1), lo, hi, 33), dt))
    # min == max in the data: the range is widened by 1 each way
    same = torch.full((1000,), 2.5, dtype=dt)
    assert torch.equal(vrs.histc(same.to(dev), bins=4).cpu(), as_out(ref_histc(same, 1.5, 3.5, 4), dt))
    assert vrs.histc(same.to(dev), bins=4).cpu().tolist() == [0.0, 0.0, 1000.0, 0.0]
    for bad in (float("nan"), float("inf")):
        broken = same.clone()
        broken[7] = bad
        with pytest.raises(vrs.VrsError, match="is not finite"):
            vrs.histc(broken.to(dev), bins=4)
    assert vrs.histc(torch.empty(0, dtype=dt, device=dev), bins=3).tolist() == [0.0, 0.0, 0.0]
    if dtype in ("float16", "bfloat16"):  # a view that starts 2 bytes into a 4-byte word
        base = linear_values(dtype, 5001, 0.0, 1.0, 10, rng)
        assert torch.equal(vrs.histc(base.to(dev)[1:], bins=10, min=0.0, max=1.0).cpu(), as_out(ref_histc(base[1:], 0.0, 1.0, 10), dt))


def test_histc_equals_torch_where_the_arithmetic_is_exact(dev):
    """integer-valued data in [0, 2^k), lo = 0, hi = 2^k, a power-of-two bin count: every operation of the rule is exact"""
    rng = np.random.default_rng(19)
    for dtype, k, bins in ((torch.float32, 10, 64), (torch.float32, 16, 1024), (torch.float64, 20, 64)):
        x = torch.from_numpy(rng.integers(0, 1 << k, 10 ** 5)).to(dtype).to(dev)
        got, want = vrs.histc(x, bins=bins, min=0, max=1 << k), torch.histc(x, bins=bins, min=0, max=1 << k)
        assert got.dtype == want.dtype and torch.equal(got, want), (dtype, k, bins)


def test_float32_count_beyond_2_24_is_exact(dev):
    """2^24 + 2 ones in one bin: integer counters converted once give 16777218.0 (a float32 sum of ones stops at 16777216.0)"""
    x = torch.ones((1 << 24) + 2, dtype=torch.float32, device=dev)
    got = vrs.histc(x, bins=4, min=0.0, max=4.0)
    assert got.tolist() == [0.0, 16777218.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------- histogram

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_histogram_with_edges_equals_torch_on_the_cpu(dev, dtype):
    rng = np.random.default_rng(23)
    dt = getattr(torch, dtype)
    edges = torch.tensor([-2.0, -1.5, 0.0, 0.25, 1.0, 3.0, 3.5, 10.0], dtype=dt)
    x = torch.from_numpy(rng.random(20011) * 14.0 - 3.0).to(dt)  # beyond the edges on both sides
    x[:800] = edges[torch.from_numpy(rng.integers(0, edges.numel(), 800))]  # on every edge, the last one included
    w = torch.from_numpy(rng.integers(-2, 6, x.numel())).to(dt)
    for weight in (None, w):
        want = torch.histogram(x, edges, weight=weight)
        got = vrs.histogram(x.to(dev), edges.to(dev), weight=None if weight is None else weight.to(dev))
        assert got[0].dtype == dt and torch.equal(got[0].cpu(), want.hist) and torch.equal(got[1].cpu(), want.bin_edges)
        dense = vrs.histogram(x.to(dev), edges.to(dev), weight=None if weight is None else weight.to(dev), density=True)
        torch.testing.assert_close(dense[0].cpu(), torch.histogram(x, edges, weight=weight, density=True).hist)
    # NaN elements are counted nowhere, here as in torch's CPU kernel: the same tensors, and torch's result without them
    xn = x.clone()
    xn[1000:1010] = float("nan")
    keep = ~torch.isnan(xn)
    for weight in (None, w):
        want = torch.histogram(xn, edges, weight=weight).hist
        assert torch.equal(want, torch.histogram(xn[keep], edges, weight=None if weight is None else weight[keep]).hist)
        got = vrs.histogram(xn.to(dev), edges.to(dev), weight=None if weight is None else weight.to(dev))
        assert torch.equal(got[0].cpu(), want)
    # a 2-D non-contiguous input
    x2 = x[:20000].view(100, 200).t()
    assert torch.equal(vrs.histogram(x2.to(dev), edges.to(dev))[0].cpu(), torch.histogram(x2, edges).hist)
    assert vrs.histogram(torch.empty(0, dtype=dt, device=dev), edges.to(dev))[0].tolist() == [0.0] * 7


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_histogram_with_int_bins_against_numpy_searchsorted(dev, dtype):
    rng = np.random.default_rng(29)
    dt = getattr(torch, dtype)
    x = torch.from_numpy(rng.standard_normal(30011) * 3.0).to(dt)
    x[5:9] = float("nan")

    def check(got, values, bins, lo_hi=None):
        hist, edges = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert edges.dtype == values.dtype and edges.size == bins + 1 and hist.dtype == values.dtype
        if lo_hi is not None:
            assert edges[0] == values.dtype.type(lo_hi[0]) and edges[-1] == values.dtype.type(lo_hi[1])
        at = np.searchsorted(edges, values, side="right") - 1
        at[values == edges[-1]] = bins - 1
        ok = (at >= 0) & (at < bins) & ~np.isnan(values)
        assert np.array_equal(hist, np.bincount(at[ok], minlength=bins).astype(values.dtype))

    for bins, rng_ in ((100, (-4.0, 4.0)), (7, (0.0, 1.0)), (1, (-1.0, 1.0))):
        check(vrs.histogram(x.to(dev), bins, range=rng_), x.numpy(), bins, rng_)
    clean = x[~torch.isnan(x)]
    check(vrs.histogram(clean.to(dev), 50), clean.numpy(), 50, (clean.min().item(), clean.max().item()))  # the last bin takes the maximum
    same = torch.full((100,), 2.0, dtype=dt)
    check(vrs.histogram(same.to(dev), 4), same.numpy(), 4, (1.5, 2.5))
    with pytest.raises(vrs.VrsError, match="is not finite"):
        vrs.histogram(x.to(dev), 10)


# ---------------------------------------------------------------------------------------------- streams and scratch

def test_non_default_stream(dev):
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.integers(0, 5000, 10 ** 6)).to(dev)
    f = torch.from_numpy(rng.random(10 ** 6).astype(np.float32)).to(dev)
    want_counts, want_hist = torch.bincount(x), ref_histc(f.cpu(), 0.0, 1.0, 100)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        c = context_for(dev)
        before = vrs.bincount_stats(c)
        counts = vrs.bincount(x)
        hist = vrs.histc(f, bins=100, min=0.0, max=1.0)
        wide = vrs.bincount(x, minlength=10 ** 5)
        after = vrs.bincount_stats(c)
    side.synchronize()
    assert torch.equal(counts, want_counts) and torch.equal(hist.cpu(), as_out(want_hist, torch.float32))
    assert torch.equal(wide[:want_counts.numel()], want_counts) and not wide[want_counts.numel():].any()
    assert c is not context_for(dev) and after["lds"] - before["lds"] == 2 and after["global"] - before["global"] == 1


def test_histc_and_the_call_never_wait_for_the_device(dev):
    rng = np.random.default_rng(37)
    f = torch.from_numpy(rng.random(2 * 10 ** 6).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.integers(0, 10 ** 5, 2 * 10 ** 6)).to(dev)
    c = context_for(dev)
    vrs.histc(f, bins=100, min=0.0, max=1.0)  # warm-up: module load, the context, torch's allocations
    count(c, x, 10 ** 5)
    torch.cuda.synchronize()
    torch.cuda._sleep(int(60e-3 * 2.0e9))  # about 60 ms of work ahead of the calls
    t0 = time.perf_counter()
    a = vrs.histc(f, bins=100, min=0.0, max=1.0)
    b, _, _ = count(c, x, 10 ** 5, want_skipped=False)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert dt < 5e-3, f"the calls took {dt * 1e3:.2f} ms on the host"
    assert busy
    assert torch.equal(a.cpu(), as_out(ref_histc(f.cpu(), 0.0, 1.0, 100), torch.float32)) and torch.equal(b, torch.bincount(x, minlength=10 ** 5))


def test_two_calls_back_to_back_keep_their_results(ctx, dev):
    """different num_bins, float outputs (counters in scratch) and int64 ones (counters in out), one context: the second call's
    clearing and scratch leave the first result alone"""
    rng = np.random.default_rng(41)
    xa, xb = make("uniform", 100003, 3000, rng, "int32"), make("uniform", 50001, 70000, rng, "int32")
    da, db = torch.from_numpy(xa.astype(np.int32)).to(dev), torch.from_numpy(xb.astype(np.int32)).to(dev)
    for out_dtype in (torch.float32, torch.int64):
        first, _, tier_a = count(ctx, da, 3000, out_dtype=out_dtype)
        second, _, tier_b = count(ctx, db, 70000, out_dtype=out_dtype)
        third, _, _ = count(ctx, da, 10, out_dtype=out_dtype)
        torch.cuda.synchronize()
        assert (tier_a, tier_b) == ("lds", "global")
        assert torch.equal(first.cpu(), as_out(ref_index(xa, 3000)[0], out_dtype))
        assert torch.equal(second.cpu(), as_out(ref_index(xb, 70000)[0], out_dtype))
        assert torch.equal(third.cpu(), as_out(ref_index(xa, 10)[0], out_dtype))
    a, b = vrs.bincount(da), vrs.bincount(db)
    assert torch.equal(a, torch.bincount(da)) and torch.equal(b, torch.bincount(db))


# ---------------------------------------------------------------------------------------------- refusals and views of the call itself

def test_bin_count_refuses_undersized_buffers(ctx, dev):
    """out, scratch, values, weights and skipped each one byte short of what the shape needs (values and weights one element short
    too; a scratch that holds the skip counters but not the 32-bit counters of a float output): VRS_ERROR_INVALID_ARGUMENT with
    'too small' and the buffer's name, before anything is enqueued -- the stats and every output stay as they were"""
    n, bins = 1000, 300
    u8 = lambda t: t.view(torch.uint8)  # noqa: E731
    cases = (  # element dtype, mode, weights' dtype, out dtype
        (torch.int32, capi.VRS_BIN_INDEX, None, torch.float32),   # the counters are in the scratch
        (torch.int32, capi.VRS_BIN_INDEX, None, torch.int64),
        (torch.int64, capi.VRS_BIN_INDEX, torch.float32, torch.float32),
        (torch.uint8, capi.VRS_BIN_INDEX, torch.float64, torch.float64),
        (torch.float16, capi.VRS_BIN_LINEAR, None, torch.float16),
        (torch.float64, capi.VRS_BIN_LINEAR, None, torch.bfloat16),
    )
    for dtype, mode, wdt, odt in cases:
        w_code = capi.VRS_BIN_NO_WEIGHTS if wdt is None else _dtype_code(torch, wdt)
        o_code = _dtype_code(torch, odt)
        need = capi.query_u64("vrs_bin_count_scratch_bytes", bins, w_code, o_code)
        assert need == 256 + (0 if wdt is not None or odt == torch.int64 else (bins * 4 + 255) // 256 * 256)
        full = {"values": torch.ones(n, dtype=dtype, device=dev), "weights": None if wdt is None else torch.ones(n, dtype=wdt, device=dev),
                "out": torch.full((bins,), 77, dtype=odt, device=dev), "skipped": torch.full((2,), -5, dtype=torch.int64, device=dev),
                "scratch": torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)}

        def call(**short):
            t = {**full, **short}
            with buffers(ctx, t["values"], t["weights"], t["out"], t["skipped"], t["scratch"]) as (v, w, o, s, scr):
                return ctx.lib.vrs_bin_count(ctx.handle, v, n, _dtype_code(torch, dtype), mode, 0.0, 4.0, bins, w, w_code, o_code, o, s, scr)

        shorts = [(name, u8(t)[:-1]) for name, t in full.items() if t is not None]
        shorts += [(name, full[name][:-1]) for name in ("values", "weights", "out") if full[name] is not None]
        if need > 256:
            shorts.append(("scratch", full["scratch"][:256]))
        before = vrs.bincount_stats(ctx)
        for name, short in shorts:
            assert call(**{name: short}) == capi.VRS_ERROR_INVALID_ARGUMENT, (dtype, wdt, odt, name)
            message = ctx.lib.vrs_last_error(ctx.handle)
            assert b"too small" in message and name.encode() in message, (name, message)
        torch.cuda.synchronize()
        assert vrs.bincount_stats(ctx) == before
        assert (full["out"] == 77).all() and (full["skipped"] == -5).all() and (full["scratch"] == 0xAB).all()
        # ... and the buffers at exactly those sizes are taken: n ones, all in bin 1 (index mode) or bin 75 (1.0 of [0, 4] in 300 bins)
        assert call() == 0, ctx.lib.vrs_last_error(ctx.handle)
        want = torch.zeros(bins, dtype=torch.float64)
        want[1 if mode == capi.VRS_BIN_INDEX else 75] = n
        assert torch.equal(full["out"].cpu().double(), want) and full["skipped"].tolist() == [0, 0]


def test_histc_refuses_a_range_whose_width_overflows(dev):
    x = torch.rand(100, dtype=torch.float32, device=dev)
    with pytest.raises(vrs.VrsError, match="width"):
        vrs.histc(x, bins=4, min=-3e38, max=3e38)
    assert vrs.histc(x.double(), bins=4, min=-3e38, max=3e38).tolist() == [0.0, 0.0, 100.0, 0.0]  # (finite in float64)


@pytest.mark.parametrize("tier", ["lds", "global"])
def test_views_that_start_off_a_vector_boundary(ctx, dev, tier):
    """views 4, 8 and 12 bytes past a 16-byte boundary, which the wrappers pass on as they are: the tiles start on the boundary before
    the view and whole vectors are loaded when the weights' vectors fall on boundaries too (w[k:] with x[k:]); otherwise (weights
    that start elsewhere) element loads.  Three tiles and a tail, so first, inner and last tiles all run."""
    rng = np.random.default_rng(43)
    ctx.setTuning(KNOB, FORCE[tier])
    bins = 97
    for dtype in INDEX_DTYPES:
        size = np.dtype(dtype).itemsize
        n = 3 * (capi.BINCOUNT_TILE_BYTES // size) + 5
        base = make("mix", n + 16, bins, rng, dtype)
        xd = torch.from_numpy(base.astype(dtype)).to(dev)
        assert xd.data_ptr() % 16 == 0
        for k in sorted({b // size for b in (4, 8, 12) if b % size == 0} | ({1} if size == 8 else set())):
            checks = [(None, 0)] + [(wd, wk) for wd in (np.float32, np.float64) for wk in (k, 0, 1)]
            for wd, wk in checks:
                w = None if wd is None else ((np.arange(n + 16) % 7) - 2).astype(wd)
                wv = None if wd is None else torch.from_numpy(w).to(dev)[wk:wk + n]
                counts, skips = ref_index(base[k:k + n], bins, None if wd is None else w[wk:wk + n])
                got, skipped, planned = count(ctx, xd[k:k + n], bins, weights=wv)
                want = torch.from_numpy(counts) if wd is None else torch.from_numpy(counts.astype(wd))
                assert planned == tier and torch.equal(got.cpu(), want) and skipped == skips, (dtype, k, wd, wk)
    # the linear rule on such views, through the wrapper (float32 and float64 views go as they are; so do 16-bit ones 4 bytes off)
    for dtype, ks in (("float32", (1, 2, 3)), ("float64", (1,)), ("bfloat16", (2, 4, 6)), ("float16", (2,))):
        f = linear_values(dtype, 3 * (capi.BINCOUNT_TILE_BYTES // getattr(torch, dtype).itemsize) + 21, 0.0, 1.0, 10, rng)
        fd = f.to(dev)
        for k in ks:
            assert torch.equal(vrs.histc(fd[k:-3], bins=10, min=0.0, max=1.0).cpu(), as_out(ref_histc(f[k:-3], 0.0, 1.0, 10), f.dtype)), (dtype, k)
