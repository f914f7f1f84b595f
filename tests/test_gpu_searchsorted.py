"""vrs.searchsorted / vrs.bucketize on the device, index for index: against torch.searchsorted on the CPU copy and on the device for
sequences without NaN, against numpy.searchsorted for sequences that end in NaNs; every tier natural and forced (asserted through
search_stats), N-D rows, sorter, promotion, streams, and two tests at the top of the size range."""
import gc
import time

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import context_for

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = ["int8", "uint8", "int16", "int32", "int64", "float16", "bfloat16", "float32", "float64"]
NARROW = ["int8", "uint8", "int16", "float16", "bfloat16"]
LDS_CAP_U32 = capi.SEARCH_LDS_BYTES_DEFAULT // 4  # ranks of a row the LDS tier takes (4-byte ranks)
DEFAULTS = {capi.VRS_TUNE_SEARCH_LDS_BYTES: capi.SEARCH_LDS_BYTES_DEFAULT,
            capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT,
            capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT}
# settings that force a tier whatever the shape (the table: narrow dtypes with one boundary row only)
FORCE = {"lds": {capi.VRS_TUNE_SEARCH_LDS_BYTES: capi.SEARCH_LDS_BYTES_MAX, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0},
         "table": {capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 1},
         "direct": {capi.VRS_TUNE_SEARCH_LDS_BYTES: 0, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 0},
         # (no LDS at all: the top level is one entry at most and the index's stride grows to cover the rest)
         "indexed": {capi.VRS_TUNE_SEARCH_LDS_BYTES: 0, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 1},
         # ... with the default room for the top level (rows beyond the LDS tier only)
         "indexed_default_top": {capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 1},
         # ... with room for 64 ranks in the top level: strides beyond 32 from 2048 index entries on (rows of up to 64 ranks: the LDS tier)
         "indexed_small_top": {capi.VRS_TUNE_SEARCH_LDS_BYTES: 256, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0,
                               capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 1}}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    yield c
    for key, value in DEFAULTS.items():
        c.setTuning(key, value)


def force(c, name):
    for key, value in DEFAULTS.items():
        c.setTuning(key, value)
    for key, value in FORCE.get(name, {}).items():
        c.setTuning(key, value)


def values(dtype, n, rng, nan=False, spread=4.0):
    """n values of the dtype with heavy ties and the dtype's special values scattered among them (NaNs of both signs: nan=True)."""
    dt = getattr(torch, dtype)
    if dt.is_floating_point:
        x = torch.from_numpy(rng.standard_normal(n) * spread).to(dt)
        ties = rng.random(n) < 0.4
        x[torch.from_numpy(ties)] = torch.round(x[torch.from_numpy(ties)])
        fi = torch.finfo(dt)
        special = [0.0, -0.0, float("inf"), float("-inf"), fi.smallest_normal / 4, -fi.smallest_normal / 4, fi.smallest_normal, fi.max, fi.min,
                   1.0, -1.0]
        if nan:
            special += [float("nan")] * 3
        pick = rng.random(n) < 0.15
        idx = torch.from_numpy(np.nonzero(pick)[0])
        x[idx] = torch.tensor(special, dtype=torch.float64).to(dt)[torch.from_numpy(rng.integers(0, len(special), idx.numel()))]
        if nan:  # NaNs with the sign bit set and another payload
            neg = idx[::2]
            isn = torch.isnan(x[neg])
            x[neg[isn]] = -x[neg[isn]]
        return x
    ii = torch.iinfo(dt)
    lo, hi = max(ii.min, -40), min(ii.max, 40)
    x = torch.from_numpy(rng.integers(lo, hi + 1, n)).to(dt)
    special = [ii.min, ii.max, 0, ii.min + 1, ii.max - 1]
    pick = torch.from_numpy(np.nonzero(rng.random(n) < 0.1)[0])
    x[pick] = torch.tensor(special, dtype=torch.int64)[torch.from_numpy(rng.integers(0, len(special), pick.numel()))].to(dt)
    return x


def sorted_seq(dtype, m, rng, spread=4.0):
    """an ascending sequence of m values without NaN (sorted on the CPU by torch)"""
    return torch.sort(values(dtype, m, rng, spread=spread), stable=True).values


def stats_delta(c, before):
    now = vrs.search_stats(c)
    return {k: now[k] - before[k] for k in now}


def check(c, seq, x, tier=None, sorter=None, device_too=True):
    """Every side and output width of vrs.searchsorted(seq, x) against torch on the CPU (and on the device); `tier`: the one that must run."""
    dev = torch.device("cuda", 0)
    seq_d, x_d = seq.to(dev), x.to(dev)
    sorter_d = sorter.to(dev) if sorter is not None else None
    for right in (False, True):
        want = torch.searchsorted(seq, x, right=right, sorter=sorter)
        want_d = torch.searchsorted(seq_d, x_d, right=right, sorter=sorter_d) if device_too else None
        for out_int32 in (False, True):
            before = vrs.search_stats(c)
            got = vrs.searchsorted(seq_d, x_d, right=right, out_int32=out_int32, sorter=sorter_d)
            assert got.dtype == (torch.int32 if out_int32 else torch.int64) and got.shape == x.shape
            assert torch.equal(got.cpu().long(), want), (seq.dtype, tuple(seq.shape), tuple(x.shape), right, out_int32, tier)
            if device_too:
                assert torch.equal(got.long(), want_d)
            if tier is not None and x.numel() and seq.numel():
                delta = stats_delta(c, before)
                assert delta[tier] == 1 and sum(delta.values()) == 1, (delta, tier)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_dtype_side_and_width_in_every_tier(ctx, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype))
    for name, m, q in (("lds", 1000, 5001), ("direct", 40001, 3000), ("indexed", 40001, 9000), ("indexed_small_top", 300007, 5000)):
        force(ctx, name)
        check(ctx, sorted_seq(dtype, m, rng), values(dtype, q, rng, nan=True), tier=name.split("_")[0])
    if dtype in NARROW:
        force(ctx, "table")
        check(ctx, sorted_seq(dtype, 40001, rng), values(dtype, 70000, rng, nan=True), tier="table")


@pytest.mark.parametrize("dtype", NARROW)
def test_views_that_start_off_a_4_byte_boundary(ctx, dev, dtype):
    """seq[1:] / x[1:] of a 1- or 2-byte dtype are contiguous but not 4-byte aligned, which vrs_buffer_wrap refuses: the drop-in raised
    'device_ptr must be 4-byte aligned' (found by tools/fuzz_ops.py)"""
    rng = np.random.default_rng(31)
    seq, x = sorted_seq(dtype, 3001, rng), values(dtype, 2001, rng, nan=True)
    seq_d, x_d = seq.to(dev), x.to(dev)
    for by in (1, 2, 3):
        for right in (False, True):
            want = torch.searchsorted(seq[by:].contiguous(), x[by:].contiguous(), right=right)
            assert torch.equal(vrs.searchsorted(seq_d[by:], x_d[by:], right=right).cpu(), want), (dtype, by, right)
            assert torch.equal(vrs.bucketize(x_d[by:], seq_d[by:], right=right).cpu(), want), (dtype, by, right)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32", "float64"])
def test_sequences_that_end_in_nans_against_numpy(ctx, dtype):
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    up = torch.float64 if dtype == "float64" else torch.float32
    for name, m, q in (("lds", 3000, 4000), ("direct", 30000, 2000), ("indexed", 30000, 2000), ("table", 30000, 2000)):
        if name == "table" and dtype not in NARROW:
            continue
        force(ctx, name)
        seq = values(dtype, m, rng, nan=True)
        seq = seq[torch.from_numpy(np.argsort(seq.to(up).numpy(), kind="stable"))]  # numpy's order: NaNs last
        assert torch.isnan(seq[-1]) and not torch.isnan(seq[0])
        x = values(dtype, q, rng, nan=True)
        for side in ("left", "right"):
            want = np.searchsorted(seq.to(up).numpy(), x.to(up).numpy(), side=side)
            got = vrs.searchsorted(seq.to(dev), x.to(dev), side=side)
            assert np.array_equal(got.cpu().numpy(), want.astype(np.int64)), (dtype, name, side)
    # the case torch answers differently
    seq = torch.tensor([1, 2, 3, float("nan"), float("nan")], dtype=getattr(torch, dtype), device=dev)
    q4 = torch.tensor([4.0, float("nan")], dtype=getattr(torch, dtype), device=dev)
    assert vrs.searchsorted(seq, q4).tolist() == [3, 3] and vrs.searchsorted(seq, q4, right=True).tolist() == [3, 5]


def test_natural_tiers_around_the_lds_capacity(ctx):
    rng = np.random.default_rng(11)
    force(ctx, "natural")
    for m, q, tier in ((LDS_CAP_U32 - 1, 3000, "lds"), (LDS_CAP_U32, 3000, "lds"), (LDS_CAP_U32 + 1, 3000, "direct"),
                       (LDS_CAP_U32 + 1, capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT, "indexed"),
                       (LDS_CAP_U32 + 1, capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT - 1, "direct")):
        check(ctx, sorted_seq("float32", m, rng, spread=300.0), values("float32", q, rng, nan=True, spread=300.0), tier=tier)
    cap64 = capi.SEARCH_LDS_BYTES_DEFAULT // 8
    for m, tier in ((cap64, "lds"), (cap64 + 1, "direct")):
        check(ctx, sorted_seq("int64", m, rng), values("int64", 2000, rng), tier=tier)
    # narrow dtypes: the table from its threshold on, the tier of the row's size below it
    tmin = capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT
    check(ctx, sorted_seq("bfloat16", 500, rng), values("bfloat16", tmin - 1, rng, nan=True), tier="lds")
    check(ctx, sorted_seq("bfloat16", 500, rng), values("bfloat16", tmin, rng, nan=True), tier="table")
    check(ctx, sorted_seq("uint8", 500, rng), values("uint8", (tmin >> 8) - 1, rng), tier="lds")
    check(ctx, sorted_seq("uint8", 500, rng), values("uint8", tmin >> 8, rng), tier="table")
    # the whole LDS of a CU
    force(ctx, "lds")
    top = capi.SEARCH_LDS_BYTES_MAX // 4
    check(ctx, sorted_seq("int32", top, rng), values("int32", 50000, rng), tier="lds")
    ctx.setTuning(capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES, 0)
    check(ctx, sorted_seq("int32", top + 1, rng), values("int32", 5000, rng), tier="direct")


@pytest.mark.parametrize("name", ["lds", "direct", "indexed", "indexed_small_top", "table"])
def test_row_lengths(ctx, name):
    """M in {0, 1, 2, 63, 64, 65, 2^k +- 1, ...}: lines, strides and top levels that do not divide M; all-equal boundaries; queries
    below and above every boundary."""
    rng = np.random.default_rng(17)
    dtype = "int16" if name == "table" else "float32"
    lengths = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 4095, 4097, 32767, 32769, 65535, 65537, 100003]
    for m in lengths:
        if name == "lds" and m > capi.SEARCH_LDS_BYTES_MAX // 4:
            continue
        tier = "lds" if name == "indexed_small_top" and m <= 64 else name.split("_")[0]
        force(ctx, name)
        seq = sorted_seq(dtype, m, rng, spread=50.0)
        x = values(dtype, 777, rng, nan=(dtype == "float32"), spread=50.0)
        check(ctx, seq, x, tier=tier if m else None, device_too=False)
        if m in (1, 65, 4097, 100003):
            same = torch.full((m,), 7, dtype=seq.dtype)
            check(ctx, same, torch.tensor([6, 7, 8], dtype=seq.dtype), tier=tier, device_too=False)
            lo, hi = seq[:1] - 1, seq[-1:] + 1
            if dtype == "float32":
                lo, hi = torch.tensor([float("-inf")]), torch.tensor([float("nan")])
            for edge, want in ((lo, 0), (hi, m)):
                got = vrs.searchsorted(seq.cuda(), edge.expand(300).contiguous().cuda(), right=(want == m))
                if not (dtype == "int16" and (seq[0] == -32768 or seq[-1] == 32767)):
                    assert torch.all(got == want), (m, want)


def test_direct_and_indexed_agree(ctx, dev):
    rng = np.random.default_rng(19)
    for dtype, m, q in (("float32", 3 * 10 ** 6 + 17, 200000), ("int64", 10 ** 6 + 5, 100000), ("float64", 777777, 70000)):
        seq = torch.sort(values(dtype, m, rng, spread=1000.0).to(dev)).values
        x = values(dtype, q, rng, nan=True, spread=1000.0).to(dev)
        outs = {}
        for name in ("direct", "indexed", "indexed_default_top", "indexed_small_top"):
            force(ctx, name)
            before = vrs.search_stats(ctx)
            outs[name] = [vrs.searchsorted(seq, x, right=r) for r in (False, True)]
            assert stats_delta(ctx, before)[name.split("_")[0]] == 2
        for k in (0, 1):
            want = torch.searchsorted(seq, x, right=bool(k))
            for name in outs:
                assert torch.equal(outs[name][k], want), (dtype, name, k)


def test_boundaries_sorted_by_the_library(ctx, dev):
    rng = np.random.default_rng(23)
    raw = values("float32", 500000, rng, nan=False, spread=100.0).to(dev)
    seq = vrs.sort(raw).values
    x = values("float32", 300000, rng, nan=True, spread=100.0).to(dev)
    force(ctx, "natural")
    before = vrs.search_stats(ctx)
    for right in (False, True):
        assert torch.equal(vrs.searchsorted(seq, x, right=right), torch.searchsorted(seq, x, right=right))
    assert stats_delta(ctx, before)["indexed"] == 2
    # each id's range after a sort
    ids = torch.randint(0, 1000, (200000,), device=dev, dtype=torch.int32)
    s = vrs.sort(ids).values
    probe = torch.arange(1000, device=dev, dtype=torch.int32)
    counts = vrs.searchsorted(s, probe, right=True) - vrs.searchsorted(s, probe)
    assert torch.equal(counts, torch.bincount(ids.long(), minlength=1000))


@pytest.mark.parametrize("name", ["natural", "lds", "direct", "indexed"])
def test_rows_of_boundaries(ctx, name):
    rng = np.random.default_rng(29)
    force(ctx, name)
    tier = None if name == "natural" else name
    # many short rows; rows whose length is no multiple of four (no vector moves); three long rows
    shapes = [(100000, 7, 5), (1000, 64, 36), (257, 301, 1001), (3, 50000, 70000), (2, 40001, 4097)]
    for b, m, q in shapes:
        if name == "lds" and m > capi.SEARCH_LDS_BYTES_MAX // 4:
            continue
        if name in ("direct", "indexed") and b == 100000:
            b = 3000
        seq = torch.sort(values("float32", b * m, rng, spread=30.0).view(b, m), dim=-1).values
        x = values("float32", b * q, rng, nan=True, spread=30.0).view(b, q)
        check(ctx, seq, x, tier=tier, device_too=(b <= 1000))
    force(ctx, "natural")
    before = vrs.search_stats(ctx)
    seq = torch.sort(values("int32", 3 * 50000, rng).view(3, 50000), dim=-1).values
    check(ctx, seq, values("int32", 3 * 70000, rng).view(3, 70000), tier="indexed")
    seq4 = torch.sort(values("int64", 2 * 3 * 100, rng).view(2, 3, 100), dim=-1).values
    check(ctx, seq4, values("int64", 2 * 3 * 50, rng).view(2, 3, 50), tier="lds")
    assert sum(stats_delta(ctx, before).values()) == 8


def test_shapes_and_empty_sides(ctx, dev):
    rng = np.random.default_rng(31)
    force(ctx, "natural")
    seq = sorted_seq("float32", 1000, rng)
    check(ctx, seq, values("float32", 2 * 3 * 50, rng).view(2, 3, 50), tier="lds")  # a 1-D sequence against a 3-D input
    check(ctx, seq, values("float32", 0, rng))                                       # Q = 0
    check(ctx, seq, values("float32", 0, rng).view(4, 0, 3))
    before = vrs.search_stats(ctx)
    for x in (values("float32", 5000, rng), values("float32", 60, rng).view(3, 20)):
        check(ctx, torch.empty(0), x)                                                 # M = 0: every output 0
    check(ctx, torch.empty(3, 0), values("float32", 60, rng).view(3, 20))
    assert sum(stats_delta(ctx, before).values()) == 0
    # a number; non-contiguous tensors; a view that is not 16-byte aligned
    s_d = seq.to(dev)
    for v in (0.5, -3, float("nan"), 10 ** 6):
        got, want = vrs.searchsorted(s_d, v), torch.searchsorted(s_d, v)
        assert got.shape == want.shape and got.dtype == want.dtype and got.item() == want.item()
    x = values("float32", 6000, rng).to(dev)
    assert torch.equal(vrs.searchsorted(s_d, x.view(60, 100).t()), torch.searchsorted(s_d, x.view(60, 100).t().contiguous()))
    assert torch.equal(vrs.searchsorted(s_d[::2], x[1::3]), torch.searchsorted(s_d[::2].contiguous(), x[1::3].contiguous()))
    assert torch.equal(vrs.searchsorted(s_d[1:], x[3:]), torch.searchsorted(s_d[1:], x[3:]))
    assert torch.equal(vrs.searchsorted(s_d, x, side="right"), torch.searchsorted(s_d, x, side="right"))
    with pytest.raises(vrs.VrsError):
        vrs.searchsorted(s_d, x, side="left", right=True)
    with pytest.raises(vrs.VrsError):
        vrs.searchsorted(s_d, x.cpu())


@pytest.mark.parametrize("name", ["lds", "direct", "indexed", "table"])
def test_sorter(ctx, name):
    rng = np.random.default_rng(37)
    dtype = "bfloat16" if name == "table" else "float32"
    force(ctx, name)
    for m, q in ((1, 50), (1000, 3000), (40001, 70000)):
        raw = values(dtype, m, rng, spread=60.0)
        sorter = torch.argsort(raw, stable=True)
        check(ctx, raw, values(dtype, q, rng, nan=True, spread=60.0), tier=name, sorter=sorter)
    if name != "table":
        raw = values("int64", 3 * 5000, rng).view(3, 5000)
        check(ctx, raw, values("int64", 3 * 4000, rng).view(3, 4000), tier=name, sorter=torch.argsort(raw, dim=-1, stable=True))


def test_unsorted_boundaries_stay_in_range(ctx, dev):
    rng = np.random.default_rng(41)
    raw = values("float32", 200001, rng, nan=True).to(dev)
    x = values("float32", 100000, rng, nan=True).to(dev)
    wild = torch.randint(-10 ** 12, 10 ** 12, (200001,), device=dev)  # a sorter with entries outside the row
    for name in ("direct", "indexed", "lds"):
        force(ctx, name)
        seq = raw if name != "lds" else raw[:30000]
        for srt in (None, wild[:seq.numel()]):
            got = vrs.searchsorted(seq, x, sorter=srt)
            assert int(got.min()) >= 0 and int(got.max()) <= seq.numel()


def test_bucketize_and_promotion(ctx, dev):
    rng = np.random.default_rng(43)
    force(ctx, "natural")
    for dtype in ("float32", "bfloat16", "int64", "uint8"):
        bnd = sorted_seq(dtype, 100, rng).to(dev)
        x = values(dtype, 100000, rng, nan=True).to(dev).view(100, 1000)
        for right in (False, True):
            for out_int32 in (False, True):
                got, want = vrs.bucketize(x, bnd, right=right, out_int32=out_int32), torch.bucketize(x, bnd, right=right, out_int32=out_int32)
                assert got.dtype == want.dtype and torch.equal(got, want)
    assert vrs.bucketize(0.25, sorted_seq("float32", 100, rng).to(dev)).shape == ()
    pairs = [("int32", "float32"), ("float32", "int64"), ("int16", "int32"), ("float16", "float32"), ("uint8", "int8"), ("int64", "float64")]
    for a, b in pairs:
        seq, x = sorted_seq(a, 3000, rng).to(dev), values(b, 5000, rng).to(dev)
        assert torch.equal(vrs.searchsorted(seq, x), torch.searchsorted(seq, x)), (a, b)
        assert torch.equal(vrs.bucketize(x, seq, right=True), torch.bucketize(x, seq, right=True)), (a, b)
    seq = sorted_seq("int32", 3000, rng).to(dev)
    for v in (2.5, -7, 10 ** 6):
        assert vrs.searchsorted(seq, v).item() == torch.searchsorted(seq, v).item()


def test_non_default_stream(dev):
    rng = np.random.default_rng(47)
    seq = sorted_seq("float32", 2 * 10 ** 6, rng).to(dev)
    x = values("float32", 10 ** 6, rng, nan=True).to(dev)
    want = torch.searchsorted(seq, x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        c = context_for(dev)
        before = vrs.search_stats(c)
        got = vrs.searchsorted(seq, x)
        small = vrs.bucketize(x, seq[::20000].contiguous())
        after = vrs.search_stats(c)
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(small, torch.bucketize(x, seq[::20000].contiguous()))
    assert c is not context_for(dev) and after["indexed"] - before["indexed"] == 1 and after["lds"] - before["lds"] == 1


def test_never_waits_for_the_device(dev):
    rng = np.random.default_rng(53)
    seq = sorted_seq("float32", 4 * 10 ** 6, rng).to(dev)
    x = values("float32", 2 * 10 ** 6, rng, nan=True).to(dev)
    bnd = seq[::4000].contiguous()
    vrs.searchsorted(seq, x)  # warm-up: module load, the context, torch's allocations
    vrs.bucketize(x, bnd)
    torch.cuda.synchronize()
    torch.cuda._sleep(int(60e-3 * 2.0e9))  # about 60 ms of work ahead of the calls
    t0 = time.perf_counter()
    a = vrs.searchsorted(seq, x)
    b = vrs.bucketize(x, bnd)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert dt < 5e-3, f"the calls took {dt * 1e3:.2f} ms on the host"
    assert busy
    assert torch.equal(a, torch.searchsorted(seq, x)) and torch.equal(b, torch.bucketize(x, bnd))


# ---------------------------------------------------------------------------------------------- the top of the size range

GB = 1 << 30
STEP = 1 << 28


def room(d, need_bytes):
    free, _ = torch.cuda.mem_get_info(d)
    if free < need_bytes + 8 * GB:
        pytest.skip(f"needs {(need_bytes + 8 * GB) / GB:.0f} GB of free HBM, {free / GB:.0f} GB free")


@pytest.fixture
def big(dev):
    yield dev
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()


def test_max_size_uint8_boundaries_direct_and_indexed(ctx, big):
    """2^32 - 1 uint8 boundaries sorted by vrs.sort_values, 10^6 queries: left = the values below, right = the values up to the query,
    from torch.bincount prefix sums; positions pass 2^31 and come out positive."""
    dev, n = big, 2 ** 32 - 1
    room(dev, 10 * n + 2 * GB)
    x = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    for a in range(0, n, STEP):
        b = min(a + STEP, n)
        i = torch.arange(a, b, dtype=torch.int64, device=dev)
        v = ((i * 2654435761) & 0xFFFFFFFF) >> 24
        v = torch.where(v < 200, v, v & 0x7F)  # uneven counts: values from 200 on fold onto 72 .. 127
        x[a:b] = v.to(torch.uint8)
        counts += torch.bincount(v, minlength=256)
        del i, v
    seq = vrs.sort_values(x)
    del x
    upto = torch.cumsum(counts, 0)
    q = torch.randint(0, 256, (10 ** 6 + 3,), device=dev, dtype=torch.uint8)
    for name in ("direct", "indexed_default_top"):
        force(ctx, name)
        before = vrs.search_stats(ctx)
        left, right = vrs.searchsorted(seq, q), vrs.searchsorted(seq, q, right=True)
        assert stats_delta(ctx, before)[name.split("_")[0]] == 2
        assert left.dtype == torch.int64
        assert torch.equal(right, upto[q.long()]), name
        assert torch.equal(left, (upto - counts)[q.long()]), name
        assert int(right.max()) == n and int(left.min()) == 0
    del seq, q


def test_more_than_2_31_queries(ctx, big):
    """2^31 + 2^20 int8 queries against a short sequence, int64 output, checked in slices against torch."""
    dev, nq = big, 2 ** 31 + 2 ** 20
    room(dev, 9 * nq + 3 * GB)
    q = torch.empty(nq, dtype=torch.int8, device=dev)
    for a in range(0, nq, STEP):
        b = min(a + STEP, nq)
        i = torch.arange(a, b, dtype=torch.int64, device=dev)
        q[a:b] = ((((i * 2654435761) & 0xFFFFFFFF) >> 24) - 128).to(torch.int8)
        del i
    seq = torch.sort(torch.randint(-128, 128, (1000,), dtype=torch.int8)).values.to(dev)
    force(ctx, "natural")
    before = vrs.search_stats(ctx)
    out = vrs.searchsorted(seq, q, right=True)
    assert stats_delta(ctx, before)["table"] == 1
    assert out.dtype == torch.int64 and out.shape == q.shape
    for a in (0, 2 ** 31 - 2 ** 16, 2 ** 31 + 2 ** 19, nq - 2 ** 22):
        b = min(a + 2 ** 22, nq)
        assert torch.equal(out[a:b], torch.searchsorted(seq, q[a:b], right=True)), a
    del out
    force(ctx, "lds")
    tail = slice(nq - 2 ** 22, nq)
    out = vrs.searchsorted(seq, q)
    assert torch.equal(out[tail], torch.searchsorted(seq, q[tail])) and torch.equal(out[:2 ** 22], torch.searchsorted(seq, q[:2 ** 22]))
    del out, q
