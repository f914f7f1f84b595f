"""The multi-rank selection on the device (vrs_quantile_segments; vkradixsort_amd.quantile / nanquantile).  The device is held to
vrs_quantile_host bit for bit in all four outputs (tests/test_quantile_cpu.py holds that one to torch); the wrappers are held to
torch.quantile / nanquantile on the CPU: the order statistics under ==, the quantile within 4 ulp of max(|lower|, |upper|)."""
import ctypes

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for
from vkradixsort_amd.quantile import INTERPOLATIONS as INTERPOLATION_CODES

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
CODES = {torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
INTERPOLATIONS = ["linear", "lower", "higher", "midpoint", "nearest"]
QS8 = [0.0, 0.1, 0.25, 0.37, 0.5, 0.75, 0.999, 1.0]
QS16 = [i / 15 for i in range(16)]
GRID_THR = 8193  # VRS_TUNE_SELECT_GRID_MIN_KEYS of the grid cases: every segment beyond the LDS tier of 4-byte ranks
TIER_NAMES = {capi.VRS_SELECT_LDS: "lds", capi.VRS_SELECT_BLOCK: "block", capi.VRS_SELECT_GRID: "grid"}


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def host(x, offsets, qs, interpolation, ignore_nan):
    lib = capi.load_library()
    S = len(offsets) - 1
    offs = np.array(offsets, dtype=np.uint32)
    q = (ctypes.c_double * len(qs))(*qs)
    outs = [torch.full((S, len(qs)), 7.0, dtype=x.dtype) for _ in range(4)]
    rc = lib.vrs_quantile_host(x.data_ptr(), x.numel(), offs.ctypes.data, S, CODES[x.dtype], q, len(qs), INTERPOLATION_CODES[interpolation],
                               capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0, *(o.data_ptr() for o in outs))
    assert rc == capi.VRS_OK
    return outs


class Device:
    """A 1-D tensor and its segments on the device, through vrs_quantile_segments on torch's stream's context."""

    def __init__(self, x, offsets):
        self.ctx = context_for(DEV)
        self.x = x.to(DEV)
        self.n, self.S, self.code = x.numel(), len(offsets) - 1, CODES[x.dtype]
        self.offsets = torch.tensor([o - (1 << 32) if o >= 1 << 31 else o for o in offsets], dtype=torch.int32, device=DEV)
        self.scratch = torch.empty(max(vrs.quantile_scratch_bytes(self.n, self.S, self.code), 8), dtype=torch.uint8, device=DEV)

    def run(self, qs, interpolation, ignore_nan, only_values=False):
        count = self.S * len(qs)
        outs = [torch.full((count + 16,), 85, dtype=torch.uint8, device=DEV).repeat_interleave(self.x.element_size()).view(self.x.dtype) for _ in range(4)]
        guard = bits(outs[0]).clone()
        q = (ctypes.c_double * len(qs))(*qs)
        with buffers(self.ctx, self.x, self.offsets, *outs, self.scratch) as (src, offs, ov, ol, ou, ow, scr):
            extra = (None, None, None) if only_values else (ol, ou, ow)
            self.ctx.check(self.ctx.lib.vrs_quantile_segments(self.ctx.handle, src, self.n, offs, self.S, self.code, q, len(qs),
                                                              INTERPOLATION_CODES[interpolation], capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0,
                                                              ov, *extra, scr))
        for i, o in enumerate(outs):
            written = count if i == 0 or not only_values else 0
            assert torch.equal(bits(o)[written:], guard[written:]), "an output written past [num_segments, num_q]"
        return [o[:count].reshape(self.S, len(qs)).cpu() for o in outs]


def check_segments(x, offsets, cases=None):
    """Every (qs, interpolation, ignore_nan) of `cases` on the segments of the 1-D CPU tensor x: the device's four outputs against
    vrs_quantile_host, bit for bit."""
    dev = Device(x, offsets)
    cases = cases or [(QS8, "linear", False), (QS8, "linear", True), (QS16, "nearest", True), ([0.5], "midpoint", True), (QS16[:5], "higher", False),
                      (QS16, "lower", True)]
    for qs, interpolation, ignore_nan in cases:
        ours = dev.run(qs, interpolation, ignore_nan)
        theirs = host(x, offsets, qs, interpolation, ignore_nan)
        for name, a, b in zip(("values", "lower", "upper", "weight"), ours, theirs):
            same = bits(a) == bits(b)
            assert bool(same.all()), (name, interpolation, ignore_nan, qs, a[~same][:8], b[~same][:8], (~same).nonzero()[:8])
    return dev


def rows_of(x):
    rows, length = x.shape
    return x.reshape(-1), [i * length for i in range(rows + 1)]


def make(dtype, shape, g, nans=True):
    """Random values of many magnitudes with ties, -0.0 and +0.0; every other row gets a few NaNs."""
    rows, length = shape
    x = (torch.randint(-4000, 4000, shape, generator=g).to(torch.float64) / 8).to(dtype) * torch.tensor(10.0, dtype=dtype) ** torch.randint(-3, 4, shape, generator=g)
    x[:, torch.randint(0, length, (max(length // 50, 1),), generator=g)] = -0.0
    x[:, torch.randint(0, length, (max(length // 50, 1),), generator=g)] = 0.0
    if nans:
        for r in range(0, rows, 2):
            x[r, torch.randint(0, length, (min(length, 3),), generator=g)] = float("nan")
    return x


def uniform_bits(dtype, shape, g):
    """uniform bit patterns: every top bin about equally full (a level-0 sieve's best case); NaN patterns replaced"""
    x = torch.randint(-(1 << 62), 1 << 62, shape, generator=g, dtype=torch.int64)
    x = (x >> 31).to(torch.int32).view(torch.float32) if dtype == torch.float32 else (x * 2).view(torch.float64)
    return torch.where(torch.isnan(x), torch.ones_like(x), x)


@pytest.fixture
def tuned():
    """Sets tuning keys on the context of torch's current stream; restores the defaults afterwards."""
    ctx = context_for(DEV)

    def set_keys(grid_min=capi.SELECT_GRID_MIN_KEYS_DEFAULT, divisor=capi.SELECT_COMPACT_DIVISOR_DEFAULT):
        ctx.setTuning(capi.VRS_TUNE_SELECT_GRID_MIN_KEYS, grid_min)
        ctx.setTuning(capi.VRS_TUNE_SELECT_COMPACT_DIVISOR, divisor)
        return ctx

    yield set_keys
    set_keys()


def predicted_tiers(offsets, n, code, grid_min):
    lib = capi.load_library()
    counts = {"lds": 0, "block": 0, "grid": 0}
    for b, e in zip(offsets[:-1], offsets[1:]):
        t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.vrs_select_tier_for(b, e, n, code, grid_min, ctypes.byref(cb), ctypes.byref(ce), ctypes.byref(t)) == capi.VRS_OK
        counts[TIER_NAMES[t.value]] += 1
    return counts


def stats_delta(ctx, before):
    now = vrs.quantile_stats(ctx)
    return {k: now[k] - before[k] for k in now}


# ---- the tiers ----

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lds_tier(dtype):
    g = torch.Generator().manual_seed(1)
    ctx = context_for(DEV)
    for length in [1, 2, 3, 63, 64, 65, 4096, 4097] + ([8192] if dtype == torch.float32 else []):
        x, offsets = rows_of(make(dtype, (3, length), g))
        before = vrs.quantile_stats(ctx)
        check_segments(x, offsets, [(QS8, "linear", False), (QS8, "linear", True)])
        tiers = predicted_tiers(offsets, x.numel(), CODES[dtype], capi.SELECT_GRID_MIN_KEYS_DEFAULT)
        assert tiers["grid"] == 0 and (tiers["block"] == 0 or (dtype == torch.float64 and length == 4097))
        d = stats_delta(ctx, before)
        assert {k: d[k] for k in tiers} == {k: 2 * v for k, v in tiers.items()} and d["sieved"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_tier(dtype):
    g = torch.Generator().manual_seed(2)
    ctx = context_for(DEV)
    for length in (8193, 16384, 16385, 40000):
        x, offsets = rows_of(make(dtype, (2, length), g))
        before = vrs.quantile_stats(ctx)
        check_segments(x, offsets, [(QS8, "linear", True), (QS16, "nearest", False), ([0.5], "midpoint", True)])
        d = stats_delta(ctx, before)
        assert (d["lds"], d["block"], d["grid"], d["sieved"]) == (0, 6, 0, 0)


@pytest.mark.parametrize("shape", [(1, 8193), (3, 20000), (2, 40000)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grid_tier_both_sides_of_the_sieve(dtype, shape, tuned):
    """key 33 lowered so that every row takes the grid tier; the default divisor and 1, on uniform bits (sieves after the first level),
    on a constant row and on a row of two values (never sieve: their live groups hold every key, more than the area does)"""
    g = torch.Generator().manual_seed(3)
    rows, length = shape
    cases = [(QS8, "linear", True), (QS16, "lower", False), ([0.5], "midpoint", False)]
    inputs = {"uniform": uniform_bits(dtype, shape, g), "constant": torch.full(shape, 2.5, dtype=dtype),
              "two": torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(-1.0, dtype=dtype), torch.tensor(3.0, dtype=dtype)),
              "mixed": make(dtype, shape, g)}
    for divisor in (capi.SELECT_COMPACT_DIVISOR_DEFAULT, 1):
        ctx = tuned(grid_min=GRID_THR, divisor=divisor)
        for name, rows_t in inputs.items():
            x, offsets = rows_of(rows_t)
            before = vrs.quantile_stats(ctx)
            check_segments(x, offsets, cases)
            d = stats_delta(ctx, before)
            assert (d["lds"], d["block"], d["grid"]) == (0, 0, rows * len(cases)), (name, d)
            if name == "uniform":  # live groups: at most 16 of 2048 about equal bins -- below len / 16 and within the area
                assert d["sieved"] == rows * len(cases), (name, divisor, d)
            elif name in ("constant", "two"):
                assert d["sieved"] == 0, (name, divisor, d)
    ctx = tuned(grid_min=GRID_THR, divisor=0)  # never
    x, offsets = rows_of(inputs["uniform"])
    before = vrs.quantile_stats(ctx)
    check_segments(x, offsets, cases)
    assert stats_delta(ctx, before)["sieved"] == 0


@pytest.mark.parametrize("shape", [(1, 8193), (3, 20000), (2, 40000)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grid_tier_sieves_after_the_second_level(dtype, shape, tuned):
    """One crowded top bin: every key is 1.0's bits plus uniform low bits, so level 0 leaves one group that holds the whole row -- more
    than the slot's area (1024 ranks per 16384 keys), at either divisor -- and the slot stays in state 0.  Level 1 spreads the row over
    256 (float32) or 128 (float64: one exponent bit is fixed) about equal bins; at most 4 targets leave at most 4 groups, about L / 32,
    below L / 16 and within the area, with two levels still to come: every slot sieves then, read from state 0 after level 1."""
    g = torch.Generator().manual_seed(4)
    rows, length = shape
    one = torch.ones(1, dtype=dtype).view(BITS[dtype]).item()
    low = torch.randint(0, 1 << (21 if dtype == torch.float32 else 52), shape, generator=g, dtype=torch.int64)
    x, offsets = rows_of((one + low).to(BITS[dtype]).view(dtype))
    cases = [([0.5], "midpoint", False), ([0.25, 0.75], "lower", True), ([0.1, 0.9], "linear", False)]
    for divisor in (capi.SELECT_COMPACT_DIVISOR_DEFAULT, 1):
        ctx = tuned(grid_min=GRID_THR, divisor=divisor)
        before = vrs.quantile_stats(ctx)
        check_segments(x, offsets, cases)
        d = stats_delta(ctx, before)
        assert (d["lds"], d["block"], d["grid"], d["sieved"]) == (0, 0, rows * len(cases), rows * len(cases)), (divisor, d)


# ---- inputs that break a multi-target select ----

def breaking_rows(dtype, length):
    """rows of `length` keys, named"""
    info = torch.finfo(dtype)
    ib = BITS[dtype]
    one = torch.ones(1, dtype=dtype).view(ib).item()  # the bits of 1.0
    idx = torch.arange(length)
    rows = {}
    rows["all equal"] = torch.full((length,), -7.25, dtype=dtype)
    rows["two values split at the median"] = torch.where(idx % 2 == 0, 1.0, 2.0).to(dtype)
    rows["lowest bit only"] = (one + (idx % 2)).to(ib).view(dtype)  # one bin down to the last level
    rows["lowest byte only"] = (one + (idx * 7 % 256)).to(ib).view(dtype)
    # 16 targets in 16 different top bins: powers of 16 -- every exponent step of 4 is another top-11-bit prefix
    rows["16 top bins"] = (torch.tensor(16.0, dtype=torch.float64) ** ((idx % 16).double() - 8)).to(dtype) * torch.where(idx % 32 < 16, 1.0, -1.0).to(dtype)
    rows["one top bin"] = (one + (idx * 2654435761 % (1 << 20))).to(ib).view(dtype)  # 16 targets in one bin of level 0
    rows["nans"] = torch.full((length,), float("nan"), dtype=dtype)
    r = torch.full((length,), float("nan"), dtype=dtype)
    r[length // 3] = 4.5
    rows["one among nans"] = r
    r = torch.where(idx % 3 == 0, 0.0, -0.0).to(dtype)
    r[: length // 4] = -1.0
    r[length // 4: length // 2 - 1] = 1.0
    rows["zeros around the median"] = r
    r = torch.linspace(-1, 1, length, dtype=torch.float64).to(dtype)
    r[::5] = float("inf")
    r[1::5] = float("-inf")
    rows["infinities"] = r
    rows["subnormals"] = ((idx * 977 % 4001).to(ib) - 2000).to(dtype) * info.smallest_normal / 64
    return rows


@pytest.mark.parametrize("length,grid", [(1000, False), (20000, False), (20000, True)], ids=["lds", "block", "grid"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_inputs_that_break_a_multi_target_select(dtype, length, grid, tuned):
    tuned(grid_min=GRID_THR if grid else capi.SELECT_GRID_MIN_KEYS_DEFAULT)
    rows = breaking_rows(dtype, length)
    x = torch.stack(list(rows.values()))
    flat, offsets = rows_of(x)
    cases = [([0.0, 1.0], "linear", False), ([0.0, 1.0], "lower", True), (QS16, "nearest", True), (QS16, "higher", False), (QS8, "linear", True),
             (QS8, "midpoint", False), ([0.5], "linear", True), ([0.5], "linear", False)]
    check_segments(flat, offsets, cases)
    # what the rows are there for, spelt out through the wrapper
    on = x.to(DEV)
    out = vrs.nanquantile(on, 0.5, dim=1).cpu()
    names = list(rows)
    assert out[names.index("all equal")] == -7.25 and out[names.index("two values split at the median")] == 1.5
    assert torch.isnan(out[names.index("nans")]) and out[names.index("one among nans")] == 4.5
    z = vrs.quantile(on[names.index("zeros around the median")], 0.5, interpolation="lower").cpu()
    assert bits(z.reshape(1))[0] == 0  # +0.0 whatever the zero's sign
    ends = vrs.quantile(on[names.index("infinities")], torch.tensor([0.0, 1.0], dtype=dtype, device=DEV), interpolation="lower").cpu()
    assert ends[0] == float("-inf") and ends[1] == float("inf")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ragged_empty_and_clamped_segments(dtype, tuned):
    g = torch.Generator().manual_seed(5)
    n = 70000
    x = make(dtype, (1, n), g).reshape(-1)
    # begins at any element; empty; end before begin; overlapping; past the end (clamped)
    offsets = [0, 1, 1, 4, 3, 4100, 4101, 13000, 9000, 30001, 69999, 70000, 1 << 31, 5, (1 << 32) - 1]
    for grid_min in (capi.SELECT_GRID_MIN_KEYS_DEFAULT, GRID_THR):
        ctx = tuned(grid_min=grid_min)
        before = vrs.quantile_stats(ctx)
        check_segments(x, offsets, [(QS8, "linear", True), (QS16, "nearest", False)])
        tiers = predicted_tiers(offsets, n, CODES[dtype], grid_min)
        d = stats_delta(ctx, before)
        assert {k: d[k] for k in tiers} == {k: 2 * v for k, v in tiers.items()}


def test_more_long_segments_than_slots(tuned):
    """overlapping long ranges: more grid-tier segments than the scratch buffer has slots (n / 8193); the rest count as grid and run in the
    BLOCK kernel"""
    g = torch.Generator().manual_seed(6)
    n = 3 * 8193 + 100
    x = make(torch.float32, (1, n), g).reshape(-1)
    offsets = [0, n, 5, n - 7, 100, 9000, 0, 8500, 1, n]  # segments (0,n) (n,5)=empty (5,n-7) (n-7,100)=empty (100,9000) (9000,0)=empty ...
    ctx = tuned(grid_min=GRID_THR)
    tiers = predicted_tiers(offsets, n, capi.VRS_SORT_FLOAT32, GRID_THR)
    assert tiers["grid"] > n // 8193
    before = vrs.quantile_stats(ctx)
    check_segments(x, offsets, [(QS8, "linear", True), (QS16, "lower", False)])
    assert stats_delta(ctx, before)["grid"] == 2 * tiers["grid"]


def test_only_values_and_nothing_to_do():
    g = torch.Generator().manual_seed(7)
    x, offsets = rows_of(make(torch.float32, (4, 300), g))
    dev = Device(x, offsets)
    v = dev.run(QS8, "linear", True, only_values=True)[0]
    assert torch.equal(bits(v), bits(host(x, offsets, QS8, "linear", True)[0]))
    ctx, q = dev.ctx, (ctypes.c_double * 1)(0.5)
    with buffers(ctx, dev.x, dev.offsets, dev.scratch) as (src, offs, scr):
        assert ctx.lib.vrs_quantile_segments(ctx.handle, src, dev.n, offs, 0, dev.code, q, 1, 0, 0, None, None, None, None, None) == capi.VRS_OK
        assert ctx.lib.vrs_quantile_segments(ctx.handle, src, dev.n, offs, 4, dev.code, q, 0, 0, 0, None, None, None, None, None) == capi.VRS_OK
        assert ctx.lib.vrs_quantile_segments(ctx.handle, src, dev.n, offs, 4, dev.code, q, 1, 0, 0, None, None, None, None, scr) == capi.VRS_ERROR_INVALID_ARGUMENT


# ---- the wrappers against torch on the CPU ----

def check_torch(x, q, dim=None, keepdim=False, interpolation="linear"):
    """quantile and nanquantile of the device tensor x against torch on the CPU: the single-entry modes under ==, linear and midpoint
    within 4 ulp of max(|lower|, |upper|) (two evaluations of one three-operation interpolation, each at most 2 ulp from the real value)"""
    xc = x.cpu()
    qc = q.cpu() if isinstance(q, torch.Tensor) else q
    eps = torch.finfo(x.dtype).eps
    for name in ("quantile", "nanquantile"):
        ours = getattr(vrs, name)(x, q, dim, keepdim, interpolation=interpolation)
        theirs = getattr(torch, name)(xc, qc, dim, keepdim, interpolation=interpolation)
        assert ours.shape == theirs.shape and ours.dtype == theirs.dtype and ours.device == x.device
        ours = ours.cpu()
        assert torch.equal(torch.isnan(ours), torch.isnan(theirs)), (name, interpolation)
        lo = getattr(torch, name)(xc, qc, dim, keepdim, interpolation="lower")
        hi = getattr(torch, name)(xc, qc, dim, keepdim, interpolation="higher")
        if interpolation in ("lower", "higher", "nearest"):
            assert bool(((ours == theirs) | torch.isnan(theirs)).all()), (name, interpolation)
        else:
            ok = torch.isnan(theirs) | ((ours - theirs).abs() <= 4 * eps * torch.maximum(lo.abs(), hi.abs()))
            assert bool(ok.all()), (name, interpolation, ours[~ok], theirs[~ok])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wrapper_q_counts_and_the_sort_path(dtype):
    """Q = 1, 8 and 9: nine q with "linear" are 18 targets, the sort path; its results equal the select path's on the same input"""
    g = torch.Generator().manual_seed(8)
    x = make(dtype, (5, 3000), g).to(DEV)
    q9 = torch.tensor([0.0, 0.01, 0.2, 0.25, 0.5, 0.62, 0.9, 0.999, 1.0], dtype=dtype, device=DEV)
    for interpolation in INTERPOLATIONS:
        check_torch(x, 0.3, 1, interpolation=interpolation)
        check_torch(x, q9[:8], 1, interpolation=interpolation)
        check_torch(x, q9, 1, interpolation=interpolation)
    ctx = context_for(DEV)
    for name in ("quantile", "nanquantile"):
        for interpolation in ("linear", "midpoint"):
            before = vrs.quantile_stats(ctx)
            by_sort = getattr(vrs, name)(x, q9, 1, interpolation=interpolation)
            assert stats_delta(ctx, before) == {"lds": 0, "block": 0, "grid": 0, "sieved": 0}  # (no selection ran)
            by_select = torch.cat([getattr(vrs, name)(x, q9[:5], 1, interpolation=interpolation), getattr(vrs, name)(x, q9[5:], 1, interpolation=interpolation)])
            assert stats_delta(ctx, before)["lds"] == 10
            assert torch.equal(bits(by_sort.cpu()), bits(by_select.cpu())), (name, interpolation)
    q17 = torch.linspace(0, 1, 17, dtype=dtype, device=DEV)
    by_sort = vrs.nanquantile(x, q17, 1, interpolation="nearest")
    by_select = torch.cat([vrs.nanquantile(x, q17[:16], 1, interpolation="nearest"), vrs.nanquantile(x, q17[16:], 1, interpolation="nearest")])
    assert torch.equal(bits(by_sort.cpu()), bits(by_select.cpu()))


def test_wrapper_dims_strides_keepdim():
    g = torch.Generator().manual_seed(9)
    x = make(torch.float32, (6, 7 * 5 * 4), g, nans=False).reshape(6, 7, 5, 4).to(DEV)
    x[1, 2, 3, 1] = float("nan")
    q = torch.tensor([0.2, 0.5, 0.81], device=DEV)
    for dim in (0, 1, 2, 3, -1, -3):
        for keepdim in (False, True):
            check_torch(x, q, dim, keepdim)
            check_torch(x, 0.4, dim, keepdim, interpolation="nearest")
    check_torch(x.permute(2, 0, 3, 1), q, 1, True)           # permuted
    check_torch(x[::2, 1:, :, ::3], q, 2)                    # strided slices
    check_torch(x[:, :, 0, :].double(), q.double(), 1)       # float64
    check_torch(x, q, None, False)                           # dim=None: all elements
    check_torch(x, q, None, True)
    check_torch(x, 0.5, None, True, interpolation="midpoint")
    check_torch(x, torch.tensor(0.5, device=DEV), 1)         # a 0-d tensor q: the reduced shape
    check_torch(torch.tensor(3.5, device=DEV), 0.5)          # a 0-d input is its own quantile
    check_torch(torch.tensor(3.5, device=DEV), q)
    check_torch(torch.tensor(3.5, device=DEV), 0.5, 0, True)
    check_torch(torch.tensor(float("nan"), device=DEV), 0.5, 0)
    assert vrs.quantile(x, torch.empty(0, device=DEV), 1).shape == torch.quantile(x.cpu(), torch.empty(0), 1).shape
    with pytest.raises(RuntimeError, match="must be non-empty"):
        vrs.quantile(torch.empty(0, device=DEV), 0.5)
    with pytest.raises(RuntimeError, match="either float or double"):
        vrs.quantile(x.half(), 0.5)
    with pytest.raises(RuntimeError, match=r"range \[0, 1\]"):
        vrs.nanquantile(x, torch.tensor([0.5, 1.5], device=DEV))


def test_wrapper_long_rows_take_the_streaming_tiers():
    g = torch.Generator().manual_seed(10)
    x = make(torch.float32, (2, 140000), g).to(DEV)  # GRID at the default threshold
    ctx = context_for(DEV)
    before = vrs.quantile_stats(ctx)
    check_torch(x, torch.tensor([0.01, 0.5, 0.99], device=DEV), 1)
    assert stats_delta(ctx, before)["grid"] == 4
    check_torch(x[:, :30000].double(), torch.tensor([0.01, 0.5, 0.99], device=DEV, dtype=torch.float64), 1, interpolation="higher")


def test_non_default_stream_and_interleaved_with_kthvalue_and_sort():
    g = torch.Generator().manual_seed(11)
    x = make(torch.float32, (4, 20000), g, nans=False).to(DEV)
    q = torch.tensor([0.1, 0.5, 0.9], device=DEV)
    ref = torch.quantile(x.cpu(), q.cpu(), 1, interpolation="lower")
    a = vrs.quantile(x, q, 1, interpolation="lower")
    k = vrs.kthvalue(x, 10000, 1)
    s = vrs.sort(x, 1)
    b = vrs.quantile(x, q, 1, interpolation="higher")
    assert torch.equal(a.cpu(), ref) and torch.equal(b.cpu(), torch.quantile(x.cpu(), q.cpu(), 1, interpolation="higher"))
    assert torch.equal(k.values.cpu(), torch.kthvalue(x.cpu(), 10000, 1).values) and torch.equal(s.values.cpu(), torch.sort(x.cpu(), 1).values)
    assert torch.equal(vrs.quantile(x, q, 1, interpolation="lower").cpu(), ref)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        y = x * 2
        c = vrs.quantile(y, q, 1, interpolation="lower")
        d = vrs.kthvalue(y, 3, 1).values
    stream.synchronize()
    assert torch.equal(c.cpu(), ref * 2) and torch.equal(d.cpu(), torch.kthvalue(x.cpu() * 2, 3, 1).values)
