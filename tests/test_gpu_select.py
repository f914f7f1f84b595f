"""The one-rank selection on the device (vrs_select_segments; vkradixsort_amd.kthvalue / median / nanmedian).  Oracle: torch.sort(x.cpu(),
stable=True) of every row, gathered at the entry j the header's rule names (restated here in Python): values bit for bit (viewed as the
integer of their width), indices exactly, every row compared; values also against torch.kthvalue / median / nanmedian on the CPU."""
import ctypes

import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INTS = [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64]
FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
CODES = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16, torch.int32: capi.VRS_SORT_INT32,
         torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16, torch.bfloat16: capi.VRS_SORT_BFLOAT16,
         torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
# NaNs of either sign with several payloads (quiet and signalling), as bit patterns
NANS = {torch.float16: [0x7E00, 0xFE01, 0x7C01, 0xFFFF], torch.bfloat16: [0x7FC0, 0xFFC1, 0x7F81, 0xFFFF],
        torch.float32: [0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF],
        torch.float64: [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, (1 << 64) - 1]}
KTH, MEDIAN, NANMEDIAN = capi.VRS_SELECT_KTH, capi.VRS_SELECT_MEDIAN, capi.VRS_SELECT_NANMEDIAN
GRID_THR = 8193  # VRS_TUNE_SELECT_GRID_MIN_KEYS of the grid cases: every segment beyond the LDS tier of 4-byte ranks
LENGTHS = [1, 2, 63, 64, 65, 4096, 4097, 8192, 8193, 16384, 16385, 40000]  # the LDS caps of both rank widths, a tile edge, two tiles and a tail
NONE = 0xFFFFFFFF


def bits(t):
    return t.view(BITS[t.dtype]) if t.dtype in BITS else t


def nan_values(dtype, count, g):
    pats = NANS[dtype]
    nb = torch.finfo(dtype).bits
    vals = torch.tensor([v - (1 << nb) if v >= 1 << (nb - 1) else v for v in pats], dtype=BITS[dtype])
    return vals[torch.randint(0, len(pats), (count,), generator=g)].view(dtype)


def make(dtype, shape, g):
    """Random values with many ties; a float's rows get -0.0 and +0.0 and, every other row, a few NaNs; ints get their extremes."""
    rows, length = shape
    n = rows * length
    if dtype.is_floating_point:
        x = (torch.randint(-40, 40, (n,), generator=g).to(torch.float64) / 4).to(dtype)
        x[torch.randint(0, n, (max(n // 50, 1),), generator=g)] = -0.0
        x = x.reshape(shape)
        for r in range(0, rows, 2):
            at = torch.randint(0, length, (min(length, 3),), generator=g)
            x[r, at] = nan_values(dtype, at.numel(), g)
    else:
        info = torch.iinfo(dtype)
        x = torch.randint(max(info.min, -60), min(info.max, 60), (n,), generator=g, dtype=torch.int64).to(dtype)
        x[torch.randint(0, n, (4,), generator=g)] = torch.tensor([info.min, info.max, info.min, info.max], dtype=torch.int64).to(dtype)
        x = x.reshape(shape)
    return x


def target(mode, k, length, nans, descending):
    """(j, valid): the header's rule for the entry of the stable order a mode asks for."""
    if length == 0:
        return 0, False
    if mode == KTH:
        return (k - 1, True) if 1 <= k <= length else (0, False)
    first_nan = 0 if descending else length - nans
    if mode == MEDIAN:
        return ((length - 1) // 2 if nans == 0 else first_nan), True
    if nans == length:
        return first_nan, True
    return (nans if descending else 0) + (length - nans - 1) // 2, True


class Oracle:
    """torch.sort(stable=True) of every segment of a 1-D CPU tensor, computed once per direction and gathered per (mode, k).  The values
    are gathered as bit patterns: copying a float16 element on its own quiets a signalling NaN."""

    def __init__(self, x, offsets):
        self.x, self.offsets, self.sorted = x, offsets, {}
        n = x.numel()
        self.bounds = [(min(b, n), min(max(b, e), n)) for b, e in zip(offsets[:-1], offsets[1:])]
        self.nans = [int(torch.isnan(x[b:e]).sum()) if x.dtype.is_floating_point else 0 for b, e in self.bounds]

    def answer(self, mode, k, descending):
        if descending not in self.sorted:
            self.sorted[descending] = [torch.sort(self.x[b:e], stable=True, descending=descending).indices for b, e in self.bounds]
        xb = bits(self.x)
        vals = torch.zeros(len(self.bounds), dtype=xb.dtype)
        idx = torch.full((len(self.bounds),), NONE, dtype=torch.int64)
        for i, ((b, e), nans, order) in enumerate(zip(self.bounds, self.nans, self.sorted[descending])):
            j, valid = target(mode, k, e - b, nans, descending)
            if valid:
                idx[i] = order[j]
                vals[i] = xb[b + order[j]]
        return vals, idx


class Device:
    """A 1-D tensor and its segments on the device, selected through vrs_select_segments on torch's stream's context."""

    def __init__(self, x, offsets):
        self.ctx = context_for(DEV)
        self.x = x.to(DEV)
        self.n, self.S, self.code = x.numel(), len(offsets) - 1, CODES[x.dtype]
        self.offsets = torch.tensor([o - (1 << 32) if o >= 1 << 31 else o for o in offsets], dtype=torch.int32, device=DEV)
        self.scratch = torch.empty(max(vrs.select_scratch_bytes(self.n, self.S, self.code), 8), dtype=torch.uint8, device=DEV)

    def select(self, mode, k, descending, indices=True):
        vals = torch.full((self.S + 16,), 85, dtype=torch.uint8, device=DEV).repeat_interleave(self.x.element_size()).view(self.x.dtype)
        idx = torch.full((self.S + 16,), 0x55555555, dtype=torch.int32, device=DEV)
        guard = bits(vals).clone()
        with buffers(self.ctx, self.x, self.offsets, vals, idx, self.scratch) as (src, offs, ov, oi, scr):
            flags = capi.VRS_SELECT_DESCENDING if descending else 0
            self.ctx.check(self.ctx.lib.vrs_select_segments(self.ctx.handle, src, self.n, offs, self.S, self.code, mode, k, flags, ov,
                                                            oi if indices else None, scr))
        assert torch.equal(bits(vals)[self.S:], guard[self.S:]), "out_values written past num_segments"
        assert bool((idx[self.S:] == 0x55555555).all()), "out_indices written past num_segments"
        if not indices:
            assert bool((idx == 0x55555555).all())
        return vals[:self.S].cpu(), (idx[:self.S].cpu().long() & 0xFFFFFFFF)


def check_segments(x, offsets, cases, oracle=None):
    """Every (mode, k, descending) of `cases` on the segments of x against the oracle; returns the device results."""
    oracle = oracle or Oracle(x, offsets)
    dev = Device(x, offsets)
    out = []
    for mode, k, descending in cases:
        vals, idx = dev.select(mode, k, descending)
        rv, ri = oracle.answer(mode, k, descending)
        assert torch.equal(idx, ri), (mode, k, descending, torch.nonzero(idx != ri)[:4].tolist())
        assert torch.equal(bits(vals), rv), (mode, k, descending)
        out.append((vals, idx))
    assert torch.equal(dev.x.cpu().view(torch.uint8), x.view(torch.uint8)), "src was written"
    return out


def ks_of(length):
    return sorted({k for k in (1, 2, length // 2, length - 1, length) if 1 <= k <= length})


def all_cases(length, directions=(False, True)):
    return [(KTH, k, d) for k in ks_of(length) for d in directions] + [(m, 0, d) for m in (MEDIAN, NANMEDIAN) for d in directions]


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
        counts[vrs.selection.TIER_NAMES[t.value]] += 1
    return counts


def stats_delta(ctx, before):
    now = vrs.select_stats(ctx)
    return {k: now[k] - before[k] for k in now}


# ---- the torch drop-ins: every dtype, every length at which the code takes another path, LDS / BLOCK and (tuned) GRID ----

def check_torch(x, dim=-1, keepdim=False, ks=None):
    """kthvalue, median and nanmedian of x along dim against the oracle and against torch on the CPU."""
    xc = x.cpu()
    length = xc.shape[dim] if xc.dim() else 1
    ref = torch.sort(xc, dim=dim, stable=True)
    nans = torch.isnan(xc).sum(dim=dim, keepdim=True) if xc.dtype.is_floating_point else torch.zeros_like(ref.indices.narrow(dim, 0, 1))
    kd = (lambda t: t) if keepdim or xc.dim() == 0 else (lambda t: t.squeeze(dim))

    def gather(j):  # j: per-row entries, the reduced dim kept; the values as bit patterns (a gather of float16 quiets signalling NaNs)
        idx = ref.indices.gather(dim, j)
        return kd(bits(xc).gather(dim, idx)), kd(idx)

    def compare(out, j, theirs, kind):
        assert isinstance(out, kind)
        rv, ri = gather(j)
        assert out.values.dtype == x.dtype and out.indices.dtype == torch.int64
        assert out.values.shape == rv.shape and out.indices.shape == ri.shape
        assert torch.equal(out.indices.cpu(), ri)
        assert torch.equal(bits(out.values.cpu()), rv)
        assert torch.allclose(out.values.cpu().double(), theirs.values.double(), rtol=0, atol=0, equal_nan=True)

    for k in ks if ks is not None else ks_of(length):
        compare(vrs.kthvalue(x, k, dim, keepdim), torch.full_like(nans, k - 1), torch.kthvalue(xc, k, dim, keepdim), torch.return_types.kthvalue)
    j_med = torch.where(nans == 0, torch.full_like(nans, (length - 1) // 2), length - nans)
    compare(vrs.median(x, dim, keepdim), j_med, torch.median(xc, dim, keepdim), torch.return_types.median)
    j_nan = torch.where(nans < length, (length - nans - 1) // 2, torch.zeros_like(nans))
    compare(vrs.nanmedian(x, dim, keepdim), j_nan, torch.nanmedian(xc, dim, keepdim), torch.return_types.nanmedian)


@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_every_dtype_and_length(dtype):
    g = torch.Generator().manual_seed(21)
    before = vrs.select_stats(context_for(DEV))
    for length in LENGTHS:
        check_torch(make(dtype, (2, length), g).to(DEV))
    d = stats_delta(context_for(DEV), before)
    assert d["grid"] == 0 and d["lds"] > 0 and d["block"] > 0  # (the default threshold: 2^17)


@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_every_dtype_in_the_grid_tier(dtype, tuned):
    g = torch.Generator().manual_seed(22)
    ctx = tuned(grid_min=GRID_THR)
    before = vrs.select_stats(ctx)
    for shape in [(1, 8193), (3, 20000), (2, 40000)]:
        check_torch(make(dtype, shape, g).to(DEV))
    d = stats_delta(ctx, before)
    assert d["grid"] == (len(ks_of(8193)) + 2) * 1 + (len(ks_of(20000)) + 2) * 3 + (len(ks_of(40000)) + 2) * 2 and d["lds"] == d["block"] == 0, d


def test_dims_strides_keepdim():
    g = torch.Generator().manual_seed(23)
    for dtype in (torch.float32, torch.int16, torch.float64):
        base = make(dtype, (1, 7 * 300 * 9), g).reshape(7, 300, 9).to(DEV)
        x = base.transpose(0, 2)[:, 1:, :]  # 3-D, non-contiguous: (9, 299, 7)
        assert not x.is_contiguous()
        for dim in (0, -1, 1):
            for keepdim in (False, True):
                check_torch(x, dim, keepdim, ks=[1, x.shape[dim]])


def test_int8_view_one_byte_into_its_allocation():
    g = torch.Generator().manual_seed(24)
    base = make(torch.int8, (1, 3 * 5001 + 1), g).reshape(-1).to(DEV)
    x = base[1:].view(3, 5001)
    assert x.data_ptr() % 4 == 1
    check_torch(x)
    y = make(torch.int16, (1, 2 * 9001 + 1), g).reshape(-1).to(DEV)[1:].view(2, 9001)
    assert y.data_ptr() % 4 == 2
    check_torch(y)


def test_edge_cases_as_torch():
    x0 = torch.tensor(2.5, device=DEV)
    for out in (vrs.kthvalue(x0, 1), vrs.median(x0, 0), vrs.nanmedian(x0, -1, keepdim=True)):
        assert out.values.shape == () and float(out.values) == 2.5 and int(out.indices) == 0 and out.indices.dtype == torch.int64
    assert float(vrs.median(x0)) == 2.5
    with pytest.raises(RuntimeError):
        vrs.kthvalue(x0, 2)
    with pytest.raises(IndexError):
        vrs.median(torch.zeros(3, 0, device=DEV), 1)
    with pytest.raises(IndexError):
        vrs.kthvalue(torch.zeros(3, 0, device=DEV), 1, 1)
    for fn in (vrs.median, vrs.nanmedian):
        assert torch.isnan(fn(torch.zeros(0, device=DEV))) and fn(torch.zeros(0, device=DEV)).is_cuda
        out = fn(torch.zeros(0, 3, device=DEV), 1)  # zero rows of three
        assert out.values.shape == (0,) and out.indices.shape == (0,) and out.indices.dtype == torch.int64
    out = vrs.kthvalue(torch.zeros(0, 3, device=DEV), 2, 1, keepdim=True)
    assert out.values.shape == (0, 1) and out.indices.shape == (0, 1)
    for k in (0, 4):
        with pytest.raises(RuntimeError):
            vrs.kthvalue(torch.zeros(2, 3, device=DEV), k)
    # dim=None: the flattened input is one segment; a 0-d value
    g = torch.Generator().manual_seed(25)
    for dtype in (torch.float32, torch.int64, torch.bfloat16):
        x = make(dtype, (1, 3 * 3001), g).reshape(3, 3001)
        x[x != x] = 1.0
        for fn, theirs in ((vrs.median, torch.median), (vrs.nanmedian, torch.nanmedian)):
            out = fn(x.to(DEV).t())  # (non-contiguous)
            assert out.shape == () and out.dtype == dtype
            assert torch.allclose(out.cpu().double(), theirs(x).double(), rtol=0, atol=0, equal_nan=True)  # (a zero's sign is the tie's)
    x = torch.tensor([1.0, float("nan"), -3.0], device=DEV)
    assert torch.isnan(vrs.median(x)) and float(vrs.nanmedian(x)) == -3.0


# ---- vrs_select_segments: inputs that break a select, every tier in one call, both directions, the compaction's three settings ----

def breaking_input(name, dtype, n, g):
    if name == "equal":
        return torch.full((n,), 7, dtype=dtype)
    if name == "8distinct":
        return (torch.randint(0, 8, (n,), generator=g) * 1000 - 3000).to(dtype)
    if name == "below_2^20":  # int64: the top digits are all equal, no level compacts until late
        return torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int64).to(dtype)
    if name == "randn":
        return torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    if name == "zeros":  # -0.0 and +0.0 are one key: the need-th of them in index order, whatever its sign
        x = torch.zeros(n, dtype=dtype)
        x[torch.randint(0, n, (n // 2,), generator=g)] = -0.0
        x[torch.randint(0, n, (n // 8,), generator=g)] = 1.0
        return x
    if name == "sorted":
        return torch.sort(torch.randn(n, generator=g, dtype=torch.float64).to(dtype)).values
    if name == "reversed":
        return torch.sort(torch.randn(n, generator=g, dtype=torch.float64).to(dtype), descending=True).values
    raise AssertionError(name)


BREAKING = [("equal", torch.int32), ("equal", torch.float64), ("8distinct", torch.int16), ("8distinct", torch.int64), ("below_2^20", torch.int64),
            ("randn", torch.float64), ("randn", torch.float32), ("zeros", torch.float32), ("zeros", torch.float64), ("sorted", torch.float64),
            ("reversed", torch.float32)]
# rows of the four grid shapes and short rows between them: LDS, BLOCK and GRID in one call (the threshold is GRID_THR)
MIXED = [5, 9000, 0, 8193, 1, 9000, 4096, 20000, 4097, 9000, 64, 20000, 8192, 40000, 9000, 20000, 2, 9000, 40000, 63]


def mixed_offsets():
    offsets = [0]
    for length in MIXED:
        offsets.append(offsets[-1] + length)
    return offsets


def run_three_divisors(x, offsets, cases, tuned, grid_min=GRID_THR):
    """The cases at VRS_TUNE_SELECT_COMPACT_DIVISOR 16, 2 and 0: each against the oracle (so the three are identical); returns the
    statistics' change per divisor."""
    oracle = Oracle(x, offsets)
    deltas = {}
    for divisor in (16, 2, 0):
        ctx = tuned(grid_min=grid_min, divisor=divisor)
        before = vrs.select_stats(ctx)
        check_segments(x, offsets, cases, oracle)
        deltas[divisor] = stats_delta(ctx, before)
        want = predicted_tiers(offsets, x.numel(), CODES[x.dtype], grid_min)
        for tier in ("lds", "block", "grid"):
            assert deltas[divisor][tier] == want[tier] * len(cases), (divisor, tier, deltas[divisor], want)
    assert deltas[0]["compacted"] == 0
    return deltas


@pytest.mark.parametrize("name,dtype", BREAKING, ids=lambda v: str(v))
def test_inputs_that_break_a_select(name, dtype, tuned):
    g = torch.Generator().manual_seed(31)
    offsets = mixed_offsets()
    x = breaking_input(name, dtype, offsets[-1], g)
    cases = [(KTH, 1, False), (KTH, 2, True), (KTH, 4500, False), (KTH, 8999, True), (KTH, 9000, False), (KTH, 20000, False), (KTH, 39999, True),
             (MEDIAN, 0, False), (MEDIAN, 0, True), (NANMEDIAN, 0, False), (NANMEDIAN, 0, True)]
    deltas = run_three_divisors(x, offsets, cases, tuned)
    if name == "randn" and dtype == torch.float64:
        assert deltas[16]["compacted"] > 0  # (uniform enough bits: the first level's bin is far below 1 / 16 of a row)
    if name == "equal":
        assert deltas[16]["compacted"] == deltas[2]["compacted"] == 0  # (every key stays in the chosen bin)


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_rows_with_nans(dtype, tuned):
    """Rows with 0, 1, L // 2 and L NaNs of mixed sign and payload, in every tier."""
    g = torch.Generator().manual_seed(32)
    lengths, offsets = [], [0]
    for length in (65, 4097, 8192, 9000, 20000):
        for nans in (0, 1, length // 2, length):
            lengths.append((length, nans))
            offsets.append(offsets[-1] + length)
    x = (torch.randint(-40, 40, (offsets[-1],), generator=g).to(torch.float64) / 4).to(dtype)
    for (length, nans), b in zip(lengths, offsets):
        at = b + torch.randperm(length, generator=g)[:nans]
        x[at] = nan_values(dtype, nans, g)
    cases = [(m, 0, d) for m in (MEDIAN, NANMEDIAN) for d in (False, True)] + [(KTH, 1, False), (KTH, 33, True), (KTH, 65, False), (KTH, 4097, False)]
    run_three_divisors(x, offsets, cases, tuned)
    # and through the drop-ins, where torch on the CPU agrees on the values
    for length in (65, 9000):
        rows = torch.stack([x[offsets[i]:offsets[i + 1]] for i, (l, _) in enumerate(lengths) if l == length])
        check_torch(rows.to(DEV), ks=[1, length // 2, length])


def test_every_k_class_of_every_shape_both_directions(tuned):
    """k in {1, 2, L // 2, L - 1, L} and the two medians, ascending and descending, per grid shape."""
    g = torch.Generator().manual_seed(33)
    tuned(grid_min=GRID_THR)
    for dtype, (rows, length) in [(torch.float32, (1, 8193)), (torch.int64, (3, 20000)), (torch.float64, (2, 40000)), (torch.uint8, (5, 9000))]:
        x = make(dtype, (rows, length), g).reshape(-1)
        check_segments(x, [i * length for i in range(rows + 1)], all_cases(length))


def test_malformed_offsets_without_indices_and_refusals(tuned):
    g = torch.Generator().manual_seed(34)
    ctx = tuned(grid_min=GRID_THR)
    n = 30000
    x = make(torch.float32, (1, n), g).reshape(-1)
    offsets = [0, 9000, 9000, 5, 3, n - 2, n + 10, n + 7, 0xFFFFFFFF, 0, n, 100, 20100]  # empty, backwards, beyond n, overlapping
    check_segments(x, offsets, [(KTH, 1, False), (KTH, 9001, False), (MEDIAN, 0, True), (NANMEDIAN, 0, False)])
    dev = Device(x, offsets)
    vals, _ = dev.select(MEDIAN, 0, False, indices=False)
    assert torch.equal(bits(vals), Oracle(x, offsets).answer(MEDIAN, 0, False)[0])
    # what is refused with a context at hand: NULL handles and a short scratch, before anything is launched
    lib, h = ctx.lib, ctx.handle
    short = torch.empty(vrs.select_scratch_bytes(n, dev.S, dev.code) - 256, dtype=torch.uint8, device=DEV)
    out_v, out_i = torch.zeros(dev.S, device=DEV), torch.zeros(dev.S, dtype=torch.int32, device=DEV)
    with buffers(ctx, dev.x, dev.offsets, out_v, out_i, dev.scratch, short) as (src, offs, ov, oi, scr, scr_short):
        good = [src, n, offs, dev.S, dev.code, KTH, 1, 0, ov, oi, scr]
        for at in (0, 2, 8, 10):
            args = list(good)
            args[at] = None
            assert lib.vrs_select_segments(h, *args) == capi.VRS_ERROR_INVALID_ARGUMENT
            assert b"NULL" in lib.vrs_last_error(h)
        args = list(good)
        args[10] = scr_short
        assert lib.vrs_select_segments(h, *args) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"scratch" in lib.vrs_last_error(h)
        for at, bad in ((4, 9), (5, 3), (7, 2)):
            args = list(good)
            args[at] = bad
            assert lib.vrs_select_segments(h, *args) == capi.VRS_ERROR_INVALID_ARGUMENT
        args = list(good)
        args[6] = 0
        assert lib.vrs_select_segments(h, *args) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert bool((out_v == 0).all()) and bool((out_i == 0).all())


def test_more_long_segments_than_slots_run_in_the_block_kernel(tuned):
    """Overlapping segments: more grid-tier segments than the scratch buffer has slots (n / 8193) count as grid and are still answered."""
    g = torch.Generator().manual_seed(35)
    ctx = tuned(grid_min=GRID_THR)
    n = 20000
    x = make(torch.int32, (1, n), g).reshape(-1)
    offsets = [0, 20000, 100, 9100, 0, 8193, 11000, 20000]  # seven segments, four of them beyond 8192; two slots
    before = vrs.select_stats(ctx)
    check_segments(x, offsets, [(KTH, 8000, False), (MEDIAN, 0, False)])
    assert stats_delta(ctx, before)["grid"] == 2 * predicted_tiers(offsets, n, CODES[x.dtype], GRID_THR)["grid"]


def test_non_default_stream():
    g = torch.Generator().manual_seed(36)
    x = make(torch.float32, (4, 20000), g)
    default_ctx = context_for(DEV)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        assert context_for(DEV) is not default_ctx  # (one context per stream, borrowing it)
        check_torch(x.to(DEV), ks=[1, 777, 20000])
    s.synchronize()


def test_interleaved_with_sort_and_topk_on_one_context(tuned):
    g = torch.Generator().manual_seed(37)
    tuned(grid_min=GRID_THR)
    x = make(torch.float32, (3, 20000), g)
    x[x != x] = 0.5  # (top-k orders NaNs its own way: none here)
    xd = x.to(DEV)
    big = torch.randint(-(1 << 31), 1 << 31, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)  # (a one-call sort: pending when the select comes)
    alone = (vrs.kthvalue(xd, 5000), vrs.median(xd, 1), vrs.sort(xd, 1), vrs.topk(xd, 7, largest=False), vrs.sort(big))
    mixed = []
    mixed.append(vrs.sort(big))
    mixed.append(vrs.kthvalue(xd, 5000))
    mixed.append(vrs.sort(xd, 1))
    mixed.append(vrs.median(xd, 1))
    mixed.append(vrs.topk(xd, 7, largest=False))
    mixed.append(vrs.kthvalue(xd, 5000))
    order = [4, 0, 2, 1, 3, 0]
    for got, at in zip(mixed, order):
        for a, b in zip(got, alone[at]):
            assert torch.equal(bits(a), bits(b))
    ref = torch.sort(x, dim=1, stable=True)
    assert torch.equal(mixed[1].indices.cpu(), ref.indices[:, 4999]) and torch.equal(mixed[2].indices.cpu(), ref.indices)
    assert torch.equal(mixed[4][1].cpu(), ref.indices[:, :7])
    assert torch.equal(mixed[0].values.cpu(), torch.sort(big.cpu()).values)
