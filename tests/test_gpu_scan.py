"""vrs_scan_rows on the device against the same order on the host (vrs_scan_rows_host), bit for bit: every dtype and op the call takes,
lengths around every edge of the tiles and the levels, widths on both sides of a wave, one and three segments; the three-launch form
against the single pass, the single pass with no polls at all (every missing word computed by the waiting wave), two runs of one input;
and vrs.cumsum / cumprod / cummax / cummin against torch on the CPU.  T = 256 throughout, so that carries appear at small sizes."""
import math

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for

from .test_scan_cpu import ARITH, CODES, MAX, MIN, PROD, SUM, WIDENED, F, bits, host_scan, tricky

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 256
LENGTHS = [1, 2, 63, 64, 65, T - 1, T, T + 1, F * T - 1, F * T, F * T + 1]
LONGEST = F * F * T + 1  # 1 048 577: three levels
WIDTHS = [3, 64, 65]
# (dtype, out_dtype, op) of everything the call takes
KINDS = ([(d, d, op) for d in ARITH for op in (SUM, PROD)] + [(d, torch.int64, op) for d in WIDENED for op in (SUM, PROD)] +
         [(d, d, op) for d in CODES for op in (MAX, MIN)])
WORDS = [torch.int32, torch.float16, torch.bfloat16, torch.float32]  # the single pass's dtypes
OP_NAMES = {SUM: "sum", PROD: "prod", MAX: "max", MIN: "min"}


def kind_id(kind):
    d, o, op = kind
    name = str(d).replace("torch.", "")
    return f"{name}{'' if o == d else '_to_int64'}-{OP_NAMES[op]}"


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    c.setTuning(capi.VRS_TUNE_SCAN_TILE_ROWS, T)
    yield c
    c.setTuning(capi.VRS_TUNE_SCAN_TILE_ROWS, capi.SCAN_TILE_ROWS_DEFAULT)
    c.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, capi.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT)
    c.setTuning(capi.VRS_TUNE_SCAN_SPIN_BUDGET, capi.SCAN_SPIN_BUDGET_DEFAULT)


def device_scan(c, x, op, out_dtype=None):
    """vrs_scan_rows itself on the [S, L, C] CPU tensor x: (out, indices or None) back on the CPU.  out, the indices and the scratch
    hold garbage on entry."""
    S, L, C = x.shape
    out_dtype = out_dtype or x.dtype
    d = torch.device("cuda", 0)
    pairs = op in (MAX, MIN)
    tile_rows = c.tuning.get(capi.VRS_TUNE_SCAN_TILE_ROWS, capi.SCAN_TILE_ROWS_DEFAULT)
    min_rows = c.tuning.get(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, capi.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT)
    need = capi.query_u64("vrs_scan_scratch_bytes", S, L, C, CODES[x.dtype], CODES[out_dtype], op, tile_rows, min_rows)
    val = x.contiguous().to(d)
    out = torch.empty(x.shape, dtype=out_dtype, device=d)
    out.view(torch.uint8).fill_(0x5B)
    idx = torch.full(x.shape, 0x5B5B, dtype=torch.int64, device=d) if pairs else None
    scratch = torch.full((need,), 0xAB, dtype=torch.uint8, device=d)
    with buffers(c, val, out, idx, scratch) as (v, r, i, s):
        c.check(c.lib.vrs_scan_rows(c.handle, v, S, L, C, CODES[x.dtype], CODES[out_dtype], op, r, i, s))
    return out.cpu(), idx.cpu() if pairs else None


def same_bits(got, want):
    """bit for bit; for floats a NaN on both sides counts as equal (which NaN an addition of two NaNs keeps is the processor's choice)"""
    if got.dtype.is_floating_point:
        both = torch.isnan(got) & torch.isnan(want)
        return torch.equal(bits(got)[~both], bits(want)[~both])
    return torch.equal(got, want)


def full_range(dtype, shape, seed):
    info = torch.iinfo(dtype)
    return torch.from_numpy(np.random.default_rng(seed).integers(info.min, info.max, shape, dtype=np.int64, endpoint=True)).to(dtype)


def values_for(dtype, shape, op, seed):
    g = torch.Generator().manual_seed(seed)
    if op in (MAX, MIN):
        return tricky(dtype, shape, seed)
    if not dtype.is_floating_point:
        if op == PROD:
            odd = torch.randint(-2, 2, shape, generator=g) * 2 + 1  # odd factors: the product wraps, never 0
            return (odd.abs() if dtype == torch.uint8 else odd).to(dtype)
        return full_range(dtype, shape, seed)
    x = torch.randn(shape, generator=g)
    if op == PROD:
        x = 1 + 0.05 * x
    x[torch.rand(shape, generator=g) < 0.01] = -0.0
    if math.prod(shape) > 1000:
        x.view(-1)[-7] = float("nan")  # everything behind it is NaN
    return x.to(dtype)


def cases():
    """(S, L, C) of the device-equals-host grid: every length, the longest too, at C = 1 and S = 1, 3; every length but the longest at the
    other widths and S = 1, 3"""
    out = [(S, L, 1) for L in LENGTHS + [LONGEST] for S in (1, 3)]
    out += [(S, L, C) for C in WIDTHS for L in LENGTHS for S in (1, 3)]
    return out


def check_against_host(c, x, op, out_dtype=None):
    got_v, got_i = device_scan(c, x, op, out_dtype)
    want_v, want_i = host_scan(c.lib, x, op, c.tuning[capi.VRS_TUNE_SCAN_TILE_ROWS], out_dtype)
    assert torch.equal(bits(got_v), bits(want_v)) if want_i is not None else same_bits(got_v, want_v), (tuple(x.shape), (bits(got_v) != bits(want_v)).nonzero()[:5])
    if want_i is not None:
        assert torch.equal(got_i, want_i), (tuple(x.shape), (got_i != want_i).nonzero()[:5])


@pytest.mark.parametrize("kind", KINDS, ids=kind_id)
def test_device_equals_host_bit_for_bit(ctx, kind):
    dtype, out_dtype, op = kind
    ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, 4 * T)  # both forms of the flat scan meet in this grid
    before = vrs.scan_stats(ctx)
    for n, (S, L, C) in enumerate(cases()):
        check_against_host(ctx, values_for(dtype, (S, L, C), op, 7 * n + op), op, out_dtype)
    used = {k: v - before[k] for k, v in vrs.scan_stats(ctx).items()}
    assert used["tile"] > 0 and used["three_launch"] > 0
    assert (used["single_pass"] > 0) == (op in (SUM, PROD) and out_dtype in WORDS)


@pytest.mark.parametrize("op", [SUM, PROD], ids=["sum", "prod"])
@pytest.mark.parametrize("dtype", WORDS, ids=lambda d: str(d).replace("torch.", ""))
def test_three_launch_and_single_pass_agree(ctx, dtype, op):
    shapes = [(S, L) for L in (T + 1, F * T - 1, F * T, F * T + 1, 3 * F * T + 77) for S in (1, 3)]
    if dtype == torch.float32:
        shapes.append((1, LONGEST))
    for n, (S, L) in enumerate(shapes):
        x = values_for(dtype, (S, L, 1), op, 100 + n)
        results = {}
        for min_rows, tier in ((0, "three_launch"), (1, "single_pass")):
            ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, min_rows)
            before = vrs.scan_stats(ctx)
            results[tier] = device_scan(ctx, x, op)[0]
            assert vrs.scan_stats(ctx)[tier] == before[tier] + 1, (S, L, tier)
        want = host_scan(ctx.lib, x, op, T)[0]
        assert same_bits(results["three_launch"], want) and same_bits(results["single_pass"], want), (S, L)
        assert torch.equal(bits(results["three_launch"]), bits(results["single_pass"])), (S, L)  # the same processor: NaNs too


@pytest.mark.parametrize("S,L", [(1, T + 1), (3, F * T - 1), (1, F * T + 1), (3, F * T + 1), (1, LONGEST)])
def test_the_take_over_path_gives_the_same_bits(ctx, S, L):
    """no polls at all: whatever word is not there at the first look is computed by the wave that needs it"""
    ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, 1)
    ctx.setTuning(capi.VRS_TUNE_SCAN_SPIN_BUDGET, 0)
    for dtype, op in ((torch.float32, SUM), (torch.int32, SUM), (torch.bfloat16, PROD)) if L != LONGEST else ((torch.float32, SUM),):
        before = vrs.scan_stats(ctx)
        check_against_host(ctx, values_for(dtype, (S, L, 1), op, 11), op)
        after = vrs.scan_stats(ctx)
        assert after["single_pass"] == before["single_pass"] + 1 and after["takeovers"] >= before["takeovers"]
        if L == LONGEST:  # 4097 tiles start faster than their words can cross the device: some wave finds a word missing and computes it
            assert after["takeovers"] > before["takeovers"]


def test_two_runs_differ_in_no_bit(ctx, dev):
    n = 10 ** 6 + 1
    x = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev)
    other = torch.randint(0, 1 << 30, (100003,), generator=torch.Generator().manual_seed(2)).to(dev)
    for tile_rows in (T, capi.SCAN_TILE_ROWS_DEFAULT):
        ctx.setTuning(capi.VRS_TUNE_SCAN_TILE_ROWS, tile_rows)
        ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, 1)
        before = vrs.scan_stats(ctx)
        first = vrs.cumsum(x, 0)
        second = vrs.cumsum(x, 0)
        vrs.sort(other)            # an unrelated call on the same context
        vrs.cummax(other, 0)
        third = vrs.cumsum(x, 0)
        assert vrs.scan_stats(ctx)["single_pass"] == before["single_pass"] + 3
        assert torch.equal(bits(first), bits(second)) and torch.equal(bits(first), bits(third))
        want = host_scan(ctx.lib, x.cpu().view(1, n, 1), SUM, tile_rows)[0].view(-1)
        assert torch.equal(bits(first.cpu()), bits(want))


# ---------------------------------------------------------------------------------------------- the torch level

SHAPES = [(1,), (5,), (1000,), (7, 300), (300, 7), (3, 5, 70), (2, 257, 3), (4, 1, 6)]


def views_of(x):
    """x itself and non-contiguous views of the same values"""
    yield x
    if x.dim() >= 2:
        yield x.transpose(0, -1).contiguous().transpose(0, -1)  # the values of x in a transposed layout
        yield x[..., ::2]
    yield x[:1].expand(x.shape) if x.shape[0] > 1 else x


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_shape_dim_and_view(ctx, dev, shape):
    g = torch.Generator().manual_seed(len(shape) + shape[0])
    base = torch.randint(-5, 6, shape, generator=g)
    for x in views_of(base):
        for dim in range(-x.dim(), x.dim()):
            assert torch.equal(vrs.cumsum(x.to(dev), dim).cpu(), torch.cumsum(x, dim))
            assert torch.equal(vrs.cumsum(x.float().to(dev), dim).cpu(), torch.cumsum(x.float(), dim))  # small integers: every order agrees
            v, i = vrs.cummax(x.to(dev), dim)
            want = torch.cummax(x, dim)
            assert torch.equal(v.cpu(), want.values) and torch.equal(i.cpu(), want.indices)
            v, i = vrs.cummin(x.float().to(dev), dim)
            want = torch.cummin(x.float(), dim)
            assert torch.equal(v.cpu(), want.values) and torch.equal(i.cpu(), want.indices)
    small = torch.randint(1, 3, shape, generator=g)
    for dim in range(-len(shape), len(shape)):
        assert torch.equal(vrs.cumprod(small.to(dev), dim).cpu(), torch.cumprod(small, dim))  # wraps where it passes 2^63


def test_zero_dim_and_empty_tensors(ctx, dev):
    for x in (torch.tensor(3), torch.tensor(-2.5)):
        for dim in (0, -1):
            for fn in ("cumsum", "cumprod"):
                got, want = getattr(vrs, fn)(x.to(dev), dim), getattr(torch, fn)(x, dim)
                assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.cpu(), want)
            for fn in ("cummax", "cummin"):
                got, want = getattr(vrs, fn)(x.to(dev), dim), getattr(torch, fn)(x, dim)
                assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]) and got[1].dtype == torch.int64
        with pytest.raises(IndexError):
            vrs.cumsum(x.to(dev), 1)
    for shape in ((0,), (0, 4), (3, 0, 2)):
        x = torch.zeros(shape, dtype=torch.int32)
        for dim in range(-len(shape), len(shape)):
            got, want = vrs.cumsum(x.to(dev), dim), torch.cumsum(x, dim)
            assert got.shape == want.shape and got.dtype == want.dtype
            got, want = vrs.cummax(x.to(dev), dim), torch.cummax(x, dim)
            assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[1].dtype == torch.int64
    with pytest.raises(IndexError):
        vrs.cumsum(torch.zeros(3, 4, device=dev), 2)
    with pytest.raises(vrs.VrsError):
        vrs.cumsum(torch.zeros(3), 0)  # not on a GPU


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64], ids=lambda d: str(d).replace("torch.", ""))
def test_integer_sums_and_products_are_exact_and_wrap(ctx, dev, dtype):
    g = torch.Generator().manual_seed(9)
    if dtype == torch.bool:
        x = torch.rand(3, 70000, generator=g) < 0.5
    else:
        x = full_range(dtype, (3, 70000), 9)
    for dim in (0, 1):
        got, want = vrs.cumsum(x.to(dev), dim), torch.cumsum(x, dim)
        assert got.dtype == want.dtype == torch.int64 and torch.equal(got.cpu(), want)
        got, want = vrs.cumprod(x.to(dev), dim), torch.cumprod(x, dim)  # wraps within a few rows
        assert got.dtype == want.dtype and torch.equal(got.cpu(), want)
    if dtype != torch.bool:
        for target in (torch.int32, torch.int16, torch.int64, torch.float32, torch.float64):
            small = (x % 3).to(dtype)
            got, want = vrs.cumsum(small.to(dev), 1, dtype=target), torch.cumsum(small, 1, dtype=target)
            assert got.dtype == want.dtype == target and torch.equal(got.cpu(), want), target  # (partial sums below 2^24: exact in float32)
        big = torch.full((5000,), torch.iinfo(dtype).max, dtype=dtype)
        assert torch.equal(vrs.cumsum(big.to(dev), 0, dtype=dtype).cpu(), torch.cumsum(big, 0, dtype=dtype))  # wraps in the narrow type


@pytest.mark.parametrize("dtype,limit", [(torch.float32, 2 ** 24), (torch.float64, 2 ** 24), (torch.float16, 2 ** 11), (torch.bfloat16, 2 ** 8)],
                         ids=["float32", "float64", "float16", "bfloat16"])
def test_float_sums_of_representable_partial_sums_are_exact(ctx, dev, dtype, limit):
    """integer-valued data whose partial sums stay below the dtype's exact integers: every order gives the same float"""
    n = 70001
    g = torch.Generator().manual_seed(4)
    sums = torch.randint(-(limit // 2), limit // 2 + 1, (2, n), generator=g)  # the partial sums; any run of x sums to a difference of two
    x = torch.diff(sums, dim=1, prepend=torch.zeros(2, 1, dtype=torch.int64)).to(dtype)
    assert torch.equal(torch.cumsum(x.double(), 1), sums.double())
    for min_rows in (0, 1):
        ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, min_rows)
        for dim, t in ((1, x), (0, x.t().contiguous())):
            got = vrs.cumsum(t.to(dev), dim).cpu()
            assert got.dtype == dtype and torch.equal(got.double(), torch.cumsum(t.double(), dim)), (dtype, dim, min_rows)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["float16", "bfloat16", "float32"])
def test_float_sums_stay_within_the_bound(ctx, dev, dtype):
    from .test_scan_cpu import half_ulp, u32

    L, C = 50000, 3
    x = (torch.rand(L, C, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(dtype)
    for dim, t in ((0, x), (1, x.t().contiguous())):
        got = vrs.cumsum(t.to(dev), dim).cpu().double()
        depth = u32(ctx.lib.vrs_scan_depth_for, L, C if dim == 0 else 1, T)
        exact = torch.cumsum(t.double(), dim)
        bound = 1.01 * depth * 2.0 ** -24 * torch.cumsum(t.double().abs(), dim)
        if dtype != torch.float32:
            bound = bound + torch.from_numpy(half_ulp(got.numpy(), dtype))
        assert ((got - exact).abs() <= bound).all(), (dtype, dim)


@pytest.mark.parametrize("dtype", list(CODES) + [torch.bool], ids=lambda d: str(d).replace("torch.", ""))
def test_cummax_and_cummin_equal_torch(ctx, dev, dtype):
    x = tricky(dtype, (3, 20011, 2), 12) if dtype != torch.bool else torch.rand(3, 20011, 2, generator=torch.Generator().manual_seed(1)) < 0.01
    for dim in (0, 1, 2, -2):
        for fn in ("cummax", "cummin"):
            got, want = getattr(vrs, fn)(x.to(dev), dim), getattr(torch, fn)(x, dim)
            assert got[0].dtype == x.dtype and torch.equal(got[1].cpu(), want[1]), (dtype, dim, fn)
            a, b = got[0].cpu(), want[0]
            assert torch.equal(bits(a) if dtype != torch.bool else a, bits(b) if dtype != torch.bool else b), (dtype, dim, fn)
