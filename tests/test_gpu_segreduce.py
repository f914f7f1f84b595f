"""vrs_segment_reduce on the device against the same order on the host (vrs_segment_reduce_host), bit for bit: every dtype and op, the
lengths around every threshold mixed in one call, widths around every lane map, with and without `order` and `init`, two and three levels
forced and natural (asserted through reduce_stats), out == init, the refusal of misaligned 8-byte values; and vrs.index_add /
index_reduce / scatter_reduce / segment_reduce against torch on the CPU and numpy."""
import ctypes
import math

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi, engine
from vkradixsort_amd._torch import buffers, context_for

from .test_segreduce_cpu import (BF16, CH, F16, F32, F64, I32, I64, LENGTHS, LR, MAX, MIN, PROD, STORAGE, SUM, from_storage, host, offsets_of,
                                 to_storage)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = [I32, I64, F16, BF16, F32, F64]
WIDTHS = [1, 2, 3, 5, 16, 63, 64, 65, 129]
OPS = [SUM, PROD, MIN, MAX]
TORCH_OF = {I32: torch.int32, I64: torch.int64, F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32, F64: torch.float64}
CARRIER = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}  # raw bytes travel as integers of the element's size


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    yield c
    c.setTuning(capi.VRS_TUNE_REDUCE_CHUNK_ROWS, CH)
    c.setTuning(capi.VRS_TUNE_REDUCE_LANE_ROWS, LR)


def to_dev(raw, dev):
    if raw is None:
        return None
    raw = np.ascontiguousarray(raw)
    return torch.from_numpy(raw.view(np.uint8).reshape(-1).copy()).to(dev).view(CARRIER[raw.itemsize])


def device(c, raw, dtype, offsets, op, init=None, order=None, ch=CH, out_is_init=False, sync=False):
    """vrs_segment_reduce itself on raw storage (numpy): the out rows as numpy raw storage.  `out` and the scratch hold garbage on entry."""
    n, C = raw.shape
    d = torch.device("cuda", 0)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    S = offsets.size - 1
    need = capi.query_u64("vrs_segment_reduce_scratch_bytes", n, C, S, dtype, ch)
    val, offs, ini = to_dev(raw, d), to_dev(offsets, d), to_dev(init, d)
    ordr = to_dev(np.ascontiguousarray(order, dtype=np.uint32), d) if order is not None else None
    out = ini if out_is_init else torch.full((S * C,), 0x5B, dtype=CARRIER[raw.itemsize], device=d)
    scratch = torch.full((need,), 0xAB, dtype=torch.uint8, device=d)
    if sync:
        torch.cuda.synchronize()
    with buffers(c, val, ordr, offs, ini, out, scratch) as (v, o, f, i, r, s):
        c.check(c.lib.vrs_segment_reduce(c.handle, v, n, C, dtype, o, f, S, op, i if not out_is_init else r, r, s))
        if sync:
            c.check(c.lib.vrs_queue_wait_idle(c.handle))
    return out.cpu().numpy().view(raw.dtype).reshape(S, C)


def same_bits(got, want, dtype):
    """bit for bit, NaNs as 'both NaN'"""
    if dtype in (I32, I64):
        return np.array_equal(got, want)
    a, b = np.asarray(from_storage(got, dtype), dtype=np.float64), np.asarray(from_storage(want, dtype), dtype=np.float64)
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(got.view(np.uint8).reshape(got.shape + (-1,))[~both], want.view(np.uint8).reshape(want.shape + (-1,))[~both])


def values_for(rng, dtype, shape, op):
    if dtype in (I32, I64):
        info = np.iinfo(STORAGE[dtype])
        x = rng.integers(info.min, info.max, shape, dtype=STORAGE[dtype], endpoint=True)
        return x | 1 if op == PROD else x
    x = rng.standard_normal(shape) * (1.0 if op != PROD else 0.05) + (0.0 if op != PROD else 1.0)
    x[rng.random(shape) < 0.002] = np.nan
    x[rng.random(shape) < 0.01] = -0.0
    return to_storage(x, dtype)


def stats_delta(c, before):
    now = vrs.reduce_stats(c)
    return {k: now[k] - before[k] for k in ("lane", "rows", "columns")}


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_equals_host_bit_for_bit(ctx, dtype, C):
    rng = np.random.default_rng(1000 * dtype + C)
    lengths = rng.permutation(LENGTHS)
    offsets = offsets_of(lengths)
    n, S = int(offsets[-1]), len(lengths)
    for op in OPS:
        raw = values_for(rng, dtype, (n, C), op)
        init = values_for(rng, dtype, (S, C), op)
        order = rng.permutation(n)
        for use_order in (False, True):
            for use_init in (False, True):
                before = vrs.reduce_stats(ctx)
                got = device(ctx, raw, dtype, offsets, op, init if use_init else None, order if use_order else None)
                want = host(ctx.lib, raw, dtype, offsets, op, init if use_init else None, order if use_order else None)
                assert same_bits(got, want, dtype), (op, use_order, use_init, np.argwhere(got != want)[:5])
                used = stats_delta(ctx, before)
                # by the rule: five lengths up to 16 rows, six single chunks; 513 = 512 + 1 and then 2 partial rows, 1023 = 512 + 511 and 2,
                # 1025 = 512 + 512 + 1 and 3
                if C < 64:
                    assert used == {"lane": 5 + 2 + 1 + 2, "rows": 6 + 1 + 2 + 2, "columns": 0}, used
                else:
                    assert used == {"lane": 0, "rows": 0, "columns": 11 + 3 + 3 + 4}, used


@pytest.mark.parametrize("C", [1, 5, 64, 65])
@pytest.mark.parametrize("dtype", [I64, BF16, F32])
def test_three_levels_forced_small(dev, dtype, C):
    """CH = 64 and 4097 rows: 65 chunks, 2 chunks, 1 chunk.  On a context of its own: max_levels is a context's running maximum."""
    rng = np.random.default_rng(2000 * dtype + C)
    lengths = [3, 4097, 0, 64, 65, 4096, 200]
    offsets = offsets_of(lengths)
    n = int(offsets[-1])
    with engine.GPUContext(0) as own:
        own.setTuning(capi.VRS_TUNE_REDUCE_CHUNK_ROWS, 64)
        assert vrs.reduce_stats(own) == {"lane": 0, "rows": 0, "columns": 0, "max_levels": 0}
        raw, init, order = values_for(rng, dtype, (n, C), SUM), values_for(rng, dtype, (len(lengths), C), SUM), rng.permutation(n)
        two = device(own, raw[:4096 + 3], dtype, [0, 3, 4099], SUM, ch=64, sync=True)
        assert vrs.reduce_stats(own)["max_levels"] == 2
        assert same_bits(two, host(own.lib, raw[:4096 + 3], dtype, [0, 3, 4099], SUM, ch=64), dtype)
        for op in (SUM, MAX):
            got = device(own, raw, dtype, offsets, op, init, order, ch=64, sync=True)
            assert same_bits(got, host(own.lib, raw, dtype, offsets, op, init, order, ch=64), dtype), op
        assert vrs.reduce_stats(own)["max_levels"] == 3


def test_three_levels_natural(dev):
    """the default CH = 512 and 262145 = 512^2 + 1 rows of one float32 column"""
    rng = np.random.default_rng(3)
    n = 262145
    raw = rng.standard_normal((n + 700, 1)).astype(np.float32)
    offsets = [0, 700, 700 + n]
    with engine.GPUContext(0) as own:
        got = device(own, raw, F32, offsets, SUM, sync=True)
        # 700 = 512 + 188 rows, then 2 partial rows | n = 512 chunks and one row, then 513 partial rows = 512 + 1, then 2
        assert vrs.reduce_stats(own) == {"lane": 1 + 3, "rows": 2 + 512 + 1, "columns": 0, "max_levels": 3}
        assert same_bits(got, host(own.lib, raw, F32, offsets, SUM), F32)
        exact = math.fsum(raw[700:, 0].astype(np.float64))
        assert abs(float(got[1, 0]) - exact) <= (n + 1) * 2.0 ** -23 * float(np.abs(raw[700:, 0]).sum())


@pytest.mark.parametrize("lane_rows", [0, 64])
def test_lane_rows_knob_moves_the_maps(ctx, lane_rows):
    rng = np.random.default_rng(4 + lane_rows)
    offsets = offsets_of(LENGTHS)
    raw = values_for(rng, F32, (int(offsets[-1]), 3), SUM)
    ctx.setTuning(capi.VRS_TUNE_REDUCE_LANE_ROWS, lane_rows)
    before = vrs.reduce_stats(ctx)
    got = device(ctx, raw, F32, offsets, SUM)
    assert same_bits(got, host(ctx.lib, raw, F32, offsets, SUM, lr=lane_rows), F32)
    # 0: only the segment without rows is a lane chunk; ten single chunks, 513 -> 2 + 1, 1023 -> 2 + 1, 1025 -> 3 + 1
    # 64: the eight lengths up to 64, the chunks of one row of 513 and 1025 and the three second levels; 65, 511, 512 and the chunks of 512 / 511 rows
    assert stats_delta(ctx, before) == ({"lane": 1, "rows": 20, "columns": 0} if lane_rows == 0 else {"lane": 13, "rows": 8, "columns": 0})


def test_the_same_call_twice_gives_equal_bits(ctx):
    rng = np.random.default_rng(5)
    lengths = [5000, 0, 17, 70000, 513]
    offsets = offsets_of(lengths)
    n = int(offsets[-1])
    for C, dtype in ((1, F32), (3, F16), (64, F32), (129, F64)):
        raw = to_storage(rng.standard_normal((n if C < 64 else n // 8, C)) * 100.0, dtype)
        offs = offsets if C < 64 else offsets // 8
        order = rng.permutation(raw.shape[0])
        first = device(ctx, raw, dtype, offs, SUM, None, order)
        for _ in range(2):
            assert np.array_equal(device(ctx, raw, dtype, offs, SUM, None, order).view(np.uint8), first.view(np.uint8))
        assert same_bits(first, host(ctx.lib, raw, dtype, offs, SUM, None, order), dtype)


def test_out_may_be_init(ctx):
    rng = np.random.default_rng(6)
    offsets = offsets_of(LENGTHS)
    for C, dtype in ((2, F32), (65, I64), (64, BF16)):
        raw, init = values_for(rng, dtype, (int(offsets[-1]), C), SUM), values_for(rng, dtype, (len(LENGTHS), C), SUM)
        got = device(ctx, raw, dtype, offsets, SUM, init, out_is_init=True)
        assert same_bits(got, host(ctx.lib, raw, dtype, offsets, SUM, init), dtype)


def test_refusals_on_the_device(ctx, dev):
    S = engine.Buffer.BufferSettings
    big = torch.zeros(4096, dtype=torch.int32, device=dev)
    assert big.data_ptr() % 8 == 0
    offs = torch.tensor([0, 10], dtype=torch.int32, device=dev)
    scratch = torch.empty(capi.query_u64("vrs_segment_reduce_scratch_bytes", 10, 1, 1, F64, CH), dtype=torch.uint8, device=dev)

    def call(values_at, out_at, dtype=F64, rows=10, scratch_bytes=None, init_at=None):
        made = [engine.Buffer(ctx, S(8 * 16), device_ptr=big.data_ptr() + values_at), engine.Buffer(ctx, S(8), device_ptr=offs.data_ptr()),
                engine.Buffer(ctx, S(8), device_ptr=big.data_ptr() + out_at),
                engine.Buffer(ctx, S(scratch_bytes or scratch.numel()), device_ptr=scratch.data_ptr())]
        if init_at is not None:
            made.append(engine.Buffer(ctx, S(8), device_ptr=big.data_ptr() + init_at))
        try:
            return ctx.lib.vrs_segment_reduce(ctx.handle, made[0].handle, rows, 1, dtype, None, made[1].handle, 1, SUM,
                                              made[4].handle if init_at is not None else None, made[2].handle, made[3].handle)
        finally:
            for b in made:
                b.release()

    assert call(0, 1024) == 0
    # 8-byte values after a 4-byte offset inside a larger buffer
    assert call(4, 1024) == capi.VRS_ERROR_INVALID_ARGUMENT and b"8-byte" in ctx.lib.vrs_last_error(ctx.handle)
    assert call(0, 1028) == capi.VRS_ERROR_INVALID_ARGUMENT and b"8-byte" in ctx.lib.vrs_last_error(ctx.handle)
    assert call(0, 1024, init_at=2052) == capi.VRS_ERROR_INVALID_ARGUMENT and b"8-byte" in ctx.lib.vrs_last_error(ctx.handle)
    assert call(4, 1028, dtype=F32) == 0                                                  # (4-byte elements may sit there)
    assert call(0, 1024, rows=17) == capi.VRS_ERROR_INVALID_ARGUMENT and b"values" in ctx.lib.vrs_last_error(ctx.handle)   # undersized
    assert call(0, 1024, scratch_bytes=256) == capi.VRS_ERROR_INVALID_ARGUMENT and b"scratch" in ctx.lib.vrs_last_error(ctx.handle)
    assert call(0, 64) == capi.VRS_ERROR_INVALID_ARGUMENT and b"alias" in ctx.lib.vrs_last_error(ctx.handle)               # out inside values
    assert call(0, 1024, init_at=1024) == 0                                               # out == init
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the torch level

TORCH_DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16]


def indices(kind, n, M, rng):
    if kind == "equal":
        return np.full(n, M // 3, dtype=np.int64)
    if kind == "distinct":
        return rng.permutation(M)[:n].astype(np.int64)
    return np.minimum((rng.zipf(1.3, n) - 1), M - 1).astype(np.int64)  # Zipf-like: destination 0 takes most, the far ones stay untouched


@pytest.mark.parametrize("kind", ["equal", "distinct", "zipf"])
@pytest.mark.parametrize("dtype", TORCH_DTYPES)
def test_index_forms_equal_torch_on_the_cpu(dev, dtype, kind):
    """integer-valued inputs whose every partial sum is an integer the dtype holds (contributions in [-1, 1] times alpha = 2, input in
    [-4, 4], at most 100 rows: within 204, and bfloat16 holds every integer up to 256), products of +-1 and one input: exact in any order"""
    rng = np.random.default_rng(hash((str(dtype), kind)) % 2 ** 32)
    M, n = 150, 100
    idx = torch.from_numpy(indices(kind, n, M, rng))
    for dim, shape in ((0, (M, 3)), (1, (2, M, 3)), (-1, (70, M)), (0, (M,))):
        src_shape = tuple(n if d == dim % len(shape) else s for d, s in enumerate(shape))
        base = torch.from_numpy(rng.integers(-4, 5, shape)).to(dtype)
        src = torch.from_numpy(rng.integers(-1, 2, src_shape)).to(dtype)
        signs = torch.from_numpy(rng.choice([-1, 1], src_shape)).to(dtype)
        for alpha in (1, 2):
            got = vrs.index_add(base.to(dev), dim, idx.to(dev), src.to(dev), alpha=alpha)
            assert torch.equal(got.cpu(), base.index_add(dim, idx, src, alpha=alpha)), (dim, alpha)
        for include_self in (True, False):
            for reduce, source in (("prod", signs), ("amax", src), ("amin", src), ("mean", src)):
                got = vrs.index_reduce(base.to(dev), dim, idx.to(dev), source.to(dev), reduce, include_self=include_self)
                want = base.index_reduce(dim, idx, source, reduce, include_self=include_self)
                assert torch.equal(got.cpu(), want), (dim, reduce, include_self)
            if len(shape) == 1:
                for reduce, source in (("sum", src), ("prod", signs), ("amax", src), ("amin", src), ("mean", src)):
                    got = vrs.scatter_reduce(base.to(dev), 0, idx.to(dev), source.to(dev), reduce, include_self=include_self)
                    want = base.scatter_reduce(0, idx, source, reduce, include_self=include_self)
                    assert torch.equal(got.cpu(), want), (reduce, include_self)
    assert (torch.bincount(idx, minlength=M) == 0).any()  # some destinations untouched


def test_index_out_of_range_raises(dev):
    base, src = torch.zeros(10, 2, device=dev), torch.ones(4, 2, device=dev)
    for bad in ([0, 1, 10, 2], [0, -1, 3, 2]):
        with pytest.raises(IndexError):
            vrs.index_add(base, 0, torch.tensor(bad, device=dev), src)
        with pytest.raises(IndexError):
            vrs.scatter_reduce(base[:, 0], 0, torch.tensor(bad, device=dev), src[:, 0], "sum")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
def test_segment_reduce_equals_torch_on_the_cpu(dev, dtype):
    rng = np.random.default_rng(7)
    lengths = torch.tensor([0, 3, 0, 0, 17, 64, 1, 0, 15], dtype=torch.int64)  # 100 rows of [-1, 1]: every partial sum within 100
    n = int(lengths.sum())
    for rest in ((), (3,), (2, 35)):
        data = torch.from_numpy(rng.integers(-1, 2, (n,) + rest)).to(dtype)
        for reduce in ("sum", "mean", "max", "min", "prod"):
            x = torch.from_numpy(rng.choice([-1, 1], (n,) + rest)).to(dtype) if reduce == "prod" else data
            for initial in (None, 2):
                want = torch.segment_reduce(x, reduce, lengths=lengths, initial=initial)
                got = vrs.segment_reduce(x.to(dev), reduce, lengths=lengths.to(dev), initial=initial)
                assert got.shape == want.shape and torch.equal(got.cpu().nan_to_num(nan=-77.0), want.nan_to_num(nan=-77.0)), (rest, reduce, initial)
            offsets = torch.cat((torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)))
            got = vrs.segment_reduce(x.to(dev), reduce, offsets=offsets.to(dev))
            assert torch.equal(got.cpu().nan_to_num(nan=-77.0), torch.segment_reduce(x, reduce, offsets=offsets).nan_to_num(nan=-77.0))
    with pytest.raises(RuntimeError, match="sum to data.size"):
        vrs.segment_reduce(torch.zeros(n + 1, device=dev), "sum", lengths=lengths.to(dev))
    with pytest.raises(RuntimeError, match="negative"):
        vrs.segment_reduce(torch.zeros(n, device=dev), "sum", lengths=torch.tensor([-1, n + 1], device=dev))
    assert vrs.segment_reduce(torch.ones(n + 5, device=dev), "sum", lengths=lengths.to(dev), unsafe=True).tolist() == lengths.tolist()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_segment_reduce_of_integers_equals_numpy(dev, dtype):
    rng = np.random.default_rng(8)
    lengths = np.array([0, 3, 1025, 0, 17, 64, 1, 513])
    offsets = offsets_of(lengths).astype(np.int64)
    T = np.int32 if dtype == torch.int32 else np.int64
    info = np.iinfo(T)
    x = rng.integers(info.min, info.max, (int(offsets[-1]), 5), dtype=T, endpoint=True)
    with np.errstate(over="ignore"):
        for reduce, fn, identity in (("sum", np.add, 0), ("prod", np.multiply, 1), ("min", np.minimum, info.max), ("max", np.maximum, info.min)):
            want = np.stack([fn.reduce(x[offsets[s]:offsets[s + 1]], axis=0, dtype=T) if lengths[s] else np.full(5, identity, dtype=T) for s in range(len(lengths))])
            got = vrs.segment_reduce(torch.from_numpy(x).to(dev), reduce, lengths=torch.from_numpy(lengths).to(dev))
            assert np.array_equal(got.cpu().numpy(), want), reduce
    small = rng.integers(-50, 50, (int(offsets[-1]), 5)).astype(T)
    sums = np.stack([small[offsets[s]:offsets[s + 1]].sum(axis=0) for s in range(len(lengths))])
    got = vrs.segment_reduce(torch.from_numpy(small).to(dev), "mean", lengths=torch.from_numpy(lengths).to(dev))
    assert np.array_equal(got.cpu().numpy(), np.floor_divide(sums, np.maximum(lengths, 1)[:, None]))


def test_random_float32_index_add_is_within_the_bound_and_reproducible(dev):
    """heavy duplicates: 200000 contributions to 50 destinations.  Within (L + 2) * 2^-23 * sum|x| of the float64 sum (L contributions and
    the input: L + 1 terms, one more rounding than the bound of a sum of L terms counts), and the same bits twice."""
    rng = np.random.default_rng(9)
    M, n, C = 50, 200000, 3
    idx = torch.from_numpy(np.minimum(rng.zipf(1.5, n) - 1, M - 1).astype(np.int64))
    src, base = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)), torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32))
    exact = base.double().index_add(0, idx, src.double())
    mass = base.double().abs().index_add(0, idx, src.double().abs())
    count = torch.bincount(idx, minlength=M).double().view(M, 1)
    first = vrs.index_add(base.to(dev), 0, idx.to(dev), src.to(dev))
    assert ((first.cpu().double() - exact).abs() <= (count + 2) * 2.0 ** -23 * mass).all()
    second = vrs.index_add(base.to(dev), 0, idx.to(dev), src.to(dev))
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    a, b = (base.to(dev).index_add(0, idx.to(dev), src.to(dev)) for _ in range(2))
    print(f"torch.index_add_ twice on the same input: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {M * C} elements differ in bits")
