"""The torch.topk drop-in on the device (vkradixsort_amd.torch_topk; vrs_topk_segments with the key types VRS_TOPK_DTYPE(d)).  The reference
is always torch.sort(x.cpu(), dim, descending=largest, stable=True) sliced to k, compared bit for bit through integer views, so NaN
payloads and zero signs count; sorted=False results are compared after ordering each row by its indices.  The context of torch's
current stream runs with VRS_TUNE_TOPK_GRID_MIN_KEYS = 20000 (as tests/test_gpu_topk.py), so all three tiers are reached at small sizes."""
import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import context_for

from ._arena import Arena

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRID_THR = 20000
INTS = [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64]
FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
NARROW = [torch.int8, torch.uint8, torch.int16, torch.float16, torch.bfloat16]
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
CODES = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16, torch.int32: capi.VRS_SORT_INT32,
         torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16, torch.bfloat16: capi.VRS_SORT_BFLOAT16,
         torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
# (+NaN, -NaN with payloads, zeros, infinities, the smallest subnormal of either sign, one) as bit patterns, per float dtype
SPECIAL_BITS = {
    torch.float16: [0x7E00, 0x7E01, 0xFE00, 0xFD55, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x0001, 0x8001, 0x3C00],
    torch.bfloat16: [0x7FC0, 0x7FC1, 0xFFC0, 0xFFAA, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x3F80],
    torch.float32: [0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFAAAAAA, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
                    0x3F800000],
    torch.float64: [0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF5555555555555, 0x0000000000000000, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x8000000000000001, 0x3FF0000000000000],
}


@pytest.fixture(scope="module", autouse=True)
def ctx():
    c = context_for(DEV)
    c.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, GRID_THR)
    yield c
    c.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, capi.TOPK_GRID_MIN_KEYS_DEFAULT)


def bits(t):
    """the tensor's elements as integers of their width"""
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    """a 1-D tensor of `dtype` with these bit patterns (unsigned, of the dtype's width)"""
    width = torch.empty(0, dtype=dtype).element_size()
    a = np.array(patterns, dtype=np.uint64).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width])
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width]).copy()).view(dtype)


def make(dtype, shape, g):
    """Half of the elements random bit patterns (floats: NaNs of both signs with payloads, infinities, subnormals), half drawn from 13
    values around zero (ties; floats: -0.0 among them)."""
    n = int(np.prod(shape))
    width = torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), generator=g, dtype=torch.int64)
    wild = (raw >> 7).to(BITS[width]).view(dtype)
    small = torch.randint(-6, 7, (n,), generator=g)
    if dtype == torch.uint8:
        tame = (small + 6).to(dtype)
    elif dtype.is_floating_point:
        tame = (small.to(torch.float64) * 0.5).to(dtype)
        tame[small == 0] = tame[small == 0] * -1.0  # (half of the zeros below become -0.0)
        tame[(small == 0) & (raw % 2 == 0)] = 0.0
    else:
        tame = small.to(dtype)
    return torch.where(raw % 3 == 0, tame, wild).reshape(shape)


_refs = {}


def sort_ref(x_cpu, dim, largest):
    """torch.sort of the CPU tensor, computed once per (tensor, dim, largest)"""
    key = (id(x_cpu), dim, largest)
    if key not in _refs:
        v, i = torch.sort(x_cpu, dim=dim, descending=largest, stable=True)
        _refs[key] = (x_cpu, v, i)  # (x_cpu kept alive: its id stays its own)
    return _refs[key][1:]


def check(x_cpu, k, dim=-1, largest=True, in_order=True, x_dev=None):
    x_dev = x_cpu.to(DEV) if x_dev is None else x_dev
    got = vrs.torch_topk(x_dev, k, dim, largest, in_order)
    assert isinstance(got, torch.return_types.topk)
    gv, gi = got.values.cpu(), got.indices.cpu()
    wv, wi = sort_ref(x_cpu, dim, largest)
    wv, wi = wv.narrow(dim, 0, k), wi.narrow(dim, 0, k)
    assert gv.dtype == x_cpu.dtype and gi.dtype == torch.int64 and gv.shape == wv.shape and gi.shape == wi.shape
    if not in_order:  # the same set: both ordered by the index
        o = torch.argsort(gi, dim=dim, stable=True)
        gv, gi = torch.gather(gv, dim, o), torch.gather(gi, dim, o)
        o = torch.argsort(wi, dim=dim, stable=True)
        wv, wi = torch.gather(wv, dim, o), torch.gather(wi, dim, o)
    assert torch.equal(gi, wi), (x_cpu.dtype, tuple(x_cpu.shape), k, dim, largest, in_order)
    assert torch.equal(bits(gv), bits(wv)), (x_cpu.dtype, tuple(x_cpu.shape), k, dim, largest, in_order)


def tier_of(dtype, length):
    cap = capi.SELECT_LDS_BYTES // (8 if dtype in (torch.int64, torch.float64) else 4)
    return "lds" if length <= cap else "grid" if length >= GRID_THR else "block"


LENGTHS = [1, 63, 64, 65, 257, 4096, 4097, 8192, 8193, 16384 + 3, 33001]


@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_every_dtype_largest_sorted_and_length(dtype, ctx):
    """[7, L] at the lengths around every tier's edge for both rank widths; each tier takes exactly the rows it should"""
    g = torch.Generator().manual_seed(1)
    for length in LENGTHS:
        x = make(dtype, (7, length), g)
        xd = x.to(DEV)
        before = vrs.topk_stats(ctx)
        calls = 0
        for largest in (False, True):
            for in_order in (False, True):
                for k in {1, min(length, 37), length // 2 or 1, length}:
                    check(x, k, -1, largest, in_order, xd)
                    calls += 1
        after = vrs.topk_stats(ctx)
        want = {t: 7 * calls if t == tier_of(dtype, length) else 0 for t in ("lds", "block", "grid")}
        assert {t: after[t] - before[t] for t in want} == want, (dtype, length)
        _refs.clear()


@pytest.mark.parametrize("dtype", NARROW, ids=str)
@pytest.mark.parametrize("shape", [(5, 1001), (3, 16387), (3, 33001)], ids=str)
def test_odd_rows_of_narrow_dtypes(dtype, shape):
    """rows that begin 1, 2 and 3 bytes off a 4-byte word: the packed loads' masked heads and tails, in all three tiers"""
    g = torch.Generator().manual_seed(2)
    x = make(dtype, shape, g)
    xd = x.to(DEV)
    for largest in (False, True):
        for k in (1, 37, shape[1] - 1):
            check(x, k, -1, largest, True, xd)
    check(x, 500, -1, True, False, xd)
    _refs.clear()


def forced_rows(dtype, length, g):
    """rows whose elements agree in every digit but the lowest: every level of the selection runs"""
    if dtype == torch.int64:
        x = torch.randint(0, 8, (3, length), generator=g, dtype=torch.int64)
        x[:, length // 3] = -(1 << 62)
        return x
    if dtype == torch.float64:
        return (1.0 + torch.randint(0, 300, (3, length), generator=g).to(torch.float64) * 2.0 ** -52)
    if dtype in (torch.float16, torch.bfloat16):  # (bit patterns 0x3C00 + j, j < 32: one top-11-bit digit, the low 5 bits vary)
        return from_bits((0x3C00 + torch.randint(0, 32, (3 * length,), generator=g)).tolist(), dtype).reshape(3, length)
    return from_bits(torch.randint(0, 256, (3 * length,), generator=g).tolist(), dtype).reshape(3, length)  # int8 / uint8: all 256 values


@pytest.mark.parametrize("dtype", [torch.int64, torch.float64, torch.bfloat16, torch.float16, torch.int8, torch.uint8], ids=str)
def test_every_level_is_forced(dtype):
    g = torch.Generator().manual_seed(3)
    for length in (1000, 9001, 20003):  # (LDS, BLOCK, GRID)
        x = forced_rows(dtype, length, g)
        xd = x.to(DEV)
        for largest in (False, True):
            for k in (1, 100, length // 2):
                check(x, k, -1, largest, True, xd)
        _refs.clear()


@pytest.mark.parametrize("dtype", [torch.int8, torch.bfloat16, torch.float32, torch.int64], ids=str)
def test_constant_rows(dtype):
    """every matching key is needed at the first level already: the early stop, and ties in index order"""
    for length in (300, 9001, 20003):
        x = torch.full((2, length), 3, dtype=dtype)
        x[1, length // 2] = 2
        for largest in (False, True):
            for k in (1, length // 2, length):
                check(x, k, -1, largest, True)
        _refs.clear()


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_float_specials(dtype, largest):
    """NaNs of both signs with distinct payloads, zeros of both signs, infinities and subnormals: k cuts inside the NaN class and inside
    the zero class, a row of NaNs only, a row of zeros only -- every element comes back with its own bits"""
    g = torch.Generator().manual_seed(4)
    sp = SPECIAL_BITS[dtype]
    for length in (77, 9001, 20003):
        pick = torch.randint(0, len(sp), (length,), generator=g)
        mixed = from_bits([sp[i] for i in pick.tolist()], dtype)
        nans = from_bits([sp[i % 4] + (i % 7 if dtype != torch.float16 else i % 3) for i in range(length)], dtype)
        zeros = from_bits([sp[4 + (i * 7 // 3) % 2] for i in range(length)], dtype)
        x = torch.stack([mixed, nans, zeros])
        assert torch.isnan(x[1]).all() and (x[2] == 0).all()
        xd = x.to(DEV)
        n_nan, n_zero = int(torch.isnan(mixed).sum()), int((mixed == 0).sum())
        below_zero = int((mixed < 0).sum()) if not largest else int((mixed > 0).sum()) + n_nan
        cuts = {1, 2, n_nan // 2, below_zero + n_zero // 2, length - n_nan + n_nan // 2, length // 2, length - 1, length}
        for k in sorted(c for c in cuts if 1 <= c <= length):
            check(x, k, -1, largest, True, xd)
        check(x, length // 3, -1, largest, False, xd)
        _refs.clear()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int64], ids=str)
def test_k_around_the_lds_sort_cap(dtype):
    """k = 4096 sorts the survivors in LDS, 4097 through the segmented pair sort (of 64-bit ranks for int64)"""
    g = torch.Generator().manual_seed(5)
    x = make(dtype, (2, 9000), g)
    xd = x.to(DEV)
    for k in (1, 2, 4500, 8999, 9000, capi.TOPK_SORT_IN_LDS_MAX_K, capi.TOPK_SORT_IN_LDS_MAX_K + 1):
        for largest in (False, True):
            check(x, k, -1, largest, True, xd)
    check(x, capi.TOPK_SORT_IN_LDS_MAX_K + 1, -1, True, False, xd)
    _refs.clear()


def test_dims_strides_and_degenerate_shapes():
    g = torch.Generator().manual_seed(6)
    x = make(torch.float32, (4, 5, 301), g)
    xd = x.to(DEV)
    for dim, k in ((0, 3), (1, 5), (2, 100), (-3, 1)):
        for largest in (False, True):
            check(x, k, dim, largest, True, xd)
    t = make(torch.bfloat16, (40, 33), g)
    check(t.t(), 7, -1, True, True, t.to(DEV).t())       # a transposed view
    check(t.t(), 7, 0, False, True, t.to(DEV).t())
    check(t[:, ::2], 9, 1, True, True, t.to(DEV)[:, ::2])  # a strided view
    b = make(torch.int8, (1002,), g)
    bd = b.to(DEV)[1:]
    assert bd.data_ptr() % 4 == 1  # (off a 4-byte boundary: the copy of _torch.aligned)
    check(b[1:], 50, 0, True, True, bd)
    _refs.clear()
    for k in (0, 1):  # a 0-d tensor, as torch
        got, ref = vrs.torch_topk(torch.tensor(2.5, device=DEV), k), torch.topk(torch.tensor(2.5), k)
        assert got.values.shape == ref.values.shape == () and got.indices.shape == () and got.values.item() == 2.5 and got.indices.item() == 0
    for shape, k, dim in (((3, 7), 0, 1), ((3, 7), 0, 0), ((3, 0), 0, 1), ((0, 7), 2, 1), ((2, 0, 4), 0, 1), ((2, 0, 4), 3, 2)):
        z = torch.zeros(shape, dtype=torch.float16)
        got, ref = vrs.torch_topk(z.to(DEV), k, dim), torch.topk(z.float(), k, dim)
        assert got.values.shape == ref.values.shape and got.indices.shape == ref.indices.shape
        assert got.values.dtype == torch.float16 and got.indices.dtype == torch.int64 and got.values.device == DEV


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.int32, torch.float64], ids=str)
def test_agrees_with_torch_topk_on_rows_without_ties(dtype):
    """distinct integers (exact in every dtype here), no NaN: torch.topk on the GPU has one answer, and it is ours"""
    g = torch.Generator().manual_seed(7)
    span, length, shift = {torch.uint8: (256, 200, 0), torch.float16: (2048, 1500, 1000)}.get(dtype, (20000, 9001, 9000))
    x = (torch.stack([torch.randperm(span, generator=g)[:length] for _ in range(3)]) - shift).to(dtype).to(DEV)
    for largest in (False, True):
        for k in (1, 33, length // 2):
            got, ref = vrs.torch_topk(x, k, -1, largest, True), torch.topk(x, k, -1, largest, True)
            assert torch.equal(got.values, ref.values) and torch.equal(got.indices, ref.indices), (dtype, largest, k)


@pytest.mark.parametrize("layout", ["round", "tight"])
@pytest.mark.parametrize("dtype", [torch.int8, torch.bfloat16, torch.float32, torch.float64], ids=str)
def test_memory_contract(dtype, layout, ctx):
    """out_keys of exactly S * k * width bytes and out_indices of S * k * 4 in a guarded, poisoned arena: nothing outside them (and the
    scratch) is written, the input and the offsets are untouched; segments of all three tiers, the first shorter than k"""
    g = torch.Generator().manual_seed(8)
    width = torch.empty(0, dtype=dtype).element_size()
    lengths, lead, k = [30, 9001, GRID_THR + 3], 3, 40
    offsets = np.concatenate([[lead], lead + np.cumsum(lengths)]).astype(np.uint32)
    n, S = int(offsets[-1]) + 5, len(lengths)
    x = make(dtype, (n,), g)
    flags = capi.VRS_TOPK_LARGEST | capi.VRS_TOPK_SORTED | (capi.VRS_TOPK_RANK64 if width == 8 else 0)
    need = capi.query_u64("vrs_topk_scratch_bytes", n, S, k, flags)
    arena = Arena(DEV, 80 + width, layout, f"torch-order topk {dtype}")
    align = 8 if width == 8 else 4
    arena.place("keys", n * width, "in", align)
    arena.place("offsets", 4 * (S + 1), "in", 4)
    arena.place("out_keys", S * k * width, "out", align, [(0, S * k * width)])
    arena.place("out_indices", S * k * 4, "out", 4, [(0, S * k * 4)])
    arena.place("scratch", need, "scratch", 8)
    arena.fill()
    arena.write("keys", x)
    arena.write("offsets", offsets)
    arena.snapshot()
    h = {name: arena.buffer(ctx, name) for name in arena.ranges}
    try:
        rc = ctx.lib.vrs_topk_segments(ctx.handle, h["keys"], n, h["offsets"], S, k, capi.VRS_TOPK_DTYPE(CODES[dtype]), flags, h["out_keys"],
                                       h["out_indices"], h["scratch"])
        assert rc == capi.VRS_OK, ctx.lib.vrs_last_error(ctx.handle)
        torch.cuda.synchronize(DEV)
        arena.check()
        got_k = arena.read("out_keys", {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width]).reshape(S, k)
        got_i = arena.read("out_indices", np.uint32).reshape(S, k)
    finally:
        arena.release()
    xb = bits(x).numpy().view(got_k.dtype)
    for s in range(S):
        b, e = int(offsets[s]), int(offsets[s + 1])
        m = min(k, e - b)
        order = torch.sort(x[b:e], descending=True, stable=True).indices[:m].numpy()
        assert np.array_equal(got_i[s, :m], order) and np.array_equal(got_k[s, :m], xb[b:e][order]), (dtype, s)
        assert (got_i[s, m:] == 0xFFFFFFFF).all() and (got_k[s, m:] == np.iinfo(got_k.dtype).max).all()


def test_between_a_pending_sort_and_a_kthvalue(ctx):
    """one torch_topk between a pending one-call sort and a kthvalue on one context equals the same call alone"""
    from vkradixsort_amd._torch import buffers

    g = torch.Generator().manual_seed(9)
    x = make(torch.bfloat16, (3, 20003), g)
    xd = x.to(DEV)
    alone = vrs.torch_topk(xd, 300)
    n = 3000001
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    kd, tmp = keys.to(DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    ctx.setTuning(capi.VRS_TUNE_ASYNC_SORT, 1)
    try:
        with buffers(ctx, kd, tmp) as (k0, k1):
            ctx.check(ctx.lib.vrs_sort_keys_u32(ctx.handle, k0, k1, n))
            assert ctx.lib.vrs_sort_pending(ctx.handle) == 1
            between = vrs.torch_topk(xd, 300)  # (settles the sort first)
            assert ctx.lib.vrs_sort_pending(ctx.handle) == 0
            kth = vrs.kthvalue(xd.float(), 17)
    finally:
        ctx.setTuning(capi.VRS_TUNE_ASYNC_SORT, 0)
    assert torch.equal(between.indices, alone.indices) and torch.equal(bits(between.values), bits(alone.values))
    assert torch.equal(kd.cpu().view(torch.int32), torch.from_numpy(np.sort(keys.numpy().view(np.uint32)).view(np.int32)))
    assert torch.equal(kth.values.cpu(), torch.kthvalue(x.float(), 17).values)
    check(x, 300, -1, True, True, xd)
    _refs.clear()
