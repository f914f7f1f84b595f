"""The torch.mode drop-in on the device (vkradixsort_amd.mode over vrs_sort_rank_keys, the bare-key sorts and vrs_sort_restore with
VRS_SORT_MODE).

The reference is numpy on the host, row by row: every element becomes a key (-0.0 canonicalised to +0.0, every NaN one key above
+inf), the smallest key of maximal count is the mode, its last occurrence the index, the input's own bits there the value.  It is
compared exactly: values viewed as integers, indices index for index.  NaN-free cases are also compared with torch.mode(x.cpu()):
values ==, and x.gather(dim, indices) == values (torch's index is unspecified).  Every case says which of the two it is.

T = 4096 is the kernels' tile (kModeTile): the boundary cases are built from it."""
import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi, engine
from vkradixsort_amd._torch import buffers, context_for, row_offsets

from .test_gpu_memory_contract import RANK_DTYPES, Case, Spec, as_bytes, rank_of, run_case, run_refusals, wrap_align

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 4096
BAD = capi.VRS_ERROR_INVALID_ARGUMENT
BITS = {torch.int8: torch.int8, torch.uint8: torch.uint8, torch.int16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64,
        torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
CODES = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16, torch.int32: capi.VRS_SORT_INT32,
         torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16, torch.bfloat16: capi.VRS_SORT_BFLOAT16,
         torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
FLOATS = {torch.float16: (0x8000, 0x7C00, 0x3C00), torch.bfloat16: (0x8000, 0x7F80, 0x3F80), torch.float32: (1 << 31, 0x7F800000, 0x3F800000),
          torch.float64: (1 << 63, 0x7FF0000000000000, 0x3FF0000000000000)}  # dtype -> the bits of the sign, of +inf, of 1.0


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    return context_for(dev)


# ---------------------------------------------------------------------------------------------- the reference

def keys_of(x):
    """a CPU tensor's elements as int64 keys in the order of the values: -0.0 is +0.0, every NaN the one largest key"""
    if not x.dtype.is_floating_point:
        return x.long().numpy()
    v = x.double().numpy() + 0.0  # (exact for every float dtype; -0.0 + 0.0 is +0.0)
    b = v.view(np.int64)
    k = np.where(b < 0, -(b & np.int64(0x7FFFFFFFFFFFFFFF)), b)
    return np.where(np.isnan(v), np.iinfo(np.int64).max, k)


def ref_mode(x2):
    """(values as integer bits, int64 indices) of a CPU tensor [rows, L], L >= 1"""
    keys, bits = keys_of(x2), x2.contiguous().view(BITS[x2.dtype]).numpy()
    rows = keys.shape[0]
    idx = np.zeros(rows, np.int64)
    for r in range(rows):
        uniq, counts = np.unique(keys[r], return_counts=True)
        modal = uniq[np.argmax(counts)]  # (the first of the largest counts: the smallest key)
        idx[r] = np.flatnonzero(keys[r] == modal)[-1]
    return bits[np.arange(rows), idx], idx


def check(x, dim=-1, keepdim=False, nan_free=True, dev=None):
    """vrs.mode of the CPU tensor x moved to the device, against the reference (and torch, when NaN-free); returns the result"""
    xg = x.to(dev or torch.device("cuda", 0))
    got = vrs.mode(xg, dim, keepdim)
    assert type(got).__name__ == "mode" and got.indices.dtype == torch.int64 and got.values.dtype == x.dtype
    assert got.values.device == xg.device and got.indices.device == xg.device
    d = dim % x.dim()
    moved = x.movedim(d, -1).contiguous()
    want_bits, want_idx = ref_mode(moved.reshape(-1, moved.shape[-1]))
    shape = list(moved.shape[:-1])
    if keepdim:
        shape.insert(d, 1)
    assert list(got.values.shape) == shape and list(got.indices.shape) == shape
    g_idx, g_bits = got.indices.cpu().numpy().reshape(-1), got.values.cpu().contiguous().view(BITS[x.dtype]).numpy().reshape(-1)
    bad = np.flatnonzero(g_idx != want_idx)
    assert bad.size == 0, f"{bad.size} indices differ, first in row {bad[0]}: {g_idx[bad[0]]}, want {want_idx[bad[0]]}"
    bad = np.flatnonzero(g_bits != want_bits)
    assert bad.size == 0, f"{bad.size} values differ, first in row {bad[0]}: {g_bits[bad[0]]:#x}, want {want_bits[bad[0]]:#x}"
    assert nan_free == (not bool(torch.isnan(x).any())) if x.dtype.is_floating_point else nan_free
    if nan_free:
        up = x.double() if x.dtype.is_floating_point else x.long()  # (exact and in the same order; torch's CPU mode takes these)
        theirs = torch.mode(up, dim, keepdim)
        ours = got.values.cpu().double() if x.dtype.is_floating_point else got.values.cpu().long()
        assert bool((ours == theirs.values).all())
        picked = xg.gather(d, got.indices if keepdim else got.indices.unsqueeze(d))
        assert bool((picked == (got.values if keepdim else got.values.unsqueeze(d))).all())
    return got


def draw(shape, alphabet, dtype, seed):
    """random elements from `alphabet` values around zero (unsigned: from zero)"""
    g = torch.Generator().manual_seed(seed)
    low = 0 if dtype == torch.uint8 else -(alphabet // 2)
    return torch.randint(low, low + alphabet, shape, generator=g).to(dtype)


def from_runs(runs, seed=0, dtype=torch.int32):
    """one row holding `count` times `value` for every (value, count), shuffled; sorted, the runs lie in the order of their values"""
    row = torch.cat([torch.full((c,), v, dtype=torch.int64) for v, c in runs])
    return row[torch.randperm(row.numel(), generator=torch.Generator().manual_seed(seed))].to(dtype).reshape(1, -1)


def singles(first, count):
    """`count` values from `first` up, once each"""
    return [(first + k, 1) for k in range(count)]


# ---------------------------------------------------------------------------------------------- one row

@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 4095, 4096, 4097, 12289])
def test_one_row(L):
    check(draw((L,), 5, torch.int32, L))
    check(draw((1, L), 7, torch.int32, L + 1), dim=1)


# ---------------------------------------------------------------------------------------------- runs against tile boundaries

BOUNDARY_ROWS = {
    "all-equal-3T+1": lambda: [(7, 3 * T + 1)],
    "across-T": lambda: singles(0, T - 6) + [(T, 12)] + singles(T + 1, T - 6),                       # the modal run at sorted [T - 6, T + 6)
    "ends-at-T": lambda: singles(0, T - 20) + [(T, 20)] + singles(T + 1, T),                           # ... at [T - 20, T)
    "last-partial-tile": lambda: singles(0, 2 * T + 40) + [(3 * T, 60)],                               # ... at [2T + 40, 2T + 100)
    "tie-tile0-tile2": lambda: singles(0, 100) + [(100, 50)] + singles(101, 2 * T - 140) + [(3 * T, 50)] + singles(3 * T + 1, T - 60),
    "tie-straddler-later": lambda: singles(0, T - 25) + [(T, 50)] + singles(T + 1, T) + [(3 * T, 50)] + singles(3 * T + 1, T - 75),
}
BOUNDARY_WANT = {"all-equal-3T+1": 7, "across-T": T, "ends-at-T": T, "last-partial-tile": 3 * T, "tie-tile0-tile2": 100, "tie-straddler-later": T}


@pytest.mark.parametrize("name", list(BOUNDARY_ROWS))
def test_runs_against_tile_boundaries(name):
    runs = BOUNDARY_ROWS[name]()
    x = from_runs(runs, seed=len(name))
    if name == "across-T":  # the cases are where they claim to be
        assert sum(c for v, c in runs if v < T) == T - 6
    if name == "tie-tile0-tile2":
        assert x.numel() == 3 * T and sum(c for v, c in runs if v < 3 * T) == 2 * T + 10
    if name == "tie-straddler-later":
        assert sum(c for v, c in runs if v < T) == T - 25 and x.numel() == 3 * T
    got = check(x, dim=1)
    assert int(got.values[0]) == BOUNDARY_WANT[name]
    check(torch.cat([x, x.flip(1), x]), dim=1)  # and as rows that follow one another


# ---------------------------------------------------------------------------------------------- rows against tile boundaries

ROW_SHAPES = [(1000, 1), (700, 3), (513, 8), (130, 63), (65, 64), (33, 127), (5, 1000), (3, 4096), (3, 4097), (2, 6000)]


def c_mode(ctx, xg):
    """the three C calls on a [rows, L] device tensor with a scratch of the test's own: (values, indices, scratch as the call left it)"""
    rows, L = xg.shape
    n = rows * L
    wide = xg.dtype in (torch.int64, torch.float64)
    rdt = torch.int64 if wide else torch.int32
    ranks, tmp = torch.empty(n, dtype=rdt, device=xg.device), torch.empty(n, dtype=rdt, device=xg.device)
    scratch = torch.full((rows,), -1, dtype=torch.int64, device=xg.device)
    values, indices = torch.empty(rows, dtype=xg.dtype, device=xg.device), torch.full((rows,), -7, dtype=torch.int64, device=xg.device)
    offsets = row_offsets(rows, L, xg.device)
    lib = ctx.lib
    with buffers(ctx, xg, ranks, tmp, scratch, values, indices, offsets) as (src, rk, rk_tmp, scr, vals, idx, offs):
        ctx.check(lib.vrs_sort_rank_keys(ctx.handle, src, n, L, CODES[xg.dtype], 0, rk, None))
        ctx.check(getattr(lib, "vrs_sort_segments_u64" if wide else "vrs_sort_segments_u32")(ctx.handle, rk, rk_tmp, n, offs, rows))
        ctx.check(lib.vrs_sort_restore(ctx.handle, src, rk, scr, n, L, CODES[xg.dtype], capi.VRS_SORT_MODE, vals, idx))
    return values, indices, scratch


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_against_tile_boundaries(ctx, dev, shape):
    rows, L = shape
    check(draw(shape, 4, torch.int32, rows + L), dim=1)
    # every element of every row the same value: the neighbouring rows begin and end with it, and every run must stop at its row's end
    same = torch.full(shape, 3, dtype=torch.int32)
    got = check(same, dim=1)
    assert bool((got.indices == L - 1).all())
    values, indices, scratch = c_mode(ctx, same.to(dev))
    # WHITE BOX: the header leaves the scratch unspecified after the call.  This reads the word today's runs kernel leaves there
    # (count << 32 | ...), an implementation detail and no contract: a later layout of the scratch changes this check, not the ABI.
    counts = (scratch.cpu().numpy().view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert (counts == L).all(), (counts.min(), counts.max(), L)
    assert bool((indices == L - 1).all()) and bool((values == 3).all())


def test_a_run_does_not_continue_into_the_next_row():
    """Sorted, row 1 begins with what row 0 ends with, and row 2 with what row 1 ends with; in both that first run is the longest.  A
    head rule that let a run continue from the row before would lose it."""
    for L in (6, 64, 1000, 4096, 4097):
        x = torch.full((3, L), 5, dtype=torch.int32)
        x[1, L // 2 + 1:] = 9  # more fives than nines
        x[2, :] = 12
        x[2, :L // 2 + 1] = 9  # more nines than twelves
        got = check(x[:, torch.randperm(L, generator=torch.Generator().manual_seed(L))], dim=1)
        assert got.values.tolist() == [5, 5, 9]


# ---------------------------------------------------------------------------------------------- the index pass

@pytest.mark.parametrize("where", ["first-tile", "last-tile", "all-tiles"])
def test_index_pass_over_three_tiles(where):
    L = 3 * T
    x = (torch.randperm(L, generator=torch.Generator().manual_seed(3)) + 10).to(torch.int32)  # every value once
    g = torch.Generator().manual_seed(len(where))
    lo, hi = {"first-tile": (0, T), "last-tile": (2 * T, L), "all-tiles": (0, L)}[where]
    at = lo + torch.randperm(hi - lo, generator=g)[:300]
    if where == "all-tiles":
        at = torch.cat([at, torch.tensor([5, T + 5, 2 * T + 5])])
    x[at] = 3
    got = check(x.reshape(1, L), dim=1)
    assert int(got.values[0]) == 3 and int(got.indices[0]) == int(at.max())


@pytest.mark.parametrize("shape", [(700, 3), (65, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_index_pass_with_many_rows_in_a_tile(shape):
    check(draw(shape, 3, torch.int16, 17), dim=1)
    check(draw(shape, 2, torch.float32, 18), dim=1)


# ---------------------------------------------------------------------------------------------- the nine dtypes

@pytest.mark.parametrize("dtype", list(CODES), ids=lambda d: str(d).split(".")[-1])
def test_nine_dtypes(dtype):
    if dtype in (torch.int8, torch.uint8):
        check(draw((3, 1000), 256, dtype, 5), dim=1)  # the whole range: 1000 elements of 256 values, long runs
    elif dtype == torch.int64:
        check(draw((2, 777), 9, dtype, 6) * (1 << 32) + 12345, dim=1)  # values that differ only above bit 32
    elif dtype == torch.float64:
        check(1.0 + draw((2, 777), 9, dtype, 7) * 2.0 ** -20, dim=1)  # ... in the mantissa's bits 32 and up
    else:
        check(draw((2, 777), 9, dtype, 8), dim=1)
    check(draw((40, 33), 5, dtype, 9), dim=1)


# ---------------------------------------------------------------------------------------------- floats

def from_bits(patterns, dtype):
    """a [1, len] tensor of `dtype` with the given bit patterns"""
    width = {torch.int16: 16, torch.int32: 32, torch.int64: 64}[BITS[dtype]]
    signed = [p - (1 << width) if p >= 1 << (width - 1) else p for p in patterns]
    return torch.tensor(signed, dtype=BITS[dtype]).view(dtype).reshape(1, -1)


@pytest.mark.parametrize("dtype", list(FLOATS), ids=lambda d: str(d).split(".")[-1])
def test_float_classes(dtype):
    sign, inf, one = FLOATS[dtype]
    two = one + 1  # (the next value above 1.0)
    nans = [inf | 1, inf | sign | 2, inf | (inf >> 3) | 5, sign | (sign - 1)]  # both signs, several payloads, all ones
    # the zero class is the mode, -0.0 and +0.0 mixed; the value is the bits of the last one
    got = check(from_bits([0, sign, one, sign, 0, two, sign, one, two], dtype), dim=1)
    assert int(got.indices[0]) == 6 and int(got.values.view(BITS[dtype])[0]) == int(from_bits([sign], dtype).view(BITS[dtype])[0, 0])
    got = check(from_bits([sign, sign, one, 0, two, one], dtype), dim=1)
    assert int(got.indices[0]) == 3 and int(got.values.view(BITS[dtype])[0]) == 0
    # the NaN class is the mode: all NaNs count together, the value is the last one's bits
    got = check(from_bits([nans[0], one, nans[1], one, two, nans[2], inf, nans[3], 0], dtype), dim=1, nan_free=False)
    assert int(got.indices[0]) == 7 and bool(torch.isnan(got.values[0]))
    # NaNs present but not modal
    got = check(from_bits([nans[0], one, nans[1], one, two, one, inf], dtype), dim=1, nan_free=False)
    assert int(got.indices[0]) == 5
    # infinities and subnormals: values of their own (a subnormal is not zero, -inf not +inf)
    sub = [1, 1, sign | 1, 1, 0, sign, inf, inf | sign, inf, 1, sign | 1, sign | 1]
    got = check(from_bits(sub, dtype), dim=1)
    assert int(got.indices[0]) == 9
    got = check(from_bits([inf, inf | sign, inf, one, inf | sign, inf, 1, 0], dtype), dim=1)
    assert int(got.indices[0]) == 5
    # and many rows of them, NaNs among them
    g = torch.Generator().manual_seed(11)
    pool = from_bits([0, sign, one, two, inf, inf | sign, 1, sign | 1] + nans, dtype).view(BITS[dtype]).reshape(-1)
    rows = pool[torch.randint(0, pool.numel(), (50, 37), generator=g)].view(dtype)
    check(rows, dim=1, nan_free=False)


# ---------------------------------------------------------------------------------------------- shapes and strides

def test_dims_of_a_3d_tensor_and_keepdim():
    x = draw((5, 7, 9), 3, torch.int32, 21)
    for dim in (0, 1, 2, -1, -3):
        check(x, dim)
        check(x, dim, keepdim=True)
    y = draw((6, 40), 4, torch.float32, 22)
    check(y, 0, keepdim=True)


def test_strides_and_offsets(dev):
    base = draw((40, 60), 4, torch.int16, 23).to(dev)
    for view in (base.t(), base[:, ::2], base[3:, 5:50], base.t()[::3]):
        assert not view.is_contiguous()
        got = vrs.mode(view, 1)
        want_bits, want_idx = ref_mode(view.cpu().contiguous())
        assert (got.indices.cpu().numpy() == want_idx).all() and (got.values.cpu().numpy() == want_bits).all()
    raw = draw((1 + 3 * 50,), 6, torch.int8, 24).to(dev)
    off = raw[1:].view(3, 50)  # an int8 view that starts 1 byte into its allocation
    assert off.data_ptr() % 4 == 1
    got = vrs.mode(off, 1)
    want_bits, want_idx = ref_mode(off.cpu().contiguous())
    assert (got.indices.cpu().numpy() == want_idx).all() and (got.values.cpu().numpy() == want_bits).all()


def test_edges_as_torch(dev):
    scalar = torch.tensor(2.5, device=dev)
    got = vrs.mode(scalar)
    theirs = torch.mode(scalar.cpu())
    assert got.values.shape == theirs.values.shape == () and float(got.values) == 2.5 and int(got.indices) == int(theirs.indices) == 0
    assert vrs.mode(scalar, 0, True).values.shape == torch.mode(scalar.cpu(), 0, True).values.shape
    empty = torch.empty((0, 5), device=dev)
    for keepdim in (False, True):
        got, theirs = vrs.mode(empty, 1, keepdim), torch.mode(empty.cpu(), 1, keepdim)
        assert got.values.shape == theirs.values.shape and got.indices.shape == theirs.indices.shape and got.indices.dtype == torch.int64
    with pytest.raises(IndexError):
        vrs.mode(empty, 0)
    with pytest.raises(IndexError):
        vrs.mode(empty, 2)


def test_on_another_stream(dev):
    x = draw((20, 3000), 6, torch.int32, 25)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        got = check(x, 1, dev=dev)
    stream.synchronize()
    again = check(x, 1, dev=dev)
    assert torch.equal(got.indices, again.indices) and torch.equal(got.values, again.values)


# ---------------------------------------------------------------------------------------------- the same bits on every run

def test_two_runs_are_the_same_bits(dev):
    cases = [from_runs(BOUNDARY_ROWS["tie-straddler-later"](), seed=1), draw((130, 63), 4, torch.int32, 2), draw((3, 4097), 4, torch.float32, 3)]
    for x in cases:
        xg = x.to(dev)
        a, b = vrs.mode(xg, 1), vrs.mode(xg, 1)
        assert torch.equal(a.indices, b.indices) and torch.equal(a.values.view(BITS[x.dtype]), b.values.view(BITS[x.dtype]))


# ---------------------------------------------------------------------------------------------- a fixed-seed deck

def test_random_deck():
    rng = np.random.default_rng(20)
    dtypes = list(CODES)
    for case in range(40):
        dtype = dtypes[case % len(dtypes)]
        nd = int(rng.integers(1, 4))
        shape = [int(rng.integers(1, 40)) for _ in range(nd)]
        dim = int(rng.integers(0, nd))
        shape[dim] = int(rng.choice([1, 2, 3, 31, 64, 65, 200, 1000, 4096, 4100, 9000]))
        while int(np.prod(shape)) > 50000 or int(np.prod(shape)) // shape[dim] > 1500:  # (the reference walks the rows one by one)
            k = int(np.argmax([s if i != dim else 0 for i, s in enumerate(shape)]))
            if shape[k] == 1 or k == dim:
                shape[dim] = max(1, shape[dim] // 2)
            else:
                shape[k] = max(1, shape[k] // 2)
        alphabet = int(rng.choice([1, 2, 3, 10, 100]))
        x = draw(tuple(shape), alphabet, dtype, 100 + case)
        with_nan = dtype.is_floating_point and case % 4 == 1
        if with_nan:
            flat = x.reshape(-1)
            flat[torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(case))[:max(1, flat.numel() // 7)]] = float("nan")
            flat[0] = float("nan")
        check(x, dim - nd if case % 2 else dim, keepdim=bool(case % 3 == 0), nan_free=not with_nan)


# ---------------------------------------------------------------------------------------------- the C call's refusals and memory contract

def test_the_c_call_refuses_on_a_live_context(ctx, dev):
    rows, L = 6, 50
    n = rows * L
    mem = torch.zeros(4096, dtype=torch.int64, device=dev)

    def buf(offset_bytes, nbytes):
        return engine.Buffer(ctx, engine.Buffer.BufferSettings(nbytes), device_ptr=mem.data_ptr() + offset_bytes)

    src, ranks, values, indices = buf(0, 4 * n), buf(2048, 4 * n), buf(4096, 4 * rows), buf(8192, 8 * rows)
    scratch, short, off = buf(12288, 8 * rows), buf(12288, 8 * rows - 1), buf(12288 + 4, 8 * rows)
    held = [src, ranks, values, indices, scratch, short, off]
    try:
        def call(scr, vals=values, idx=indices, s=src, rk=ranks, flags=capi.VRS_SORT_MODE):
            return ctx.lib.vrs_sort_restore(ctx.handle, s.handle if s else None, rk.handle if rk else None, scr.handle if scr else None, n, L,
                                            capi.VRS_SORT_INT32, flags, vals.handle if vals else None, idx.handle if idx else None)

        assert call(scratch) == capi.VRS_OK
        torch.cuda.synchronize(dev)
        before = mem.clone()
        assert call(None) == BAD and b"NULL" in ctx.lib.vrs_last_error(ctx.handle)
        assert call(short) == BAD and b"too small" in ctx.lib.vrs_last_error(ctx.handle)
        assert call(off) == BAD and b"8-byte boundary" in ctx.lib.vrs_last_error(ctx.handle)
        assert call(scratch, idx=None) == BAD and b"NULL" in ctx.lib.vrs_last_error(ctx.handle)
        assert call(scratch, vals=None) == BAD and call(scratch, s=None) == BAD and call(scratch, rk=None) == BAD
        assert call(scratch, flags=capi.VRS_SORT_MODE | capi.VRS_SORT_DESCENDING) == BAD
        assert call(scratch, flags=capi.VRS_SORT_MODE | 4) == BAD and b"flag" in ctx.lib.vrs_last_error(ctx.handle)
        assert ctx.lib.vrs_sort_rank_keys(ctx.handle, src.handle, n, L, capi.VRS_SORT_INT32, capi.VRS_SORT_MODE, ranks.handle, None) == BAD
        assert ctx.lib.vrs_sort_restore(ctx.handle, None, None, None, 0, L, capi.VRS_SORT_INT32, capi.VRS_SORT_MODE, None, None) == BAD  # NULLs, even at 0
        assert ctx.lib.vrs_sort_restore(ctx.handle, src.handle, ranks.handle, scratch.handle, 0, L, capi.VRS_SORT_INT32, capi.VRS_SORT_MODE,
                                        values.handle, indices.handle) == capi.VRS_OK  # num_elements == 0: nothing done
        torch.cuda.synchronize(dev)
        assert torch.equal(mem, before)  # nothing was enqueued by any of them
    finally:
        for b in held:
            b.release()


CONTRACT = {"5x1000-float16": (5, 1000, torch.float16), "1x9000-int64": (1, 9000, torch.int64)}


def mode_case(name):
    rows, L, dtype = CONTRACT[name]
    code = CODES[dtype]
    if dtype == torch.float16:  # few values, both zeros and two NaNs among them
        pool = torch.tensor([0, -0x8000, 0x3C00, 0x3C01, 0x7C00, 0x7E00, -0x200, 0x4000], dtype=torch.int16)
        x = pool[torch.randint(0, pool.numel(), (rows, L), generator=torch.Generator().manual_seed(31))].view(dtype)
    else:
        x = draw((rows, L), 40, dtype, 32) * (1 << 33) + 7
    storage = RANK_DTYPES[code][0]
    u = x.contiguous().view(BITS[dtype]).numpy().view(storage).reshape(-1)
    ranks = np.sort(rank_of(u, code, False).reshape(rows, L), axis=1).reshape(-1)
    want_bits, want_idx = ref_mode(x)
    eb, rb = u.itemsize, ranks.itemsize
    specs = [Spec("src", rows * L * eb, "in", wrap_align(eb), u), Spec("ranks", rows * L * rb, "in", wrap_align(rb), ranks),
             Spec("positions", 8 * rows, "scratch", 8), Spec("out_values", rows * eb, "out", wrap_align(eb)), Spec("out_indices", 8 * rows, "out", 8)]

    def call(c, h):
        return c.lib.vrs_sort_restore(c.handle, h["src"], h["ranks"], h["positions"], rows * L, L, code, capi.VRS_SORT_MODE, h["out_values"], h["out_indices"])

    return Case(specs, call, {"out_values": as_bytes(want_bits), "out_indices": as_bytes(want_idx)},
                refuse={"positions": 1, "out_values": eb, "out_indices": 8, "ranks": rb, "src": eb}, misalign={"positions": 4})


@pytest.mark.parametrize("name", list(CONTRACT))
def test_memory_contract(ctx, dev, name):
    """src and ranks are never written, positions is scratch, the two outputs are written in their num_rows entries, nothing else changes
    (both layouts, two poisons, the same output bits under both)"""
    run_case(ctx, dev, f"sort_restore mode {name}", mode_case(name))


def test_memory_contract_refusals(ctx, dev):
    run_refusals(ctx, dev, "sort_restore mode", mode_case("5x1000-float16"))
