"""Run-length decode on the device.  C level: vrs_search_sorted with queries == NULL (query row i = 0, 1, ..., query_row_len - 1)
against numpy.searchsorted(b, arange(Q), side) and against the same call with those queries uploaded, index for index; torch level:
vrs.repeat_interleave against torch.repeat_interleave on the CPU, in values, shape and dtype.  Every comparison is exact."""
import ctypes
import time

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 4096  # kSearchChunk: outputs per work item
MS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5]
QS = [1, 4095, 4096, 4097, 8192, 100003]
CODES = {"int32": capi.VRS_SORT_INT32, "int64": capi.VRS_SORT_INT64}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    return context_for(dev)


def flags_of(right, out64):
    return (capi.VRS_SEARCH_RIGHT if right else 0) | (capi.VRS_SEARCH_OUT_INT64 if out64 else 0)


def identity_call(ctx, b_d, m, rows, q_len, code, right, out64, out=None):
    """vrs_search_sorted(queries = NULL) over the boundaries b_d (rows of m): the rows * q_len outputs as a tensor."""
    if out is None:
        out = torch.empty(rows * q_len, dtype=torch.int64 if out64 else torch.int32, device=b_d.device)
    with buffers(ctx, b_d, out) as (bnd, res):
        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, bnd, b_d.numel(), m, None, rows * q_len, q_len, code, flags_of(right, out64), None, res, None))
    return out


def uploaded_call(ctx, b_d, m, rows, q_len, code, right, out64):
    """The same call with the queries materialised: rows of arange(q_len) of the boundaries' dtype."""
    q_d = torch.arange(q_len, dtype=b_d.dtype, device=b_d.device).repeat(rows)
    out = torch.empty(rows * q_len, dtype=torch.int64 if out64 else torch.int32, device=b_d.device)
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(ctx.lib.vrs_search_plan(ctx.handle, b_d.numel(), m, rows * q_len, q_len, code, 0, ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=b_d.device) if need.value else None
    with buffers(ctx, b_d, q_d, out, scratch) as (bnd, qry, res, scr):
        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, bnd, b_d.numel(), m, qry, rows * q_len, q_len, code, flags_of(right, out64), None, res, scr))
    return out


def check(ctx, dev, b, q_len, dtype, out64, rows=1):
    """Both sides of the identity call over the ascending boundaries b ([m] or [b_rows, m], numpy) against numpy and the uploaded call."""
    b = np.asarray(b, dtype=dtype)
    m = b.shape[-1]
    b_rows = b.reshape(-1, m)
    b_d = torch.from_numpy(b.reshape(-1)).to(dev)
    arange = np.arange(q_len, dtype=dtype)
    for right in (False, True):
        side = "right" if right else "left"
        want = np.concatenate([np.searchsorted(b_rows[r if b_rows.shape[0] > 1 else 0], arange, side) for r in range(rows)])
        got = identity_call(ctx, b_d, m, rows, q_len, CODES[dtype], right, out64)
        assert got.dtype == (torch.int64 if out64 else torch.int32)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (dtype, m, q_len, rows, side, out64)
        assert torch.equal(got, uploaded_call(ctx, b_d, m, rows, q_len, CODES[dtype], right, out64)), (dtype, m, q_len, rows, side, out64)


@pytest.mark.parametrize("out64", [False, True], ids=["out32", "out64"])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_identity_call_equals_numpy_and_the_uploaded_queries(ctx, dev, dtype, out64):
    for m in MS:
        steps = np.arange(1, m + 1)                 # every run of length one
        equal = np.full(m, 4000)                    # m - 1 runs of length zero
        negative = np.arange(m) * 3 - 100           # negative leading boundaries
        for q_len in QS:                            # (Q below the last boundary: m = 12293, Q = 1; above it: m = 1, Q = 100003)
            for b in (steps, equal, negative):
                check(ctx, dev, b, q_len, dtype, out64)


@pytest.mark.parametrize("out64", [False, True], ids=["out32", "out64"])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_runs_across_chunks_and_at_their_edges(ctx, dev, dtype, out64):
    j0 = CHUNK
    check(ctx, dev, [100, 100 + 3 * CHUNK], 5 * CHUNK + 7, dtype, out64)                      # one run crossing three chunks
    check(ctx, dev, [3] + [CHUNK + 77] * 10000 + [2 * CHUNK + 1], 3 * CHUNK, dtype, out64)    # 10000 equal boundaries inside one chunk
    check(ctx, dev, [j0 - 1, j0, j0 + 4095, j0 + 4096], 3 * CHUNK, dtype, out64)              # the edges of the chunk at j0
    for single in (j0 - 1, j0, j0 + 4095, j0 + 4096):
        check(ctx, dev, [single], 3 * CHUNK, dtype, out64)
    check(ctx, dev, [-7, -7, -1, 0, 0, 1, 5, 5, 9], 12, dtype, out64)                         # negative leading boundaries, zeros
    check(ctx, dev, [10, 20, 10 ** 6], 5000, dtype, out64)                                    # Q below the last boundary
    check(ctx, dev, [10, 20, 30], 5000, dtype, out64)                                         # Q above it: the tail is m
    info = np.iinfo(dtype)
    check(ctx, dev, [info.min, 0, 0, info.max], CHUNK + 1, dtype, out64)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_rows(ctx, dev, dtype):
    rng = np.random.default_rng(5)
    three = np.sort(rng.integers(-50, 6000, (3, 777)), axis=1)
    for out64 in (False, True):
        check(ctx, dev, three, 5000, dtype, out64, rows=3)      # three boundary rows against three query rows
        check(ctx, dev, three[0], 5000, dtype, out64, rows=3)   # one boundary row against three query rows: every row starts again at 0
        check(ctx, dev, three[:, :5], 5, dtype, out64, rows=3)  # rows that are no multiple of four outputs: the scalar stores


@pytest.mark.parametrize("out64,skip", [(False, 1), (False, 2), (False, 3), (True, 1)], ids=["int32+4", "int32+8", "int32+12", "int64+8"])
def test_out_that_starts_off_a_16_byte_boundary(ctx, dev, out64, skip):
    rng = np.random.default_rng(6)
    b = np.sort(rng.integers(0, 3 * CHUNK, 5000))
    q_len = 3 * CHUNK + 3
    b_d = torch.from_numpy(b).to(dev)
    whole = torch.full((q_len + 8,), -1, dtype=torch.int64 if out64 else torch.int32, device=dev)
    view = whole[skip:skip + q_len]
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == skip * whole.element_size()
    for right in (False, True):
        whole.fill_(-1)
        identity_call(ctx, b_d, b.size, 1, q_len, capi.VRS_SORT_INT64, right, out64, out=view)
        got = whole.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[skip:skip + q_len], np.searchsorted(b, np.arange(q_len), "right" if right else "left"))
        assert (got[:skip] == -1).all() and (got[skip + q_len:] == -1).all()


@pytest.mark.parametrize("out64", [False, True], ids=["out32", "out64"])
def test_shuffled_boundaries_stay_inside_the_row_and_inside_out(ctx, dev, out64):
    rng = np.random.default_rng(7)
    for m, q_len in ((20000, 20001), (5, 3 * CHUNK), (70000, 4097)):
        b = rng.integers(-100, 30000, m)
        b_d = torch.from_numpy(b).to(dev)
        whole = torch.full((q_len + 64,), -1, dtype=torch.int64 if out64 else torch.int32, device=dev)
        for right in (False, True):
            whole.fill_(-1)
            identity_call(ctx, b_d, m, 1, q_len, capi.VRS_SORT_INT64, right, out64, out=whole[:q_len])
            got = whole.cpu().numpy()
            assert (got[:q_len] >= 0).all() and (got[:q_len] <= m).all()
            assert (got[q_len:] == -1).all()  # the sentinel words behind out


def test_no_boundaries_and_no_counter(ctx, dev):
    before = vrs.search_stats(ctx)
    b_d = torch.arange(1, 5001, dtype=torch.int64, device=dev)
    got = identity_call(ctx, b_d, 5000, 1, 6000, capi.VRS_SORT_INT64, True, True)
    assert torch.equal(got.cpu(), torch.clamp(torch.arange(6000), max=5000))
    out = torch.full((100,), -1, dtype=torch.int32, device=dev)
    with buffers(ctx, out) as (res,):  # num_boundaries == 0: zeros
        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, None, 0, 0, None, 100, 100, capi.VRS_SORT_INT32, 0, None, res, None))
        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, None, 0, 0, None, 0, 0, capi.VRS_SORT_INT32, 0, None, res, None))  # num_queries == 0
    assert (out == 0).all()
    assert vrs.search_stats(ctx) == before  # none of the four counters moved


def test_refusals(ctx, dev):
    b_d = torch.arange(1, 11, dtype=torch.int64, device=dev)
    out = torch.full((16,), -1, dtype=torch.int64, device=dev)
    sorter = torch.arange(10, dtype=torch.int64, device=dev)
    lib, h = ctx.lib, ctx.handle
    with buffers(ctx, b_d, out, sorter) as (bnd, res, srt):
        for code in (capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64, capi.VRS_SORT_INT16, capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8,
                     capi.VRS_SORT_FLOAT16, capi.VRS_SORT_BFLOAT16):
            with pytest.raises(vrs.VrsError, match="VRS_SORT_INT32 or VRS_SORT_INT64"):
                ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, 16, 16, code, 0, None, res, None))
        with pytest.raises(vrs.VrsError, match="sorter"):
            ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, 16, 16, capi.VRS_SORT_INT64, 0, srt, res, None))
        # refused on its arguments alone: no buffer of 2^31 + 1 entries exists
        with pytest.raises(vrs.VrsError, match="2\\^31"):
            ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, (1 << 31) + 1, (1 << 31) + 1, capi.VRS_SORT_INT32, 0, None, res, None))
        with pytest.raises(vrs.VrsError, match="NULL"):
            ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, 16, 16, capi.VRS_SORT_INT64, 0, None, None, None))
        with pytest.raises(vrs.VrsError, match="out buffer is too small"):
            ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, 17, 17, capi.VRS_SORT_INT64, capi.VRS_SEARCH_OUT_INT64, None, res, None))
        with pytest.raises(vrs.VrsError, match="flag"):
            ctx.check(lib.vrs_search_sorted(h, bnd, 10, 10, None, 16, 16, capi.VRS_SORT_INT64, 4, None, res, None))
    torch.cuda.synchronize()
    assert (out == -1).all()  # nothing was enqueued


# ---------------------------------------------------------------------------------------------- torch level

def same(got, want):
    """values (bit for bit), shape and dtype"""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    g, w = got.cpu().contiguous(), want.contiguous()
    if g.dtype == torch.bool:
        assert torch.equal(g, w)
    else:
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[g.element_size()]
        assert torch.equal(g.view(bits), w.view(bits))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_one_argument_form(dev, dtype):
    rng = np.random.default_rng(11)
    for m, high in ((1, 5), (7, 4), (5000, 6), (100000, 3), (3, 20000)):
        r = torch.from_numpy(rng.integers(0, high, m)).to(dtype)
        same(vrs.repeat_interleave(r.to(dev)), torch.repeat_interleave(r))
        total = int(r.sum())
        same(vrs.repeat_interleave(r.to(dev), output_size=total), torch.repeat_interleave(r, output_size=total))
    zeros = torch.zeros(50, dtype=dtype)
    same(vrs.repeat_interleave(zeros.to(dev)), torch.repeat_interleave(zeros))
    empty = torch.empty(0, dtype=dtype)
    same(vrs.repeat_interleave(empty.to(dev)), torch.repeat_interleave(empty))


def test_int_repeats_and_broadcast_repeats(dev):
    x = torch.arange(5 * 7 * 3, dtype=torch.float32).reshape(5, 7, 3)
    x_d = x.to(dev)
    for dim in (None, 0, 1, -1):
        for r in (0, 1, 3):
            same(vrs.repeat_interleave(x_d, r, dim), torch.repeat_interleave(x, r, dim))
            same(vrs.repeat_interleave(x_d.transpose(0, 2), r, dim), torch.repeat_interleave(x.transpose(0, 2), r, dim))
        for r in (torch.tensor(2), torch.tensor([3]), torch.tensor([0], dtype=torch.int32), torch.tensor(1, dtype=torch.int32)):
            same(vrs.repeat_interleave(x_d, r.to(dev), dim), torch.repeat_interleave(x, r, dim))
    same(vrs.repeat_interleave(x_d, 2, 1, output_size=14), torch.repeat_interleave(x, 2, 1, output_size=14))
    assert vrs.repeat_interleave(x_d, 1).data_ptr() != x_d.data_ptr()
    same(vrs.repeat_interleave(torch.tensor(5.0, device=dev), 3), torch.repeat_interleave(torch.tensor(5.0), 3))
    same(vrs.repeat_interleave(torch.tensor(5.0, device=dev), torch.tensor(3, device=dev)), torch.repeat_interleave(torch.tensor(5.0), torch.tensor(3)))


@pytest.mark.parametrize("rdtype", [torch.int32, torch.int64])
def test_every_dim_of_a_tensor_and_of_a_transposed_view(dev, rdtype):
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((5, 7, 3)).astype(np.float32))
    for t, t_d in ((x, x.to(dev)), (x.transpose(0, 1), x.to(dev).transpose(0, 1)), (x.transpose(0, 2), x.to(dev).transpose(0, 2))):
        for dim in (0, 1, -1, None):
            size = t.numel() if dim is None else t.shape[dim]
            r = torch.from_numpy(rng.integers(0, 4, size)).to(rdtype)  # zeros among the repeats
            same(vrs.repeat_interleave(t_d, r.to(dev), dim), torch.repeat_interleave(t, r, dim))
            total = int(r.sum())
            same(vrs.repeat_interleave(t_d, r.to(dev), dim, output_size=total), torch.repeat_interleave(t, r, dim, output_size=total))


@pytest.mark.parametrize("dtype", [torch.bool, torch.bfloat16, torch.float64, torch.int8])
def test_any_dtype_keeps_its_bits(dev, dtype):
    rng = np.random.default_rng(13)
    n = 9001
    if dtype == torch.bool:
        x = torch.from_numpy(rng.random(n) < 0.5)
    elif dtype == torch.int8:
        x = torch.from_numpy(rng.integers(-128, 128, n).astype(np.int8))
    elif dtype == torch.float64:
        x = torch.from_numpy(rng.standard_normal(n))
        x[::7] = torch.tensor([0x7FF8000000000123, -0x0007FFFFFFFFFEDC, -0x8000000000000000], dtype=torch.int64).view(torch.float64)[torch.arange(len(x[::7])) % 3]
    else:
        x = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dtype)
        x[::7] = torch.tensor([0x7FC1, -0x003F, -0x8000], dtype=torch.int16).view(torch.bfloat16)[torch.arange(len(x[::7])) % 3]  # NaN payloads, -0.0
    r = torch.from_numpy(rng.integers(0, 5, n))
    same(vrs.repeat_interleave(x.to(dev), r.to(dev)), torch.repeat_interleave(x, r))
    same(vrs.repeat_interleave(x.to(dev).reshape(-1, 1), r.to(dev), 0), torch.repeat_interleave(x.reshape(-1, 1), r, 0))


def test_empty_shapes(dev):
    for shape, r, dim in (((0, 3), torch.empty(0, dtype=torch.int64), 0), ((0, 3), torch.tensor([2]), 0), ((0, 3), torch.tensor([2, 2, 2]), 1),
                          ((4, 0), torch.tensor([1, 0, 2, 3]), 0), ((0,), torch.tensor(4), None), ((3, 2), torch.zeros(3, dtype=torch.int32), 0)):
        x = torch.empty(shape)
        same(vrs.repeat_interleave(x.to(dev), r.to(dev), dim), torch.repeat_interleave(x, r, dim))
    same(vrs.repeat_interleave(torch.tensor([1, 2], device=dev), output_size=0), torch.empty(0, dtype=torch.int64))


def test_errors_as_torch(dev):
    x = torch.arange(6.0, device=dev).reshape(2, 3)
    with pytest.raises(RuntimeError, match="negative"):
        vrs.repeat_interleave(x, torch.tensor([1, -1], device=dev), 0)
    with pytest.raises(RuntimeError, match="negative"):
        vrs.repeat_interleave(torch.tensor([3, -2, 5], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="negative"):
        vrs.repeat_interleave(x, -1)
    with pytest.raises(RuntimeError, match="Long or Int"):
        vrs.repeat_interleave(x, torch.tensor([1.0, 2.0], device=dev), 0)
    with pytest.raises(RuntimeError, match="same size"):
        vrs.repeat_interleave(x, torch.tensor([1, 2, 3], device=dev), 0)
    with pytest.raises(RuntimeError, match="0-dim or 1-dim"):
        vrs.repeat_interleave(x, torch.tensor([[1, 2]], device=dev), 0)
    with pytest.raises(RuntimeError, match="1D"):
        vrs.repeat_interleave(torch.tensor(3, device=dev))
    with pytest.raises(RuntimeError, match="output_size"):
        vrs.repeat_interleave(x, 2, 0, output_size=5)
    with pytest.raises(IndexError):
        vrs.repeat_interleave(x, 2, 5)
    with pytest.raises(vrs.VrsError, match="GPU"):
        vrs.repeat_interleave(x, torch.tensor([1, 2]), 0)
    with pytest.raises(vrs.VrsError, match="2\\^32"):
        vrs.repeat_interleave(torch.tensor([1 << 31, 1 << 31], device=dev))


def test_a_wrong_output_size_never_indexes_out_of_range(dev):
    x = torch.arange(10.0, device=dev)
    r = torch.tensor([1] * 10, device=dev)
    got = vrs.repeat_interleave(x, r, output_size=5000)  # the caller's error: the outputs past the total repeat the last element
    assert torch.equal(got[:10], x) and (got[10:] == 9.0).all()
    assert torch.equal(vrs.repeat_interleave(x, r, output_size=4), x[:4])
    idx = vrs.repeat_interleave(torch.tensor([2, -1, 3], device=dev), output_size=6000)  # not ascending: still inside the input
    assert int(idx.min()) >= 0 and int(idx.max()) <= 2


def test_output_size_never_waits_for_the_device(dev):
    rng = np.random.default_rng(14)
    x = torch.from_numpy(rng.standard_normal((200000, 4)).astype(np.float32)).to(dev)
    r = torch.from_numpy(rng.integers(0, 6, 200000)).to(dev)
    total = int(r.sum())
    vrs.repeat_interleave(x, r, 0, output_size=total)  # warm-up: module load, the context, torch's allocations
    torch.cuda.synchronize()
    torch.cuda._sleep(int(60e-3 * 2.0e9))  # about 60 ms of work ahead of the call
    t0 = time.perf_counter()
    got = vrs.repeat_interleave(x, r, 0, output_size=total)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert dt < 5e-3, f"the call took {dt * 1e3:.2f} ms on the host"
    assert busy
    same(got, torch.repeat_interleave(x.cpu(), r.cpu(), 0))


def test_round_trip_of_unique_consecutive(dev):
    rng = np.random.default_rng(15)
    for dtype in (torch.int32, torch.int64, torch.float32, torch.float64):
        x = torch.from_numpy(np.repeat(rng.integers(-5, 5, 30000), rng.integers(1, 9, 30000))).to(dtype).to(dev)
        v, c = vrs.unique_consecutive(x, return_counts=True)
        assert v.numel() < x.numel()
        assert torch.equal(vrs.repeat_interleave(v, c), x)
        assert torch.equal(vrs.repeat_interleave(c)[:-1] != vrs.repeat_interleave(c)[1:], x[:-1] != x[1:])
