"""The row form of the ordered compaction on the device (vrs_compact_outputs.row_elems = W >= 2: every flag a dense row), bit for bit
against the host restatement (vrs_compact_host) and against torch on the CPU: the shapes of tests/test_mask_index_cpu.py and sizes
around a tile (T = 16384, the default) and a chunk, bases off the 16-byte boundary (every word width down to one byte), rows wide
enough for several slices per tile and for the row-by-row walk, red zones behind every output, a num_selected below the true count,
flat + coords + rows from one call; then vrs.mask_index / mask_index_put against x[mask] / torch.index_put, and one case whose bytes
and words per chunk pass 2^32.  All comparisons are of bytes: there are no tolerances."""
import ctypes

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for

from .test_mask_index_cpu import PATTERNS, ROWS, SIZES, host_rows, pattern

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = capi.COMPACT_TILE_ELEMS_DEFAULT
SENTINEL = 0xA5
GUARD_ROWS = 2
VALUE_DTYPES = {1: torch.uint8, 2: torch.float16, 4: torch.float32, 8: torch.int64}
DEVICE_ROWS = ROWS + [(3, 2), (8, 2), (3, 8)]  # (float16 rows, and a row of 24 bytes: 8-byte words)
DEVICE_SIZES = SIZES + [T, T + 1, 3 * T + 5]


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    assert c.tuning.get(capi.VRS_TUNE_COMPACT_TILE_ELEMS, T) == T
    return c


@pytest.fixture(scope="module")
def lib_cpu():
    return capi.load_library()


def random_rows(seed, rows, row_bytes):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (rows, row_bytes), generator=g, dtype=torch.uint8)


def as_bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def place(dev, body, offset, guard_bytes):
    """body's bytes on the device `offset` bytes behind a 16-byte boundary, sentinels in front and behind: (everything, the body)"""
    raw = torch.full((offset + body.numel() + guard_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    inner = raw[offset:offset + body.numel()]
    inner.copy_(body.reshape(-1))
    return raw, inner


def take_back(raw, inner_bytes, offset):
    """the body back on the CPU; the sentinels around it must be intact"""
    host = raw.cpu()
    assert (host[:offset] == SENTINEL).all() and (host[offset + inner_bytes:] == SENTINEL).all(), "a byte outside the output was written"
    return host[offset:offset + inner_bytes]


def device_rows(c, mask, W, vb, values, source=None, *, limit=None, offsets=(0, 0, 0), flat=False, coords_shape=None, rows=True):
    """vrs_compact_count + one vrs_compact_emit on the CPU tensors mask [n] and values / source [rows, W * vb] of bytes.  offsets: bytes
    behind a 16-byte boundary of (values and scatter_input, source, the outputs).  limit: num_selected, when not the true count.
    Answers a dict: R, gather [limit, row_bytes], scatter [n, row_bytes] (with source), flat, coords."""
    d = torch.device("cuda", 0)
    n, rb = mask.numel(), W * vb
    need = capi.query_u64("vrs_compact_scratch_bytes", n, T)
    flags = mask.to(d)
    scratch = torch.full((need,), 0xAB, dtype=torch.uint8, device=d)
    got = ctypes.c_uint64(1 << 40)
    with buffers(c, flags, scratch) as (f, s):
        c.check(c.lib.vrs_compact_count(c.handle, f, n, capi.VRS_COMPACT_BOOL, s, None, ctypes.byref(got)))
    R = got.value
    L = R if limit is None else limit
    o = capi.CompactOutputs()
    o.num_selected, o.row_elems, o.value_bytes = L, W, vb
    guard = GUARD_ROWS * rb
    _, vals = place(d, values, offsets[0], 0)
    blank = lambda r: torch.full((r * rb,), SENTINEL, dtype=torch.uint8)  # noqa: E731
    g_raw, g_out = place(d, blank(L), offsets[2], guard)
    src = s_raw = s_out = None
    if source is not None:
        _, src = place(d, source[:max(L, 0)] if limit is not None else source, offsets[1], 0)
        s_raw, s_out = place(d, blank(n), offsets[2], guard)
    fl = torch.full((L,), 0x5B5B, dtype=torch.int64, device=d) if flat else None
    co = torch.full((L, len(coords_shape)), 0x5B5B, dtype=torch.int64, device=d) if coords_shape else None
    with buffers(c, flags, scratch, fl, co, vals, g_out, src, s_out) as (f, s, hf, hc, hv, hg, hs, ho):
        ptr = lambda h: h.value if h is not None else None  # noqa: E731
        o.flat, o.coords, o.coords_layout = ptr(hf), ptr(hc), capi.VRS_COMPACT_ROWS
        if coords_shape:
            o.ndim, o.shape = len(coords_shape), (ctypes.c_uint32 * 8)(*coords_shape)
        if rows:
            o.gather_values, o.gather_out = ptr(hv), ptr(hg)
        if source is not None:
            o.scatter_input, o.scatter_source, o.scatter_out = ptr(hv), ptr(hs), ptr(ho)
        c.check(c.lib.vrs_compact_emit(c.handle, f, n, capi.VRS_COMPACT_BOOL, s, ctypes.byref(o)))
    out = {"R": R, "gather": take_back(g_raw, L * rb, offsets[2]).reshape(L, rb)}
    if source is not None:
        out["scatter"] = take_back(s_raw, n * rb, offsets[2]).reshape(n, rb)
    if flat:
        out["flat"] = fl.cpu()
    if coords_shape:
        out["coords"] = co.cpu()
    return out


def want_scatter(mask, values, source, limit):
    """out row i = flag[i] && rank(i) < limit ? source row rank(i) : values row i, by torch on the CPU"""
    rank = torch.cumsum(mask.long(), 0) - 1
    take = mask & (rank < limit)
    want = values.clone()
    want[take] = source[rank[take]]
    return want


def check_against_host_and_torch(c, lib_cpu, mask, W, vb, values, source, **how):
    got = device_rows(c, mask, W, vb, values, source, **how)
    R = int(mask.sum())
    assert got["R"] == R
    # torch on the CPU, in the values' own dtype (a float16 or float32 NaN keeps its payload through an index)
    typed = values.view(VALUE_DTYPES[vb]) if vb in VALUE_DTYPES else values
    assert torch.equal(got["gather"], as_bytes(typed[mask]).reshape(R, W * vb))
    assert torch.equal(got["scatter"], want_scatter(mask, values, source, R))
    # the host restatement
    flags = mask.numpy()
    h_out, h_got = np.zeros((R, W * vb), dtype=np.uint8), np.zeros(tuple(values.shape), dtype=np.uint8)
    assert host_rows(lib_cpu, flags, W, vb, values=values.numpy(), gather_out=h_out, scatter=(values.numpy(), source.numpy()), scatter_out=h_got) == R
    assert np.array_equal(got["gather"].numpy(), h_out) and np.array_equal(got["scatter"].numpy(), h_got)


# ---------------------------------------------------------------------------------------------- the device against the host and torch

@pytest.mark.parametrize("W,vb", DEVICE_ROWS, ids=[f"{w}x{b}" for w, b in DEVICE_ROWS])
def test_device_rows_equal_host_and_torch(ctx, lib_cpu, W, vb):
    for n in DEVICE_SIZES:
        values, source = random_rows(n + W, n, W * vb), random_rows(n + W + 1, n, W * vb)
        for name in PATTERNS:
            mask = torch.from_numpy(pattern(name, n))
            check_against_host_and_torch(ctx, lib_cpu, mask, W, vb, values, source)


# (W, value_bytes, bytes behind the 16-byte boundary): the word the copy may use is 8, 4, 2 or 1 bytes
OFF_BOUNDARY = [(4, 4, 4), (4, 4, 8), (3, 4, 4), (2, 8, 8), (6, 2, 4), (5, 2, 4), (3, 2, 0), (16, 1, 4), (16, 1, 8), (3, 1, 0), (4100, 1, 4), (1025, 4, 4)]


@pytest.mark.parametrize("W,vb,off", OFF_BOUNDARY, ids=[f"{w}x{b}+{o}" for w, b, o in OFF_BOUNDARY])
def test_a_base_off_the_16_byte_boundary(ctx, lib_cpu, W, vb, off):
    """a slice that starts one element (or 4 or 8 bytes: a buffer starts on 4) into its allocation, for every buffer in turn"""
    n = T + 1 if W < 1000 else 4097
    mask = torch.from_numpy(pattern("half", n))
    values, source = random_rows(off + W, n, W * vb), random_rows(off + W + 1, n, W * vb)
    for moved in range(3):
        offsets = tuple(off if k == moved else 0 for k in range(3))
        check_against_host_and_torch(ctx, lib_cpu, mask, W, vb, values, source, offsets=offsets)


def test_the_word_rule_picks_what_the_cases_above_say():
    """the cases of the two tests above do reach every word width: the rule restated (16 bytes when the row and every base are multiples
    of 16, else the largest of 8, 4, 2, 1 that divides them all)"""
    def word(row_bytes, off):
        return next(w for w in (16, 8, 4, 2, 1) if row_bytes % w == 0 and off % w == 0)
    assert {word(W * vb, off) for W, vb, off in OFF_BOUNDARY} == {8, 4, 2, 1}
    assert {word(W * vb, 0) for W, vb in DEVICE_ROWS} == {16, 8, 4, 2, 1}


# ---------------------------------------------------------------------------------------------- slices, and the row-by-row walk

WIDE = [("20_rows_of_1MiB", 20, 1 << 18, 4), ("33000_rows_of_4100", 33000, 1025, 4), ("5_rows_of_2^20+1", 5, (1 << 20) + 1, 1)]


@pytest.mark.parametrize("n,W,vb", [w[1:] for w in WIDE], ids=[w[0] for w in WIDE])
def test_rows_wide_enough_for_several_slices(ctx, lib_cpu, n, W, vb):
    """a tile's bytes pass the slice size many times over, so its chunk is copied by many workgroups; the last case's row holds more than
    2^20 words of one byte, which are walked row by row"""
    assert min(n, T) * W * vb > 4 * 256 * 1024
    mask = torch.from_numpy(pattern("half", n))
    values, source = random_rows(n, n, W * vb), random_rows(n + 1, n, W * vb)
    check_against_host_and_torch(ctx, lib_cpu, mask, W, vb, values, source)


# ---------------------------------------------------------------------------------------------- red zones, and a smaller num_selected

@pytest.mark.parametrize("W,vb", [(3, 4), (256, 4), (3, 1)], ids=["3x4", "256x4", "3x1"])
def test_a_smaller_num_selected_writes_only_that_many_rows(ctx, W, vb):
    """(every call of this file has sentinel rows behind row R of gather_out and row n of scatter_out: device_rows checks them)"""
    n = 3 * T + 5
    mask = torch.from_numpy(pattern("half", n))
    R = int(mask.sum())
    values, source = random_rows(7, n, W * vb), random_rows(8, n, W * vb)
    full = values[mask]
    for limit in (R - 5, R // 2, 1, 0):
        got = device_rows(ctx, mask, W, vb, values, source, limit=limit)
        assert got["R"] == R
        assert torch.equal(got["gather"], full[:limit])
        assert torch.equal(got["scatter"], want_scatter(mask, values, source, limit))


# ---------------------------------------------------------------------------------------------- one call, several outputs

def test_flat_coords_and_rows_from_one_call(ctx):
    n, W, vb = 3 * T + 5 - 1, 5, 4  # (n = 2 x 24578)
    shape = (2, n // 2)
    mask = torch.from_numpy(pattern("half", n))
    values, source = random_rows(9, n, W * vb), random_rows(10, n, W * vb)
    together = device_rows(ctx, mask, W, vb, values, source, flat=True, coords_shape=shape)
    only_rows = device_rows(ctx, mask, W, vb, values, source)
    only_flat = device_rows(ctx, mask, W, vb, values, flat=True, rows=False)
    only_coords = device_rows(ctx, mask, W, vb, values, coords_shape=shape, rows=False)
    assert torch.equal(together["gather"], only_rows["gather"]) and torch.equal(together["scatter"], only_rows["scatter"])
    assert torch.equal(together["flat"], only_flat["flat"]) and torch.equal(together["coords"], only_coords["coords"])
    assert torch.equal(together["flat"], torch.nonzero(mask)[:, 0])
    assert torch.equal(together["coords"], torch.nonzero(mask.reshape(shape)))
    assert torch.equal(together["gather"], values[mask])


# ---------------------------------------------------------------------------------------------- mask_index, mask_index_put

# (id, x's shape, mask.dim(), dtype)
INDEX_CASES = [("1d_mask1", (4099,), 1, torch.float32), ("2d_mask1", (T + 1, 7), 1, torch.float16), ("2d_mask2", (37, 301), 2, torch.int64),
               ("4d_mask1", (300, 3, 5, 2), 1, torch.uint8), ("4d_mask2", (30, 11, 5, 2), 2, torch.float32), ("4d_mask4", (6, 5, 7, 3), 4, torch.float16),
               ("complex128_mask1", (4099, 3), 1, torch.complex128), ("complex128_mask2", (41, 5), 2, torch.complex128),
               ("float64_mask1", (4099, 2), 1, torch.float64), ("bool_mask1", (4099, 3), 1, torch.bool),
               ("0dim_mask", (5, 3), 0, torch.float32), ("0dim_both", (), 0, torch.float32),
               ("empty_N", (0, 5), 1, torch.float32), ("zero_tail", (7, 0, 3), 1, torch.float32), ("zero_tail_mask2", (4, 3, 0), 2, torch.int64)]


def random_tensor(seed, shape, dtype):
    """random bytes as a tensor of dtype (NaNs with payloads among the floats); bool from bytes that are 0 or 1"""
    count = int(np.prod(shape))
    if dtype == torch.bool:
        return (random_rows(seed, 1, count).reshape(shape) & 1).bool()
    size = torch.empty(0, dtype=dtype).element_size()
    return random_rows(seed, 1, count * size).reshape(-1).view(dtype).reshape(shape)


def masks_for(shape, dims):
    if dims == 0:
        return [torch.tensor(True), torch.tensor(False)]
    lead = shape[:dims]
    count = int(np.prod(lead))
    return [torch.from_numpy(pattern(name, count)).reshape(lead) for name in (["half", "none", "all"] if count else ["none"])]


def torch_put(x, m, values):
    """torch.index_put(x, (m,), values) on the CPU.  Under a 0-dim mask the functional form trips an internal assertion of torch's CPU
    kernel for every values but a scalar, so there the reference is the assignment it stands for, y = x.clone(); y[m] = values."""
    if m.dim():
        return torch.index_put(x, (m,), values)
    y = x.clone()
    y[m] = values
    if values.dim() == 0 and x.dim():
        assert torch.equal(as_bytes(y), as_bytes(torch.index_put(x, (m,), values)))
    return y


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(as_bytes(a), as_bytes(b))


@pytest.mark.parametrize("shape,dims,dtype", [c[1:] for c in INDEX_CASES], ids=[c[0] for c in INDEX_CASES])
def test_mask_index_and_put_against_torch(dev, shape, dims, dtype):
    x = random_tensor(1, shape, dtype)
    tail = shape[dims:]
    for m in masks_for(shape, dims):
        want = x[m]
        got = vrs.mask_index(x.to(dev), m.to(dev))
        assert got.device.type == "cuda" and got.is_contiguous() and same_bits(got.cpu(), want), (shape, dims)
        R = want.shape[0]
        exact = random_tensor(2, (R, *tail), dtype)
        candidates = [random_tensor(3, (), dtype), random_tensor(4, tail, dtype), random_tensor(5, (1, *tail), dtype), exact]
        if R:
            candidates.append(torch.cat([exact, exact], 0)[::2])  # [R, *tail], not contiguous
        for values in candidates:
            want_put = torch_put(x, m, values)
            got_put = vrs.mask_index_put(x.to(dev), m.to(dev), values.to(dev))
            assert got_put.is_contiguous() and same_bits(got_put.cpu(), want_put), (shape, dims, tuple(values.shape))


def test_tensors_that_are_not_contiguous(dev):
    base = random_tensor(6, (301, 2 * 37), torch.float32)
    g = base.to(dev)
    mbase = torch.from_numpy(pattern("half", 2 * 37))
    views = [(lambda t: t.t(), mbase), (lambda t: t.t()[::2], mbase[::2]), (lambda t: t[:, ::2], torch.from_numpy(pattern("half", 301)))]
    for view, m in views:
        x, gx, gm = view(base), view(g), m.to(dev)  # (the same view of the same bytes on both sides)
        assert not x.is_contiguous() and gx.stride() == x.stride() and gx.shape == x.shape
        assert same_bits(vrs.mask_index(gx, gm).cpu(), x[m])
        values = random_tensor(7, x[m].shape, torch.float32)
        assert same_bits(vrs.mask_index_put(gx, gm, values.to(dev)).cpu(), torch.index_put(x, (m,), values))


def test_put_refusals_that_need_R(dev):
    x, m = torch.ones(6, 3, device=dev), torch.tensor([True, False, True, True, False, False], device=dev)
    with pytest.raises(RuntimeError):
        vrs.mask_index_put(x, m, torch.ones(2, 3, device=dev))  # (R is 3)
    with pytest.raises(RuntimeError):
        torch.index_put(x.cpu(), (m.cpu(),), torch.ones(2, 3))
    assert torch.equal(vrs.mask_index_put(x, m, 2.5), torch.index_put(x, (m,), torch.tensor(2.5, device=dev)))


def test_past_2_32_bytes_and_words(dev):
    """uint8 [257, 2^24 + 1] (4.3 GB) under a random half of a 1-D mask: the odd row length forces one-byte words, so the one chunk's
    span holds more than 2^32 words and byte offsets pass 2^32; compared on the device against torch's own x[mask] and index_put"""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 16 << 30:
        pytest.skip(f"needs 16 GB of free device memory (x, the result and torch's own twice over), the device has {free >> 30} GB free")
    n, row = 257, (1 << 24) + 1
    x = torch.randint(0, 256, (n, row), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = torch.from_numpy(pattern("half", n)).to(dev)
    m[-1] = True  # (the last row, behind byte 2^32, moves)
    got = vrs.mask_index(x, m)
    assert got.shape[0] == int(m.sum()) and got.numel() > 1 << 31
    want = x[m]
    assert torch.equal(got, want)
    del want
    values = got.flip(0)
    del got
    put = vrs.mask_index_put(x, m, values)
    assert torch.equal(put, torch.index_put(x, (m,), values))
