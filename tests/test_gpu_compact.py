"""Ordered stream compaction on the device: vrs_compact_count + vrs_compact_emit against the host restatement (vrs_compact_host) and
against torch on the CPU copy of the same input, bit for bit -- every dtype, sizes around every edge of a wave, a workgroup, a tile and
the carries' block, the flag patterns that put survivors on those edges; then vrs.nonzero / argwhere / where / count_nonzero /
masked_select / masked_scatter against torch's CPU results.  T = its minimum throughout (so that tiles and carries appear at small
sizes), except for the index-width test, which runs at the default."""
import ctypes

import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for

from .test_compact_cpu import CODES, DTYPES, bits, host_compact, name_of, specials, truth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T0 = capi.COMPACT_TILE_ELEMS_MIN
CARRY_BLOCK = capi.COMPACT_CARRY_BLOCK  # tiles the carries take per step: one workgroup, four per lane
SMALL = [1, 63, 64, 65, 255, 256, 257, T0 - 1, T0, T0 + 1, 3 * T0 + 17]
# around the carries' block: one tile fewer, exactly one block, one tile more (a second step for a tile of one element)
CARRY_EDGES = [(CARRY_BLOCK - 1) * T0, CARRY_BLOCK * T0, CARRY_BLOCK * T0 + 1]
PATTERNS = ["none", "all", "first", "last", "tile_edges", "alternating", "random_1", "random_50", "random_99", "runs_1000"]
SIZES = {"small": SMALL, "carry_minus": CARRY_EDGES[:1], "carry_exact": CARRY_EDGES[1:2], "carry_plus": CARRY_EDGES[2:]}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    c.setTuning(capi.VRS_TUNE_COMPACT_TILE_ELEMS, T0)
    yield c
    c.setTuning(capi.VRS_TUNE_COMPACT_TILE_ELEMS, capi.COMPACT_TILE_ELEMS_DEFAULT)


_masks = {}


def pattern(name, n):
    """the bool mask of a flag pattern over n elements (made once per size and shared; never written)"""
    if (name, n) in _masks:
        return _masks[name, n]
    i = torch.arange(n)
    if name == "none":
        m = torch.zeros(n, dtype=torch.bool)
    elif name == "all":
        m = torch.ones(n, dtype=torch.bool)
    elif name == "first":
        m = i == 0
    elif name == "last":
        m = i == n - 1
    elif name == "tile_edges":  # only the last element of a tile together with the first of the next
        m = ((i % T0 == T0 - 1) & (i + 1 < n)) | ((i % T0 == 0) & (i > 0))
    elif name == "alternating":
        m = i % 2 == 1
    elif name.startswith("random_"):
        g = torch.Generator().manual_seed(n % 1000 + int(name[7:]))
        m = torch.rand(n, generator=g) < int(name[7:]) / 100
    else:  # runs of 1000 set, 1000 clear: T0 is no multiple of 1000, so they straddle the tiles' boundaries
        m = (i // 1000) % 2 == 0
    _masks[name, n] = m
    return m


def dress(mask, dtype):
    """a tensor of dtype that is nonzero exactly where mask is set: every kind of nonzero (NaNs of both signs, subnormals, infinities,
    the minimum) and both zeros"""
    s = specials(dtype)
    t = torch.from_numpy(truth(s))
    nz, z = s[t], s[~t]
    n = mask.numel()
    cycle = lambda v: bits(v).repeat(-(-n // v.numel()))[:n]  # noqa: E731
    return torch.where(mask.reshape(-1), cycle(nz), cycle(z)).view(dtype).reshape(mask.shape)


def device_compact(c, x):
    """vrs_compact_count and vrs_compact_emit themselves on the 1-D CPU tensor x: (R, flat, coords as [R, 1]) back on the CPU.  The
    scratch and the outputs hold garbage on entry."""
    d = torch.device("cuda", 0)
    n = x.numel()
    need = capi.query_u64("vrs_compact_scratch_bytes", n, c.tuning[capi.VRS_TUNE_COMPACT_TILE_ELEMS])
    flags = x.contiguous().to(d)
    scratch = torch.full((need,), 0xAB, dtype=torch.uint8, device=d)
    got = ctypes.c_uint64(1 << 40)
    with buffers(c, flags, scratch) as (f, s):
        c.check(c.lib.vrs_compact_count(c.handle, f, n, CODES[x.dtype], s, None, ctypes.byref(got)))
    R = got.value
    assert R <= n
    flat = torch.full((R,), 0x5B5B, dtype=torch.int64, device=d)
    coords = torch.full((R, 1), 0x5B5B, dtype=torch.int64, device=d)
    if R:
        o = capi.CompactOutputs()
        o.num_selected, o.coords_layout, o.ndim = R, capi.VRS_COMPACT_ROWS, 1
        o.shape = (ctypes.c_uint32 * 8)(n)
        with buffers(c, flags, scratch, flat, coords) as (f, s, fl, co):
            o.flat, o.coords = fl.value, co.value
            c.check(c.lib.vrs_compact_emit(c.handle, f, n, CODES[x.dtype], s, ctypes.byref(o)))
    return R, flat.cpu(), coords.cpu()


@pytest.mark.parametrize("sizes", list(SIZES), ids=list(SIZES))
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_device_equals_host_and_torch(ctx, lib_cpu, dtype, sizes):
    for n in SIZES[sizes]:
        for name in PATTERNS:
            if name == "tile_edges" and n <= T0:
                continue  # (there is no next tile)
            x = dress(pattern(name, n), dtype)
            want = torch.nonzero(x)
            R, flat, coords = device_compact(ctx, x)
            assert R == want.shape[0], (n, name)
            assert torch.equal(coords, want), (n, name)
            assert torch.equal(flat, want[:, 0]), (n, name)
            host = host_compact(lib_cpu, x, flat=True)
            assert host["count"] == R and torch.equal(host["flat"], flat), (n, name)


@pytest.fixture(scope="module")
def lib_cpu():
    return capi.load_library()


# ---------------------------------------------------------------------------------------------- nonzero, argwhere, where, count_nonzero

SHAPES = [(), (0,), (5, 0, 3), (1,), (4097,), (3, 4099), (17, 5, 33), (2, 3, 1, 4, 2, 1, 3, 5), (2, 1, 3, 2, 1, 2, 3, 2, 2)]


def shaped_inputs():
    """(id, contiguous CPU tensor, the view to take of it) of every shape, and of a transposed, a strided and an expanded view"""
    same = lambda t: t  # noqa: E731
    out = []
    for k, shape in enumerate(SHAPES):
        n = 1
        for s in shape:
            n *= s
        dtype = DTYPES[k % len(DTYPES)]
        out.append(("x".join(map(str, shape)) or "scalar", dress(pattern("random_50", n), dtype).reshape(shape), same))
    base = dress(pattern("random_50", 3 * 4099), torch.float32).reshape(3, 4099)
    out.append(("transposed", base, lambda t: t.t()))
    out.append(("strided", base, lambda t: t[:, ::3]))
    out.append(("expanded", dress(pattern("random_50", 4099), torch.int16).reshape(1, 4099), lambda t: t.expand(3, 4099)))
    out.append(("scalar_zero", torch.tensor(-0.0), same))
    return out


INPUTS = shaped_inputs()


@pytest.mark.parametrize("base,view", [(b, v) for _, b, v in INPUTS], ids=[i for i, _, _ in INPUTS])
def test_nonzero_argwhere_where_count_nonzero(ctx, dev, base, view):
    x, g = view(base), view(base.to(dev))  # (the same view of the same bytes on both sides)
    assert g.stride() == x.stride() and g.shape == x.shape
    rows = vrs.nonzero(g)
    assert rows.dtype == torch.int64 and rows.device == g.device
    assert torch.equal(rows.cpu(), torch.nonzero(x))
    assert torch.equal(vrs.argwhere(g).cpu(), torch.argwhere(x))
    for ours, theirs in ((vrs.nonzero(g, as_tuple=True), torch.nonzero(x, as_tuple=True)), (vrs.where(g), torch.where(x))):
        assert isinstance(ours, tuple) and len(ours) == len(theirs)
        for a, b in zip(ours, theirs):
            assert a.is_contiguous() and a.dtype == torch.int64 and torch.equal(a.cpu(), b)
    count = vrs.count_nonzero(g)
    assert count.dim() == 0 and count.dtype == torch.int64 and count.device == g.device
    assert count.item() == torch.count_nonzero(x).item()


# ---------------------------------------------------------------------------------------------- masked_select, masked_scatter

VALUE_DTYPES = [torch.uint8, torch.bfloat16, torch.float32, torch.int64]  # 1, 2, 4 and 8 bytes
ROWS_, COLS_ = 37, 301


def values_of(dtype, seed):
    """[ROWS_, COLS_] of dtype with NaN payloads, both zeros and the extremes in it"""
    n = ROWS_ * COLS_
    g = torch.Generator().manual_seed(seed)
    s = specials(dtype)
    v = s[torch.randint(0, s.numel(), (n,), generator=g)]
    if dtype == torch.float32:  # NaNs with payloads of their own
        raw = bits(v)
        nan = torch.isnan(v)
        raw[nan] = raw[nan] | torch.randint(1, 1 << 22, (int(nan.sum()),), generator=g, dtype=torch.int32)
        v = raw.view(dtype)
        assert torch.isnan(v).sum() == nan.sum() > 0
    return v.reshape(ROWS_, COLS_)


def masks():
    g = torch.Generator().manual_seed(9)
    return {"full": torch.rand(ROWS_, COLS_, generator=g) < 0.5, "row": torch.rand(1, COLS_, generator=g) < 0.5,
            "column": torch.rand(ROWS_, 1, generator=g) < 0.5, "all_false": torch.zeros(ROWS_, COLS_, dtype=torch.bool),
            "all_true": torch.ones(ROWS_, COLS_, dtype=torch.bool)}


MASKS = masks()


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("dtype", VALUE_DTYPES, ids=name_of)
def test_masked_select(ctx, dev, dtype, mask):
    x, m = values_of(dtype, 11), MASKS[mask]
    got = vrs.masked_select(x.to(dev), m.to(dev))
    want = torch.masked_select(x, m)
    assert got.dtype == dtype and got.dim() == 1 and got.device.type == "cuda"
    assert torch.equal(bits(got.cpu()), bits(want))


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("dtype", VALUE_DTYPES, ids=name_of)
def test_masked_scatter(ctx, dev, dtype, mask):
    x, m = values_of(dtype, 12), MASKS[mask]
    R = int(torch.broadcast_to(m, x.shape).sum())
    longer = values_of(dtype, 13).reshape(-1)
    longer = torch.cat([longer, longer[:5]])  # (five more than any mask sets)
    for source in (longer[:R], longer):
        got = vrs.masked_scatter(x.to(dev), m.to(dev), source.to(dev))
        want = torch.masked_scatter(x, m, source)
        assert got.dtype == dtype and got.shape == want.shape
        assert torch.equal(bits(got.cpu()), bits(want))
        # where the mask is false the result is the input bit for bit, -0.0 and NaN payloads included
        keep = ~torch.broadcast_to(m, x.shape)
        assert torch.equal(bits(got.cpu())[keep], bits(x)[keep])
    if R:
        with pytest.raises(RuntimeError):
            vrs.masked_scatter(x.to(dev), m.to(dev), longer[:R - 1].to(dev))
        with pytest.raises(RuntimeError):
            torch.masked_scatter(x, m, longer[:R - 1])  # (torch on the CPU refuses the same)


def test_masked_scatter_broadcasts_the_input_too(ctx, dev):
    x, m = values_of(torch.float32, 14)[:1], MASKS["full"]
    source = values_of(torch.float32, 15)
    got = vrs.masked_scatter(x.to(dev), m.to(dev), source.to(dev))
    assert torch.equal(bits(got.cpu()), bits(torch.masked_scatter(x, m, source)))


# ---------------------------------------------------------------------------------------------- other checks

def test_two_runs_give_identical_outputs(ctx, dev):
    x = dress(pattern("random_50", 3 * T0 + 17), torch.float32).to(dev)
    v = torch.arange(x.numel(), dtype=torch.int64, device=dev)
    first = (vrs.nonzero(x), vrs.masked_select(v, x != 0), vrs.count_nonzero(x))
    second = (vrs.nonzero(x), vrs.masked_select(v, x != 0), vrs.count_nonzero(x))
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_interleaved_with_cumsum_and_sort(ctx, dev):
    """scratch and stream reuse: the three families on one context, one after the other, twice"""
    x = dress(pattern("random_50", 3 * T0 + 17), torch.int32)
    f = torch.rand(50000, generator=torch.Generator().manual_seed(3))
    gx, gf = x.to(dev), f.to(dev)
    for _ in range(2):
        rows = vrs.nonzero(gx)
        sums = vrs.cumsum(gx, 0)
        values, indices = vrs.sort(gf)
        picked = vrs.masked_select(gf, gf > 0.5)
        assert torch.equal(rows.cpu(), torch.nonzero(x))
        assert torch.equal(sums.cpu(), torch.cumsum(x, 0))
        want = torch.sort(f, stable=True)
        assert torch.equal(values.cpu(), want.values) and torch.equal(indices.cpu(), want.indices)
        assert torch.equal(picked.cpu(), f[f > 0.5])
    stats = vrs.compact_stats(ctx)
    assert stats["count_calls"] >= 4 and stats["emit_calls"] >= 4 and stats["elements"] >= 4 * 50000


def test_index_width_past_2_31(dev):
    """n = 2^31 + 4097 bool at the default T: positions and tile starts pass 2^31 (about 2 GB, read twice, four survivors)"""
    n = 2 ** 31 + 4097
    at = [0, 2 ** 31 - 1, 2 ** 31, n - 1]
    x = torch.zeros(n, dtype=torch.bool, device=dev)
    x[torch.tensor(at, device=dev)] = True
    assert context_for(dev).tuning.get(capi.VRS_TUNE_COMPACT_TILE_ELEMS, capi.COMPACT_TILE_ELEMS_DEFAULT) == capi.COMPACT_TILE_ELEMS_DEFAULT
    assert vrs.nonzero(x).cpu().tolist() == [[p] for p in at]
    assert vrs.count_nonzero(x).item() == 4
    two_d = x[:2 ** 31].view(2 ** 15, 2 ** 16)
    assert vrs.nonzero(two_d).cpu().tolist() == [[0, 0], [2 ** 15 - 1, 2 ** 16 - 1]]
