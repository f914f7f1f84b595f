"""The torch.sort drop-in on the device (vkradixsort_amd.sort / sort_values / argsort over vrs_sort_rank_keys, the segmented sorts and
vrs_sort_restore): values bit for bit (viewed as integers) and indices index for index against torch.sort(x.cpu(), stable=True), and
against torch.sort on the device where there are no NaNs or zeros.  The 64-bit segmented sorts through the C ABI against numpy's stable
argsort per segment."""

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INTS = [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64]
FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
# bit patterns of every float's special values: ±0, ±inf, NaNs of either sign with several payloads (quiet and signalling), denormals
SPECIALS = {
    torch.float16: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01, 0xFFFF, 0x0001, 0x8001, 0x03FF],
    torch.bfloat16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81, 0xFFFF, 0x0001, 0x8001, 0x007F],
    torch.float32: [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF, 0x00000001,
                    0x80000001, 0x007FFFFF],
    torch.float64: [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001,
                    (1 << 64) - 1, 1, (1 << 63) | 1, 0x000FFFFFFFFFFFFF],
}


def bits(t):
    return t.view(BITS[t.dtype]) if t.dtype in BITS else t


def specials(dtype):
    w = BITS[dtype]
    nb = torch.finfo(dtype).bits
    vals = [v - (1 << nb) if v >= 1 << (nb - 1) else v for v in SPECIALS[dtype]]
    return torch.tensor(vals, dtype=w).view(dtype)


def make(dtype, shape, g, special=True):
    """Random values with many ties; floats with every special value scattered in; ints with their extremes."""
    n = int(np.prod(shape)) if len(shape) else 1
    if dtype.is_floating_point:
        x = (torch.randint(-40, 40, (n,), generator=g).to(torch.float64) / 4).to(dtype)
        if special and n:
            sp = specials(dtype)
            at = torch.randint(0, n, (min(n, 3 * sp.numel()),), generator=g)
            x[at] = sp.repeat(3)[:at.numel()]
    else:
        info = torch.iinfo(dtype)
        x = torch.randint(max(info.min, -60), min(info.max, 60), (n,), generator=g, dtype=torch.int64).to(dtype)
        if n:
            x[torch.randint(0, n, (4,), generator=g)] = torch.tensor([info.min, info.max, info.min, info.max], dtype=torch.int64).to(dtype)
    return x.reshape(shape)


def check(x, dim=-1, descending=False, device_ref=False):
    ref = torch.sort(x.cpu(), dim=dim, descending=descending, stable=True)
    out = vrs.sort(x, dim=dim, descending=descending)
    assert isinstance(out, torch.return_types.sort)
    assert out.values.dtype == x.dtype and out.indices.dtype == torch.int64
    assert out.values.shape == x.shape and out.indices.shape == x.shape
    assert torch.equal(bits(out.values.cpu()), bits(ref.values))
    assert torch.equal(out.indices.cpu(), ref.indices)
    v = vrs.sort_values(x, dim=dim, descending=descending)
    assert torch.equal(bits(v.cpu()), bits(ref.values))
    i = vrs.argsort(x, dim=dim, descending=descending)
    assert torch.equal(i.cpu(), ref.indices)
    if device_ref:
        d = torch.sort(x, dim=dim, descending=descending, stable=True)
        assert torch.equal(bits(out.values), bits(d.values)) and torch.equal(out.indices, d.indices)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_every_dtype(dtype, descending):
    g = torch.Generator().manual_seed(11)
    for shape in [(5000,), (37, 1000), (300, 7)]:
        check(make(dtype, shape, g).to(DEV), descending=descending)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_device_torch_agrees_without_nan_or_zero(dtype, descending):
    g = torch.Generator().manual_seed(12)
    x = make(dtype, (64, 777), g, special=False)
    if dtype.is_floating_point:
        x = torch.where(x == 0, torch.ones_like(x), x)
    check(x.to(DEV), descending=descending, device_ref=True)


@pytest.mark.parametrize("dtype", [torch.int8, torch.uint8, torch.int16, torch.float16, torch.bfloat16], ids=str)
def test_a_view_that_starts_off_a_4_byte_boundary(dtype):
    """x[1:] of a 1- or 2-byte dtype is contiguous but not 4-byte aligned, which vrs_buffer_wrap refuses: the drop-in raised 'device_ptr
    must be 4-byte aligned' (found by tools/fuzz_ops.py) where it documents any shape and strides"""
    g = torch.Generator().manual_seed(13)
    base = make(dtype, (4269,), g).to(DEV)
    for by in (1, 2, 3):
        assert base[by:].is_contiguous() and (base[by:].data_ptr() % 4 != 0 or by * base.element_size() % 4 == 0)
        check(base[by:])
        check(base[by:by + 4200].view(100, 42), dim=0, descending=True)


def test_torch_order_of_specials():
    x = torch.tensor([1, float("nan"), -0.0, 0.0, -float("nan"), -1, 0.0, -0.0, float("inf"), -float("inf")], device=DEV)
    assert vrs.argsort(x).tolist() == [9, 5, 2, 3, 6, 7, 0, 8, 1, 4]
    for dtype in FLOATS:
        sp = specials(dtype)
        for desc in (False, True):
            check(sp.to(DEV), descending=desc)
            check(sp.flip(0).repeat(50).to(DEV), descending=desc)


# every tier boundary of the 64-bit segmented sorts (wave 896, block-small 4096, block 6656 pairs / 13312 keys), a few of the
# 32-bit ones, and the one-call threshold (2^20): rows of that length, several rows so that the segmented sort runs
@pytest.mark.parametrize("length", [2, 255, 256, 257, 895, 896, 897, 1789, 1790, 4095, 4096, 4097, 6655, 6656, 6657, 13311, 13312, 13313,
                                    14333, 14334, 40000])
@pytest.mark.parametrize("dtype", [torch.int64, torch.float64, torch.int32, torch.float32], ids=str)
def test_row_lengths_at_tier_boundaries(dtype, length):
    g = torch.Generator().manual_seed(length)
    x = make(dtype, (3, length), g).to(DEV)
    check(x)
    check(x, descending=True)


@pytest.mark.parametrize("length", [(1 << 20) - 1, 1 << 20, (1 << 20) + 1])
@pytest.mark.parametrize("dtype", [torch.int64, torch.float64], ids=str)
def test_row_lengths_at_one_call_threshold(dtype, length):
    g = torch.Generator().manual_seed(length)
    x = make(dtype, (2, length), g).to(DEV)
    if dtype.is_floating_point:
        x[0] = torch.randn(length, generator=g, dtype=dtype).to(DEV)  # (one row of wide keys: all eight digits vary)
    else:
        x[0] = torch.randint(-(1 << 62), 1 << 62, (length,), generator=g, dtype=torch.int64).to(DEV)
    check(x)


def test_global_tier_counts():
    ctx = vrs._torch.context_for(DEV)
    before = vrs.segmented_stats(ctx)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-(1 << 40), 1 << 40, (8, 1 << 17), generator=g, dtype=torch.int64).to(DEV)
    check(x, device_ref=True)
    after = vrs.segmented_stats(ctx)
    assert after["global"] - before["global"] >= 8  # sort and argsort: pairs; sort_values: bare keys


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32, torch.bfloat16, torch.int8], ids=str)
def test_shapes_and_dims(dtype):
    g = torch.Generator().manual_seed(3)
    x = make(dtype, (6, 50, 9), g).to(DEV)
    for dim in (0, 1, 2, -1, -2, -3):
        check(x, dim=dim)
        check(x, dim=dim, descending=True)
    y = make(dtype, (40, 33), g).to(DEV)
    check(y, dim=0)
    check(y, dim=1)
    check(y.t(), dim=1)                    # non-contiguous
    check(y[:, ::2], dim=-1)               # strided
    check(y[::3, 1:], dim=0, descending=True)
    check(make(dtype, (1000,), g).to(DEV)[::7])


def test_empty_short_rows_and_scalars():
    for dtype in (torch.int64, torch.float32, torch.float16):
        for shape in [(0,), (0, 5), (5, 0), (4, 0, 3)]:
            x = torch.empty(shape, dtype=dtype, device=DEV)
            for dim in range(-len(shape), len(shape)):
                check(x, dim=dim)
        g = torch.Generator().manual_seed(1)
        check(make(dtype, (100, 1), g).to(DEV))                 # rows of length 1
        check(make(dtype, (1, 100), g).to(DEV), dim=0)
        check(make(dtype, (1,), g).to(DEV))
        s = make(dtype, (), g).to(DEV)                          # 0-d
        out = vrs.sort(s)
        ref = torch.sort(s.cpu())
        assert out.values.shape == () and torch.equal(bits(out.values.cpu()), bits(ref.values)) and out.indices.item() == 0
        assert vrs.argsort(s, dim=0).item() == 0


def test_errors():
    with pytest.raises(vrs.VrsError):
        vrs.sort(torch.ones(4, dtype=torch.bool, device=DEV))
    with pytest.raises(vrs.VrsError):
        vrs.sort(torch.ones(4, dtype=torch.complex64, device=DEV))
    with pytest.raises(vrs.VrsError):
        vrs.sort(torch.ones(4, dtype=torch.float32))  # CPU
    with pytest.raises(IndexError):
        vrs.sort(torch.ones(4, device=DEV), dim=1)


def test_single_row_1e8_int64_with_indices():
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randint(-(1 << 62), 1 << 62, (10 ** 8,), generator=g, dtype=torch.int64, device=DEV)
    x[::1000] = 12345  # ties
    out = vrs.sort(x)
    ref = torch.sort(x, stable=True)
    assert torch.equal(out.values, ref.values) and torch.equal(out.indices, ref.indices)


# ---- the 64-bit segmented sorts through the C ABI

@pytest.fixture(scope="module")
def ctx():
    c = vrs.GPUContext(0)
    c.init()
    c.setTuning(capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, 1 << 16)  # the one-call tier at a size the test can afford
    yield c
    c.shutdown()


def run_u64(c, keys, offsets, vals=None):
    n, S = keys.size, offsets.size - 1
    B = vrs.Buffer.BufferSettings
    bufs = [vrs.Buffer.fillDeviceWithStagingBuffer(c, B(8 * n), keys), vrs.Buffer(c, B(8 * n)),
            vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * (S + 1)), offsets.astype(np.uint32))]
    lib = c.lib
    if vals is not None:
        bufs += [vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * n), vals), vrs.Buffer(c, B(4 * n))]
        c.check(lib.vrs_sort_segments_pairs_u64(c.handle, bufs[0].handle, bufs[1].handle, bufs[3].handle, bufs[4].handle, n,
                                                bufs[2].handle, S))
    else:
        c.check(lib.vrs_sort_segments_u64(c.handle, bufs[0].handle, bufs[1].handle, n, bufs[2].handle, S))
    ok = np.empty_like(keys)
    bufs[0].downloadWithStagingBuffer(ok)
    ov = None
    if vals is not None:
        ov = np.empty_like(vals)
        bufs[3].downloadWithStagingBuffer(ov)
    for b in bufs:
        b.release()
    return ok, ov


def reference_u64(keys, vals, ranges):
    rk, rv = keys.copy(), None if vals is None else vals.copy()
    for b, e in ranges:
        order = np.argsort(keys[b:e], kind="stable")
        rk[b:e] = keys[b:e][order]
        if vals is not None:
            rv[b:e] = vals[b:e][order]
    return rk, rv


@pytest.mark.parametrize("pairs", [False, True])
def test_c_abi_ragged_segments_u64(ctx, pairs):
    rng = np.random.default_rng(9)
    lengths = [0, 1, 2, 300, 896, 897, 3000, 4097, 6656, 6657, 13312, 13313, 70000, 1, 0, 500]
    head = 17  # in front of offsets[0]: never touched
    offs = np.concatenate([[0], np.cumsum(lengths)]) + head
    n = int(offs[-1]) + 29  # behind offsets[S]: never touched
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    keys[head: head + 5000] &= np.uint64(0xFF00000000000FFF)  # few varying bits
    keys[head + 5000: head + 9000] = np.uint64(0xDEADBEEF00000000) | (keys[head + 5000: head + 9000] % np.uint64(7))  # ties
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    ok, ov = run_u64(ctx, keys, offs, vals)
    rk, rv = reference_u64(keys, vals, list(zip(offs[:-1], offs[1:])))
    assert np.array_equal(ok, rk)
    if pairs:
        assert np.array_equal(ov, rv)


@pytest.mark.parametrize("pairs", [False, True])
def test_c_abi_malformed_offsets_u64(ctx, pairs):
    rng = np.random.default_rng(10)
    n = 20000
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    # a segment ending before it begins (empty at its begin), one cut at n, and ones beyond n (empty at n)
    offs = np.array([100, 1000, 900, 900, 5000, 19990, 25000, 30000, 0xFFFFFFFF], dtype=np.uint64)
    ok, ov = run_u64(ctx, keys, offs.astype(np.uint32), vals)
    rk, rv = reference_u64(keys, vals, [(5000, 19990), (19990, n)])
    # [100, 1000) and [900, 5000) overlap: their union's contents are unspecified; the rest is exact and nothing outside is touched
    assert np.array_equal(ok[:100], keys[:100]) and np.array_equal(ok[5000:], rk[5000:])
    if pairs:
        assert np.array_equal(ov[5000:], rv[5000:])


def test_c_abi_rejects_bad_arguments(ctx):
    lib = ctx.lib
    B = vrs.Buffer.BufferSettings
    small, offs = vrs.Buffer(ctx, B(8 * 10)), vrs.Buffer(ctx, B(8))
    assert lib.vrs_sort_segments_u64(ctx.handle, small.handle, small.handle, 11, offs.handle, 1) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_rank_keys(ctx.handle, small.handle, 10, 3, capi.VRS_SORT_INT32, 0, small.handle, None) == \
        capi.VRS_ERROR_INVALID_ARGUMENT  # 10 is not a whole number of rows of 3
    assert lib.vrs_sort_rank_keys(ctx.handle, small.handle, 10, 10, 42, 0, small.handle, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_rank_keys(ctx.handle, small.handle, 10, 10, capi.VRS_SORT_INT32, 4, small.handle, None) == \
        capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_restore(ctx.handle, small.handle, small.handle, None, 10, 10, capi.VRS_SORT_FLOAT32, 0, small.handle, None) == \
        capi.VRS_ERROR_INVALID_ARGUMENT  # a float's values need positions
    assert lib.vrs_sort_restore(ctx.handle, None, small.handle, None, 10, 10, capi.VRS_SORT_INT32, 0, None, small.handle) == \
        capi.VRS_ERROR_INVALID_ARGUMENT  # indices need positions
    small.release()
    offs.release()
