"""Segmented sorts on the device (vrs_sort_segments_u32 / _pairs_u32, vkradixsort_amd.sort_rows), every result against numpy per
segment: np.sort for keys, a gather by np.argsort(kind="stable") for pairs."""
import ctypes

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

pytestmark = pytest.mark.gpu

THR = 1 << 16  # VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS of the test contexts: the one-call tier at a size the tests can afford
SENTINEL = np.uint32(0xA5A5A5A5)


@pytest.fixture(scope="module")
def ctx():
    c = vrs.GPUContext(0)
    c.init()
    c.setTuning(capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, THR)
    yield c
    c.shutdown()


def reference(keys, offsets, vals=None):
    """Each segment [offsets[i], offsets[i+1]) of ascending offsets sorted (pairs: stably by key); everything else as it was."""
    lo, hi = int(offsets[0]), int(offsets[-1])
    lengths = np.diff(offsets.astype(np.int64))
    seg = np.repeat(np.arange(lengths.size, dtype=np.uint64), lengths)
    order = np.argsort((seg << np.uint64(32)) | keys[lo:hi].astype(np.uint64), kind="stable")
    rk = keys.copy()
    rk[lo:hi] = keys[lo:hi][order]
    if vals is None:
        return rk, None
    rv = vals.copy()
    rv[lo:hi] = vals[lo:hi][order]
    return rk, rv


def stats(c):
    return np.array(list(vrs.segmented_stats(c).values()), dtype=np.int64)


def host_tiers(lib, offsets, n, pairs, min_keys):
    counts = np.zeros(4, dtype=np.int64)
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    for b, e in zip(offsets[:-1], offsets[1:]):
        assert lib.vrs_segment_tier_for(int(b), int(e), n, pairs, min_keys, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == 0
        counts[t.value] += 1
    return counts


def run(c, keys, offsets, vals=None):
    """Uploads, sorts the segments, downloads; returns (keys, values)."""
    n, S = keys.size, offsets.size - 1
    B = vrs.Buffer.BufferSettings
    bufs = [vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * n), keys), vrs.Buffer(c, B(4 * n)),
            vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * (S + 1)), offsets.astype(np.uint32))]
    if vals is not None:
        bufs += [vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * n), vals), vrs.Buffer(c, B(4 * n))]
        vrs.sort_segments(c, bufs[0], bufs[1], bufs[2], n, S, values=bufs[3], values_tmp=bufs[4])
    else:
        vrs.sort_segments(c, bufs[0], bufs[1], bufs[2], n, S)
    ok = np.empty_like(keys)
    bufs[0].downloadWithStagingBuffer(ok)
    ov = None
    if vals is not None:
        ov = np.empty_like(vals)
        bufs[3].downloadWithStagingBuffer(ov)
    for b in bufs:
        b.release()
    return ok, ov


def distribution(name, rng, n):
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return {
        "uniform": u,
        "24bit": u & np.uint32(0xFFFFFF),
        "duplicates": (u % np.uint32(16)) * np.uint32(0x01010101),
        "equal": np.full(n, 0xDEADBEEF, dtype=np.uint32),
        "sorted": np.sort(u),
        "reverse": np.sort(u)[::-1].copy(),
        "bit31": (u & np.uint32(1)) << np.uint32(31),
    }[name]


BOUNDARY_LENGTHS = [0, 1, 2, 255, 256, 257, 1788, 1789, 1790, 4095, 4096, 4097, 13311, 13312, 13313, 14332, 14333, 14334, 40000,
                    THR - 1, THR, THR + 1]


def boundary_layout(lead, tail):
    """offsets of the boundary lengths with empty segments between them, starting at `lead`; n leaves `tail` elements behind"""
    lengths = []
    for L in BOUNDARY_LENGTHS:
        lengths += [L, 0]
    offsets = lead + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return offsets, int(offsets[-1]) + tail


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("dist", ["uniform", "24bit", "duplicates", "equal", "sorted", "reverse", "bit31"])
def test_distributions_at_every_tier_boundary(ctx, dist, pairs):
    rng = np.random.default_rng(len(dist) * 2 + int(pairs))
    offsets, n = boundary_layout(lead=3, tail=5)  # offsets[0] > 0 and offsets[S] < n: the margins stay as they were
    keys = distribution(dist, rng, n)
    keys[:3] = SENTINEL
    keys[-5:] = SENTINEL
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    before = stats(ctx)
    ok, ov = run(ctx, keys, offsets, vals)
    rk, rv = reference(keys, offsets, vals)
    assert np.array_equal(ok[:3], keys[:3]) and np.array_equal(ok[-5:], keys[-5:])
    assert np.array_equal(ok, rk)
    if pairs:
        assert np.array_equal(ov, rv)
    # every tier ran, as the host-side classification says
    want = host_tiers(ctx.lib, offsets, n, int(pairs), THR)
    assert np.array_equal(stats(ctx) - before, want)
    assert (want > 0).all()


@pytest.mark.parametrize("pairs", [False, True])
def test_misaligned_starts(ctx, pairs):
    rng = np.random.default_rng(7)
    lengths = []
    for mis in range(4):
        for L in (3, 61, 700, 1789, 3001, 9000, 14000, 20000):
            lengths += [L + mis, mis]  # every start at every residue mod 4, empty segments between some
    offsets = 1 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1]) + 2
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if pairs else None
    ok, ov = run(ctx, keys, offsets, vals)
    rk, rv = reference(keys, offsets, vals)
    assert np.array_equal(ok, rk)
    if pairs:
        assert np.array_equal(ov, rv)


@pytest.mark.parametrize("pairs", [False, True])
def test_a_million_small_segments(ctx, pairs):
    rng = np.random.default_rng(11)
    lengths = rng.integers(1, 201, 10 ** 6)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1])
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFF00FF)
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    ok, ov = run(ctx, keys, offsets, vals)
    rk, rv = reference(keys, offsets, vals)
    assert np.array_equal(ok, rk)
    if pairs:
        assert np.array_equal(ov, rv)


def test_log_uniform_lengths_1e8_bit_exact():
    """case (e) of the timing tool, on a context with the library's default threshold (segments from 2^20 keys take the one-call tier)"""
    rng = np.random.default_rng(5)
    total, lengths = 10 ** 8, []
    while sum(lengths) < total:
        lengths.append(int(np.exp(rng.uniform(0, np.log(1 << 21)))))
    lengths[-1] -= sum(lengths) - total
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    keys = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    c = vrs.GPUContext(0)
    c.init()
    try:
        before = stats(c)
        ok, _ = run(c, keys, offsets)
        want = host_tiers(c.lib, offsets, total, 0, capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT)
        assert np.array_equal(stats(c) - before, want) and want[capi.VRS_SEGMENT_ONE_CALL] > 0
    finally:
        c.shutdown()
    rk, _ = reference(keys, offsets)
    assert np.array_equal(ok, rk)


def test_whole_sorts_before_and_after_on_the_same_context(ctx):
    """the one-call sort's scratch and its pending second half are shared with the segmented sort's one-call tier"""
    rng = np.random.default_rng(3)
    big = rng.integers(0, 1 << 32, (1 << 22) + 4099, dtype=np.uint64).astype(np.uint32)
    B = vrs.Buffer.BufferSettings(4 * big.size)

    def whole():
        k0, k1 = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B, big), vrs.Buffer(ctx, B)
        ctx.check(ctx.lib.vrs_sort_keys_u32(ctx.handle, k0.handle, k1.handle, big.size))
        return k0, k1

    first = whole()  # still pending (own-stream context: enqueue only) when the segmented sort starts
    offsets, n = boundary_layout(lead=0, tail=0)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ok, _ = run(ctx, keys, offsets)
    second = whole()
    ref = np.sort(big)
    for k0, k1 in (first, second):
        out = np.empty_like(big)
        k0.downloadWithStagingBuffer(out)
        assert np.array_equal(out, ref)
        k0.release()
        k1.release()
    assert np.array_equal(ok, reference(keys, offsets)[0])


def test_borrowed_stream_context():
    torch = pytest.importorskip("torch")
    c = vrs.GPUContext(0, stream=torch.cuda.current_stream().cuda_stream)
    c.init()
    try:
        c.setTuning(capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, THR)
        rng = np.random.default_rng(9)
        offsets, n = boundary_layout(lead=2, tail=1)
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFF0FFFFF)
        vals = np.arange(n, dtype=np.uint32)
        ok, ov = run(c, keys, offsets, vals)
    finally:
        c.shutdown()
    rk, rv = reference(keys, offsets, vals)
    assert np.array_equal(ok, rk) and np.array_equal(ov, rv)


def test_degenerate_and_malformed_calls(ctx):
    rng = np.random.default_rng(13)
    n = 50000
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    B = vrs.Buffer.BufferSettings
    k0, k1 = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B(4 * n), keys), vrs.Buffer(ctx, B(4 * n))
    bad = np.array([40000, 100, 1 << 31, 0xFFFFFFFF, 20000, 30000, 25000, 60000, 5], dtype=np.uint32)  # e < b, beyond n, overlaps
    off = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B(4 * bad.size), bad)
    lib = ctx.lib
    assert lib.vrs_sort_segments_u32(ctx.handle, k0.handle, k1.handle, 0, off.handle, 8) == capi.VRS_OK
    assert lib.vrs_sort_segments_u32(ctx.handle, k0.handle, k1.handle, n, off.handle, 0) == capi.VRS_OK
    assert lib.vrs_sort_segments_u32(ctx.handle, k0.handle, k1.handle, n + 1, off.handle, 8) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_u32(ctx.handle, k0.handle, k1.handle, n, off.handle, 9) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_pairs_u32(ctx.handle, k0.handle, k1.handle, None, None, n, off.handle, 8) == capi.VRS_ERROR_INVALID_ARGUMENT
    out = np.empty_like(keys)
    k0.downloadWithStagingBuffer(out)
    assert np.array_equal(out, keys)  # nothing was enqueued
    # malformed offsets: clamped, nothing faults; the multiset stays and [0, 100) -- no clamped range reaches it -- is untouched
    assert lib.vrs_sort_segments_u32(ctx.handle, k0.handle, k1.handle, n, off.handle, 8) == capi.VRS_OK
    k0.downloadWithStagingBuffer(out)
    assert np.array_equal(out[:100], keys[:100])
    for b in (k0, k1, off):
        b.release()


@pytest.mark.parametrize("dtype", ["int32", "float32"])
@pytest.mark.parametrize("shape", [(1000, 37), (64, 4096), (3, 20000), (7, 1)])
def test_sort_rows_matches_torch_sort(dtype, shape):
    torch = pytest.importorskip("torch")
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    if dtype == "int32":
        x = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda", generator=g)
        x[:, ::3] = x[:, :1].clone()  # ties
    else:
        x = torch.randn(shape, dtype=torch.float32, device="cuda", generator=g) * 1e3
        x[:, ::4] = torch.round(x[:, ::4])  # ties
        x[x == 0] = 1.0  # (no -0.0: the library orders it before +0.0)
    ref_v, ref_i = torch.sort(x, dim=-1, stable=True)
    v, i = vrs.sort_rows(x, return_indices=True)
    torch.cuda.synchronize()
    assert torch.equal(v, ref_v) and torch.equal(i, ref_i)
    assert torch.equal(vrs.sort_rows(x), ref_v)
