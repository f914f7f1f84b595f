"""Top-k selection on the device (vrs_topk_segments, vkradixsort_amd.topk), every result bit-exact against numpy per segment:
np.argsort(r, kind="stable")[:k] of the rank r.  Unsorted results are compared after ordering each segment by (r, index)."""
import ctypes
import time

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd.topk import scratch_bytes

pytestmark = pytest.mark.gpu

GRID_THR = 20000  # VRS_TUNE_TOPK_GRID_MIN_KEYS of the test context: all three tiers at sizes the tests can afford
LDS = capi.TOPK_LDS_MAX
FILL = np.uint32(0xFFFFFFFF)
SENTINEL = np.uint32(0xA5A5A5A5)
KT = {"u32": capi.VRS_TOPK_U32, "i32": capi.VRS_TOPK_I32, "f32": capi.VRS_TOPK_F32}


@pytest.fixture(scope="module")
def ctx():
    c = vrs.GPUContext(0)
    c.init()
    c.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, GRID_THR)
    yield c
    c.shutdown()


def rank(x, kt, largest):
    x = x.astype(np.uint32)
    if kt == "i32":
        r = x ^ np.uint32(0x80000000)
    elif kt == "f32":
        r = x ^ np.where(x >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    else:
        r = x
    return ~r if largest else r


def clamp(b, e, n):
    lo = min(b, n)
    return lo, min(max(b, e), n)


def ref_segment(r, k):
    """np.argsort(r, kind="stable")[:k], without sorting everything when k is small."""
    m = min(k, r.size)
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    if m >= r.size // 4:
        return np.argsort(r, kind="stable")[:m]
    t = np.partition(r, m - 1)[m - 1]
    cand = np.nonzero(r <= t)[0]
    return cand[np.argsort(r[cand], kind="stable")][:m]


def reference(keys, offsets, k, kt, largest):
    n, S = keys.size, offsets.size - 1
    r_all = rank(keys, kt, largest)
    ok = np.full(S * k, FILL, dtype=np.uint32)
    oi = np.full(S * k, FILL, dtype=np.uint32)
    for i in range(S):
        b, e = clamp(int(offsets[i]), int(offsets[i + 1]), n)
        order = ref_segment(r_all[b:e], k)
        ok[i * k:i * k + order.size] = keys[b + order]
        oi[i * k:i * k + order.size] = order
    return ok, oi


def run(c, keys, offsets, k, kt="u32", largest=False, sorted=True, indices=True, pad=64):
    """Uploads, selects, downloads; returns (out_keys, out_indices or None).  Checks that the input, the offsets and the sentinels
    past S * k are untouched."""
    n, S = keys.size, offsets.size - 1
    B = vrs.Buffer.BufferSettings
    kb = vrs.Buffer.fillDeviceWithStagingBuffer(c, B(max(4 * n, 4)), keys if n else np.zeros(1, np.uint32))
    ob = vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * (S + 1)), offsets.astype(np.uint32))
    sent = np.full(S * k + pad, SENTINEL, dtype=np.uint32)
    outk = vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * sent.size), sent)
    outi = vrs.Buffer.fillDeviceWithStagingBuffer(c, B(4 * sent.size), sent) if indices else None
    need = scratch_bytes(n, S, k, largest, sorted)
    scr = vrs.Buffer(c, B(max(need, 4)))
    vrs.topk_segments(c, kb, ob, n, S, k, outk, outi, scr, key_type=kt, largest=largest, sorted=sorted)
    rk = np.empty(sent.size, np.uint32)
    outk.downloadWithStagingBuffer(rk)
    ri = None
    if indices:
        ri = np.empty(sent.size, np.uint32)
        outi.downloadWithStagingBuffer(ri)
        assert np.all(ri[S * k:] == SENTINEL), "out_indices written past S * k"
        ri = ri[:S * k]
    assert np.all(rk[S * k:] == SENTINEL), "out_keys written past S * k"
    if n:
        back = np.empty(n, np.uint32)
        kb.downloadWithStagingBuffer(back)
        assert np.array_equal(back, keys), "keys were written"
    ob_back = np.empty(S + 1, np.uint32)
    ob.downloadWithStagingBuffer(ob_back)
    assert np.array_equal(ob_back, offsets.astype(np.uint32)), "offsets were written"
    for b in (kb, ob, outk, outi, scr):
        if b is not None:
            b.release()
    return rk[:S * k], ri


def check(c, keys, offsets, k, kt="u32", largest=False, sorted=True, indices=True):
    ok, oi = run(c, keys, offsets, k, kt, largest, sorted, indices)
    rk, ri = reference(keys, offsets, k, kt, largest)
    if not sorted:  # each segment's m entries in some order: order them by (r, index) first
        S = offsets.size - 1
        ok, oi = ok.copy(), (oi.copy() if oi is not None else None)
        r = rank(ok, kt, largest).astype(np.uint64)
        for i in range(S):
            sl = slice(i * k, (i + 1) * k)
            live = ok[sl] != FILL if oi is None else oi[sl] != FILL
            m = int(live.sum())
            sub = np.arange(m)
            key = (r[sl][:m] << np.uint64(32)) | (oi[sl][:m].astype(np.uint64) if oi is not None else sub.astype(np.uint64))
            o = np.argsort(key, kind="stable")
            ok[sl][:m] = ok[sl][:m][o]
            if oi is not None:
                oi[sl][:m] = oi[sl][:m][o]
    assert np.array_equal(ok, rk), f"keys differ at {np.nonzero(ok != rk)[0][:8]}"
    if oi is not None:
        assert np.array_equal(oi, ri), f"indices differ at {np.nonzero(oi != ri)[0][:8]}"


def distribution(name, rng, n):
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    f = rng.standard_normal(n).astype(np.float32)
    if name == "uniform":
        return u, "u32"
    if name == "24bit":
        return u & np.uint32(0xFFFFFF), "u32"
    if name == "8distinct":
        return (u % np.uint32(8)) * np.uint32(0x10000001), "u32"
    if name == "equal":
        return np.full(n, 0x12345678, np.uint32), "u32"
    if name == "ascending":
        return np.arange(n, dtype=np.uint32), "u32"
    if name == "descending":
        return np.arange(n, dtype=np.uint32)[::-1].copy(), "u32"
    if name == "int32":
        return (rng.integers(-1000, 1000, n).astype(np.int32)).view(np.uint32), "i32"
    if name == "float":
        return f.view(np.uint32), "f32"
    if name == "float_special":
        specials = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, 1e-45, -1e-45, 1e-40, -1e-40], dtype=np.float32).view(np.uint32)
        specials = np.concatenate([specials, np.array([0xFFC00000, 0x7FC00001], dtype=np.uint32)])  # -NaN, a NaN with payload
        x = f.view(np.uint32).copy()
        pick = rng.integers(0, n, n // 3)
        x[pick] = specials[rng.integers(0, specials.size, pick.size)]
        return x, "f32"
    raise ValueError(name)


DISTS = ["uniform", "24bit", "8distinct", "equal", "ascending", "descending", "int32", "float", "float_special"]
# one segment per tier boundary and a few more: 0, 1, LDS cap +- 1, grid threshold +- 1
MIX = [0, 1, 5, 100, LDS - 1, LDS, LDS + 1, GRID_THR - 1, GRID_THR, GRID_THR + 1, 70000]


def mixed_offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)


@pytest.mark.parametrize("dist", DISTS)
def test_distributions_every_tier(ctx, dist):
    rng = np.random.default_rng(DISTS.index(dist))
    offsets = mixed_offsets(MIX)
    keys, kt = distribution(dist, rng, int(offsets[-1]))
    for k in (1, 63, 64, 65, 1000):
        for largest in (False, True):
            check(ctx, keys, offsets, k, kt, largest, sorted=True)
    check(ctx, keys, offsets, 64, kt, True, sorted=False)
    check(ctx, keys, offsets, 5000, kt, False, sorted=True)  # the survivors go through the segmented sort


@pytest.mark.parametrize("length", [5000, LDS, 30000, 70000])
@pytest.mark.parametrize("dist", ["uniform", "8distinct", "float_special"])
def test_k_near_length(ctx, length, dist):
    rng = np.random.default_rng(length)
    keys, kt = distribution(dist, rng, length)
    offsets = np.array([0, length], dtype=np.uint32)
    for k in (length - 1, length, length + 3):
        for largest in (False, True):
            check(ctx, keys, offsets, k, kt, largest, sorted=(k != length))


def stats(c):
    return np.array(list(vrs.topk_stats(c).values()), dtype=np.int64)


def host_tiers(lib, offsets, n, thr):
    counts = np.zeros(3, dtype=np.int64)
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    for b, e in zip(offsets[:-1], offsets[1:]):
        assert lib.vrs_topk_tier_for(int(b), int(e), n, thr, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == 0
        counts[t.value] += 1
    return counts


def test_tier_counts_match_classification(ctx):
    rng = np.random.default_rng(7)
    offsets = mixed_offsets(MIX * 3)
    keys = rng.integers(0, 1 << 32, int(offsets[-1]), dtype=np.uint64).astype(np.uint32)
    before = stats(ctx)
    check(ctx, keys, offsets, 100)
    got = stats(ctx) - before
    want = host_tiers(ctx.lib, offsets, keys.size, GRID_THR)
    assert np.array_equal(got, want), (got, want)
    assert np.all(want > 0), "every tier ran"


def test_log_uniform_mixed_lengths(ctx):
    rng = np.random.default_rng(11)
    lengths = np.exp(rng.uniform(0, np.log(300000), 400)).astype(np.int64)
    lengths[rng.integers(0, lengths.size, 20)] = 0
    offsets = mixed_offsets(lengths)
    keys = rng.standard_normal(int(offsets[-1])).astype(np.float32).view(np.uint32)
    for k in (10, 300):
        check(ctx, keys, offsets, k, "f32", largest=True)
    check(ctx, keys, offsets, 300, "f32", largest=False, sorted=False)


def test_malformed_overlapping_offsets_and_gaps(ctx):
    rng = np.random.default_rng(13)
    n = 150000
    keys = rng.integers(0, 1 << 12, n, dtype=np.uint32)  # many ties
    offsets = np.array([100, 50, 60000, 40000, 140000, 20, n + 5, 0xFFFFFFFF, 3, 30000, 30000, n, 0, 90000, 10], dtype=np.uint32)
    for k in (1, 77, 9000):
        check(ctx, keys, offsets, k)
    # overlapping ranges: every segment is a suffix of the buffer
    offsets = np.array([0, n, 1000, n, 5000, n, 50000, n], dtype=np.uint32)
    check(ctx, keys, offsets, 500)


def test_no_indices_same_keys(ctx):
    rng = np.random.default_rng(17)
    offsets = mixed_offsets(MIX)
    keys, kt = distribution("float_special", rng, int(offsets[-1]))
    for k in (64, 5000):
        with_i, _ = run(ctx, keys, offsets, k, kt, True, True, indices=True)
        without, none = run(ctx, keys, offsets, k, kt, True, True, indices=False)
        assert none is None and np.array_equal(with_i, without)
    check(ctx, keys, offsets, 64, kt, False, sorted=True, indices=False)


def test_empty_input_gets_filler(ctx):
    ok, oi = run(ctx, np.zeros(0, np.uint32), np.zeros(4, np.uint32), 5)
    assert np.all(ok == FILL) and np.all(oi == FILL)


def test_repeated_calls_reuse_state(ctx):
    rng = np.random.default_rng(19)
    for it in range(12):
        S = int(rng.integers(1, 40))
        lengths = rng.integers(0, 40000, S)
        offsets = mixed_offsets(lengths)
        keys = rng.integers(0, 1 << int(rng.integers(4, 33)), int(offsets[-1]), dtype=np.uint64).astype(np.uint32)
        k = int(rng.choice([1, 7, 64, 129, 2000, 4096, 4097]))
        check(ctx, keys, offsets, k, largest=bool(it % 2), sorted=bool(it % 3))


@pytest.mark.parametrize("largest", [False, True])
def test_1e8_one_segment_default_tuning(largest):
    import torch

    n, k = 10 ** 8, 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, device="cuda", generator=g)
    v, i = vrs.topk(x, k, largest=largest)
    torch.cuda.synchronize()
    keys = x.cpu().numpy().view(np.uint32)
    order = ref_segment(rank(keys, "f32", largest), k)
    assert np.array_equal(i.cpu().numpy(), order)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), keys[order])
    ctx = vrs._torch.context_for(x.device)
    assert vrs.topk_stats(ctx)["grid"] >= 1


def test_never_waits_for_the_device():
    import torch

    rng = np.random.default_rng(23)
    x = torch.from_numpy(rng.standard_normal((64, 50000)).astype(np.float32)).cuda()
    vrs.topk(x, 100)  # warm-up: module load, the context
    torch.cuda.synchronize()
    torch.cuda._sleep(int(60e-3 * 2.0e9))  # about 60 ms of work ahead of the call
    t0 = time.perf_counter()
    v, i = vrs.topk(x, 100)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert dt < 5e-3, f"the call took {dt * 1e3:.2f} ms on the host"
    assert busy
    keys = x.cpu().numpy().view(np.uint32)
    rk, ri = reference(keys.ravel(), mixed_offsets([50000] * 64), 100, "f32", True)
    assert np.array_equal(v.cpu().numpy().view(np.uint32).ravel(), rk)
    assert np.array_equal(i.cpu().numpy().ravel(), ri.astype(np.int64))


@pytest.mark.parametrize("shape", [(1000,), (100000,), (1, 300000), (64, 4096), (300, 20000), (7, 50000)])
@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_torch_topk_equal_on_distinct_values(shape, dtype):
    import torch

    rng = np.random.default_rng(sum(shape))
    size = int(np.prod(shape))
    rows = 1 if len(shape) == 1 else shape[0]
    length = shape[-1]
    # distinct values within every row
    base = np.stack([rng.permutation(length) for _ in range(rows)]).astype(np.int64) - length // 2
    if dtype == "float32":
        x = torch.from_numpy((base * 0.37).astype(np.float32).reshape(shape)).cuda()
    else:
        x = torch.from_numpy((base * 3).astype(np.int32).reshape(shape)).cuda()
    assert x.numel() == size
    for k in (1, 50, min(1024, length)):
        for largest in (True, False):
            v, i = vrs.topk(x, k, largest=largest)
            tv, ti = torch.topk(x, k, dim=-1, largest=largest, sorted=True)
            assert v.dtype == x.dtype and i.dtype == torch.int64 and v.shape == tv.shape
            assert torch.equal(v, tv) and torch.equal(i, ti)
            v2, i2 = vrs.topk(x, k, largest=largest, sorted=False)  # same set
            assert torch.equal(torch.sort(i2, dim=-1)[0], torch.sort(ti, dim=-1)[0])


def test_torch_level_ties_follow_stable_rule():
    import torch

    rng = np.random.default_rng(29)
    x = torch.from_numpy(rng.integers(0, 5, (33, 3000)).astype(np.int32)).cuda()
    for largest in (True, False):
        v, i = vrs.topk(x, 700, largest=largest)
        xs = x.cpu().numpy()
        for row in range(xs.shape[0]):
            r = rank(xs[row].view(np.uint32), "i32", largest)
            order = np.argsort(r, kind="stable")[:700]
            assert np.array_equal(i[row].cpu().numpy(), order)
            assert np.array_equal(v[row].cpu().numpy(), xs[row][order])
