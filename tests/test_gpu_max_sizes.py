"""The newer operations at the top of the size range: up to 2^32 - 1 elements (num_elements is a uint32).

Run-length encoding, unique, top-k, the one-call sorts of pairs and 64-bit keys (the contract stages from 2^30 keys on), the segmented
sorts and the torch.sort drop-ins, at sizes inside the ranges where a 32-bit index wraps (2^32 - 2^21 < n for the grid-stride loops,
2^32 - 16384 < len for the top-k tile count, S * k > 2^32 - 2^21 for top-k's sort area).

All data is made on the device with torch in int64 chunks of 2^28 elements and wrapped with vrs.Buffer(..., device_ptr=...): nothing
of this size goes through host memory.  A reference sort cannot run at these sizes, so the results are checked by exact O(n)
certificates, chunk by chunk on the device:
  * h(i) = i * 2654435761 mod 2^32 is a bijection of [0, 2^32); its inverse is multiplication by 244002641.  mix(i) = i * 0x9E3779B97F4A7C15
    mod 2^64 is a bijection of [0, 2^64) (every bit of the key varies).
  * sorted pairs (key, payload = input position): (key, payload) strictly increasing, key == f(payload), payload in range.  Then the
    payloads are distinct, hence a permutation, and the output is exactly the stable sort.
  * sorted distinct keys f(i): strictly increasing and f^-1(key) < n, n of them.
  * unique / run-length encoding / top-k: constructions whose runs, counts, offsets, inverse and smallest keys are known in closed form.
Each test skips when the device has less free memory than its footprint + 8 GB, and frees everything before the next one.
"""
import gc
import importlib

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd.topk import scratch_bytes as topk_scratch_bytes

uq = importlib.import_module("vkradixsort_amd.unique")  # (vkradixsort_amd.unique is the function)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = vrs.Buffer.BufferSettings
GB = 1 << 30
STEP = 1 << 28
M32 = 0xFFFFFFFF
GOLD, GOLD_INV = 2654435761, 244002641
MIX = 0x9E3779B97F4A7C15
MIX_INV = pow(MIX, -1, 1 << 64)
TOP64 = -(1 << 63)
N_MAX = 2 ** 32 - 1
N_MID = 2 ** 31 + 12345
assert GOLD * GOLD_INV % (1 << 32) == 1


def _i64(c):  # a 64-bit pattern as the int64 torch multiplies by (wrapping)
    return c - (1 << 64) if c >= 1 << 63 else c


def h(i):
    return (i * GOLD) & M32


def h_inv(k):
    return (k * GOLD_INV) & M32


def mix(i):
    return i * _i64(MIX)


def mix_inv(k):
    return k * _i64(MIX_INV)


def as_i32(v):  # values in [0, 2^32) -> their int32 bit patterns
    return ((v ^ 0x80000000) - 0x80000000).to(torch.int32)


def u32(t):  # int32 storage -> the uint32 values, as int64
    return t.to(torch.int64) & M32


def ulo(t):  # int64 storage of uint64 keys -> int64 values in the same (unsigned) order
    return t ^ TOP64


@pytest.fixture
def dev(gpu_context):
    d = torch.device("cuda", gpu_context.device_ordinal)
    yield d
    gc.collect()
    torch.cuda.synchronize(d)
    torch.cuda.empty_cache()


def room(d, need_bytes):
    free, _ = torch.cuda.mem_get_info(d)
    if free < need_bytes + 8 * GB:
        pytest.skip(f"needs {(need_bytes + 8 * GB) / GB:.0f} GB of free HBM, {free / GB:.0f} GB free")


def build(n, dtype, fn, d):
    out = torch.empty(n, dtype=dtype, device=d)
    for a in range(0, n, STEP):
        b = min(a + STEP, n)
        out[a:b] = fn(torch.arange(a, b, dtype=torch.int64, device=d))
    return out


def chunks(n, overlap=0):
    for a in range(0, n, STEP):
        yield a, min(a + STEP + overlap, n)


def wrap(ctx, *tensors):
    return [vrs.Buffer(ctx, S(max(t.numel() * t.element_size(), 4)), device_ptr=t.data_ptr()) for t in tensors]


def run(ctx, call, *tensors):
    """call(*buffers) on the context's stream, between torch's work before and after."""
    torch.cuda.synchronize()
    bufs = wrap(ctx, *tensors)
    try:
        call(*bufs)
        ctx.waitIdle()
    finally:
        for b in bufs:
            b.release()


def all_true(cond, what):
    assert bool(cond.all().item()), what


def check_lex_increasing(key, pay, n, bounds=None):
    """(key, pay) strictly increasing lexicographically over [0, n) (key, pay: int64 views in the intended order); with segment
    bounds, only between neighbours of one segment."""
    for a, b in chunks(n, overlap=1):
        k, p = key(a, b), pay(a, b)
        ok = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (p[1:] > p[:-1]))
        if bounds is not None:
            pos = torch.arange(a + 1, b, dtype=torch.int64, device=k.device)
            ok |= torch.isin(pos, bounds)  # (a segment starts at pos: no order between pos - 1 and pos)
        all_true(ok, f"not strictly increasing in [{a}, {b})")


# ---------------------------------------------------------------------------------------------- run-length encoding

def test_rle_u32_max_size_all_outputs(gpu_context, dev):
    """n = 2^32 - 1: runs of 16 (key i >> 4), then all-distinct keys (R = n: the counts kernel's loop runs to 2^32 - 1)."""
    n = N_MAX
    room(dev, 4 * 4 * n + 4 * (n + 1) + 4 * GB)
    ctx = gpu_context
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    ok_, off, cnt, rid = (torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n + 1, n, n))
    nr = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(uq.rle_scratch_bytes(n, 4), dtype=torch.uint8, device=dev)
    for shift in (4, 0):
        for a, b in chunks(n):
            keys[a:b] = as_i32(torch.arange(a, b, dtype=torch.int64, device=dev) >> shift)
        run(ctx, lambda k, o1, o2, o3, o4, r, s: uq.run_length_encode(ctx, k, n, r, s, 4, o1, o2, o3, o4), keys, ok_, off, cnt, rid, nr,
            scratch)
        L = 1 << shift
        R = (n + L - 1) // L
        assert int(u32(nr).item()) == R
        for a, b in chunks(R):
            j = torch.arange(a, b, dtype=torch.int64, device=dev)
            all_true(u32(ok_[a:b]) == j, f"run keys in [{a}, {b})")
            all_true(u32(off[a:b]) == j * L, f"run offsets in [{a}, {b})")
            want = torch.where(j == R - 1, n - (R - 1) * L, L)
            all_true(u32(cnt[a:b]) == want, f"run counts in [{a}, {b})")
        assert int(u32(off[R]).item()) == n
        for a, b in chunks(n):
            all_true(u32(rid[a:b]) == torch.arange(a, b, dtype=torch.int64, device=dev) >> shift, f"run ids in [{a}, {b})")
    del keys, ok_, off, cnt, rid, nr, scratch


def test_rle_u64_every_bit_varying(gpu_context, dev):
    """n = 2^31 + 12345 64-bit keys mix(i >> 3): runs of 8 (the last one of 1), keys that differ in every bit position."""
    n = N_MID
    L = 8
    R = (n + L - 1) // L
    room(dev, 8 * n + 8 * n + 4 * (n + 1) + 4 * n + 4 * n + 2 * GB)
    ctx = gpu_context
    keys = build(n, torch.int64, lambda i: mix(i >> 3), dev)
    ok_ = torch.empty(n, dtype=torch.int64, device=dev)
    off, cnt, rid = (torch.empty(m, dtype=torch.int32, device=dev) for m in (n + 1, n, n))
    nr = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(uq.rle_scratch_bytes(n, 8), dtype=torch.uint8, device=dev)
    run(ctx, lambda k, o1, o2, o3, o4, r, s: uq.run_length_encode(ctx, k, n, r, s, 8, o1, o2, o3, o4), keys, ok_, off, cnt, rid, nr, scratch)
    assert int(u32(nr).item()) == R
    for a, b in chunks(R):
        j = torch.arange(a, b, dtype=torch.int64, device=dev)
        all_true(ok_[a:b] == mix(j), f"run keys in [{a}, {b})")
        all_true(u32(off[a:b]) == j * L, f"run offsets in [{a}, {b})")
        all_true(u32(cnt[a:b]) == torch.where(j == R - 1, n - (R - 1) * L, L), f"run counts in [{a}, {b})")
    assert int(u32(off[R]).item()) == n and int(u32(cnt[R - 1]).item()) == 1
    for a, b in chunks(n):
        all_true(u32(rid[a:b]) == torch.arange(a, b, dtype=torch.int64, device=dev) >> 3, f"run ids in [{a}, {b})")
    del keys, ok_, off, cnt, rid, nr, scratch


# ---------------------------------------------------------------------------------------------- unique

def test_unique_u32_max_size_counts(gpu_context, dev):
    """n = 2^32 - 1 keys h(i) >> 8 (the rank map's loop runs to 2^32 - 1): unique is arange(2^24), every count 256 but that of
    h(2^32 - 1) >> 8, which is 255."""
    n = N_MAX
    room(dev, 3 * 4 * n + uq.unique_scratch_bytes(n, "u32", counts=True) + 2 * GB)
    ctx = gpu_context
    keys = build(n, torch.int32, lambda i: as_i32(h(i) >> 8), dev)
    out, cnt = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    nr = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(uq.unique_scratch_bytes(n, "u32", counts=True), dtype=torch.uint8, device=dev)
    run(ctx, lambda k, o, c, r, s: uq.unique_keys(ctx, k, n, o, r, s, "u32", out_counts=c), keys, out, cnt, nr, scratch)
    R = 1 << 24
    assert int(u32(nr).item()) == R
    j = torch.arange(R, dtype=torch.int64, device=dev)
    all_true(u32(out[:R]) == j, "unique keys")
    missing = h(N_MAX) >> 8
    all_true(u32(cnt[:R]) == torch.where(j == missing, 255, 256), "unique counts")
    del keys, out, cnt, nr, scratch


@pytest.mark.parametrize("key_type", ["u32", "u64"])
def test_unique_with_inverse_past_2_31(gpu_context, dev, key_type):
    """n = 2^31 + 12345 keys f(i mod 2^24) (f = h, or mix for 64-bit keys): 2^24 distinct keys; their order, counts (q or q + 1) and
    every element's inverse follow from the order of f(0 .. 2^24 - 1), which torch sorts."""
    n, M = N_MID, 1 << 24
    wide = key_type == "u64"
    kb = 8 if wide else 4
    dt = torch.int64 if wide else torch.int32
    room(dev, 2 * kb * n + 4 * n * 2 + uq.unique_scratch_bytes(n, key_type, inverse=True, counts=True) + 2 * GB)
    ctx = gpu_context
    f = (lambda i: mix(i)) if wide else (lambda i: as_i32(h(i)))
    keys = build(n, dt, lambda i: f(i % M), dev)
    out = torch.empty(n, dtype=dt, device=dev)
    cnt, inv = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    nr = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(uq.unique_scratch_bytes(n, key_type, inverse=True, counts=True), dtype=torch.uint8, device=dev)
    run(ctx, lambda k, o, c, v, r, s: uq.unique_keys(ctx, k, n, o, r, s, key_type, out_counts=c, out_inverse=v), keys, out, cnt, inv, nr,
        scratch)
    assert int(u32(nr).item()) == M
    j = torch.arange(M, dtype=torch.int64, device=dev)
    base = f(j)
    order = torch.sort(ulo(base) if wide else u32(base)).indices  # the distinct keys' ascending (unsigned) order
    all_true(out[:M] == base[order], "unique keys")
    q, r = divmod(n, M)
    all_true(u32(cnt[:M]) == torch.where(order < r, q + 1, q), "unique counts")
    rank = torch.empty_like(order)
    rank[order] = j
    for a, b in chunks(n):
        all_true(u32(inv[a:b]) == rank[torch.arange(a, b, dtype=torch.int64, device=dev) % M], f"inverse in [{a}, {b})")
    del keys, out, cnt, inv, nr, scratch, base, order, rank


# ---------------------------------------------------------------------------------------------- top-k

def _topk_expect(k, largest, key_type):
    """The k smallest (largest) keys of h(0 .. 2^32 - 2) as uint32 bit patterns, in order (h(2^32 - 1) = 0x61C8864F is in neither end)."""
    j = np.arange(k, dtype=np.int64)
    if key_type == "i32":
        r = (M32 - j) if largest else j  # ranks: x ^ 0x80000000
        return r ^ 0x80000000
    r = (M32 - j) if largest else j  # ranks by the IEEE-754 total order: x ^ (sign ? 0xFFFFFFFF : 0x80000000)
    return np.where(r & 0x80000000, r ^ 0x80000000, r ^ M32)


def _check_topk(values, idx, k, largest, key_type):
    bits = values.view(torch.int32)
    want = torch.tensor(_topk_expect(k, largest, key_type), dtype=torch.int64, device=values.device)
    all_true(u32(bits) == want, f"top-k values ({key_type}, largest={largest})")
    pos = u32(idx) if idx.dtype == torch.int32 else idx  # (the C ABI's uint32 positions; vrs.topk's int64 ones as returned)
    all_true(pos == h_inv(want), f"top-k indices ({key_type}, largest={largest})")


def test_topk_one_segment_max_size(dev):
    """vrs.topk of a 1-D tensor of 2^32 - 1 keys h(i), k = 1000 (the grid tier's tile count (len + 16383) / 16384 wrapped to 0 here):
    int32 and float32, smallest and largest; then the ties of h(i) >> 2, broken by the lower index."""
    n, k = N_MAX, 1000
    room(dev, 4 * n + 2 * GB)
    x = build(n, torch.int32, lambda i: as_i32(h(i)), dev)
    for key_type, t in (("i32", x), ("f32", x.view(torch.float32))):
        for largest in (False, True):
            v, i = vrs.topk(t, k, largest=largest, sorted=True)
            _check_topk(v, i, k, largest, key_type)
    for a, b in chunks(n):
        x[a:b] = as_i32(h(torch.arange(a, b, dtype=torch.int64, device=dev)) >> 2)
    v, i = vrs.topk(x, k, largest=False, sorted=True)
    c = torch.arange(k, dtype=torch.int64, device=dev)
    all_true(v.to(torch.int64) == c // 4, "tied top-k values")
    cand = h_inv(c).view(-1, 4)  # the four indices of value c // 4 (h^-1 of 4v .. 4v + 3), lowest first
    all_true(i == torch.sort(cand, dim=1).values.reshape(-1), "tied top-k indices")
    del x, v, i


def test_topk_block_tier_max_size(dev):
    """The same segment on the BLOCK tier (VRS_TUNE_TOPK_GRID_MIN_KEYS = 0): one workgroup walks 2^32 - 1 keys in 16384-key tiles."""
    n, k = N_MAX, 1000
    room(dev, 4 * n + 2 * GB)
    x = build(n, torch.int32, lambda i: as_i32(h(i)), dev)
    offs = torch.tensor([0, n - (1 << 32)], dtype=torch.int32, device=dev)
    with vrs.GPUContext(dev.index) as ctx:
        ctx.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, 0)
        for largest in (False, True):
            ov, oi = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.int32, device=dev)
            scratch = torch.empty(max(topk_scratch_bytes(n, 1, k, largest, True), 4), dtype=torch.uint8, device=dev)
            run(ctx, lambda kk, o, a, b, s: vrs.topk_segments(ctx, kk, o, n, 1, k, a, b, s, key_type="i32", largest=largest, sorted=True),
                x, offs, ov, oi, scratch)
            _check_topk(ov, oi, k, largest, "i32")
        assert vrs.topk_stats(ctx) == {"lds": 0, "block": 2, "grid": 0}
    del x


def test_topk_sorted_big_k_sort_area(gpu_context, dev):
    """S = 1,048,000 segments of 8 keys, k = 4097, sorted: S * k = 4.2937e9 slots go through the segmented sort (the sort area's loops
    run past 2^32 - 2^21).  Every segment's 8 keys sorted, lowest index first among equal keys, then 4089 fillers."""
    S_, L, k = 1048000, 8, 4097
    n, sk = S_ * L, S_ * k
    room(dev, 2 * 4 * sk + topk_scratch_bytes(n, S_, k, False, True) + 2 * GB)
    ctx = gpu_context
    keys = build(n, torch.int32, lambda i: as_i32(h(i) >> 29), dev)  # 3-bit keys: ties in every segment
    offs = as_i32(torch.arange(S_ + 1, dtype=torch.int64, device=dev) * L)
    ov, oi = torch.empty(sk, dtype=torch.int32, device=dev), torch.empty(sk, dtype=torch.int32, device=dev)
    scratch = torch.empty(topk_scratch_bytes(n, S_, k, False, True), dtype=torch.uint8, device=dev)
    run(ctx, lambda kk, o, a, b, s: vrs.topk_segments(ctx, kk, o, n, S_, k, a, b, s, key_type="u32", sorted=True), keys, offs, ov, oi, scratch)
    del scratch
    seg = u32(keys).view(S_, L)
    order = torch.sort(seg * L + torch.arange(L, device=dev), dim=1).values % L  # stable order within each segment
    ov2, oi2 = ov.view(S_, k), oi.view(S_, k)
    all_true(u32(ov2[:, :L]) == torch.gather(seg, 1, order), "sorted top-k keys")
    all_true(oi2[:, :L].to(torch.int64) == order, "sorted top-k indices")
    rows = STEP // k
    for a in range(0, S_, rows):
        all_true((ov2[a:a + rows, L:] == -1) & (oi2[a:a + rows, L:] == -1), f"fillers of segments [{a}, {a + rows})")
    del keys, offs, ov, oi, seg, order


# ---------------------------------------------------------------------------------------------- one-call sorts (contract form)

@pytest.mark.parametrize("variant", ["pairs_u32", "pairs_u32_ties", "keys_u64", "pairs_u64_ties"])
def test_one_call_sort_contract_form(gpu_context, dev, variant):
    """n = 2^31 + 12345 (the contract stages: vrs_sort_form_for says so, tests/test_index_width_cpu.py): uint32 pairs with distinct keys
    h(i) and with ties h(i) >> 20, 64-bit keys mix(i), 64-bit pairs with ties mix(i) >> 44; payload = input position."""
    n = N_MID
    wide, pairs = "u64" in variant, "pairs" in variant
    kb = 8 if wide else 4
    room(dev, 2 * kb * n + (8 * n if pairs else 0) + 2 * GB)
    ctx = gpu_context
    if wide:
        f = (lambda i: ((mix(i) >> 44) & 0xFFFFF)) if "ties" in variant else mix
        keys = build(n, torch.int64, f, dev)
    else:
        f = (lambda i: h(i) >> 20) if "ties" in variant else h
        keys = build(n, torch.int32, lambda i: as_i32(f(i)), dev)
    ktmp = torch.empty_like(keys)
    w = "u64" if wide else "u32"
    if pairs:
        vals = build(n, torch.int32, lambda i: as_i32(i), dev)
        vtmp = torch.empty_like(vals)
        run(ctx, lambda a, b, c, d: ctx.check(getattr(ctx.lib, f"vrs_sort_pairs_{w}")(ctx.handle, a.handle, b.handle, c.handle, d.handle, n)),
            keys, ktmp, vals, vtmp)
        del ktmp, vtmp
        kv = (lambda a, b: ulo(keys[a:b])) if wide else (lambda a, b: u32(keys[a:b]))
        check_lex_increasing(kv, lambda a, b: u32(vals[a:b]), n)
        for a, b in chunks(n):
            p = u32(vals[a:b])
            all_true(p < n, f"payloads in [{a}, {b})")
            got = keys[a:b] if wide else u32(keys[a:b])
            all_true(got == f(p), f"key != f(payload) in [{a}, {b})")
        del vals
    else:
        run(ctx, lambda a, b: ctx.check(ctx.lib.vrs_sort_keys_u64(ctx.handle, a.handle, b.handle, n)), keys, ktmp)
        del ktmp
        for a, b in chunks(n, overlap=1):
            k = ulo(keys[a:b])
            all_true(k[1:] > k[:-1], f"not strictly increasing in [{a}, {b})")
            src = mix_inv(keys[a:b])
            all_true((src >= 0) & (src < n), f"a key that is no mix(i), i < n, in [{a}, {b})")
    del keys


# ---------------------------------------------------------------------------------------------- segmented sorts

def _segments(first, last, lengths, big):
    """Segment bounds from `first` to `last`: the cycle of `lengths` up to each fixed segment of `big` ([begin, end), in order), and
    after the last one up to `last` (a final segment ends there exactly)."""
    bounds = [first]
    for b, e in big + [(last, last)]:
        pos, c = bounds[-1], 0
        while pos + lengths[c % len(lengths)] < b:
            pos += lengths[c % len(lengths)]
            bounds.append(pos)
            c += 1
        if bounds[-1] != b:
            bounds.append(b)
        if e != b:
            bounds.append(e)
    assert bounds[-1] == last and all(x <= y for x, y in zip(bounds, bounds[1:]))
    return bounds


@pytest.mark.parametrize("width", ["u32_pairs", "u64_keys", "u64_pairs"])
def test_segmented_sort_max_size(gpu_context, dev, width):
    """Every tier: lengths 0, 1, up to and past each LDS cap, global-tier segments, one-call segments; one straddling 2^31, a one-call
    segment of 2^30 + 17 keys past 2^31.  uint32 pairs at n = 2^32 - 1 (the last segment ends at n, the keys before offsets[0] stay as
    they were); 64-bit keys and pairs at n = 2^31 + 12345 (keys outside [offsets[0], offsets[S]) at both ends untouched)."""
    wide, pairs = width.startswith("u64"), width.endswith("pairs")
    n = N_MID if wide else N_MAX
    kb = 8 if wide else 4
    room(dev, 2 * kb * n + (8 * n if pairs else 0) + 4 * GB)
    ctx = gpu_context
    wave = capi.SEGMENT_WAVE_MAX_U64 if wide else capi.SEGMENT_WAVE_MAX
    block = ((capi.SEGMENT_BLOCK_MAX_PAIRS_U64 if pairs else capi.SEGMENT_BLOCK_MAX_KEYS_U64) if wide
             else capi.SEGMENT_BLOCK_MAX_PAIRS)
    lengths = [2, 3, 64, 256, 257, wave, wave + 1, 4096, 4097, block, block + 1, 200000, 0, 1, 999999]
    t31 = 1 << 31
    if wide:  # (12345 keys past 2^31)
        big = [(t31 - 2 ** 22, t31 - 2 ** 21),                # one-call tier
               (t31 - 90000, t31 + 5000)]                     # global tier, straddling 2^31
    else:
        big = [(t31 - 2 ** 27, t31 - 2 ** 26),                # one-call tier below 2^31
               (t31 - 90000, t31 + 90000),                    # global tier, straddling 2^31
               (t31 + 2 ** 21, t31 + 2 ** 21 + 2 ** 30 + 17)]  # one-call tier past 2^31
    first, last = (777, n) if not wide else (1000, n - 999)
    bounds = _segments(first, last, lengths, big)
    nseg = len(bounds) - 1
    offs = as_i32(torch.tensor(bounds, dtype=torch.int64, device=dev))
    bnd = torch.tensor(bounds, dtype=torch.int64, device=dev)
    if wide:
        f = (lambda i: (mix(i) >> 44) & 0xFFFFF) if pairs else mix
        keys = build(n, torch.int64, f, dev)
    else:
        f = lambda i: h(i) >> 8  # noqa: E731
        keys = build(n, torch.int32, lambda i: as_i32(f(i)), dev)
    ktmp = torch.empty_like(keys)
    w = "u64" if wide else "u32"
    if pairs:
        vals = build(n, torch.int32, lambda i: as_i32(i), dev)
        vtmp = torch.empty_like(vals)
        run(ctx, lambda a, b, c, d, o: ctx.check(getattr(ctx.lib, f"vrs_sort_segments_pairs_{w}")(ctx.handle, a.handle, b.handle, c.handle,
                                                                                                      d.handle, n, o.handle, nseg)),
            keys, ktmp, vals, vtmp, offs)
        del vtmp
    else:
        run(ctx, lambda a, b, o: ctx.check(ctx.lib.vrs_sort_segments_u64(ctx.handle, a.handle, b.handle, n, o.handle, nseg)), keys, ktmp, offs)
    del ktmp
    st = vrs.segmented_stats(ctx)
    assert st["global"] > 0 and st["one_call"] > 0 and st["wave"] > 0 and st["block"] > 0

    kv = (lambda a, b: ulo(keys[a:b])) if wide else (lambda a, b: u32(keys[a:b]))
    for a, b in chunks(n):
        i = torch.arange(a, b, dtype=torch.int64, device=dev)
        inside = (i >= first) & (i < last)
        p = u32(vals[a:b]) if pairs else mix_inv(keys[a:b])  # the input position each output element came from
        # outside the segments: as made; inside: from the same segment
        all_true(inside | (p == i), f"an element outside [offsets[0], offsets[S]) moved in [{a}, {b})")
        same = torch.searchsorted(bnd, p, right=True) == torch.searchsorted(bnd, i, right=True)
        all_true(~inside | same, f"an element left its segment in [{a}, {b})")
        got = keys[a:b] if wide else u32(keys[a:b])
        all_true(got == f(p), f"key != f(position) in [{a}, {b})")
    # within a segment (key, position) strictly increasing: with the two checks above, each segment holds a permutation of its
    # elements in stable order
    pay = (lambda a, b: u32(vals[a:b])) if pairs else (lambda a, b: torch.zeros(b - a, dtype=torch.int64, device=dev))
    starts = torch.cat([torch.arange(0, first + 1, device=dev), bnd, torch.arange(last, n, device=dev)])
    check_lex_increasing(kv, pay, n, bounds=starts)
    del keys, offs, bnd, starts
    if pairs:
        del vals


# ---------------------------------------------------------------------------------------------- torch.sort drop-ins

def _rank_f32_desc(v):
    """torch's descending order of float32 as one int64 per element, ascending: NaNs first, then larger values; -0.0 == +0.0."""
    bits = v.view(torch.int32).to(torch.int64)
    mag = torch.where(bits < 0, -(bits & 0x7FFFFFFF), bits)  # a total order of the non-NaN values, -0.0 and +0.0 both 0
    return torch.where(torch.isnan(v), torch.iinfo(torch.int64).min, -mag)


def test_sort_int32_ties_past_2_31(dev):
    """vrs.sort, vrs.argsort and vrs.sort_rows of 1-D int32 with ties (h(i) >> 12 as int32: 2^20 values, 2^11 of each), n = 2^31 + 6:
    indices past 2^31 come back as int64 positions, not as negative int32 views."""
    n = 2 ** 31 + 6
    room(dev, 4 * n * 6 + 8 * n + 2 * GB)
    x = build(n, torch.int32, lambda i: (h(i) >> 12).to(torch.int32) - (1 << 19), dev)
    v, idx = vrs.sort(x)
    for a, b in chunks(n):
        ii = idx[a:b]
        all_true((ii >= 0) & (ii < n), f"indices out of range in [{a}, {b})")
        all_true(v[a:b] == x[ii], f"values != x[indices] in [{a}, {b})")
    check_lex_increasing(lambda a, b: v[a:b].to(torch.int64), lambda a, b: idx[a:b], n)
    del v
    ai = vrs.argsort(x)
    for a, b in chunks(n):
        all_true(ai[a:b] == idx[a:b], f"argsort != sort's indices in [{a}, {b})")
    del ai
    rv, ri = vrs.sort_rows(x.view(1, n), return_indices=True)
    for a, b in chunks(n):
        all_true((ri[0, a:b] == idx[a:b]) & (rv[0, a:b] == x[idx[a:b]]), f"sort_rows != sort in [{a}, {b})")
    del x, idx, rv, ri


def test_sort_float32_rows_descending(dev):
    """vrs.sort of a [3, 2^30 + 3] float32 tensor along dim 1, descending: ±0.0, NaNs and infinities among 2^21 distinct bit patterns."""
    rows, L = 3, 2 ** 30 + 3
    n = rows * L
    room(dev, 4 * n * 6 + 8 * n + 2 * GB)
    x = build(n, torch.int32, lambda i: as_i32(h(i) & 0xFF800FFF), dev).view(torch.float32).view(rows, L)
    v, idx = vrs.sort(x, dim=1, descending=True)
    step = STEP // 2
    for r in range(rows):
        for a in range(0, L, step):
            b = min(a + step + 1, L)
            ii = idx[r, a:b]
            all_true((ii >= 0) & (ii < L), f"indices out of range in row {r} [{a}, {b})")
            got = x[r][ii]
            all_true(v[r, a:b].view(torch.int32) == got.view(torch.int32), f"values != x[indices] bit for bit in row {r} [{a}, {b})")
            k = _rank_f32_desc(got)
            ok = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (ii[1:] > ii[:-1]))
            all_true(ok, f"(torch order, index) not strictly increasing in row {r} [{a}, {b})")
    del x, v, idx


def test_sort_values_int8_max_size(dev):
    """vrs.sort_values of 2^32 - 1 int8 (the bare-key path): nondecreasing, and every value as often as in the input (2^24 each, one
    value 2^24 - 1)."""
    n = N_MAX
    room(dev, n + n + 4 * n * 2 + 2 * GB)
    x = build(n, torch.int8, lambda i: ((h(i) >> 24) - 128).to(torch.int8), dev)
    v = vrs.sort_values(x)
    c_in = torch.zeros(256, dtype=torch.int64, device=dev)
    c_out = torch.zeros(256, dtype=torch.int64, device=dev)
    for a, b in chunks(n, overlap=1):
        s = v[a:b]
        all_true(s[1:] >= s[:-1], f"not nondecreasing in [{a}, {b})")
    for a, b in chunks(n):
        c_in += torch.bincount(x[a:b].to(torch.int64) + 128, minlength=256)
        c_out += torch.bincount(v[a:b].to(torch.int64) + 128, minlength=256)
    assert torch.equal(c_in, c_out)
    want = torch.full((256,), 1 << 24, dtype=torch.int64, device=dev)
    want[(h(N_MAX) >> 24)] -= 1
    assert torch.equal(c_in, want)
    del x, v
