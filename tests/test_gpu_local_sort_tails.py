"""The LDS local sorts' handling of slots WITHOUT a key (vrs_local_sort.hpp: lean_sort_body, wave_sort_body).  A bucket is read and written as
rows of 16-byte vectors; the slots of its first and last vectors that hold no key of the bucket take a dummy counter in both 9-bit passes and
are put in their place afterwards (every counter read is issued first, the selects follow: DESIGN.md K5c).  What can go wrong is a bucket whose
size or placement puts those slots somewhere unusual, so the inputs here are built bucket by bucket:

  * key = (prefix << 18) | 18 random bits, P 14-bit prefixes that include 0 and 16383 (a 32-bit key range), N = 2^22 + {1, 2, 3, 1021} keys;
    P = 2800 / 1366 / 683 / 341 gives buckets of about 1500 / 3070 / 6140 / 12300 keys: the one-wave kernel, 256 x 16, 256 x 28 (rows 6 and 7:
    what 10^8 uniform keys give) and 512 x 28;
  * for every n mod (4 THREADS) in {0, 1, 2, 3, 4 THREADS - 3 .. 4 THREADS - 1} and every misalignment 0 .. 3 of the bucket's place one bucket
    is made exactly so, one bucket ends in the middle of each row count, and one has the shape's largest size (which also decides the shape:
    the pool form enqueues the one-wave kernel from N alone and retries in the shape the fullest bucket needs).

The pool form reads a bucket from its own aligned region (slots without a key at the end only); the counted hybrid form sorts it in place
(slots in front of the bucket as well).  Both must equal numpy.sort bit for bit, and must have been taken: a refusal fails the test.
local_pass (the pairs' bodies) shares the scans' wave sum: one stable-argsort case per pairs body at the end."""
import ctypes
import functools

import numpy as np
import pytest

import vkradixsort_amd as vrs  # noqa: F401
from vkradixsort_amd import capi

from .test_gpu_one_call import hybrid_sorts, sort_keys
from .test_gpu_pool import POOL_MIN, sort_and_stats, sort_pairs_and_stats

# shape: (P, threads of a row, rows, the next smaller shape's capacity, local sorts the pool form launches)
SHAPES = {
    "wave": (2800, 64, 7, 0, 1),
    "256x16": (1366, 256, 4, 64 * 28 - 3, 2),
    "256x28": (683, 256, 7, 256 * 16 - 3, 2),
    "512x28": (341, 512, 7, 256 * 28 - 3, 2),
}
SIZES = [(1 << 22) + extra for extra in (1, 2, 3, 1021)]
CASES = [(n, shape) for shape in SHAPES for n in SIZES]
GPU_CASES = [(n, shape, form) for n, shape in CASES for form in ("pool", "counted")]  # the two forms of one input run back to back


def capacity(shape):
    _, threads, rows, _, _ = SHAPES[shape]
    return 4 * threads * rows - 3


def forced_buckets(shape, mean):
    """[(misalignment, keys)] of the buckets made on purpose: every residue of n by a row x every misalignment, around the mean bucket; the middle
    of every row count; the shape's capacity"""
    _, threads, rows, _, _ = SHAPES[shape]
    row = 4 * threads
    near = max(round(mean / row), 1) * row
    want = [(mis, near + r) for r in (0, 1, 2, 3, -3, -2, -1) for mis in range(4)]
    want += [(r % 4, r * row - row // 2 + 1) for r in range(1, rows + 1)]
    want.append((3, capacity(shape)))
    return want


def bucket_plan(n, shape, seed):
    """(prefixes ascending, keys per prefix): the forced buckets, each behind a filler bucket that sets its misalignment, and the rest of the n
    keys dealt out evenly (multinomial) over the other prefixes"""
    P = SHAPES[shape][0]
    rs = np.random.RandomState(seed)
    prefixes = np.sort(np.concatenate(([0, 16383], rs.choice(np.arange(1, 16383), P - 2, replace=False)))).astype(np.uint32)
    counts = np.zeros(P, np.int64)
    want = forced_buckets(shape, n / P)
    forced = np.zeros(P, bool)
    at = 1 + 2 * np.arange(len(want)) * ((P - 2) // (2 * len(want)))  # (filler, forced) pairs spread over the prefixes
    for i, (mis, keys) in zip(at, want):
        counts[i + 1] = keys
        forced[i] = forced[i + 1] = True
    free = ~forced
    filler_mean = n // P
    rest = n - counts.sum() - filler_mean * len(want)
    counts[free] = rs.multinomial(rest, np.full(free.sum(), 1.0 / free.sum()))
    # the fillers, in ascending order: whatever lies before them is final by now
    for i, (mis, keys) in zip(at, want):
        before = int(counts[:i].sum())
        counts[i] = filler_mean - 4 + (mis - before - (filler_mean - 4)) % 4
    counts[np.flatnonzero(free)[-1]] += n - counts.sum()  # (the fillers' rounding)
    return prefixes, counts


@functools.lru_cache(maxsize=2)
def tail_keys(n, shape):
    """(keys, numpy.sort(keys)) -- built once per (n, shape) and shared by the two forms' cases, which GPU_CASES orders one after the other"""
    prefixes, counts = bucket_plan(n, shape, seed=n % 1009 + len(shape))
    rs = np.random.RandomState(n % 977)
    keys = (np.repeat(prefixes, counts) << np.uint32(18)) | rs.randint(0, 1 << 18, size=n).astype(np.uint32)
    keys = keys[rs.permutation(n)]
    keys.setflags(write=False)
    ref = np.sort(keys)
    ref.setflags(write=False)
    return keys, ref


@pytest.mark.parametrize("n,shape", CASES)
def test_the_generator_gives_the_intended_buckets(n, shape):
    """CPU only: bucket sizes, residues, misalignments and row counts are what the GPU tests below rely on"""
    P, threads, rows, below, _ = SHAPES[shape]
    prefixes, counts = bucket_plan(n, shape, seed=n % 1009 + len(shape))
    assert counts.sum() == n and counts.min() > 0 and prefixes[0] == 0 and prefixes[-1] == 16383 and np.unique(prefixes).size == P
    assert below < counts.max() == capacity(shape)  # the fullest bucket needs exactly this shape
    row = 4 * threads
    mis = (np.cumsum(counts) - counts) % 4  # (the sorted output starts on a 16-byte boundary)
    seen = {(int(m), int(c % row)) for m, c in zip(mis, counts)}
    for r in (0, 1, 2, 3, row - 3, row - 2, row - 1):
        for m in range(4):
            assert (m, r) in seen, (m, r)
    assert {int(v) for v in (mis + counts + row - 1) // row} >= set(range(1, rows + 1))  # every row count
    # the typical bucket is the module docstring's (1500 / 3070 / 6140 / 12300 keys)
    assert abs(np.median(counts) - n / P) < 0.05 * n / P
    if n == SIZES[0]:  # the keys themselves, once per shape
        keys, ref = tail_keys(n, shape)
        assert np.array_equal(np.bincount(keys >> np.uint32(18), minlength=1 << 14)[prefixes], counts)
        assert int(keys.max()).bit_length() == 32 and ref[0] >> 18 == 0


def pool_retries(ctx):
    r = ctypes.c_uint64()
    ctx.check(ctx.lib.vrs_one_call_pool_retries(ctx.handle, ctypes.byref(r)))
    return r.value


def pool_form(ctx, n, shape, keys, ref):
    # the buckets the form cuts at this size are the keys' 14-bit prefixes (7 + 7 bits): a coarser cut would merge the buckets built above
    first, second = ctypes.c_uint32(), ctypes.c_uint32()
    ctx.check(ctx.lib.vrs_pool_form_shape_ex(n, 0, 7, ctypes.byref(first), ctypes.byref(second), None, None))
    assert first.value + second.value == 14
    ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, POOL_MIN)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL_MIN_KEYS, POOL_MIN)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 2)
    r0 = pool_retries(ctx)
    try:
        out, stats, (took, refused) = sort_and_stats(ctx, keys)
    finally:
        ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 1)
        ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, capi.HYBRID_MIN_KEYS_DEFAULT)
    launches = SHAPES[shape][4]
    # the form took the sort; N alone enqueues the one-wave kernel, and the fullest bucket (the shape's capacity, above the next smaller
    # shape's: the CPU test above) decides which larger shape finishes it -- the host takes the smallest shape that holds it
    assert (took, refused) == (1, 0), stats
    assert pool_retries(ctx) - r0 == launches - 1 and stats["local_sort"] == launches and stats["digit_tables"] == 0, stats
    assert stats["pool_pass_a"] == 1 and stats["pool_pass_b"] == 1, stats
    assert np.array_equal(out, ref)


def counted_form(ctx, keys, ref):
    """VRS_TUNE_MSD_POOL = 0: the counted hybrid form at the smallest size the library takes it (VRS_TUNE_HYBRID_MIN_KEYS = 2^22), blocking, so
    that the plan picks the local sort's shape from the fullest bucket (one wave / 256 x 28 / 512 x 28).  The buckets are sorted where they lie:
    slots in front of a bucket hold the neighbour's keys."""
    ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, 1 << 22)
    ctx.setTuning(capi.VRS_TUNE_HYBRID, 1)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 0)
    ctx.setTuning(capi.VRS_TUNE_ASYNC_SORT, 0)
    h0 = hybrid_sorts(ctx)
    try:
        out, stats = sort_keys(ctx, keys)
    finally:
        ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, capi.HYBRID_MIN_KEYS_DEFAULT)
        ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 1)
        ctx.setTuning(capi.VRS_TUNE_ASYNC_SORT, 1)
    assert hybrid_sorts(ctx) - h0 == 1 and stats["local_sort"] == 1 and stats["lookback_scatter"] == 2, stats
    assert np.array_equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape,form", GPU_CASES)
def test_buckets_with_every_tail(gpu_context, n, shape, form):
    keys, ref = tail_keys(n, shape)
    if form == "pool":
        pool_form(gpu_context, n, shape, keys, ref)
    else:
        counted_form(gpu_context, keys, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("body", ["pool_packed", "pool_unpacked", "counted"])
def test_pairs_bodies_against_a_stable_argsort(gpu_context, body):
    """local_pass serves local_sort_packed_pairs_to, local_sort_bucket_to (the pool form's two pairs bodies) and the counted form's pairs
    kernel: 2^22 + 1021 pairs whose keys tie often (12 random bits below the 14-bit bucket), payload = input position."""
    ctx = gpu_context
    n = SIZES[-1]
    rs = np.random.RandomState(77)
    keys = (rs.randint(0, 1 << 14, size=n).astype(np.uint32) << np.uint32(18)) | (rs.randint(0, 1 << 12, size=n).astype(np.uint32) << np.uint32(3))
    keys[:2] = (0, 0xFFFFFFFF)
    vals = np.arange(n, dtype=np.uint32)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, POOL_MIN)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL_MIN_KEYS, POOL_MIN)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 2 if body != "counted" else 0)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL_PAIRS_PACKED, 1 if body == "pool_packed" else 0)
    h0 = hybrid_sorts(ctx)
    try:
        ok, ov, stats, (took, refused) = sort_pairs_and_stats(ctx, keys, vals)
    finally:
        ctx.setTuning(capi.VRS_TUNE_MSD_POOL_PAIRS_PACKED, -1)
        ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 1)
        ctx.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, capi.HYBRID_MIN_KEYS_DEFAULT)
    assert (took, refused) == ((1, 0) if body != "counted" else (0, 0)), stats
    assert hybrid_sorts(ctx) - h0 == 1 and stats["local_sort"] == 1, stats
    assert np.array_equal(ov, order) and np.array_equal(ok, keys[order])
