"""GPU tests of the pool form's two scatter passes (pool_pass_a_kernel / pool_pass_b_kernel, vrs_msd_pool.hip) at the form's floor of
2^22 keys, where a tile's every route can still be taken: the passes put their key loads in flight before they look at the plan, the
placement and the claim, and a tile whose runs all lie in primary slots takes a plain write-out.  Every case compares bit for bit with
numpy.sort and asserts through vrs_one_call_pool_sorts that the form ran (or refused) as expected."""
import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

from .test_gpu_one_call import sort_pairs_once
from .test_gpu_pool import POOL_MIN, pool_counts, pool_ctx, pool_layouts, sort_and_stats  # noqa: F401  (pool_ctx: a fixture)

pytestmark = pytest.mark.gpu

TILE, SAMPLE, ROOM_FLOOR = 8192, 256, 320  # kPoolTile, kPoolSampleKeys, kPoolRoomFloor (vrs_kernels.h)


def uniform(n, seed):
    return np.random.RandomState(seed).randint(0, 2 ** 32, size=n, dtype=np.uint32)


def skewed(n, seed):
    """the second half of the input drawn from the lowest quarter of the key range: slices 4 .. 7 hold four times the keys per region
    in a quarter of the regions"""
    k = uniform(n, seed)
    k[n // 2:] >>= np.uint32(2)
    return k


def first_pass_regions(keys, top_bits=7):
    """pool_layout_kernel's arithmetic on the host (float32 as there), for 32-bit keys: per (slice, top digit) the keys the region
    really receives, its primary slots, its overflow room and its longest run (one tile's keys with that digit)"""
    n = keys.size
    tiles = (n + TILE - 1) // TILE
    per = max((tiles + 7) // 8, 1)
    digit = keys >> np.uint32(32 - top_bits)
    sampled_pos = (np.arange(n) % TILE) < SAMPLE
    out = []
    for s in range(8):
        a, b = min(s * per * TILE, n), min((s + 1) * per * TILE, n)
        length = b - a
        if length == 0:
            continue
        true = np.bincount(digit[a:b], minlength=1 << top_bits)
        m = np.bincount(digit[a:b][sampled_pos[a:b]], minlength=1 << top_bits)
        sampled = (length // TILE) * SAMPLE + min(length % TILE, SAMPLE)
        r = np.float32(length) / np.float32(sampled)
        est = np.minimum((m.astype(np.float32) * r * np.float32(0.999999)).astype(np.uint32), np.uint32(length))
        cap = est & ~np.uint32(31)
        dev = (np.float32(6.0) * np.sqrt(r * (est.astype(np.float32) + r))).astype(np.uint32)
        room = (dev + (est - cap) + np.uint32(ROOM_FLOOR + 31)) & ~np.uint32(31)
        tile_of = np.arange(length) // TILE
        runs = np.bincount(tile_of * (1 << top_bits) + digit[a:b], minlength=(tile_of[-1] + 1) << top_bits).reshape(-1, 1 << top_bits)
        out.append((true.astype(np.int64), cap.astype(np.int64), room.astype(np.int64), runs.max(axis=0).astype(np.int64)))
    return out


def test_the_skewed_input_overflows_primary_regions_without_outgrowing_their_room():
    """(no GPU: the inputs' own check) in the skewed case runs must straddle into overflow slots and lie wholly in them -- pass A's slow
    store -- and no region may outgrow its room, which would refuse the sort"""
    regions = first_pass_regions(skewed(POOL_MIN, seed=21))
    over = sum(int(np.count_nonzero(true > cap)) for true, cap, _, _ in regions)
    # more than two runs behind the primary part: the run that crosses its end covers at most one of them, whole runs the rest
    deep = sum(int(np.count_nonzero(true > cap + 2 * run)) for true, cap, _, run in regions)
    assert over >= 100 and deep >= 10
    assert all(np.all(true <= cap + room) for true, cap, room, _ in regions)


@pytest.mark.parametrize("n", [POOL_MIN, POOL_MIN + 8191, POOL_MIN + 1])
def test_uniform_keys_and_ragged_last_tiles(pool_ctx, n):
    """uniform keys: the plain write-out on both passes; + 8191 / + 1: a ragged last tile per slice and per top byte, the padding key's digit"""
    keys = uniform(n, seed=n % 1013)
    out, stats, (took, refused) = sort_and_stats(pool_ctx, keys)
    assert np.array_equal(out, np.sort(keys))
    assert (took, refused) == (1, 0)
    assert stats["pool_pass_a"] == 1 and stats["pool_pass_b"] == 1 and stats["local_sort"] == 1 and stats["digit_tables"] == 0


def test_skewed_second_half_takes_the_slow_store(pool_ctx):
    keys = skewed(POOL_MIN, seed=21)
    out, stats, (took, refused) = sort_and_stats(pool_ctx, keys)
    assert np.array_equal(out, np.sort(keys))
    assert (took, refused) == (1, 0) and stats["pool_pass_a"] == 1 and stats["digit_tables"] == 0


def test_sorted_keys(pool_ctx):
    """uniform-digit waves, tiles wholly inside one digit"""
    keys = np.sort(uniform(POOL_MIN, seed=5))
    out, _, (took, refused) = sort_and_stats(pool_ctx, keys)
    assert np.array_equal(out, keys)
    assert took + refused == 1  # (ordered input: whether a verdict refuses is the form's business, tests/test_gpu_pool.py)


def test_28_bit_keys(pool_ctx):
    """the bucket shift below 18"""
    keys = uniform(POOL_MIN, seed=6) >> np.uint32(4)
    out, stats, (took, refused) = sort_and_stats(pool_ctx, keys)
    assert np.array_equal(out, np.sort(keys))
    assert (took, refused) == (1, 0) and stats["pool_pass_a"] == 1 and stats["pool_pass_b"] == 1


def test_kept_layout_then_a_stale_one():
    """two sorts back to back on one context -- the second in the first one's layout and rooms --, then 28-bit keys: stale, run again"""
    with vrs.GPUContext(0) as gpu:
        gpu.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, POOL_MIN)
        gpu.setTuning(capi.VRS_TUNE_MSD_POOL_MIN_KEYS, POOL_MIN)
        gpu.setTuning(capi.VRS_TUNE_MSD_POOL, 2)
        for seed, layouts, samples in ((1, (0, 0), 1), (2, (1, 0), 0)):
            keys = uniform(POOL_MIN, seed=seed)
            out, stats, (took, refused) = sort_and_stats(gpu, keys)
            assert np.array_equal(out, np.sort(keys))
            assert (took, refused) == (1, 0) and stats["pool_sample"] == samples and stats["pool_pass_a"] == 1
            assert pool_layouts(gpu) == layouts
        keys = uniform(POOL_MIN, seed=3) >> np.uint32(4)
        out, stats, (took, refused) = sort_and_stats(gpu, keys)
        assert np.array_equal(out, np.sort(keys))
        assert (took, refused) == (1, 0) and stats["pool_sample"] == 1 and stats["pool_pass_a"] == 2
        assert pool_layouts(gpu) == (2, 1)


def test_pairs_stay_stable(pool_ctx):
    """the stable passes share the entry sequence: many ties, compared with a stable argsort"""
    n = POOL_MIN
    keys = uniform(n, seed=8) & np.uint32(0xFFFF00FF)
    vals = np.arange(n, dtype=np.uint32)
    before = pool_counts(pool_ctx)
    ok, ov = sort_pairs_once(pool_ctx, keys, vals)
    after = pool_counts(pool_ctx)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(ok, keys[order]) and np.array_equal(ov, vals[order])
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)


def test_key_loads_ahead_of_the_placement_check():
    """The first pass loads its tile before it looks at where it runs.  With the probed order rotated (the hook as tests/test_gpu_pool.py
    sets it) every workgroup still finds its list by the XCC it runs on: taken, exact -- neither VRS_TUNE_DEBUG_XCC_ROTATE nor
    VRS_TUNE_DEBUG_XCC_STRAY_BLOCK can make a pool pass refuse (the first leaves the form taken, the second keeps it from starting).  With odd tiles read from the neighbouring slice
    (VRS_TUNE_DEBUG_MISPLACE_STREAMS) and slices that differ, the regions the sample sized do not fit: whatever the verdict, the caller's
    keys come back sorted -- after a refusal from the untouched input, by the counted form."""
    with vrs.GPUContext(0) as gpu:
        gpu.setTuning(capi.VRS_TUNE_HYBRID_MIN_KEYS, POOL_MIN)
        gpu.setTuning(capi.VRS_TUNE_MSD_POOL_MIN_KEYS, POOL_MIN)
        gpu.setTuning(capi.VRS_TUNE_MSD_POOL, 2)
        gpu.setTuning(capi.VRS_TUNE_DEBUG_XCC_ROTATE, 3)
        keys = uniform(POOL_MIN + 8191, seed=9)
        out, _, (took, refused) = sort_and_stats(gpu, keys)
        assert np.array_equal(out, np.sort(keys))
        assert (took, refused) == (1, 0)
        gpu.setTuning(capi.VRS_TUNE_DEBUG_MISPLACE_STREAMS, 1)
        keys = uniform(POOL_MIN, seed=10)
        keys[: POOL_MIN // 2] >>= np.uint32(1)
        keys[POOL_MIN // 2:] |= np.uint32(0x80000000)
        out, stats, (took, refused) = sort_and_stats(gpu, keys)
        assert np.array_equal(out, np.sort(keys))
        assert took + refused == 1
        if refused:
            assert stats["digit_tables"] >= 1  # the counted form ran on the untouched input
