"""The top-k selection's classification (vrs_topk_tier_for), scratch size (vrs_topk_scratch_bytes) and argument checks: no device."""
import ctypes

import pytest

from vkradixsort_amd import capi

LDS = capi.TOPK_LDS_MAX
MIB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def tier_for(lib, b, e, n, grid_min=capi.TOPK_GRID_MIN_KEYS_DEFAULT):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_topk_tier_for(b, e, n, grid_min, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
    return t.value, cb.value, ce.value


def segment_clamp(lib, b, e, n):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for(b, e, n, 0, 0, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
    return cb.value, ce.value


def scratch(lib, n, S, k, flags=capi.VRS_TOPK_SORTED):
    out = ctypes.c_uint64(12345)
    rc = lib.vrs_topk_scratch_bytes(n, S, k, flags, ctypes.byref(out))
    return rc, out.value


def test_every_tier_boundary(lib):
    thr = capi.TOPK_GRID_MIN_KEYS_DEFAULT
    n = 1 << 24
    cases = {0: capi.VRS_TOPK_LDS, 1: capi.VRS_TOPK_LDS, LDS - 1: capi.VRS_TOPK_LDS, LDS: capi.VRS_TOPK_LDS, LDS + 1: capi.VRS_TOPK_BLOCK,
             thr - 1: capi.VRS_TOPK_BLOCK, thr: capi.VRS_TOPK_GRID, thr + 1: capi.VRS_TOPK_GRID, n: capi.VRS_TOPK_GRID}
    for length, tier in cases.items():
        for b in (0, 3, 12345):
            if b + length <= n:
                assert tier_for(lib, b, b + length, n) == (tier, b, b + length), (length, b)


def test_threshold_setting(lib):
    n = 1 << 24
    assert tier_for(lib, 0, 1 << 23, n, 0)[0] == capi.VRS_TOPK_BLOCK  # 0: never the grid tier
    assert tier_for(lib, 0, n, n, 0)[0] == capi.VRS_TOPK_BLOCK
    for thr in (20000, 20001):
        assert tier_for(lib, 0, thr - 1, n, thr)[0] == capi.VRS_TOPK_BLOCK
        assert tier_for(lib, 0, thr, n, thr)[0] == capi.VRS_TOPK_GRID
        assert tier_for(lib, 0, thr + 1, n, thr)[0] == capi.VRS_TOPK_GRID
    # the LDS tier comes first, whatever the threshold
    for thr in (1, 100, LDS):
        assert tier_for(lib, 0, LDS, n, thr)[0] == capi.VRS_TOPK_LDS
        assert tier_for(lib, 0, LDS + 1, n, thr)[0] == capi.VRS_TOPK_GRID


def test_malformed_ranges_clamp_as_segmented(lib):
    n = 100000
    for b, e in [(5, 3), (n - 2, n + 10), (n + 7, n + 20), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (40000, 40000), (123, 99999),
                 (n, n), (0, n), (n + 1, 5)]:
        t, cb, ce = tier_for(lib, b, e, n)
        assert (cb, ce) == segment_clamp(lib, b, e, n), (b, e)
        assert cb <= ce <= n
        assert t == (capi.VRS_TOPK_LDS if ce - cb <= LDS else capi.VRS_TOPK_BLOCK)
    assert tier_for(lib, 5, 3, n) == (capi.VRS_TOPK_LDS, 5, 5)
    assert tier_for(lib, n - 2, n + 10, n) == (capi.VRS_TOPK_LDS, n - 2, n)


def test_tier_for_null_outputs(lib):
    t = ctypes.c_int()
    assert lib.vrs_topk_tier_for(0, 1, 1, 0, ctypes.byref(t), None, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_scratch_bytes_monotone_and_bounded(lib):
    ns = [0, 1, 1000, 8192, 8193, 16384, 100000, 1 << 20, 10 ** 8, (1 << 32) - 1]
    Ss = [1, 2, 64, 4096, 100000, 1 << 20]
    ks = [1, 10, 64, 1024, 4096, 4097, 65536]
    for flags in (0, capi.VRS_TOPK_SORTED, capi.VRS_TOPK_SORTED | capi.VRS_TOPK_LARGEST):
        for S in Ss:
            for k in ks:
                if S * k >= 1 << 32:
                    continue
                prev = -1
                for n in ns:
                    rc, b = scratch(lib, n, S, k, flags)
                    assert rc == capi.VRS_OK
                    assert b <= 4 * n + 16 * S * k + MIB, (n, S, k, flags, b)
                    assert b >= prev, (n, S, k, flags)
                    prev = b
        for n in (1000, 10 ** 6, 10 ** 8):
            for k in ks:
                prev = -1
                for S in Ss:
                    if S * k >= 1 << 32:
                        continue
                    b = scratch(lib, n, S, k, flags)[1]
                    assert b >= prev
                    prev = b
            for S in Ss:
                prev = -1
                for k in ks:
                    if S * k >= 1 << 32:
                        continue
                    b = scratch(lib, n, S, k, flags)[1]
                    assert b >= prev
                    prev = b


def test_scratch_bytes_rejects(lib):
    assert scratch(lib, 100, 1 << 16, 1 << 16)[0] == capi.VRS_ERROR_INVALID_ARGUMENT  # S * k == 2^32
    assert scratch(lib, 100, (1 << 16) + 1, 1 << 16)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert scratch(lib, 100, 0xFFFFFFFF, 2)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert scratch(lib, 100, (1 << 16) - 1, 1 << 16)[0] == capi.VRS_OK
    assert scratch(lib, 100, 4, 8, 4)[0] == capi.VRS_ERROR_INVALID_ARGUMENT  # unknown flag bit
    assert scratch(lib, 100, 0, 8) == (capi.VRS_OK, 0)
    assert scratch(lib, 100, 4, 0) == (capi.VRS_OK, 0)
    assert lib.vrs_topk_scratch_bytes(1, 1, 1, 0, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def call(lib, ctx=None, key_type=capi.VRS_TOPK_F32, flags=capi.VRS_TOPK_SORTED, S=1, k=1):
    return lib.vrs_topk_segments(ctx, None, 10, None, S, k, key_type, flags, None, None, None)


def test_invalid_arguments(lib):
    assert call(lib) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"NULL" in lib.vrs_last_error(None)
    for kt in (-1, 3, 99):
        assert call(lib, key_type=kt) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"key_type" in lib.vrs_last_error(None)
    for fl in (4, 8, -1, 1 << 30):
        assert call(lib, flags=fl) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"flag" in lib.vrs_last_error(None)
    assert call(lib, S=1 << 16, k=1 << 16) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"2^32" in lib.vrs_last_error(None)
    s = ctypes.c_uint64()
    assert lib.vrs_topk_stats(None, ctypes.byref(s), None, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_torch_level_refusals():
    torch = pytest.importorskip("torch")
    from vkradixsort_amd import VrsError, topk

    with pytest.raises(VrsError):
        topk(torch.arange(10, dtype=torch.float32), 3)  # a CPU tensor
    if not torch.cuda.is_available():
        return
    dev = "cuda"
    for dt in (torch.float64, torch.int64, torch.float16, torch.uint8):
        with pytest.raises(VrsError):
            topk(torch.zeros(8, dtype=dt, device=dev), 2)
    x = torch.zeros(4, 8, dtype=torch.float32, device=dev)
    with pytest.raises(VrsError):
        topk(x, 2, dim=0)
    with pytest.raises(VrsError):
        topk(x, 9)
    with pytest.raises(VrsError):
        topk(torch.zeros(2, 2, 2, device=dev), 1)


def test_torch_level_refusals_without_device():
    """The checks that come before any device work: dtype, dim and k are refused for CPU tensors too (the GPU check comes first)."""
    torch = pytest.importorskip("torch")
    from vkradixsort_amd import VrsError, topk

    for args in [(torch.zeros(8, dtype=torch.float64), 2), (torch.zeros(4, 8), 2, 0), (torch.zeros(4, 8), 9)]:
        with pytest.raises(VrsError):
            topk(*args)
