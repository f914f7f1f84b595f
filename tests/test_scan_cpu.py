"""The prefix scan over rows (vrs_scan_rows, header section "K14") without a device: the host restatement of the fixed order against
numpy, torch on the CPU and an independent evaluation of the order's formulas, its rounding-error bound, and the pure companions.

vrs_scan_rows_host compiles the functions the kernels compile (csrc/vrs_scan_order.hpp); tests/test_gpu_scan.py holds the device to it
bit for bit, so what is pinned here is pinned for the device too.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from vkradixsort_amd import capi

ROOT = Path(__file__).resolve().parent.parent
F = capi.SCAN_FAN
SUM, PROD, MAX, MIN = capi.VRS_SCAN_SUM, capi.VRS_SCAN_PROD, capi.VRS_SCAN_MAX, capi.VRS_SCAN_MIN
CODES = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16, torch.int32: capi.VRS_SORT_INT32,
         torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16, torch.bfloat16: capi.VRS_SORT_BFLOAT16,
         torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
ARITH = [torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64]
WIDENED = [torch.int8, torch.uint8, torch.int16, torch.int32]


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def bits(t):
    """the tensor's bytes as integers of its width (NaN payloads and the sign of zero compare)"""
    return t.contiguous().view(BITS[t.element_size()])


def host_scan(lib, x, op, T, out_dtype=None):
    """vrs_scan_rows_host of the [S, L, C] torch tensor x: (out, indices or None)"""
    S, L, C = x.shape
    out_dtype = out_dtype or x.dtype
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=out_dtype)
    idx = torch.empty(x.shape, dtype=torch.int64) if op in (MAX, MIN) else None
    rc = lib.vrs_scan_rows_host(x.data_ptr(), S, L, C, CODES[x.dtype], CODES[out_dtype], op, T, out.data_ptr(), idx.data_ptr() if idx is not None else None)
    assert rc == capi.VRS_OK, rc
    return out, idx


def u32(fn, *args):
    out = ctypes.c_uint32()
    assert fn(*args, ctypes.byref(out)) == capi.VRS_OK
    return out.value


def levels_of(L, T):
    tiles = -(-L // T)
    if tiles <= 1:
        return 0
    K, cap = 1, F
    while cap < tiles:
        K, cap = K + 1, cap * F
    return K


# ---------------------------------------------------------------------------------------------- the order, evaluated independently

def order_in_python(x, T, flat, op):
    """out of one column x (1-D float32) by the formulas of the header's section K14, in numpy float32 arithmetic, all tiles at once."""
    f32 = np.float32
    comb = (lambda a, b: a + b) if op == SUM else (lambda a, b: a * b)
    ident = f32(0) if op == SUM else f32(1)
    L = len(x)
    tiles = -(-L // T)
    padded = np.full(tiles * T, ident, dtype=f32)
    padded[:L] = x
    if flat:
        nc = T // 256
        X = padded.reshape(tiles, nc, 64, 4)
        a = np.full((tiles, nc, 64), ident, dtype=f32)
        for k in range(4):
            a = comb(a, X[..., k])
        d = 1
        while d < 64:
            nxt = a.copy()
            nxt[..., d:] = comb(a[..., :-d], a[..., d:])
            a, d = nxt, d * 2
        E = np.concatenate((np.full((tiles, nc, 1), ident, dtype=f32), a[..., :-1]), axis=-1)
        Q = np.full((tiles, nc + 1), ident, dtype=f32)
        for q in range(nc):
            Q[:, q + 1] = comb(Q[:, q], a[:, q, 63])
        v = comb(Q[:, :nc, None], E)
        incl = np.empty_like(X)
        for k in range(4):
            v = comb(v, X[..., k])
            incl[..., k] = v
        aggregate = Q[:, nc]
    else:
        runs = T // 16
        X = padded.reshape(tiles, runs, 16)
        local = np.full((tiles, runs), ident, dtype=f32)
        locals_ = np.empty_like(X)
        for r in range(16):
            local = comb(local, X[..., r])
            locals_[..., r] = local
        Q = np.full((tiles, runs + 1), ident, dtype=f32)
        for q in range(runs):
            Q[:, q + 1] = comb(Q[:, q], local[:, q])
        incl = comb(Q[:, :runs, None], locals_)
        aggregate = Q[:, runs]
    incl = incl.reshape(tiles, T)
    if tiles == 1:
        return incl.reshape(-1)[:L]
    K = levels_of(L, T)
    A = [aggregate]
    for k in range(1, K):
        full = tiles // F ** k
        below = A[k - 1][:full * F].reshape(full, F)
        acc = np.full(full, ident, dtype=f32)
        for i in range(F):
            acc = comb(acc, below[:, i])
        A.append(acc)
    j = np.arange(tiles)
    P = np.full(tiles, ident, dtype=f32)
    for k in range(K - 1, -1, -1):
        lo, hi = F * (j // F ** (k + 1)), j // F ** k
        words = np.concatenate((A[k], np.full(1, ident, dtype=f32)))
        for i in range(F - 1):
            m = lo + i
            P = np.where(m < hi, comb(P, words[np.minimum(m, len(words) - 1)]), P)
    return comb(P[:, None], incl).reshape(-1)[:L]


ORDER_CASES = [(1, 256), (255, 256), (256, 256), (257, 256), (700, 512), (F * 256, 256), (F * 256 + 1, 256), (3 * F * 256 + 77, 256), (F * F * 256 + 1, 256),
               (F * F * 256 + F * 256 + 300, 256), (5000, 2048), (F * 512 + 9, 512)]


@pytest.mark.parametrize("L,T", ORDER_CASES)
@pytest.mark.parametrize("op", [SUM, PROD], ids=["sum", "prod"])
def test_flat_order_is_the_formulas(lib, L, T, op):
    rng = np.random.default_rng(L + T + op)
    x = rng.standard_normal(L).astype(np.float32) if op == SUM else (1 + 0.01 * rng.standard_normal(L)).astype(np.float32)
    got, _ = host_scan(lib, torch.from_numpy(x).view(1, L, 1), op, T)
    want = order_in_python(x, T, True, op)
    assert np.array_equal(got.view(-1).numpy().view(np.uint32), want.view(np.uint32)), (L, T)


@pytest.mark.parametrize("L,T", [(1, 256), (15, 256), (16, 256), (17, 256), (256, 256), (257, 256), (F * 256 + 1, 256), (F * F * 256 + 1, 256), (1300, 512)])
@pytest.mark.parametrize("op", [SUM, PROD], ids=["sum", "prod"])
def test_columns_order_is_the_formulas(lib, L, T, op):
    rng = np.random.default_rng(L * 3 + T + op)
    C = 2
    x = rng.standard_normal((L, C)).astype(np.float32) if op == SUM else (1 + 0.01 * rng.standard_normal((L, C))).astype(np.float32)
    got, _ = host_scan(lib, torch.from_numpy(x).view(1, L, C), op, T)
    for c in range(C):
        want = order_in_python(np.ascontiguousarray(x[:, c]), T, False, op)
        assert np.array_equal(got[0, :, c].contiguous().numpy().view(np.uint32), want.view(np.uint32)), (L, T, c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_16_bit_sums_are_the_float32_order_rounded_once(lib, dtype):
    L, T = 3 * 256 + 41, 256
    x = (torch.rand(L, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dtype)
    got, _ = host_scan(lib, x.view(1, L, 1), SUM, T)
    want = torch.from_numpy(order_in_python(x.float().numpy(), T, True, SUM)).to(dtype)  # (torch rounds to nearest even)
    assert torch.equal(bits(got.view(-1)), bits(want))


def test_a_float_sum_starts_at_plus_zero(lib):
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        x = torch.tensor([-0.0, -0.0, 0.0], dtype=dtype)
        got, _ = host_scan(lib, x.view(1, 3, 1), SUM, 256)
        want = torch.cumsum(x, 0)
        assert torch.equal(bits(got.view(-1)), bits(want)) and not torch.signbit(got).any()


# ---------------------------------------------------------------------------------------------- the rounding-error bound

def half_ulp(v, dtype):
    """half a unit in the last place of the float16 / bfloat16 values v (given as float64)"""
    p, lowest = (10, -24) if dtype == torch.float16 else (7, -133)
    _, e = np.frexp(np.abs(v))
    return 0.5 * np.exp2(np.maximum(e - 1 - p, lowest).astype(np.float64))


@pytest.mark.parametrize("L,C,T", [(100000, 1, 256), (100000, 1, 2048), (F * F * 256 + 1, 1, 256), (40000, 3, 256), (40000, 3, 8192)])
def test_float32_error_grows_with_depth_not_length(lib, L, C, T):
    x = torch.randn(1, L, C, generator=torch.Generator().manual_seed(L + C + T))
    got, _ = host_scan(lib, x, SUM, T)
    depth = u32(lib.vrs_scan_depth_for, L, C, T)
    exact = torch.cumsum(x.double(), 1)
    bound = 1.01 * depth * 2.0 ** -24 * torch.cumsum(x.double().abs(), 1)
    assert depth <= T + F * (levels_of(L, T) + 1)
    assert ((got.double() - exact).abs() <= bound).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("L,C,T", [(3000, 1, 256), (3000, 2, 256), (3000, 1, 2048)])
def test_16_bit_error_bound(lib, dtype, L, C, T):
    x = (torch.rand(1, L, C, generator=torch.Generator().manual_seed(L + C + T)) * 2 - 1).to(dtype)
    got, _ = host_scan(lib, x, SUM, T)
    depth = u32(lib.vrs_scan_depth_for, L, C, T)
    exact = torch.cumsum(x.double(), 1)
    bound = 1.01 * depth * 2.0 ** -24 * torch.cumsum(x.double().abs(), 1) + torch.from_numpy(half_ulp(got.double().numpy(), dtype))
    assert ((got.double() - exact).abs() <= bound).all()


@pytest.mark.parametrize("L", [2 ** 24, 2 ** 32 - 1])
def test_depth_stays_within_the_bound(lib, L):
    for T in (256, 512, 2048, 4096, 8192):
        K = u32(lib.vrs_scan_levels_for, L, T)
        assert K == levels_of(L, T)
        for C in (1, 2, 64, 1000):
            depth = u32(lib.vrs_scan_depth_for, L, C, T)
            assert 0 < depth <= T + F * (K + 1), (L, T, C, depth)
    assert u32(lib.vrs_scan_levels_for, 2 ** 24, 256) == 3 and u32(lib.vrs_scan_levels_for, 2 ** 32 - 1, 256) == 4


# ---------------------------------------------------------------------------------------------- integers against numpy

def wrapped(fn, x, np_dtype):
    with np.errstate(over="ignore"):
        return fn(x.astype(np_dtype), axis=1, dtype=np_dtype)


@pytest.mark.parametrize("dtype,np_dtype", [(torch.int32, np.int32), (torch.int64, np.int64)], ids=["int32", "int64"])
@pytest.mark.parametrize("S,L,C", [(1, 1, 1), (2, 257, 1), (1, F * 256 + 3, 1), (3, 1000, 3), (1, 600, 65)])
def test_integer_scans_wrap_like_numpy(lib, dtype, np_dtype, S, L, C):
    info = np.iinfo(np_dtype)
    rng = np.random.default_rng(S + L + C)
    x = rng.integers(info.min, info.max, size=(S, L, C), dtype=np_dtype, endpoint=True)
    for op, fn in ((SUM, np.cumsum), (PROD, np.cumprod)):
        y = x if op == SUM else rng.integers(-3, 4, size=(S, L, C)).astype(np_dtype) | 1
        got, _ = host_scan(lib, torch.from_numpy(y), op, 256)
        assert np.array_equal(got.numpy(), wrapped(fn, y, np_dtype)), (op, S, L, C)


@pytest.mark.parametrize("dtype", WIDENED, ids=lambda d: str(d).replace("torch.", ""))
def test_the_widening_load_gives_int64(lib, dtype):
    info = torch.iinfo(dtype)
    x = torch.randint(info.min, info.max + 1, (2, 777, 3), dtype=torch.int64, generator=torch.Generator().manual_seed(3)).to(dtype)
    for op, fn in ((SUM, torch.cumsum), (PROD, torch.cumprod)):
        got, _ = host_scan(lib, x, op, 256, out_dtype=torch.int64)
        assert torch.equal(got, fn(x, 1))  # (torch promotes to int64 and wraps)


# ---------------------------------------------------------------------------------------------- MAX and MIN against torch

def tricky(dtype, shape, seed):
    """ties, -0.0 next to +0.0, infinities and NaNs (floats); ties and the type's ends (integers)"""
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        pool = torch.tensor([0.0, -0.0, 1.0, 1.0, -1.0, 2.5, -2.5, float("inf"), -float("inf"), float("nan"), 3.0, 3.0, 1e-3, -1e-3], dtype=dtype)
        weights = torch.tensor([4.0, 4, 3, 3, 3, 2, 2, 1, 1, 0.3, 2, 2, 1, 1])
    else:
        info = torch.iinfo(dtype)
        pool = torch.tensor([info.min, info.max, 0, 0, 1, 1, 2, 5, 5, 7], dtype=dtype)
        weights = torch.ones(10)
    n = int(np.prod(shape))
    return pool[torch.multinomial(weights, n, replacement=True, generator=g)].view(shape)


@pytest.mark.parametrize("dtype", list(CODES), ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("S,L,C", [(1, 7, 1), (2, 300, 1), (1, F * 256 + 5, 1), (2, 530, 3)])
def test_cummax_cummin_equal_torch(lib, dtype, S, L, C):
    x = tricky(dtype, (S, L, C), S + L + C)
    for op, fn in ((MAX, torch.cummax), (MIN, torch.cummin)):
        got_v, got_i = host_scan(lib, x, op, 256)
        want_v, want_i = fn(x, 1)
        assert torch.equal(got_i, want_i), (dtype, op)
        assert torch.equal(bits(got_v), bits(want_v)), (dtype, op)


def test_the_index_follows_the_latest_nan(lib):
    x = torch.tensor([1, 3, 3, float("nan"), 5, float("nan"), 2])
    _, idx = host_scan(lib, x.view(1, 7, 1), MAX, 256)
    assert idx.view(-1).tolist() == [0, 1, 2, 3, 3, 5, 5] == torch.cummax(x, 0)[1].tolist()


# ---------------------------------------------------------------------------------------------- the pure companions

def tier_of(lib, S, L, C, dtype, out_dtype, op, T, min_rows):
    tier = ctypes.c_int(-1)
    rc = lib.vrs_scan_tier_for(S, L, C, CODES[dtype], CODES[out_dtype], op, T, min_rows, ctypes.byref(tier))
    return rc, tier.value


def test_tier_for_over_its_edges(lib):
    T, M = 2048, 1 << 20
    f32 = torch.float32
    for S, L, C, dtype, out_dtype, op, min_rows, want in [
        (1, T, 1, f32, f32, SUM, M, capi.VRS_SCAN_TILE),
        (10 ** 6, 1000, 1, f32, f32, SUM, M, capi.VRS_SCAN_TILE),             # many short segments: still one tile each
        (1, T + 1, 1, f32, f32, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),           # below the single pass's start
        (1, M, 1, f32, f32, SUM, M, capi.VRS_SCAN_SINGLE_PASS),
        (1, M - 1, 1, f32, f32, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),
        (512, T + 1, 1, f32, f32, PROD, M, capi.VRS_SCAN_SINGLE_PASS),         # rows per call, not per segment
        (1, M, 1, f32, f32, SUM, 0, capi.VRS_SCAN_THREE_LAUNCH),               # 0: never
        (1, M, 2, f32, f32, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),               # columns
        (1, M, 1, torch.float64, torch.float64, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),  # 8-byte accumulators
        (1, M, 1, torch.int32, torch.int64, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),
        (1, M, 1, torch.int32, torch.int32, SUM, M, capi.VRS_SCAN_SINGLE_PASS),
        (1, M, 1, torch.float16, torch.float16, SUM, M, capi.VRS_SCAN_SINGLE_PASS),
        (1, M, 1, torch.bfloat16, torch.bfloat16, PROD, M, capi.VRS_SCAN_SINGLE_PASS),
        (1, M, 1, f32, f32, MAX, M, capi.VRS_SCAN_THREE_LAUNCH),               # pairs
        (1, 2 ** 32 - 1, 1, f32, f32, SUM, M, capi.VRS_SCAN_SINGLE_PASS),
        (65537, 65535, 1, f32, f32, SUM, M, capi.VRS_SCAN_SINGLE_PASS),        # S * L = 2^32 - 1
        (2 ** 32 - 1, 1, 1, f32, f32, SUM, M, capi.VRS_SCAN_TILE),
        (1, 2 ** 32 - 1, 2 ** 32 - 1, f32, f32, SUM, M, capi.VRS_SCAN_THREE_LAUNCH),
    ]:
        assert tier_of(lib, S, L, C, dtype, out_dtype, op, T, min_rows) == (capi.VRS_OK, want), (S, L, C, dtype, op, min_rows)
    # the tile's length moves the first edge
    assert tier_of(lib, 1, 257, 1, f32, f32, SUM, 256, 0)[1] == capi.VRS_SCAN_THREE_LAUNCH
    assert tier_of(lib, 1, 8192, 1, f32, f32, SUM, 8192, 1)[1] == capi.VRS_SCAN_TILE


def test_levels_for_over_its_edges(lib):
    for T in (256, 2048, 8192):
        for L, want in [(0, 0), (1, 0), (T, 0), (T + 1, 1), (F * T, 1), (F * T + 1, 2), (F * F * T, 2), (F * F * T + 1, 3)]:
            assert u32(lib.vrs_scan_levels_for, L, T) == want == levels_of(L, T), (L, T)
    assert u32(lib.vrs_scan_levels_for, 2 ** 32 - 1, 8192) == 4 and u32(lib.vrs_scan_levels_for, F ** 3 * 256, 256) == 3


def scratch(lib, S, L, C, dtype, out_dtype, op, T, min_rows):
    out = ctypes.c_uint64()
    rc = lib.vrs_scan_scratch_bytes(S, L, C, CODES[dtype], CODES[out_dtype], op, T, min_rows, ctypes.byref(out))
    return rc, out.value


def words_of(L, T):
    tiles = -(-L // T)
    return [-(-tiles // F ** k) for k in range(levels_of(L, T))]


@pytest.mark.parametrize("S,L", [(1, 2 ** 32 - 1), (65537, 65535), (1, 2 ** 31), (3, 2 ** 30 + 5), (1, 2049), (7, 10 ** 6 + 1)])
def test_scratch_bytes_over_its_edges(lib, S, L):
    T, f32 = 2048, torch.float32
    tiles = -(-L // T)
    slack = 256 * 8
    # the single pass: a ticket and one 8-byte word per A(k)_m
    rc, got = scratch(lib, S, L, 1, f32, f32, SUM, T, 1)
    need = 8 * S * sum(words_of(L, T))
    assert rc == capi.VRS_OK and need <= got < need + slack, (S, L, got)
    # three launches: every level and P, in accumulators of 4, 8 or 16 bytes, per column
    for C, dtype, op, a in [(1, f32, SUM, 4), (3, f32, SUM, 4), (1, torch.float64, PROD, 8), (2, torch.int8, MAX, 16), (1, torch.float16, SUM, 4)]:
        rc, got = scratch(lib, S, L, C, dtype, dtype, op, T, 0)
        need = a * C * S * (sum(words_of(L, T)) + tiles)
        assert rc == capi.VRS_OK and need <= got < need + slack, (S, L, C, dtype, got)
    assert scratch(lib, 2 ** 32 - 1, 1, 1, f32, f32, SUM, T, 1) == (capi.VRS_OK, 0)  # the tile tier takes none
    assert scratch(lib, 5, T, 7, f32, f32, MAX, T, 1) == (capi.VRS_OK, 0)


def test_the_keys_are_37_38_39_in_the_header_and_in_capi():
    header = (ROOT / "include" / "vkradixsort_amd_tune.h").read_text()
    for name, key in (("VRS_TUNE_SCAN_TILE_ROWS", 37), ("VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS", 38), ("VRS_TUNE_SCAN_SPIN_BUDGET", 39)):
        assert re.search(rf"\b{name}\s*=\s*{key}\b", header), name
        assert getattr(capi, name) == key
    header = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    for name, value in (("VRS_SCAN_SUM", 0), ("VRS_SCAN_PROD", 1), ("VRS_SCAN_MAX", 2), ("VRS_SCAN_MIN", 3), ("VRS_SCAN_TILE", 0),
                        ("VRS_SCAN_THREE_LAUNCH", 1), ("VRS_SCAN_SINGLE_PASS", 2)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", header) and getattr(capi, name) == value, name


def test_refusals_need_no_device(lib):
    f32, bad = torch.float32, capi.VRS_ERROR_INVALID_ARGUMENT
    ok_T = 2048
    # dtype / out_dtype / op triples
    for dtype, out_dtype, op in [(torch.int8, torch.int8, SUM), (torch.uint8, torch.int32, SUM), (torch.int16, torch.int16, PROD), (f32, torch.float64, SUM),
                                 (torch.int64, torch.int32, SUM), (torch.float16, f32, SUM), (f32, torch.int64, SUM), (torch.int8, torch.int64, MAX),
                                 (f32, torch.float16, MIN)]:
        assert tier_of(lib, 1, 10, 1, dtype, out_dtype, op, ok_T, 0)[0] == bad, (dtype, out_dtype, op)
        assert scratch(lib, 1, 10, 1, dtype, out_dtype, op, ok_T, 0)[0] == bad
    tier = ctypes.c_int()
    for op in (-1, 4):
        assert lib.vrs_scan_tier_for(1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, op, ok_T, 0, ctypes.byref(tier)) == bad
    for code in (-1, 9):
        assert lib.vrs_scan_tier_for(1, 10, 1, code, code, SUM, ok_T, 0, ctypes.byref(tier)) == bad
    # T out of range, or no multiple of 256
    for T in (0, 255, 128, 300, 8192 + 256, 2 ** 31):
        assert tier_of(lib, 1, 10, 1, f32, f32, SUM, T, 0)[0] == bad, T
        out = ctypes.c_uint32()
        assert lib.vrs_scan_levels_for(10, T, ctypes.byref(out)) == bad and lib.vrs_scan_depth_for(10, 1, T, ctypes.byref(out)) == bad
        x = torch.zeros(1, 10, 1)
        assert lib.vrs_scan_rows_host(x.data_ptr(), 1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, SUM, T, x.data_ptr(), None) == bad
    for T in (256, 512, 8192):
        assert tier_of(lib, 1, 10, 1, f32, f32, SUM, T, 0)[0] == capi.VRS_OK
    # 2^32 rows in all, no columns, NULL results
    assert tier_of(lib, 65536, 65536, 1, f32, f32, SUM, ok_T, 0)[0] == bad
    assert tier_of(lib, 1, 10, 0, f32, f32, SUM, ok_T, 0)[0] == bad
    assert lib.vrs_scan_tier_for(1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, SUM, ok_T, 0, None) == bad
    assert lib.vrs_scan_levels_for(10, ok_T, None) == bad and lib.vrs_scan_depth_for(10, 1, ok_T, None) == bad
    assert lib.vrs_scan_scratch_bytes(1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, SUM, ok_T, 0, None) == bad
    assert lib.vrs_scan_stats(None, None, None, None, None) == bad
    x = torch.zeros(1, 10, 1)
    assert lib.vrs_scan_rows_host(x.data_ptr(), 1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, MAX, ok_T, x.data_ptr(), None) == bad  # no indices
    assert lib.vrs_scan_rows_host(None, 1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, SUM, ok_T, x.data_ptr(), None) == bad
    assert lib.vrs_scan_rows(None, None, 1, 10, 1, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT32, SUM, None, None, None) == bad


def test_the_wrappers_are_exported():
    import vkradixsort_amd as v

    for name in ("cumsum", "cumprod", "cummax", "cummin", "scan_stats"):
        assert callable(getattr(v, name)) and getattr(v.scan, name) is getattr(v, name)
