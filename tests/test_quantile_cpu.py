"""CPU tests of the multi-rank selection's host side (vrs_quantile_*) and of the quantile / nanquantile wrappers' argument checks: the
target rule and the host evaluation against torch.quantile / torch.nanquantile on the CPU, the level table, the tiers it shares with the
one-rank selection, the scratch function and every refusal.  No device."""
import ctypes

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd.quantile import INTERPOLATIONS as INTERPOLATION_CODES

torch = pytest.importorskip("torch")

INTERPOLATIONS = ["linear", "lower", "higher", "midpoint", "nearest"]
CODE = {torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
QS = [0.0, 0.1, 0.25, 0.37, 0.5, 0.999, 1.0]
LENGTHS = [1, 2, 3, 7, 100, 1001, 65537, 1 << 24]


@pytest.fixture(scope="module")
def lib():
    from vkradixsort_amd import build
    build.build_library()
    return capi.load_library()


def target(lib, dtype, interpolation, q, length, nans, ignore_nan):
    lo, hi, w, valid = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double(), ctypes.c_int()
    rc = lib.vrs_quantile_target_for(CODE[dtype], INTERPOLATION_CODES[interpolation], q, length, nans, int(ignore_nan),
                                     ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(w), ctypes.byref(valid))
    assert rc == capi.VRS_OK
    return lo.value, hi.value, w.value, bool(valid.value)


def lerp(np_t, a, b, w):
    """the header's interpolation in numpy scalars of the dtype: every operation rounded on its own"""
    a, b, w = np_t(a), np_t(b), np_t(w)
    d = b - a
    return a + w * d if w < np_t(0.5) else b - d * (np_t(1) - w)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_target_rule_equals_torch_on_arange_rows(lib, dtype, interpolation):
    """torch.quantile / nanquantile of rows 0, 1, ..., L' - 1 followed by NaNs: there the order statistics are their own indices, so the
    answer is the interpolation of (lower, upper, weight) itself.  Bit for bit wherever there is an answer.  A row with NaNs under
    torch.quantile has none (torch answers NaN, the rule valid = 0): up to 65537 keys torch is asked, at 2^24 keys its NaN is written
    down instead of sorting 2^24 keys three more times per case, and only `valid` is checked there."""
    np_t = NP[dtype]
    single = interpolation in ("lower", "higher", "nearest")
    for length in LENGTHS:
        for nans in sorted({0, 1, length - 1, length} & set(range(length + 1))):
            row = torch.arange(length, dtype=dtype)
            row[length - nans:] = float("nan")
            q = torch.tensor(QS, dtype=dtype)
            for ignore_nan in (False, True):
                if not ignore_nan and nans:  # (torch answers NaN; at 2^24 keys that is written down, not computed: see the docstring)
                    theirs = torch.full((len(QS),), float("nan"), dtype=dtype) if length > 70000 else torch.quantile(row, q, interpolation=interpolation)
                else:
                    theirs = (torch.nanquantile if ignore_nan else torch.quantile)(row, q, interpolation=interpolation)
                ours = []
                for qv in QS:
                    lo, hi, w, valid = target(lib, dtype, interpolation, qv, length, nans, ignore_nan)
                    live = length - nans if ignore_nan else length
                    assert valid == (live > 0 and (ignore_nan or nans == 0))
                    if not valid:
                        ours.append(float("nan"))
                        continue
                    assert lo <= hi <= live - 1 and hi - lo <= 1
                    if single:
                        assert lo == hi and w == 0.0
                        ours.append(np_t(lo))
                    else:
                        ours.append(lerp(np_t, lo, hi, w))
                ours = torch.tensor(np.array(ours, dtype=np_t))
                assert torch.equal(torch.isnan(ours), torch.isnan(theirs)), (length, nans, ignore_nan)
                keep = ~torch.isnan(ours)
                assert same_bits(ours[keep], theirs[keep]), (length, nans, ignore_nan, ours, theirs)


def test_target_rule_above_2_24_clamps_and_is_monotonic(lib):
    """float32 rows longer than 2^24: float(L - 1) may round up past the last index.  torch refuses such rows on the CPU ('input tensor is
    too large'), so only the clamp and the monotonicity in q are checked."""
    for length in ((1 << 24) + 4, (1 << 24) + 5, (1 << 25) + 7, (1 << 31) + 129, (1 << 32) - 1):
        for interpolation in INTERPOLATIONS:
            prev = (0, 0)
            for qv in [0.0, 1e-9, 0.1, 0.25, 0.37, 0.5, 0.75, 0.999, 0.9999999, 1.0]:
                lo, hi, w, valid = target(lib, torch.float32, interpolation, qv, length, 0, False)
                assert valid and lo <= hi <= length - 1 and 0.0 <= w < 1.0
                assert lo >= prev[0] and hi >= prev[1], (length, interpolation, qv)
                prev = (lo, hi)
            assert target(lib, torch.float32, interpolation, 1.0, length, 0, False)[:2] == (length - 1, length - 1)
            lo, hi, _, _ = target(lib, torch.float32, interpolation, 1.0, length, 3, True)
            assert lo == hi == length - 4


def host(lib, x, offsets, qs, interpolation, ignore_nan):
    """vrs_quantile_host on the segments of a 1-D CPU tensor: (values, lower, upper, weight), each [S, Q]"""
    S = len(offsets) - 1
    offs = np.array(offsets, dtype=np.uint32)
    q = (ctypes.c_double * max(len(qs), 1))(*qs)
    outs = [torch.full((S, len(qs)), 7.0, dtype=x.dtype) for _ in range(4)]
    rc = lib.vrs_quantile_host(x.data_ptr(), x.numel(), offs.ctypes.data, S, CODE[x.dtype], q, len(qs),
                               INTERPOLATION_CODES[interpolation], capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0,
                               *(o.data_ptr() for o in outs))
    assert rc == capi.VRS_OK
    return outs


def random_rows(dtype, rows, length, g, nans, zeros):
    x = (torch.rand(rows, length, generator=g, dtype=torch.float64) * 2 - 1) * 10.0 ** torch.randint(-30, 30, (rows, length), generator=g).double()
    x = x.to(dtype)  # |x| < 1e30
    if zeros:
        x[:, torch.randint(0, length, (max(length // 4, 1),), generator=g)] = 0.0
        x[:, torch.randint(0, length, (max(length // 4, 1),), generator=g)] = -0.0
    if nans:
        for r in range(0, rows, 2):
            x[r, torch.randint(0, length, (min(length, 3),), generator=g)] = float("nan")
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_host_evaluation_against_torch(lib, dtype):
    """vrs_quantile_host against torch.quantile / nanquantile on the CPU: the two order statistics equal under == (NaNs in the same
    places), the quantile within 4 ulp of max(|lower|, |upper|) -- two evaluations of one three-operation interpolation of the same
    operands, each at most 2 ulp from the real value."""
    g = torch.Generator().manual_seed(16)
    eps = torch.finfo(dtype).eps
    differed = total = 0
    for length in (1, 2, 5, 64, 1000):
        for nans, zeros in ((False, False), (True, False), (False, True), (True, True)):
            x = random_rows(dtype, 6, length, g, nans, zeros)
            offsets = [i * length for i in range(7)]
            q = torch.tensor(QS, dtype=dtype)
            for ignore_nan in (False, True):
                fn = torch.nanquantile if ignore_nan else torch.quantile
                lower = fn(x, q, dim=1, interpolation="lower").T
                upper = fn(x, q, dim=1, interpolation="higher").T
                for interpolation in INTERPOLATIONS:
                    v, lo, hi, w = host(lib, x.reshape(-1), offsets, QS, interpolation, ignore_nan)
                    theirs = fn(x, q, dim=1, interpolation=interpolation).T
                    if interpolation in ("linear", "midpoint"):
                        for mine, ref in ((lo, lower), (hi, upper)):
                            assert torch.equal(torch.isnan(mine), torch.isnan(ref))
                            assert bool(((mine == ref) | torch.isnan(ref)).all())
                        assert bool(((w >= 0) & (w < 1) | torch.isnan(w)).all())
                    else:
                        assert torch.equal(torch.isnan(lo), torch.isnan(theirs)) and bool(((lo == hi) | torch.isnan(lo)).all())
                        assert bool(((w == 0) | torch.isnan(w)).all())
                    assert torch.equal(torch.isnan(v), torch.isnan(theirs)), (length, interpolation)
                    scale = torch.maximum(lo.abs(), hi.abs())
                    err = (v - theirs).abs()
                    ok = torch.isnan(theirs) | (err <= 4 * eps * scale)
                    assert bool(ok.all()), (length, interpolation, v[~ok], theirs[~ok])
                    differed += int((~torch.isnan(theirs) & (v != theirs)).sum())
                    total += theirs.numel()
    print(f"{dtype}: {differed} of {total} quantiles differ from torch's at all")


def test_host_evaluation_canonical_values_and_empty_segments(lib):
    """±0.0 answers +0.0, a segment without an answer the quiet NaN in all four outputs; ragged, empty and clamped segments."""
    x = torch.tensor([-0.0, -0.0, 3.0, float("nan"), float("nan"), 1.0, float("inf"), float("-inf")], dtype=torch.float32)
    offsets = [0, 2, 2, 3, 5, 6, 8, 100]
    for interpolation in INTERPOLATIONS:
        v, lo, hi, w = host(lib, x, offsets, [0.5], interpolation, True)
        assert v.view(torch.int32)[0, 0] == 0 and lo.view(torch.int32)[0, 0] == 0  # +0.0
        for out in (v, lo, hi, w):
            assert out.view(torch.int32)[1, 0] == 0x7FC00000 and out.view(torch.int32)[3, 0] == 0x7FC00000 and out.view(torch.int32)[6, 0] == 0x7FC00000
        assert v[2, 0] == 3.0 and v[4, 0] == 1.0
        if interpolation in ("linear", "midpoint"):
            assert v.view(torch.int32)[5, 0] == 0x7FC00000  # (inf - inf, as torch)
            assert lo[5, 0] == float("-inf") and hi[5, 0] == float("inf")


def test_level_table(lib):
    for bits, widths in ((32, [11, 8, 8, 5]), (64, [11, 8, 8, 8, 8, 8, 8, 5])):
        left = bits
        for level, width in enumerate(widths):
            shift, mask, levels = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
            assert lib.vrs_quantile_level_for(bits, level, ctypes.byref(shift), ctypes.byref(mask), ctypes.byref(levels)) == capi.VRS_OK
            left -= width
            assert (shift.value, mask.value, levels.value) == (left, (1 << width) - 1, len(widths))
        assert left == 0
        assert lib.vrs_quantile_level_for(bits, len(widths), ctypes.byref(shift), ctypes.byref(mask), ctypes.byref(levels)) != capi.VRS_OK
    assert lib.vrs_quantile_level_for(16, 0, ctypes.byref(shift), ctypes.byref(mask), ctypes.byref(levels)) != capi.VRS_OK


def test_tier_cuts_are_the_selections(lib):
    """the tiers vrs_quantile_segments takes are vrs_select_tier_for's: ranks of 32 KB, then VRS_TUNE_SELECT_GRID_MIN_KEYS"""
    def tier(length, code, grid_min=capi.SELECT_GRID_MIN_KEYS_DEFAULT, n=1 << 20):
        t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.vrs_select_tier_for(0, length, n, code, grid_min, ctypes.byref(cb), ctypes.byref(ce), ctypes.byref(t)) == capi.VRS_OK
        return t.value
    f32, f64 = capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64
    assert tier(0, f32) == tier(8192, f32) == tier(4096, f64) == capi.VRS_SELECT_LDS
    assert tier(8193, f32) == tier(4097, f64) == tier((1 << 17) - 1, f32) == capi.VRS_SELECT_BLOCK
    assert tier(1 << 17, f32) == tier(1 << 17, f64) == tier(8193, f32, 8193) == capi.VRS_SELECT_GRID
    assert tier(1 << 19, f32, 0) == capi.VRS_SELECT_BLOCK and tier(8192, f32, 100) == capi.VRS_SELECT_LDS
    assert tier(1 << 21, f32, n=5000) == capi.VRS_SELECT_LDS  # (clamped to the 5000 elements)


def test_scratch_bytes_is_monotonic(lib):
    for code in (capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64):
        assert vrs.quantile_scratch_bytes(10 ** 6, 0, code) == 0
        for S in (1, 2, 100, 5000, 10 ** 6):
            prev = 0
            for n in (0, 1, 8192, 8193, 16386, 10 ** 6, 10 ** 8, (1 << 32) - 1):
                b = vrs.quantile_scratch_bytes(n, S, code)
                assert b >= prev and b > 0
                prev = b
        for n in (0, 8193, 10 ** 8, (1 << 32) - 1):
            prev = 0
            for S in (1, 2, 100, 5000, 10 ** 6, (1 << 32) - 1):
                b = vrs.quantile_scratch_bytes(n, S, code)
                assert b >= prev
                prev = b
    for n, S in ((10 ** 8, 3), (10 ** 6, 1000), (8193, 1)):
        assert vrs.quantile_scratch_bytes(n, S, capi.VRS_SORT_FLOAT64) >= vrs.quantile_scratch_bytes(n, S, capi.VRS_SORT_FLOAT32)
    with pytest.raises(vrs.VrsError):
        vrs.quantile_scratch_bytes(100, 1, capi.VRS_SORT_INT32)
    with pytest.raises(vrs.VrsError):
        vrs.quantile_scratch_bytes(100, 1, capi.VRS_SORT_FLOAT16)


def test_refusals(lib):
    """everything refused before a context is looked at: the same checks guard vrs_quantile_segments, _host and _target_for"""
    INV = capi.VRS_ERROR_INVALID_ARGUMENT
    x = torch.arange(8, dtype=torch.float32)
    offs = np.array([0, 8], dtype=np.uint32)
    out = torch.zeros(32, dtype=torch.float64)

    def run(code=capi.VRS_SORT_FLOAT32, qs=(0.5,), interpolation=capi.VRS_QUANTILE_LINEAR, flags=0, S=1):
        q = (ctypes.c_double * max(len(qs), 1))(*qs)
        a = lib.vrs_quantile_host(x.data_ptr(), 8, offs.ctypes.data, S, code, q, len(qs), interpolation, flags, out.data_ptr(), None, None, None)
        b = lib.vrs_quantile_segments(None, None, 8, None, S, code, q, len(qs), interpolation, flags, None, None, None, None, None)
        return a, b

    assert run() == (capi.VRS_OK, INV)  # (the device call: no context)
    for code in (capi.VRS_SORT_FLOAT16, capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_INT32, capi.VRS_SORT_INT64, -1, 9):
        assert run(code=code) == (INV, INV)
    assert run(interpolation=5) == (INV, INV) and run(interpolation=-1) == (INV, INV)
    assert run(flags=2) == (INV, INV) and run(flags=3) == (INV, INV)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf"), -0.5):
        assert run(qs=(0.5, bad)) == (INV, INV)
    assert run(qs=(0.5,) * 8)[0] == capi.VRS_OK and run(qs=(0.5,) * 9) == (INV, INV)  # linear: two targets per q
    assert run(qs=(0.5,) * 8, interpolation=capi.VRS_QUANTILE_MIDPOINT)[0] == capi.VRS_OK
    assert run(qs=(0.5,) * 9, interpolation=capi.VRS_QUANTILE_MIDPOINT) == (INV, INV)
    for single in (capi.VRS_QUANTILE_LOWER, capi.VRS_QUANTILE_HIGHER, capi.VRS_QUANTILE_NEAREST):
        assert run(qs=(0.5,) * 16, interpolation=single)[0] == capi.VRS_OK and run(qs=(0.5,) * 17, interpolation=single) == (INV, INV)
    assert run(S=0)[0] == capi.VRS_OK and run(qs=())[0] == capi.VRS_OK  # nothing to do
    assert lib.vrs_quantile_host(x.data_ptr(), 8, offs.ctypes.data, 1, capi.VRS_SORT_FLOAT32, None, 1, 0, 0, out.data_ptr(), None, None, None) == INV
    lo, hi, w, valid = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double(), ctypes.c_int()
    refs = (ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(w), ctypes.byref(valid))
    assert lib.vrs_quantile_target_for(capi.VRS_SORT_FLOAT32, 0, 0.5, 10, 11, 1, *refs) == INV  # more NaNs than keys
    assert lib.vrs_quantile_target_for(capi.VRS_SORT_FLOAT16, 0, 0.5, 10, 0, 0, *refs) == INV
    assert lib.vrs_quantile_target_for(capi.VRS_SORT_FLOAT32, 7, 0.5, 10, 0, 0, *refs) == INV
    assert lib.vrs_quantile_target_for(capi.VRS_SORT_FLOAT32, 0, 1.5, 10, 0, 0, *refs) == INV
    assert lib.vrs_quantile_target_for(capi.VRS_SORT_FLOAT32, 0, 0.5, 10, 0, 0, None, None, None, None) == INV
    assert lib.vrs_quantile_stats(None, None, None, None, None) == INV
    assert lib.vrs_quantile_scratch_bytes(10, 1, capi.VRS_SORT_FLOAT32, None) == INV


def _message(fn):
    with pytest.raises(Exception) as e:
        fn()
    return type(e.value), str(e.value).splitlines()[0]


@pytest.mark.parametrize("name", ["quantile", "nanquantile"])
def test_wrapper_errors_are_torchs(name):
    """what the wrappers refuse before any device work, against torch's own exception and first line of text, on CPU tensors"""
    ours, theirs = getattr(vrs, name), getattr(torch, name)
    x = torch.arange(10.0)
    cases = [
        lambda f: f(x.int(), 0.5),
        lambda f: f(x.half(), 0.5),
        lambda f: f(x.bfloat16(), 0.5),
        lambda f: f(x.long(), 0.5),
        lambda f: f(x, 1.5),
        lambda f: f(x, -0.1),
        lambda f: f(x, float("nan")),
        lambda f: f(x, torch.tensor([0.5, 1.5])),
        lambda f: f(x, torch.tensor([0.5], dtype=torch.float64)),
        lambda f: f(x, torch.tensor([[0.5]])),
        lambda f: f(torch.empty(0), 0.5),
        lambda f: f(torch.empty(3, 0), 0.5, dim=1),
        lambda f: f(torch.empty(0, 3), 0.5, dim=1),
        lambda f: f(x, 0.5, interpolation="cubic"),
        lambda f: f(x, 0.5, dim=3),
        lambda f: f(x, 0.5, dim=-2),
    ]
    for case in cases:
        a, b = _message(lambda: case(ours)), _message(lambda: case(theirs))
        assert a == b
        assert issubclass(a[0], (RuntimeError, IndexError))
    # past torch's checks a CPU tensor is refused: there is no quiet fall-back
    with pytest.raises(vrs.VrsError):
        ours(x, 0.5)
