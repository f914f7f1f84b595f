"""The membership form of vrs_search_sorted (VRS_SEARCH_MEMBER) and vrs.isin on the device, byte for byte: the C call against
numpy.isin of the same arrays for the nine dtypes in every tier they can take (forced, asserted through search_stats), both invert
values, rows, sorter, the word and the byte store with canaries around the output, unsorted boundaries, empty sides, streams; and
vrs.isin against torch.isin on the CPU copy.  No tolerance anywhere: the outputs are 0 / 1 bytes."""
import ctypes
import time

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import buffers, context_for
from vkradixsort_amd.sort import _dtype_code

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = ["int8", "uint8", "int16", "int32", "int64", "float16", "bfloat16", "float32", "float64"]
NARROW = ["int8", "uint8", "int16", "float16", "bfloat16"]
MEMBER, INVERT = capi.VRS_SEARCH_MEMBER, capi.VRS_SEARCH_MEMBER_INVERT
DEFAULTS = {capi.VRS_TUNE_SEARCH_LDS_BYTES: capi.SEARCH_LDS_BYTES_DEFAULT,
            capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT,
            capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT}
# settings that force a tier whatever the shape (the table: narrow dtypes with one boundary row only), as tests/test_gpu_searchsorted.py
FORCE = {"lds": {capi.VRS_TUNE_SEARCH_LDS_BYTES: capi.SEARCH_LDS_BYTES_MAX, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0},
         "table": {capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 1},
         "direct": {capi.VRS_TUNE_SEARCH_LDS_BYTES: 0, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 0},
         "indexed": {capi.VRS_TUNE_SEARCH_LDS_BYTES: 0, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: 0, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: 1}}
BITS = {"float16": (torch.int16, 16, 10), "bfloat16": (torch.int16, 16, 7), "float32": (torch.int32, 32, 23), "float64": (torch.int64, 64, 52)}
NS = [1, 3, 4, 5, 4095, 4096, 4097, 8193]  # a tail that is no multiple of four, one whole chunk, a chunk boundary
CANARY = 0xAB


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    c = context_for(dev)
    yield c
    for key, value in DEFAULTS.items():
        c.setTuning(key, value)


def force(c, name):
    for key, value in DEFAULTS.items():
        c.setTuning(key, value)
    for key, value in FORCE.get(name, {}).items():
        c.setTuning(key, value)


def stats_delta(c, before):
    now = vrs.search_stats(c)
    return {k: now[k] - before[k] for k in now}


def as_numpy(t):
    """the values numpy compares: bfloat16 as its float32 values (exact)"""
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


def nans(dtype):
    """NaNs of both signs, quiet and with a payload, and the all-ones pattern"""
    view, bits, mant = BITS[dtype]
    inf = ((1 << (bits - 1 - mant)) - 1) << mant
    patterns = [inf | 1 << (mant - 1), inf | 1 << (mant - 1) | 1 << (bits - 1), inf | 5, (1 << bits) - 1]
    signed = [p - (1 << bits) if p >= 1 << (bits - 1) else p for p in patterns]
    out = torch.tensor(signed, dtype=torch.int64).to(view).view(getattr(torch, dtype))
    assert bool(torch.isnan(out).all())
    return out


def pools(dtype, variant, rng):
    """(values the boundaries are drawn from, values the queries are drawn from, values every query row holds) of one variant.
    floats 0: +0.0, NaNs, +-inf and a subnormal among the boundaries; -0.0, NaNs, +-inf, subnormals of both signs queried
    floats 1: -0.0, -inf, a negative subnormal and no NaN among the boundaries; +0.0, NaNs, +inf and the largest finite queried: above
              every boundary (count == m)
    floats 2: NaNs, +0.0 and +inf among the boundaries; no NaN queried; -inf and the lowest finite are below every boundary
    integers 0: small values with ties; the dtype's ends queried: below and above every boundary
    integers 1: the dtype's ends (its largest rank is all ones, the floats' NaN class) among the boundaries and queried
    integers 2: ties only"""
    dt = getattr(torch, dtype)
    if dt.is_floating_point:
        fi = torch.finfo(dt)
        sub = fi.smallest_normal / 4
        rand = torch.from_numpy(rng.integers(-24, 25, 64) / 4.0).to(dt)
        f = lambda xs: torch.tensor(xs, dtype=torch.float64).to(dt)  # noqa: E731
        if variant == 0:
            return (torch.cat([f([0.0, float("inf"), float("-inf"), sub, 1.0]), nans(dtype), rand[:40]]),
                    torch.cat([rand, f([fi.max])]), torch.cat([f([-0.0, float("inf"), float("-inf"), sub, -sub, 2 * sub]), nans(dtype)]))
        if variant == 1:
            return (torch.cat([f([-0.0, float("-inf"), -sub, -1.0]), rand[:40]]),
                    rand, torch.cat([f([0.0, float("inf"), fi.max, fi.min, sub, -sub]), nans(dtype)]))
        return (torch.cat([f([0.0, float("inf"), 2 * sub]), nans(dtype), rand[:40]]),
                rand, f([-0.0, 0.0, float("inf"), float("-inf"), fi.min, 2 * sub, -2 * sub]))
    ii = torch.iinfo(dt)
    lo, hi = max(ii.min + 2, -30), min(ii.max - 2, 30)
    rand = torch.from_numpy(rng.integers(lo, hi + 1, 64)).to(dt)
    ends = torch.tensor([ii.min, ii.max, ii.min + 1, ii.max - 1, 0], dtype=torch.int64).to(dt)
    if variant == 0:
        return rand[:40], rand, ends
    if variant == 1:
        return torch.cat([ends, rand[:40]]), rand, ends
    return rand[:8], rand, rand[:3]


def draw(pool, must, n, rng):
    """n values: every one of `must` first (as many as fit, rotated so that short rows differ), the rest drawn from both"""
    both = torch.cat([must, pool])
    x = both[torch.from_numpy(rng.integers(0, both.numel(), n))]
    k = min(n, must.numel())
    x[:k] = torch.roll(must, int(rng.integers(0, must.numel())))[:k]
    return x


def boundaries_of(dtype, variant, m, rng):
    """m boundaries ascending in the library's order (torch.sort on the CPU: NaNs last, -0.0 == +0.0), with duplicates"""
    pool, _, _ = pools(dtype, variant, rng)
    k = min(m, 9 if pool.dtype.is_floating_point and variant != 1 else 5)
    b = draw(pool[k:], pool[:k], m, rng)  # (the variant's special values lead its pool)
    if m >= 5:
        b[-1] = b[-2]
    return torch.sort(b, stable=True).values


def member(c, code, bounds, queries, *, m=None, q_len=None, invert=False, sorter=None, out=None, flags=None):
    """one vrs_search_sorted call in the membership form over device tensors; returns (status, the uint8 output on the device)"""
    nb, nq = bounds.numel(), queries.numel()
    m = nb if m is None else m
    q_len = nq if q_len is None else q_len
    if out is None:
        out = torch.empty(nq, dtype=torch.uint8, device=queries.device)
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    c.check(c.lib.vrs_search_plan(c.handle, nb, m, nq, q_len, code, int(sorter is not None), ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=queries.device) if need.value else None
    flags = (MEMBER | (INVERT if invert else 0)) if flags is None else flags
    with buffers(c, bounds, queries, sorter, out, scratch) as (bnd, qry, srt, res, scr):
        rc = c.lib.vrs_search_sorted(c.handle, bnd, nb, m, qry, nq, q_len, code, flags, srt, res, scr)
    return rc, out


def check(c, dtype, bounds, queries, tier=None):
    """both invert values of one shared boundary row against numpy.isin; the canaries around the output; `tier`: the one that must run"""
    dev = torch.device("cuda", 0)
    code = _dtype_code(torch, bounds.dtype)
    b_d, q_d = bounds.to(dev), queries.to(dev)
    n = queries.numel()
    for invert in (False, True):
        want = np.isin(as_numpy(queries), as_numpy(bounds), invert=invert)
        buf = torch.full((n + 32,), CANARY, dtype=torch.uint8, device=dev)
        before = vrs.search_stats(c)
        rc, _ = member(c, code, b_d, q_d, invert=invert, out=buf[16:16 + n])
        assert rc == capi.VRS_OK, c.lib.vrs_last_error(c.handle)
        got = buf.cpu().numpy()
        assert np.array_equal(got[16:16 + n], want.astype(np.uint8)), (dtype, tier, bounds.numel(), n, invert,
                                                                       np.nonzero(got[16:16 + n] != want)[0][:8])
        assert (got[:16] == CANARY).all() and (got[16 + n:] == CANARY).all(), (dtype, tier, bounds.numel(), n)
        if tier is not None:
            delta = stats_delta(c, before)
            assert delta[tier] == 1 and sum(delta.values()) == 1, (delta, tier)


def past_capacity(dtype):
    """a row one element past what the LDS tier can ever take: the direct tier even when the LDS tier is forced"""
    return capi.SEARCH_LDS_BYTES_MAX // (8 if dtype in ("int64", "float64") else 4) + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_call_every_dtype_in_every_tier_against_numpy(ctx, dtype):
    rng = np.random.default_rng(190 + DTYPES.index(dtype))
    variant = 0
    for name in ("lds", "direct", "indexed"):
        # (past the forced capacity: forced LDS turns direct there; with no LDS at all the index's stride grows beyond its first size)
        for m in (1, 2, 5, 1000, past_capacity(dtype) if name == "lds" else 70001):
            force(ctx, name)
            tier = "direct" if name == "lds" and m > 1000 else name
            ns = NS if m <= 1000 else [5, 4097]
            for n in ns:
                variant = (variant + 1) % 3
                bounds = boundaries_of(dtype, variant, m, rng)
                _, pool, must = pools(dtype, variant, rng)
                q = draw(pool, must, n, rng)
                q[-1] = bounds[m // 2]  # (the last query of the tail is a boundary, unless that is a NaN)
                check(ctx, dtype, bounds, q, tier=tier)
            for variant in (0, 1, 2):
                bounds = boundaries_of(dtype, variant, m, rng)
                _, pool, must = pools(dtype, variant, rng)
                check(ctx, dtype, bounds, bounds.clone(), tier=tier)                       # a query row identical to the boundaries
                check(ctx, dtype, bounds, bounds[m // 2].expand(4097).contiguous(), tier=tier)  # all queries equal: a member
                check(ctx, dtype, bounds, must[-1].expand(4097).contiguous(), tier=tier)   # ... and one of the variant's special values
                check(ctx, dtype, bounds, torch.cat([must, must, must]), tier=tier)        # every special value against every variant's row


@pytest.mark.parametrize("dtype", NARROW)
def test_c_call_table_tier(ctx, dtype):
    rng = np.random.default_rng(290 + DTYPES.index(dtype))
    n = 300 if dtype in ("int8", "uint8") else 2 ** 16 + 3
    for m in (1, 2, 5, 1000):
        for variant in (0, 1, 2):
            force(ctx, "table")
            bounds = boundaries_of(dtype, variant, m, rng)
            _, pool, must = pools(dtype, variant, rng)
            check(ctx, dtype, bounds, draw(pool, must, n, rng), tier="table")
            check(ctx, dtype, bounds, torch.cat([must, bounds, must[-1].expand(7)]), tier="table")
    # every bit pattern of the dtype, NaNs of every payload included, against a row that holds NaNs and +0.0
    view = torch.uint8 if dtype == "uint8" else torch.int8 if dtype == "int8" else torch.int16
    every = torch.arange(256 if view != torch.int16 else 65536, dtype=torch.int64).to(view).view(getattr(torch, dtype))
    check(ctx, dtype, boundaries_of(dtype, 0, 1000, rng), every, tier="table")


@pytest.mark.parametrize("name", ["lds", "direct", "indexed"])
def test_rows_of_boundaries(ctx, dev, name):
    """3 rows of 5 boundaries and 3 query rows of 7, each row with another set (rows of 7 bytes: the second and third output rows start
    3 and 2 bytes off a 4-byte boundary and are stored byte by byte); rows of 8 (words); one shared row against 3 query rows"""
    rng = np.random.default_rng(390)
    for dtype in ("float32", "int64", "bfloat16", "uint8"):
        code = _dtype_code(torch, getattr(torch, dtype))
        for rows, m, q_len in ((3, 5, 7), (3, 5, 8), (3, 5, 5), (3, 6, 4102), (2, 7, 4100), (5, 1000, 4097)):
            bounds = torch.stack([boundaries_of(dtype, r % 3, m, rng) for r in range(rows)])
            qs = torch.stack([draw(pools(dtype, r % 3, rng)[1], pools(dtype, r % 3, rng)[2], q_len, rng) for r in range(rows)])
            qs[:, -1] = bounds[:, 0]
            for invert in (False, True):
                for shared in (False, True):
                    force(ctx, name)
                    b = bounds[1:2] if shared else bounds
                    want = np.stack([np.isin(as_numpy(qs[r]), as_numpy(b[0 if shared else r]), invert=invert) for r in range(rows)])
                    buf = torch.full((rows * q_len + 32,), CANARY, dtype=torch.uint8, device=dev)
                    before = vrs.search_stats(ctx)
                    rc, _ = member(ctx, code, b.to(dev), qs.to(dev), m=m, q_len=q_len, invert=invert, out=buf[16:16 + rows * q_len])
                    assert rc == capi.VRS_OK
                    got = buf.cpu().numpy()
                    assert np.array_equal(got[16:-16].reshape(rows, q_len), want.astype(np.uint8)), (dtype, rows, m, q_len, invert, shared)
                    assert (got[:16] == CANARY).all() and (got[-16:] == CANARY).all()
                    assert stats_delta(ctx, before)[name] == 1


@pytest.mark.parametrize("name", ["lds", "direct", "indexed", "table"])
def test_sorter(ctx, dev, name):
    """shuffled boundaries with their int64 argsort"""
    rng = np.random.default_rng(490)
    for dtype in (("bfloat16", "int8") if name == "table" else ("float32", "int64", "float16")):
        code = _dtype_code(torch, getattr(torch, dtype))
        for m, n in ((1, 5), (5, 4097), (1000, 4097), (20000 if name == "lds" else 70001, 8193)):  # (20000 int64 ranks still fit the LDS)
            for variant in (0, 1):
                force(ctx, name)
                raw = boundaries_of(dtype, variant, m, rng)[torch.from_numpy(rng.permutation(m))]
                sorter = torch.argsort(raw, stable=True)
                _, pool, must = pools(dtype, variant, rng)
                q = draw(pool, must, n, rng)
                for invert in (False, True):
                    before = vrs.search_stats(ctx)
                    rc, out = member(ctx, code, raw.to(dev), q.to(dev), invert=invert, sorter=sorter.to(dev))
                    assert rc == capi.VRS_OK
                    assert np.array_equal(out.cpu().numpy(), np.isin(as_numpy(q), as_numpy(raw), invert=invert).astype(np.uint8)), (dtype, m, n, invert)
                    assert stats_delta(ctx, before)[name] == 1
    if name in ("direct", "indexed"):  # a sorter per row
        raw = torch.stack([boundaries_of("int64", r, 5000, rng)[torch.from_numpy(rng.permutation(5000))] for r in range(3)])
        q = torch.stack([draw(*pools("int64", r, rng)[1:], 4001, rng) for r in range(3)])
        force(ctx, name)
        rc, out = member(ctx, capi.VRS_SORT_INT64, raw.to(dev), q.to(dev), m=5000, q_len=4001, sorter=torch.argsort(raw, dim=-1, stable=True).to(dev))
        assert rc == capi.VRS_OK
        want = np.stack([np.isin(q[r].numpy(), raw[r].numpy()) for r in range(3)])
        assert np.array_equal(out.cpu().numpy().reshape(3, 4001), want.astype(np.uint8))


@pytest.mark.parametrize("name", ["lds", "direct", "indexed"])
def test_output_and_query_alignment_with_canaries(ctx, dev, name):
    """Outputs that start 4, 8 and 12 bytes off a 16-byte boundary are stored as words; queries off their vector alignment (int64 8 bytes
    off 16, int32 4 / 8 / 12 off 16, int16 4 off 8) take the byte path.  A view that starts 1, 2 or 3 bytes off a 4-byte boundary cannot
    be handed to the C call at all: vrs_buffer_wrap refuses it, so those output addresses are reached by rows of 5, 6 and 7 bytes (and
    in test_rows_of_boundaries).  The bytes before and behind out's num_queries bytes keep their canary."""
    rng = np.random.default_rng(590)
    for dtype, q_offs in (("int64", (0, 1)), ("int32", (0, 1, 2, 3)), ("int16", (0, 2)), ("float32", (0, 1, 3)), ("uint8", (0, 4))):
        code = _dtype_code(torch, getattr(torch, dtype))
        bounds = boundaries_of(dtype, 0, 1000, rng)
        _, pool, must = pools(dtype, 0, rng)
        for n in (4, 5, 4099):
            qbuf = draw(pool, must, n + 8, rng).to(dev)
            for q_off in q_offs:
                for o_off in (16, 20, 24, 28):
                    force(ctx, name)
                    q = qbuf[q_off:q_off + n]
                    buf = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev)
                    rc, _ = member(ctx, code, bounds.to(dev), q, invert=(o_off == 24), out=buf[o_off:o_off + n])
                    assert rc == capi.VRS_OK
                    got = buf.cpu().numpy()
                    want = np.isin(as_numpy(q.cpu()), as_numpy(bounds), invert=(o_off == 24))
                    assert np.array_equal(got[o_off:o_off + n], want.astype(np.uint8)), (dtype, n, q_off, o_off)
                    assert (got[:o_off] == CANARY).all() and (got[o_off + n:] == CANARY).all(), (dtype, n, q_off, o_off)
    # 1, 2, 3 bytes off: refused where the buffer is made, nothing written
    buf = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    for by in (1, 2, 3):
        with pytest.raises(vrs.VrsError, match="4-byte aligned"):
            member(ctx, capi.VRS_SORT_INT32, torch.arange(5, dtype=torch.int32, device=dev), torch.arange(8, dtype=torch.int32, device=dev),
                   out=buf[16 + by:24 + by])
    assert bool((buf == CANARY).all())
    # ... and reached by rows: 3 rows of 5, 6, 7 queries start 1 to 3 bytes off
    bounds = boundaries_of("float32", 0, 1000, rng)
    for q_len in (5, 6, 7):
        qs = draw(*pools("float32", 0, rng)[1:], 3 * q_len, rng)
        buf = torch.full((3 * q_len + 32,), CANARY, dtype=torch.uint8, device=dev)
        force(ctx, name)
        rc, _ = member(ctx, capi.VRS_SORT_FLOAT32, bounds.repeat(3).to(dev), qs.to(dev), m=1000, q_len=q_len, out=buf[16:16 + 3 * q_len])
        assert rc == capi.VRS_OK
        got = buf.cpu().numpy()
        assert np.array_equal(got[16:-16], np.isin(as_numpy(qs), as_numpy(bounds)).astype(np.uint8)), q_len
        assert (got[:16] == CANARY).all() and (got[-16:] == CANARY).all()


def test_unsorted_boundaries_give_zero_or_one(ctx, dev):
    """boundaries in no order, and a sorter with entries outside the row: VRS_OK, every byte 0 or 1 (the shape of
    test_unsorted_boundaries_stay_in_range)"""
    rng = np.random.default_rng(41)
    raw = torch.from_numpy(rng.standard_normal(200001).astype(np.float32) * 4).round()
    raw[::7] = float("nan")
    x = torch.from_numpy(rng.standard_normal(100000).astype(np.float32) * 4).round()
    x[::11] = float("nan")
    raw, x = raw.to(dev), x.to(dev)
    wild = torch.randint(-10 ** 12, 10 ** 12, (200001,), device=dev)
    for name in ("direct", "indexed", "lds"):
        seq = raw if name != "lds" else raw[:30000]
        for srt in (None, wild[:seq.numel()]):
            for invert in (False, True):
                force(ctx, name)
                rc, out = member(ctx, capi.VRS_SORT_FLOAT32, seq, x, invert=invert, sorter=srt)
                assert rc == capi.VRS_OK
                assert int(out.max()) <= 1
                assert bool((out[::11] == int(invert)).all())  # a NaN is a member of nothing, whatever the boundaries hold


def test_empty_sides(ctx, dev):
    q = torch.arange(5000, dtype=torch.int32, device=dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    before = vrs.search_stats(ctx)
    for invert in (False, True):
        buf = torch.full((5000 + 32,), CANARY, dtype=torch.uint8, device=dev)
        rc, _ = member(ctx, capi.VRS_SORT_INT32, none, q, invert=invert, out=buf[16:-16])  # no boundaries: nothing is a member
        assert rc == capi.VRS_OK
        assert bool((buf[16:-16] == int(invert)).all()) and bool((buf[:16] == CANARY).all()) and bool((buf[-16:] == CANARY).all())
        rc, _ = member(ctx, capi.VRS_SORT_INT32, q, none, invert=invert, out=buf[:16])  # no queries: VRS_OK, nothing written
        assert rc == capi.VRS_OK and bool((buf[:16] == CANARY).all())
    # three empty boundary rows against three query rows
    rc, out = member(ctx, capi.VRS_SORT_INT32, none, q[:60], m=0, q_len=20, invert=True)
    assert rc == capi.VRS_OK and bool((out == 1).all())
    assert sum(stats_delta(ctx, before).values()) == 0  # (calls without queries or without boundaries run in no tier)


def test_refusals_on_a_valid_context(ctx, dev):
    bad = capi.VRS_ERROR_INVALID_ARGUMENT
    b, q = torch.arange(10, dtype=torch.int32, device=dev), torch.arange(16, dtype=torch.int32, device=dev)
    buf = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    for flags in (MEMBER | capi.VRS_SEARCH_RIGHT, MEMBER | capi.VRS_SEARCH_OUT_INT64, INVERT, MEMBER | 4, MEMBER | 8):
        assert member(ctx, capi.VRS_SORT_INT32, b, q, flags=flags, out=buf)[0] == bad
    assert member(ctx, capi.VRS_SORT_INT32, b, q, out=buf[:12])[0] == bad  # fewer than num_queries bytes
    assert b"out" in ctx.lib.vrs_last_error(ctx.handle)
    with buffers(ctx, b, buf) as (bnd, res):  # the identity queries have no membership form
        assert ctx.lib.vrs_search_sorted(ctx.handle, bnd, 10, 10, None, 16, 16, capi.VRS_SORT_INT32, MEMBER, None, res, None) == bad
        assert b"queries" in ctx.lib.vrs_last_error(ctx.handle)
    assert member(ctx, capi.VRS_SORT_INT32, b, q, out=buf[:16])[0] == capi.VRS_OK  # exactly num_queries bytes
    torch.cuda.synchronize()
    assert bool((buf[16:] == CANARY).all())
    assert buf[:16].tolist() == [1] * 10 + [0] * 6


def test_counting_form_is_what_it_was(ctx, dev):
    """the counting call next to the membership call on one context: the same tiers, and torch.searchsorted's positions"""
    rng = np.random.default_rng(690)
    seq = torch.sort(torch.from_numpy(rng.integers(-1000, 1000, 50000)).to(torch.int32)).values.to(dev)
    x = torch.from_numpy(rng.integers(-1100, 1100, 9000)).to(torch.int32).to(dev)
    for name in ("lds", "direct", "indexed"):
        force(ctx, name)
        before = vrs.search_stats(ctx)
        rc, out = member(ctx, capi.VRS_SORT_INT32, seq[:30000] if name == "lds" else seq, x)
        assert rc == capi.VRS_OK
        s = seq[:30000] if name == "lds" else seq
        for right in (False, True):
            assert torch.equal(vrs.searchsorted(s, x, right=right), torch.searchsorted(s, x, right=right))
        assert torch.equal(out.bool(), torch.isin(x, s))
        assert stats_delta(ctx, before)[name] == 3


def test_non_default_stream(dev):
    rng = np.random.default_rng(47)
    seq = torch.sort(torch.from_numpy(rng.standard_normal(2 * 10 ** 6).astype(np.float32)).round(decimals=3)).values.to(dev)
    x = torch.from_numpy(rng.standard_normal(10 ** 6).astype(np.float32)).round(decimals=3).to(dev)
    want = torch.isin(x, seq)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        c = context_for(dev)
        before = vrs.search_stats(c)
        rc, got = member(c, capi.VRS_SORT_FLOAT32, seq, x)
        rc2, small = member(c, capi.VRS_SORT_FLOAT32, seq[::20000].contiguous(), x, invert=True)
        whole = vrs.isin(x, seq)
        after = vrs.search_stats(c)
    side.synchronize()
    assert rc == capi.VRS_OK and rc2 == capi.VRS_OK
    assert torch.equal(got.bool(), want) and torch.equal(whole, want)
    assert torch.equal(small.bool(), torch.isin(x, seq[::20000].contiguous(), invert=True))
    assert c is not context_for(dev) and after["indexed"] - before["indexed"] == 2 and after["lds"] - before["lds"] == 1


def test_never_waits_for_the_device(dev):
    rng = np.random.default_rng(53)
    seq = torch.sort(torch.from_numpy(rng.standard_normal(4 * 10 ** 6).astype(np.float32))).values.to(dev)
    x = torch.from_numpy(rng.standard_normal(2 * 10 ** 6).astype(np.float32)).to(dev)
    x[::2] = seq[::4]
    bnd = seq[::4000].contiguous()
    c = context_for(dev)
    member(c, capi.VRS_SORT_FLOAT32, seq, x)  # warm-up: module load, the context, torch's allocations
    member(c, capi.VRS_SORT_FLOAT32, bnd, x, invert=True)
    torch.cuda.synchronize()
    torch.cuda._sleep(int(60e-3 * 2.0e9))  # about 60 ms of work ahead of the calls
    t0 = time.perf_counter()
    _, a = member(c, capi.VRS_SORT_FLOAT32, seq, x)
    _, b = member(c, capi.VRS_SORT_FLOAT32, bnd, x, invert=True)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert dt < 5e-3, f"the calls took {dt * 1e3:.2f} ms on the host"
    assert busy
    assert torch.equal(a.bool(), torch.isin(x, seq)) and torch.equal(b.bool(), torch.isin(x, bnd, invert=True))


# ---------------------------------------------------------------------------------------------- vrs.isin against torch.isin

def torch_values(dtype, n, rng):
    _, pool, must = pools(dtype, 0, rng)
    return draw(pool, must, n, rng)


@pytest.mark.parametrize("dtype", DTYPES)
def test_isin_against_torch_on_the_cpu_copy(ctx, dev, dtype):
    rng = np.random.default_rng(790 + DTYPES.index(dtype))
    force(ctx, "natural")
    tests = [torch_values(dtype, 37, rng), torch_values(dtype, 2003, rng), torch_values(dtype, 60, rng).view(3, 20),  # duplicates; 2-D
             boundaries_of(dtype, 1, 1, rng), torch_values(dtype, 0, rng)]
    shapes = [(0,), (7, 0, 3), (), (4097,), (3, 5, 7)]
    for t in tests:
        for shape in shapes:
            x = torch_values(dtype, int(np.prod(shape)), rng).view(shape)
            for invert in (False, True):
                want = torch.isin(x, t, invert=invert)
                got = vrs.isin(x.to(dev), t.to(dev), invert=invert)
                assert got.dtype == torch.bool and got.shape == want.shape and got.device == dev
                assert torch.equal(got.cpu(), want), (dtype, tuple(t.shape), shape, invert)
        # not contiguous: [5, 7] transposed
        x = torch_values(dtype, 35, rng).view(5, 7).t()
        assert not x.is_contiguous()
        got = vrs.isin(x.to(dev).t().contiguous().t(), t.to(dev))
        assert got.shape == (7, 5) and torch.equal(got.cpu(), torch.isin(x, t))
        same = vrs.isin(x.to(dev), t.to(dev), assume_unique=True)
        assert torch.equal(same.cpu(), torch.isin(x, t, assume_unique=False))
    if dtype in NARROW:  # enough elements for the table
        x, t = torch_values(dtype, 2 ** 16 + 3, rng), torch_values(dtype, 500, rng)
        before = vrs.search_stats(ctx)
        assert torch.equal(vrs.isin(x.to(dev), t.to(dev), invert=True).cpu(), torch.isin(x, t, invert=True))
        assert stats_delta(ctx, before)["table"] == 1


def test_isin_numbers_promotion_and_documented_answers(ctx, dev):
    force(ctx, "natural")
    nan = float("nan")
    x = torch.tensor([nan, 0.0, -0.0, 1.0, 2.0], device=dev)
    few = torch.tensor([nan, -0.0, 2.0], device=dev)
    many = torch.cat([few, torch.arange(5.0, 2005.0, device=dev)])
    for t in (few, many):
        assert vrs.isin(x, t).tolist() == [False, True, True, False, True]
        assert vrs.isin(x, t, invert=True).tolist() == [True, False, False, True, False]
    # promotion: both sides to torch.result_type
    got = vrs.isin(torch.tensor([1, 2, 3], dtype=torch.int32, device=dev), torch.tensor([2.0, 3.5], device=dev))
    assert got.tolist() == [False, True, False]
    h, b = torch.tensor([1.0, 1.0009765625, 3.0, nan], dtype=torch.float16), torch.tensor([1.0, 3.0, nan, 1.0078125], dtype=torch.bfloat16)
    assert torch.equal(vrs.isin(h.to(dev), b.to(dev)).cpu(), torch.isin(h, b))
    assert torch.equal(vrs.isin(b.to(dev), h.to(dev), invert=True).cpu(), torch.isin(b, h, invert=True))
    # (integers that become floats are drawn from the small values, exact in the float type: distinct int64 elements that collide in
    #  float64 are told apart by neither side, and torch's sorted path on the CPU then reports them as members of each other)
    for a, va, t, vt in (("int16", 0, "int64", 0), ("uint8", 0, "int8", 0), ("int64", 2, "float64", 0), ("float32", 0, "int32", 2)):
        rng = np.random.default_rng(890)
        xa, tt = draw(*pools(a, va, rng)[1:], 999, rng), draw(*pools(t, vt, rng)[1:], 77, rng)
        assert torch.equal(vrs.isin(xa.to(dev), tt.to(dev)).cpu(), torch.isin(xa, tt)), (a, t)
    # Python numbers on either side
    ints = torch.tensor([[1, 2], [2, 5]], device=dev)
    assert vrs.isin(ints, 2).tolist() == [[False, True], [True, False]] and vrs.isin(ints, 2.0, invert=True).tolist() == [[True, False], [False, True]]
    assert vrs.isin(ints, 2.5).tolist() == [[False, False], [False, False]]
    for v, want in ((2, True), (3, False), (2.5, False), (nan, False)):
        got = vrs.isin(v, ints)
        assert got.shape == () and got.dtype == torch.bool and got.device == dev and got.item() is want
    assert vrs.isin(nan, few).item() is False and vrs.isin(-0.0, torch.tensor([0.0], device=dev)).item() is True
    # an empty test set
    assert vrs.isin(torch.tensor([1.0], device=dev), torch.tensor([], device=dev)).tolist() == [False]
    assert vrs.isin(torch.tensor([1.0], device=dev), torch.tensor([], device=dev), invert=True).tolist() == [True]
    before = vrs.search_stats(ctx)
    vrs.isin(torch.empty(7, 0, 3, device=dev), few)
    vrs.isin(x, torch.empty(0, device=dev))
    assert sum(stats_delta(ctx, before).values()) == 0  # no launch for an empty side
    with pytest.raises(vrs.VrsError):
        vrs.isin(x, few.cpu())
    with pytest.raises(RuntimeError, match="Bool"):
        vrs.isin(x > 0, few)
