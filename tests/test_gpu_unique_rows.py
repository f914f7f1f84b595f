"""The row form of vrs_unique / vrs_run_length_encode on the device (VRS_UNIQUE_COLUMNS(C), unique(dim=d), unique_consecutive(dim=d)):
the C calls against numpy (np.unique(axis=0) of the rank-mapped unsigned view; the runs of bit-identical rows), their memory contract
in the guarded arena, the torch wrappers against torch's CPU results, and row-form calls interleaved with the word form and the sort on
one context.  Every comparison is bit-exact."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

from .test_gpu_memory_contract import Case, Spec, as_bytes, run_case, run_refusals, wrap_align
from .test_gpu_unique import KT, PAD, SENTINEL, download, garbage_scratch, rank, sentinel_buffer, upload

uq = importlib.import_module("vkradixsort_amd.unique")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TILE = capi.RLE_TILE
COLS = capi.VRS_UNIQUE_COLUMNS
SIZES = [1, 2, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
# one group; two groups with a lone column 0; three groups (4-byte words) -- one group per column (8-byte words)
COLUMNS = {4: [2, 3, 5], 8: [2, 3]}
KT_COLS = [(kt, c) for kt in KT for c in COLUMNS[8 if kt.endswith("64") else 4]]
KINDS = ["equal", "distinct", "few", "last_column", "first_column", "tile_edges", "negative", "specials"]


@pytest.fixture(scope="module")
def ctx():
    c = vrs.GPUContext(0)
    c.init()
    yield c
    c.shutdown()


def word_dtype(kt):
    return np.uint64 if kt.endswith("64") else np.uint32


def pool_of(kind, kt):
    wide = kt.endswith("64")
    if kind == "negative":  # two's complement extremes and small negatives
        top = 1 << (63 if wide else 31)
        vals = [0, 1, top - 1, top, top + 1, 2 * top - 1, 2 * top - 2]
    elif wide:  # specials: -0.0, +0.0, +-inf, NaNs of both signs and two payloads, +-1.0
        vals = [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000,
                0xFFF8000000000001, 0x3FF0000000000000, 0xBFF0000000000000]
    else:
        vals = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC00001, 0x3F800000, 0xBF800000]
    return np.array(vals, dtype=np.uint64).astype(word_dtype(kt))


def sorted_tile_edge_rows(n, C, dt):
    """rows in sorted order whose runs end at multiples of the tile and one before and after; neighbouring runs differ in column 0 or
    only in the last column"""
    cuts = sorted({t * TILE + d for t in range(1, n // TILE + 2) for d in (-1, 0, 1) if 0 < t * TILE + d < n})
    heads = np.zeros(n, np.int64)
    heads[cuts] = 1
    r = np.cumsum(heads)
    a = np.full((n, C), 7, dt)
    a[:, 0] = r // 2
    a[:, C - 1] = r % 2
    return a


def rows_input(kind, kt, n, C, seed):
    rng = np.random.default_rng(seed)
    dt = word_dtype(kt)
    if kind == "equal":
        a = np.tile(rng.integers(0, 1 << 31, C).astype(dt), (n, 1))
    elif kind == "distinct":
        a = rng.integers(0, 3, (n, C)).astype(dt)
        a[:, rng.integers(0, C)] = rng.permutation(n).astype(dt) * dt(2654435761)
    elif kind == "few":
        a = rng.integers(0, 3, (n, C)).astype(dt)
    elif kind == "last_column":
        a = np.tile(rng.integers(0, 1 << 31, C).astype(dt), (n, 1))
        a[:, C - 1] = rng.integers(0, 5, n).astype(dt)
    elif kind == "first_column":
        a = np.tile(rng.integers(0, 1 << 31, C).astype(dt), (n, 1))
        a[:, 0] = rng.integers(0, 5, n).astype(dt)
    elif kind == "tile_edges":
        a = sorted_tile_edge_rows(n, C, dt)[rng.permutation(n)]
    else:
        pool = pool_of(kind, kt)
        a = pool[rng.integers(0, pool.size, (n, C))]
        a[:, : C - 1] = a[rng.integers(0, min(n, 3), n), : C - 1]  # few distinct prefixes: rows that tie in all but the last column
    return np.ascontiguousarray(a)


def ref_unique_rows(bits, kt):
    """(first occurrence of each distinct row in sorted order, inverse, counts) by numpy on the rank-mapped unsigned words"""
    _, first, inv, cnt = np.unique(rank(bits, kt), axis=0, return_index=True, return_inverse=True, return_counts=True)
    return first, inv.reshape(-1).astype(np.uint32), cnt.astype(np.uint32)


def ref_row_runs(a):
    """(rows, offsets incl. n, counts, run ids) of the runs of bit-identical consecutive rows"""
    n = a.shape[0]
    heads = np.ones(n, bool)
    heads[1:] = np.any(a[1:] != a[:-1], axis=1)
    starts = np.flatnonzero(heads)
    offsets = np.append(starts, n).astype(np.uint32)
    return a[starts], offsets, np.diff(offsets).astype(np.uint32), (np.cumsum(heads) - 1).astype(np.uint32)


def collect(bufs, live, dtypes):
    """downloads every given buffer, checks the sentinel pad past its live entries, releases it"""
    got = {}
    for name, b in bufs.items():
        if b is None:
            continue
        dt = np.dtype(dtypes[name])
        whole = download(b, dt, b.getSizeBytes() // dt.itemsize)
        assert np.all(whole[live[name]:].view(np.uint8) == SENTINEL), f"{name} written past {live[name]} entries"
        got[name] = whole[:live[name]]
        b.release()
    return got


def run_unique_rows(c, bits, kt, inverse=True, counts=True, seed=0):
    n, C = bits.shape
    kb = upload(c, bits)
    bufs = {"keys": sentinel_buffer(c, bits.dtype, n * C), "counts": sentinel_buffer(c, np.uint32, n) if counts else None,
            "inverse": sentinel_buffer(c, np.uint32, n) if inverse else None}
    runs = upload(c, np.full(1, 0xDEADBEEF, np.uint32))
    scr = garbage_scratch(c, uq.unique_scratch_bytes(n, kt, inverse, counts, columns=C), seed)
    uq.unique_keys(c, kb, n, bufs["keys"], runs, scr, key_type=kt, out_counts=bufs["counts"], out_inverse=bufs["inverse"], columns=C)
    R = int(download(runs, np.uint32, 1)[0])
    got = collect(bufs, {"keys": R * C, "counts": R, "inverse": n}, {"keys": bits.dtype, "counts": np.uint32, "inverse": np.uint32})
    assert np.array_equal(download(kb, bits.dtype, n * C).reshape(n, C), bits), "the input was written"
    for b in (kb, runs, scr):
        b.release()
    return R, got


def check_unique_rows(c, bits, kt, inverse=True, counts=True, seed=0):
    R, got = run_unique_rows(c, bits, kt, inverse, counts, seed)
    first, inv, cnt = ref_unique_rows(bits, kt)
    assert R == first.size
    assert np.array_equal(got["keys"].reshape(R, -1), bits[first]), "rows differ"
    if counts:
        assert np.array_equal(got["counts"], cnt), "counts differ"
    if inverse:
        assert np.array_equal(got["inverse"], inv), "inverse differs"


ALL = ("keys", "offsets", "counts", "run_ids")
COMBOS = [set(s) for r in range(len(ALL) + 1) for s in itertools.combinations(ALL, r)]


def run_encode_rows(c, a, outputs, seed=0):
    n, C = a.shape
    width = a.dtype.itemsize
    kb = upload(c, a)
    bufs = {"keys": sentinel_buffer(c, a.dtype, n * C) if "keys" in outputs else None,
            "offsets": sentinel_buffer(c, np.uint32, n + 1) if "offsets" in outputs else None,
            "counts": sentinel_buffer(c, np.uint32, n) if "counts" in outputs else None,
            "run_ids": sentinel_buffer(c, np.uint32, n) if "run_ids" in outputs else None}
    runs = upload(c, np.full(1, 0xDEADBEEF, np.uint32))
    scr = garbage_scratch(c, uq.rle_scratch_bytes(n, width, counts="counts" in outputs and "offsets" not in outputs, columns=C), seed)
    uq.run_length_encode(c, kb, n, runs, scr, width, out_keys=bufs["keys"], out_offsets=bufs["offsets"], out_counts=bufs["counts"],
                         out_run_ids=bufs["run_ids"], columns=C)
    R = int(download(runs, np.uint32, 1)[0])
    got = collect(bufs, {"keys": R * C, "offsets": R + 1, "counts": R, "run_ids": n},
                  {"keys": a.dtype, "offsets": np.uint32, "counts": np.uint32, "run_ids": np.uint32})
    assert np.array_equal(download(kb, a.dtype, n * C).reshape(n, C), a), "the input was written"
    for b in (kb, runs, scr):
        b.release()
    return R, got


def check_encode_rows(c, a, outputs, seed=0):
    R, got = run_encode_rows(c, a, outputs, seed)
    rows, offsets, counts, ids = ref_row_runs(a)
    assert R == rows.shape[0]
    ref = {"keys": rows.reshape(-1), "offsets": offsets, "counts": counts, "run_ids": ids}
    for name, v in got.items():
        assert np.array_equal(v, ref[name]), f"{name} differs at {np.flatnonzero(v != ref[name])[:8]}"


# ---- the C calls -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kt,C", KT_COLS)
def test_unique_rows_against_numpy(ctx, kt, C, kind):
    for n in SIZES:
        check_unique_rows(ctx, rows_input(kind, kt, n, C, n + C), kt, seed=n)


@pytest.mark.parametrize("kt,C", KT_COLS)
def test_unique_rows_every_output_combination(ctx, kt, C):
    bits = rows_input("few", kt, TILE + 1, C, 3)
    for inverse, counts in itertools.product((True, False), repeat=2):
        check_unique_rows(ctx, bits, kt, inverse, counts, seed=int(inverse) + 2 * int(counts))


def encode_input(kind, kt, n, C, seed):
    """rows with runs: the kinds of rows_input in an order that has them (sorted by rank, or the tile edges as they are)"""
    if kind == "tile_edges":
        return sorted_tile_edge_rows(n, C, word_dtype(kt))
    a = rows_input(kind, kt, n, C, seed)
    if kind in ("few", "negative", "specials"):
        a = a[np.random.default_rng(seed).integers(0, min(n, 4), n)]  # long runs in any order
        return np.ascontiguousarray(np.repeat(a[::3], 3, axis=0)[:n]) if n >= 3 else a
    return a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width,C", [(w, c) for w in (4, 8) for c in COLUMNS[w]])
def test_encode_rows_against_the_runs_of_rows(ctx, width, C, kind):
    kt = "f64" if width == 8 else "f32"
    for n in SIZES:
        check_encode_rows(ctx, encode_input(kind, kt, n, C, n + C), set(ALL), seed=n)


@pytest.mark.parametrize("width,C", [(4, 3), (8, 2)])
def test_encode_rows_every_output_combination(ctx, width, C):
    a = encode_input("tile_edges", "u64" if width == 8 else "u32", TILE + 1, C, 1)
    for i, outputs in enumerate(COMBOS):
        check_encode_rows(ctx, a, outputs, seed=i)


@pytest.mark.parametrize("kt", list(KT))
def test_one_column_with_the_bit_field_set_is_the_plain_call(ctx, kt):
    n = TILE + 77
    bits = rows_input("few", kt, n, 1, 5).reshape(-1)
    width = bits.dtype.itemsize
    lib = ctx.lib

    def unique_call(key_type):
        kb, ok, oc, oi = upload(ctx, bits), sentinel_buffer(ctx, bits.dtype, n), sentinel_buffer(ctx, np.uint32, n), sentinel_buffer(ctx, np.uint32, n)
        runs, scr = upload(ctx, np.full(1, 0xDEADBEEF, np.uint32)), garbage_scratch(ctx, uq.unique_scratch_bytes(n, kt, True, True), 1)
        assert lib.vrs_unique(ctx.handle, kb.handle, n, key_type, ok.handle, oc.handle, oi.handle, runs.handle, scr.handle) == capi.VRS_OK
        out = [download(b, np.uint8, b.getSizeBytes()).tobytes() for b in (ok, oc, oi, runs)]
        for b in (kb, ok, oc, oi, runs, scr):
            b.release()
        return out

    def encode_call(key_bytes):
        kb, ok, oo = upload(ctx, bits), sentinel_buffer(ctx, bits.dtype, n), sentinel_buffer(ctx, np.uint32, n + 1)
        oc, oi = sentinel_buffer(ctx, np.uint32, n), sentinel_buffer(ctx, np.uint32, n)
        runs, scr = upload(ctx, np.full(1, 0xDEADBEEF, np.uint32)), garbage_scratch(ctx, uq.rle_scratch_bytes(n, width), 1)
        assert lib.vrs_run_length_encode(ctx.handle, kb.handle, n, key_bytes, ok.handle, oo.handle, oc.handle, oi.handle, runs.handle,
                                         scr.handle) == capi.VRS_OK
        out = [download(b, np.uint8, b.getSizeBytes()).tobytes() for b in (ok, oo, oc, oi, runs)]
        for b in (kb, ok, oo, oc, oi, runs, scr):
            b.release()
        return out

    plain = unique_call(KT[kt])
    assert unique_call(KT[kt] | COLS(1)) == plain and unique_call(KT[kt] | COLS(0)) == plain
    plain = encode_call(width)
    assert encode_call(width | COLS(1)) == plain


def sort_form(lib, n, key_bytes):
    form = ctypes.c_int()
    assert lib.vrs_sort_form_for(n, key_bytes, 1, None, 0, ctypes.byref(form), None) == 0
    return capi.FORM_NAMES[form.value]


def first_n_past_the_small_forms(lib, key_bytes):
    """the smallest N whose pair sort of such keys is neither the single nor the contract form (the forms come in order of size)"""
    lo, hi = 1, 1 << 22
    assert sort_form(lib, lo, key_bytes) in ("single", "contract") and sort_form(lib, hi, key_bytes) not in ("single", "contract")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sort_form(lib, mid, key_bytes) in ("single", "contract"):
            lo = mid
        else:
            hi = mid
    return hi


@pytest.mark.parametrize("key_bytes,kt,C", [(4, "i32", 3), (8, "i64", 2)])
def test_unique_rows_where_the_inner_sort_leaves_the_small_forms(key_bytes, kt, C):
    """two groups, few distinct words: i32 x 3 sorts 64-bit keys and then the lone column's 32-bit keys, i64 x 2 64-bit keys twice"""
    with vrs.GPUContext(0) as c:  # a fresh context: the defaults vrs_sort_form_for assumes
        n = first_n_past_the_small_forms(c.lib, key_bytes)
        assert sort_form(c.lib, n - 1, key_bytes) in ("single", "contract")
        for m in (n - 1, n):
            check_unique_rows(c, rows_input("few", kt, m, C, m), kt, seed=m)


def test_refusals_on_the_device_leave_everything_alone(ctx):
    n, C = 1000, 3
    bits = rows_input("few", "u32", n, C, 1)
    kb, ok = upload(ctx, bits), sentinel_buffer(ctx, np.uint32, n * C)
    runs = upload(ctx, np.full(1, 0xDEADBEEF, np.uint32))
    scr = garbage_scratch(ctx, uq.unique_scratch_bytes(n, "u32", True, True, columns=C), 0)
    small = upload(ctx, np.zeros(n * C - 1, np.uint32))
    lib, h = ctx.lib, ctx.handle
    bad = capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_unique(h, kb.handle, n, 6 | COLS(C), ok.handle, None, None, runs.handle, scr.handle) == bad  # an unknown low byte
    assert lib.vrs_unique(h, kb.handle, n, -1, ok.handle, None, None, runs.handle, scr.handle) == bad
    assert lib.vrs_unique(h, kb.handle, n, capi.VRS_UNIQUE_U32 | COLS(C), small.handle, None, None, runs.handle, scr.handle) == bad  # rows x C words
    assert lib.vrs_unique(h, small.handle, n, capi.VRS_UNIQUE_U32 | COLS(C), ok.handle, None, None, runs.handle, scr.handle) == bad
    assert lib.vrs_unique(h, kb.handle, n, capi.VRS_UNIQUE_U32 | COLS(C), ok.handle, None, None, runs.handle, small.handle) == bad  # the scratch
    assert lib.vrs_unique(h, kb.handle, n, capi.VRS_UNIQUE_U32 | COLS((1 << 23) - 1), ok.handle, None, None, runs.handle, scr.handle) == bad  # n x C >= 2^32
    assert lib.vrs_run_length_encode(h, kb.handle, n, 5 | COLS(C), None, None, None, None, runs.handle, scr.handle) == bad
    assert lib.vrs_run_length_encode(h, kb.handle, n, 4 | COLS(C), small.handle, None, None, None, runs.handle, scr.handle) == bad
    assert lib.vrs_run_length_encode(h, kb.handle, n, 8 | COLS(C), None, None, None, None, runs.handle, scr.handle) == bad  # 8-byte words: keys too small
    assert download(runs, np.uint32, 1)[0] == 0xDEADBEEF
    assert np.all(download(ok, np.uint8, ok.getSizeBytes()) == SENTINEL)
    for b in (kb, ok, runs, scr, small):
        b.release()


# ---- the memory contract ---------------------------------------------------------------------------------------------------------------

N_ARENA = 2 * TILE + 77  # three tiles of the look-back, a tail that is no multiple of 64


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def actx(dev):
    from vkradixsort_amd._torch import context_for
    return context_for(dev)  # the torch stream's context: reading the arena is ordered after the call


def unique_rows_case(kt, C, inverse, counts):
    n = N_ARENA
    a = rows_input("few", kt, n, C, 9)
    width = a.dtype.itemsize
    first, inv, cnt = ref_unique_rows(a, kt)
    R = first.size
    flags = (capi.VRS_UNIQUE_INVERSE if inverse else 0) | (capi.VRS_UNIQUE_COUNTS if counts else 0)
    key_type = KT[kt] | COLS(C)
    need = capi.query_u64("vrs_unique_scratch_bytes", n, key_type, flags)
    specs = [Spec("keys", n * C * width, "in", wrap_align(width), a), Spec("num_runs", 4, "out", 4), Spec("scratch", need, "scratch", 8),
             Spec("out_keys", n * C * width, "out", wrap_align(width), writable=[(0, R * C * width)])]
    expect = {"num_runs": np.uint32(R).tobytes(), "out_keys": as_bytes(a[first])}
    refuse = {"scratch": 1, "num_runs": 1, "out_keys": width, "keys": width}
    if counts:
        specs.append(Spec("out_counts", n * 4, "out", 4, writable=[(0, R * 4)]))
        expect["out_counts"], refuse["out_counts"] = as_bytes(cnt), 4
    if inverse:
        specs.append(Spec("out_inverse", n * 4, "out", 4))
        expect["out_inverse"], refuse["out_inverse"] = as_bytes(inv), 4

    def call(c, h):
        return c.lib.vrs_unique(c.handle, h["keys"], n, key_type, h["out_keys"], h["out_counts"], h["out_inverse"], h["num_runs"], h["scratch"])

    return Case(specs, call, expect, refuse=refuse, misalign={"scratch": 4})


ARENA_COMBOS = {"none": (), "all": ALL, "keys-alone": ("keys",), "counts-alone": ("counts",), "offsets-and-run-ids": ("offsets", "run_ids")}


def encode_rows_case(width, C, combo):
    n = N_ARENA
    a = encode_input("tile_edges", "u64" if width == 8 else "u32", n, C, 5)
    rows, offsets, counts, ids = ref_row_runs(a)
    R = rows.shape[0]
    outputs = ARENA_COMBOS[combo]
    key_bytes = width | COLS(C)
    need = capi.query_u64("vrs_run_length_encode_scratch_bytes", n, key_bytes, 0)
    specs = [Spec("keys", n * C * width, "in", wrap_align(width), a), Spec("num_runs", 4, "out", 4), Spec("scratch", need, "scratch", 8)]
    expect, refuse = {"num_runs": np.uint32(R).tobytes()}, {"scratch": 1, "num_runs": 1, "keys": width}
    for name, entries, live, want, item in (("out_keys", n * C, R * C, rows, width), ("out_offsets", n + 1, R + 1, offsets, 4),
                                            ("out_counts", n, R, counts, 4), ("out_run_ids", n, n, ids, 4)):
        if name[4:] in outputs:
            specs.append(Spec(name, entries * item, "out", wrap_align(item), writable=[(0, live * item)]))
            expect[name], refuse[name] = as_bytes(want), item

    def call(c, h):
        return c.lib.vrs_run_length_encode(c.handle, h["keys"], n, key_bytes, h["out_keys"], h["out_offsets"], h["out_counts"], h["out_run_ids"],
                                           h["num_runs"], h["scratch"])

    return Case(specs, call, expect, refuse=refuse, misalign={"scratch": 4})


@pytest.mark.parametrize("outputs", ["keys-only", "inverse", "counts", "inverse-and-counts"])
@pytest.mark.parametrize("kt,C", [("i32", 2), ("f32", 3), ("u32", 5), ("f64", 2), ("i64", 3)])
def test_unique_rows_memory_contract(actx, dev, kt, C, outputs):
    run_case(actx, dev, f"unique rows {kt} x {C} {outputs}", unique_rows_case(kt, C, "inverse" in outputs, "counts" in outputs))


@pytest.mark.parametrize("combo", list(ARENA_COMBOS))
@pytest.mark.parametrize("width,C", [(4, 2), (4, 3), (8, 2), (8, 3)])
def test_encode_rows_memory_contract(actx, dev, width, C, combo):
    run_case(actx, dev, f"encode rows {width}-byte x {C}, {combo}", encode_rows_case(width, C, combo))


def test_row_forms_refuse_short_and_misaligned_buffers(actx, dev):
    run_refusals(actx, dev, "unique rows", unique_rows_case("f64", 3, True, True))
    run_refusals(actx, dev, "unique rows, one group", unique_rows_case("i32", 2, True, True))
    run_refusals(actx, dev, "encode rows", encode_rows_case(4, 3, "all"))
    run_refusals(actx, dev, "encode rows, the offsets in the scratch", encode_rows_case(8, 2, "keys-alone"))


# ---- torch -----------------------------------------------------------------------------------------------------------------------------

DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64]
FLAGS = list(itertools.product((False, True), repeat=2))


def torch_rows(dtype, shape, distinct, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randint(0, distinct, shape, device="cuda", generator=g)
    if dtype.is_floating_point:
        return (v.to(dtype) - distinct / 2) * 0.25 + 0.125  # no NaN, no -0.0
    return (v - distinct // 2).to(dtype) * 977


def same(a, b):
    b = b.cuda()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b)


def tuples(got, ref):
    got, ref = (got, ref) if isinstance(ref, tuple) else ((got,), (ref,))
    assert isinstance(got, tuple) and len(got) == len(ref)
    return list(zip(got, ref))


def check_torch(x, d):
    cpu = x.cpu()
    for inv, cnt in FLAGS:
        for srt in (True, False):
            for a, b in tuples(vrs.unique(x, sorted=srt, return_inverse=inv, return_counts=cnt, dim=d),
                               torch.unique(cpu, sorted=True, return_inverse=inv, return_counts=cnt, dim=d)):
                same(a, b)
        for a, b in tuples(vrs.unique_consecutive(x, return_inverse=inv, return_counts=cnt, dim=d),
                           torch.unique_consecutive(cpu, return_inverse=inv, return_counts=cnt, dim=d)):
            same(a, b)
    values, inverse = vrs.unique(x, return_inverse=True, dim=d)
    assert torch.equal(values.index_select(d, inverse), x)  # the inverse rebuilds x
    again = vrs.unique(x, return_inverse=True, return_counts=True, dim=d)
    for a, b in zip(again, vrs.unique(x, return_inverse=True, return_counts=True, dim=d)):
        assert torch.equal(a, b)  # two runs, the same bits
    values, inverse = vrs.unique_consecutive(x, return_inverse=True, dim=d)
    assert torch.equal(values.index_select(d, inverse), x)


def check_torch_once(x, d):
    """check_torch with one call of each function: every result at once.  For rows of thousands of columns, where a call is thousands of
    rounds: the flags choose among the same results (check_torch covers the choosing on every narrower row)."""
    cpu = x.cpu()
    got = vrs.unique(x, return_inverse=True, return_counts=True, dim=d)
    for a, b in tuples(got, torch.unique(cpu, return_inverse=True, return_counts=True, dim=d)):
        same(a, b)
    assert torch.equal(got[0].index_select(d, got[1]), x)
    got = vrs.unique_consecutive(x, return_inverse=True, return_counts=True, dim=d)
    for a, b in tuples(got, torch.unique_consecutive(cpu, return_inverse=True, return_counts=True, dim=d)):
        same(a, b)
    assert torch.equal(got[0].index_select(d, got[1]), x)


SHAPES = [lambda n: (n,), lambda n: (n, 2), lambda n: (2, n), lambda n: (7, n, 3)]
SHAPE_DIMS = [(k, d) for k, rank_ in enumerate((1, 2, 2, 3)) for d in range(-rank_, rank_)]


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("k,d", SHAPE_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_unique_along_every_dim_equals_torch(dtype, k, d, n):
    """shapes [N], [N, 2], [2, N] and [7, N, 3], every dim"""
    x = torch_rows(dtype, SHAPES[k](n), 3, 10 * n + k)
    rounds = x.numel() // x.shape[d] * x.element_size() // 8
    (check_torch if rounds <= 64 else check_torch_once)(x, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_unique_of_a_small_cube_along_every_dim(dtype):
    x = torch_rows(dtype, (4, 5, 6), 2, 77)
    for d in range(-3, 3):
        check_torch(x, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_transposed_and_strided_inputs(dtype):
    base = torch_rows(dtype, (130, 6), 2, 11)
    for x, dims in ((base.t(), (0, 1, -1)), (base[::2], (0, 1)), (base[:, 1::2], (0, -1)), (base.t()[1::2, 3:100:3], (0, 1))):
        assert not x.is_contiguous()
        for d in dims:
            check_torch(x, d)
    edges = torch_rows(dtype, (2, 4097), 40, 12)  # edge_index[2, E], dim=1
    check_torch(edges, 1)
    check_torch(torch.sort(edges[0])[0].reshape(-1, 1).expand(-1, 2), 0)  # a stride of zero


def test_torch_empty_and_error_cases():
    for fn, theirs in ((vrs.unique, torch.unique), (vrs.unique_consecutive, torch.unique_consecutive)):
        for shape, d in (((0, 3), 0), ((4, 0, 3), 1), ((0,), 0), ((0,), -1), ((2, 0), -1)):
            x = torch.empty(shape, dtype=torch.int64, device="cuda")
            for inv, cnt in FLAGS:
                for a, b in tuples(fn(x, return_inverse=inv, return_counts=cnt, dim=d), theirs(x.cpu(), return_inverse=inv, return_counts=cnt, dim=d)):
                    same(a, b)
        for shape, d in (((3, 0), 0), ((2, 0, 3), 2), ((0, 0), 0), ((0, 4, 0), 0)):
            x = torch.empty(shape, dtype=torch.float32, device="cuda")
            with pytest.raises(RuntimeError, match="There are 0 sized dimensions, and they aren't selected, so unique cannot be applied") as e:
                fn(x, dim=d)
            assert not isinstance(e.value, vrs.VrsError)
            with pytest.raises(RuntimeError):
                theirs(x.cpu(), dim=d)
        for x, d in ((torch.zeros(3, 4, device="cuda"), 2), (torch.zeros(3, device="cuda"), -2), (torch.tensor(1.0, device="cuda"), 0)):
            with pytest.raises(IndexError) as ours:
                fn(x, dim=d)
            with pytest.raises(IndexError) as ref:
                theirs(x.cpu(), dim=d)
            assert str(ours.value) == str(ref.value)
        with pytest.raises(vrs.VrsError, match="int32"):
            fn(torch.zeros(4, 2, dtype=torch.int16, device="cuda"), dim=0)
        with pytest.raises(vrs.VrsError, match="contiguous"):  # dim=None keeps refusing strides
            fn(torch.zeros(4, 6, device="cuda")[:, ::2])


def test_row_form_calls_interleaved_with_the_word_form_and_the_sort():
    """40 seeded cases on the torch stream's context: a pending one-call sort is settled by the next call, the scratch of every call is
    a fresh allocation that the caching allocator hands out again"""
    rng = np.random.default_rng(2024)
    for case in range(40):
        dtype = DTYPES[int(rng.integers(0, 4))]
        n = int(rng.choice([1, 2, 63, 4096, 4097, 9001, 20000]))
        C = int(rng.integers(2, 7))
        x = torch_rows(dtype, (n, C), int(rng.integers(2, 6)), case)
        flat = torch_rows(dtype, (int(rng.integers(1, 30000)),), 50, 1000 + case)
        order = rng.permutation(4)
        for step in order:
            if step == 0:
                for a, b in tuples(vrs.unique(x, return_inverse=True, return_counts=True, dim=0),
                                   torch.unique(x.cpu(), return_inverse=True, return_counts=True, dim=0)):
                    same(a, b)
            elif step == 1:
                for a, b in tuples(vrs.unique(flat, return_inverse=True, return_counts=True), torch.unique(flat.cpu(), return_inverse=True, return_counts=True)):
                    same(a, b)
            elif step == 2:
                values, _ = vrs.sort(flat, stable=True)
                same(values, torch.sort(flat.cpu(), stable=True)[0])
            else:
                y = x[torch.sort(x[:, 0], stable=True)[1]]
                for a, b in tuples(vrs.unique_consecutive(y, return_inverse=True, return_counts=True, dim=0),
                                   torch.unique_consecutive(y.cpu(), return_inverse=True, return_counts=True, dim=0)):
                    same(a, b)
