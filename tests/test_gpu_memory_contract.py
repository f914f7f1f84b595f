"""Every C call's memory contract, in one guarded and poisoned arena (tests/_arena.py).

The headers promise where a call may write ("keys is never written", "entries past R are never written", "gaps no segment covers are
not touched"), what it needs ("scratch: at least vrs_*_scratch_bytes(...) bytes") and what it may assume ("scratch contents on entry
unspecified").  A case here lays ALL buffers of one call into one allocation -- each of exactly its documented bytes, wrapped with
vrs_buffer_wrap at that size, guards between them -- fills everything with seeded random bytes, and runs the call in two layouts
("round": 256-byte starts; "tight": each range on its demanded alignment and off the next one) under two seeds.  It asserts
  (a) no byte outside the writable intervals changed, anywhere in the arena;
  (b) the outputs equal a CPU reference, bit for bit;
  (c) the outputs under the two poisons are the same bits;
  (d) the tier or stats counter shows that the intended path ran.
Size refusals: each output and scratch range, once per entry point, is also handed one element (scratch: one byte) short; the call
must answer VRS_ERROR_INVALID_ARGUMENT and leave the whole arena as it was.

One case per entry point and kernel path, at the smallest shape that reaches the path (thresholds lowered with vrs_set_tuning as the
per-op tests do, defaults restored afterwards).  Not covered: the distributed header, context-owned scratch (a test cannot place it),
reads out of bounds (poison cannot see them) and the torch wrappers above these calls."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi
from vkradixsort_amd._torch import context_for

from ._arena import LAYOUTS, Arena
from .test_compact_cpu import CODES as COMPACT_CODES
from .test_compact_cpu import host_compact
from .test_gpu_unique import KT, rank as unique_rank, ref_runs, rle_input, unique_input
from .test_scan_cpu import CODES, F, MAX, SUM, bits, host_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (11, 12)
BAD = capi.VRS_ERROR_INVALID_ARGUMENT


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    """the torch stream's context (reading the arena is ordered after the call); whatever a test tunes is set back afterwards"""
    c = context_for(dev)
    before = dict(c.tuning)
    c._contract_touched = set()
    yield c
    for key in c._contract_touched:
        c.setTuning(key, before.get(key, DEFAULTS[key]))


DEFAULTS = {
    capi.VRS_TUNE_SCAN_TILE_ROWS: capi.SCAN_TILE_ROWS_DEFAULT,
    capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS: capi.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT,
    capi.VRS_TUNE_COMPACT_TILE_ELEMS: capi.COMPACT_TILE_ELEMS_DEFAULT,
    capi.VRS_TUNE_HYBRID_MIN_KEYS: capi.HYBRID_MIN_KEYS_DEFAULT,
    capi.VRS_TUNE_MSD_POOL_MIN_KEYS: 1 << 22,
    capi.VRS_TUNE_MSD_POOL: 1,
    capi.VRS_TUNE_SEARCH_LDS_BYTES: capi.SEARCH_LDS_BYTES_DEFAULT,
    capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT,
    capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT,
    capi.VRS_TUNE_BINCOUNT_LDS_BYTES: capi.BINCOUNT_LDS_BYTES_DEFAULT,
    capi.VRS_TUNE_REDUCE_CHUNK_ROWS: capi.REDUCE_CHUNK_ROWS_DEFAULT,
    capi.VRS_TUNE_REDUCE_LANE_ROWS: capi.REDUCE_LANE_ROWS_DEFAULT,
    capi.VRS_TUNE_TOPK_GRID_MIN_KEYS: capi.TOPK_GRID_MIN_KEYS_DEFAULT,
    capi.VRS_TUNE_SELECT_GRID_MIN_KEYS: capi.SELECT_GRID_MIN_KEYS_DEFAULT,
    capi.VRS_TUNE_SELECT_COMPACT_DIVISOR: capi.SELECT_COMPACT_DIVISOR_DEFAULT,
    capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS: capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT,
}


def tune(c, key, value):
    c._contract_touched.add(key)
    c.setTuning(key, value)


@dataclass
class Spec:
    """one range of a case.  data: what an input (or an inout range) holds on entry; writable: an output's byte intervals (None: all)"""
    name: str
    nbytes: int
    role: str
    align: int
    data: object = None
    writable: list = None


@dataclass
class Case:
    specs: list
    call: object                # (ctx, {name: handle or None}) -> the call's return code
    expect: dict                # out / inout range -> the bytes its writable intervals must hold afterwards
    counters: object = None     # ctx -> a tuple of cumulative counters ...
    ran: object = None          # ... (before, after) -> True when the intended path ran
    refuse: dict = field(default_factory=dict)  # range -> bytes to hand the call fewer (once per entry point)
    first: object = None        # a call in two steps (compaction: count, then emit): the first step alone ...
    second: object = None       # ... and the second, which is the one that refuses the ranges in `late`
    late: tuple = ()
    canon: object = None        # outputs -> outputs in a canonical order, where the header leaves the order open
    misalign: dict = field(default_factory=dict)  # range -> an alignment below the one the header demands, which the call refuses


def wrap_align(itemsize):
    """what vrs_buffer_wrap demands of a range of such elements"""
    return 8 if itemsize == 8 else 4


def as_bytes(x):
    if isinstance(x, torch.Tensor):
        return bits(x).numpy().tobytes()
    return np.ascontiguousarray(x).tobytes()


class Handles(dict):
    def __missing__(self, name):  # a NULL optional buffer is simply not placed
        return None


def lay(case, dev, seed, layout, name):
    a = Arena(dev, seed, layout, case=name)
    for s in case.specs:
        writable = s.writable if s.role in ("out", "inout") else None
        if s.role in ("out", "inout") and writable is None:
            writable = [(0, s.nbytes)]
        a.place(s.name, s.nbytes, s.role, s.align, writable)
    a.fill()
    for s in case.specs:
        if s.data is not None:
            a.write(s.name, s.data)
    a.snapshot()
    return a


def run_case(ctx, dev, name, case):
    for layout in LAYOUTS:
        runs = []
        for seed in SEEDS:
            a = lay(case, dev, seed, layout, name)
            try:
                before = case.counters(ctx) if case.counters else None
                h = Handles({s.name: a.buffer(ctx, s.name) for s in case.specs})
                rc = case.call(ctx, h)
                assert rc == capi.VRS_OK, (name, layout, rc, ctx.lib.vrs_last_error(ctx.handle))
                a.check()                                                     # (a)
                got = a.outputs()
                if case.canon:
                    got = {**got, **case.canon(got)}
                for out, want in case.expect.items():                         # (b)
                    assert len(got[out]) == len(want), (name, layout, out, len(got[out]), len(want))
                    if got[out] != want:
                        g, w = np.frombuffer(got[out], np.uint8), np.frombuffer(want, np.uint8)
                        at = np.flatnonzero(g != w)
                        raise AssertionError(f"{name}, {layout}, seed {seed}: '{out}' differs from the reference in {at.size} bytes, first at byte {at[0]}")
                if case.ran:                                                  # (d)
                    after = case.counters(ctx)
                    assert case.ran(before, after), (name, layout, before, after)
                runs.append(got)
            finally:
                a.release()
        assert runs[0] == runs[1], (name, layout, "the outputs depend on what the buffers held on entry")  # (c)


def run_refusals(ctx, dev, name, case):
    """each listed range handed short: a refusal on the host that leaves every byte of the arena alone"""
    assert case.refuse
    for short, fewer in case.refuse.items():
        a = lay(case, dev, SEEDS[0], "round", f"{name}: {short} {fewer} bytes short")
        try:
            sizes = {s.name: s.nbytes for s in case.specs}
            assert sizes[short] > fewer, (name, short)
            h = Handles({s.name: a.buffer(ctx, s.name, sizes[s.name] - fewer if s.name == short else None) for s in case.specs})
            if short in case.late:  # the first step runs as it should; what it left is what the refused second step must leave alone
                assert case.first(ctx, h) == capi.VRS_OK
                a.snapshot()
            rc = (case.second if short in case.late else case.call)(ctx, h)
            assert rc == BAD, (name, short, rc)
            a.check(nothing_writable=True)
        finally:
            a.release()
    for name_, align in case.misalign.items():
        specs = [Spec(s.name, s.nbytes, s.role, align if s.name == name_ else s.align, s.data, s.writable) for s in case.specs]
        a = lay(Case(specs, case.call, case.expect), dev, SEEDS[0], "tight", f"{name}: {name_} off its boundary")
        try:
            assert a.ptr(name_) % (2 * align) == align
            assert case.call(ctx, Handles({s.name: a.buffer(ctx, s.name) for s in specs})) == BAD, (name, name_, align)
            a.check(nothing_writable=True)
        finally:
            a.release()
    # and the sizes under guard themselves are taken (the refusals above are about the one byte, not about the case)
    a = lay(case, dev, SEEDS[0], "round", name)
    try:
        assert case.call(ctx, Handles({s.name: a.buffer(ctx, s.name) for s in case.specs})) == capi.VRS_OK
        a.check()
    finally:
        a.release()


def delta(keys):
    """ran(before, after) for dict counters: exactly one call more in each of `keys`, none in the other tiers"""
    def ran(before, after):
        return all(after[k] - before[k] == (1 if k in keys else 0) for k in before if k != "takeovers")
    return ran


# ---------------------------------------------------------------------------------------------- vrs_scan_rows

T = capi.SCAN_TILE_ROWS_MIN
# (S, L, C, dtype, out dtype, op, single-pass threshold, tier): the tile tier (no scratch at all), the three launches with one and two
# levels of carries, the single pass; the flat map and the columns map; a sum, a max with its row numbers, a widened load
SCAN_CASES = {
    "tile-flat-sum-f32": (3, T - 1, 1, torch.float32, None, SUM, 0, "tile"),
    "tile-columns-max-i16": (2, 37, 5, torch.int16, None, MAX, 0, "tile"),
    "three-launch-flat-sum-f32": (3, F * T + 1, 1, torch.float32, None, SUM, 0, "three_launch"),
    "three-launch-flat-max-f64": (1, T + 3, 1, torch.float64, None, MAX, 0, "three_launch"),
    "three-launch-columns-max-f32": (2, T + 3, 65, torch.float32, None, MAX, 0, "three_launch"),
    "three-launch-columns-sum-i8-to-i64": (1, 2 * T + 1, 3, torch.int8, torch.int64, SUM, 0, "three_launch"),
    "single-pass-sum-f32": (3, F * T + 1, 1, torch.float32, None, SUM, 1, "single_pass"),
    "single-pass-sum-bf16": (1, T + 1, 1, torch.bfloat16, None, SUM, 1, "single_pass"),
}


def scan_case(ctx, key):
    S, L, C, dtype, out_dtype, op, min_rows, tier = SCAN_CASES[key]
    out_dtype = out_dtype or dtype
    tune(ctx, capi.VRS_TUNE_SCAN_TILE_ROWS, T)
    tune(ctx, capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, min_rows)
    g = torch.Generator().manual_seed(L + C)
    x = torch.randn(S, L, C, generator=g).to(dtype) if dtype.is_floating_point else torch.randint(-100, 100, (S, L, C), generator=g).to(dtype)
    want, want_idx = host_scan(ctx.lib, x, op, T, out_dtype)
    need = capi.query_u64("vrs_scan_scratch_bytes", S, L, C, CODES[dtype], CODES[out_dtype], op, T, min_rows)
    assert (need == 0) == (tier == "tile")
    eb, ob = x.element_size(), want.element_size()
    specs = [Spec("values", S * L * C * eb, "in", wrap_align(eb), x), Spec("out", S * L * C * ob, "out", wrap_align(ob))]
    expect, refuse = {"out": as_bytes(want)}, {"out": ob}
    if want_idx is not None:
        specs.append(Spec("out_indices", S * L * C * 8, "out", 8))
        expect["out_indices"], refuse["out_indices"] = as_bytes(want_idx), 8
    if need:
        specs.append(Spec("scratch", need, "scratch", 16))
        refuse["scratch"] = 1

    def call(c, h):
        return c.lib.vrs_scan_rows(c.handle, h["values"], S, L, C, CODES[dtype], CODES[out_dtype], op, h["out"], h["out_indices"], h["scratch"])

    return Case(specs, call, expect, vrs.scan_stats, delta({tier}), refuse, misalign={"scratch": 8} if need else {})


@pytest.mark.parametrize("key", list(SCAN_CASES))
def test_scan_rows(ctx, dev, key):
    run_case(ctx, dev, f"scan_rows {key}", scan_case(ctx, key))


def test_scan_rows_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "scan_rows", scan_case(ctx, "three-launch-columns-max-f32"))


# ---------------------------------------------------------------------------------------------- vrs_compact_count + vrs_compact_emit

T0 = capi.COMPACT_TILE_ELEMS_MIN
N_COMPACT = 2 * T0 + 4099  # three tiles, the last neither whole nor a multiple of a chunk or of four


def compact_mask(name, n):
    if name == "none":
        return torch.zeros(n, dtype=torch.bool)
    if name == "all":
        return torch.ones(n, dtype=torch.bool)
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5


# what emit is asked for: flat; coords in either layout; gather; scatter; all of them in one call; the row form
COMPACT_FORMS = ["flat", "coords-rows", "coords-columns", "gather-2", "scatter-8", "all-4", "rows-3", "rows-1025"]


def compact_case(ctx, form, mask_name):
    tune(ctx, capi.VRS_TUNE_COMPACT_TILE_ELEMS, T0)
    W = int(form.split("-")[1]) if form.startswith("rows") else 1
    n = N_COMPACT if W < 1025 else 261  # (the wide rows: a few hundred flags move a quarter of a million elements)
    dims = (3, n // 3) if n % 3 == 0 else (n,)
    flags_dtype = torch.bool if W > 1 else torch.float32 if form == "all-4" else torch.uint8
    mask = compact_mask(mask_name, n)
    flags = mask.to(flags_dtype) if flags_dtype != torch.float32 else torch.where(mask, torch.tensor(float("nan")), torch.tensor(-0.0))
    R = int(mask.sum())
    vb = {"gather-2": 2, "scatter-8": 8, "all-4": 4}.get(form, 4 if W > 1 else 0)
    carrier = {0: None, 2: torch.int16, 4: torch.int32, 8: torch.int64}[vb]
    want_flat = "flat" in form or form == "all-4" or W > 1
    coords = capi.VRS_COMPACT_COLUMNS if form == "coords-columns" else capi.VRS_COMPACT_ROWS if form in ("coords-rows", "all-4") else None
    gather = form in ("gather-2", "all-4") or W > 1
    scatter = form in ("scatter-8", "all-4") or W > 1
    g = torch.Generator().manual_seed(7)
    values = torch.randint(-30000, 30000, (n, W), generator=g).to(carrier) if gather else None
    s_input = torch.randint(-30000, 30000, (n, W), generator=g).to(carrier) if scatter else None
    s_source = torch.randint(-30000, 30000, (max(R, 1), W), generator=g).to(carrier) if scatter else None
    host = host_compact(ctx.lib, flags.reshape(dims), flat=want_flat, coords=coords)
    assert host["count"] == R
    scratch_bytes = capi.query_u64("vrs_compact_scratch_bytes", n, T0)
    fb = flags.element_size()
    specs = [Spec("flags", n * fb, "in", wrap_align(fb), flags), Spec("scratch", scratch_bytes, "scratch", 16), Spec("count", 8, "out", 8)]
    expect, refuse = {"count": np.int64(R).tobytes()}, {"scratch": 1, "count": 1}
    # every output sized to exactly R entries (R x W for rows); an output of no bytes is not given
    if want_flat and R:
        specs.append(Spec("flat", 8 * R, "out", 8))
        expect["flat"], refuse["flat"] = as_bytes(host["flat"]), 8
    if coords is not None and R:
        specs.append(Spec("coords", 8 * R * len(dims), "out", 8))
        expect["coords"], refuse["coords"] = as_bytes(host["coords"]), 8
    if gather:
        specs.append(Spec("gather_values", n * W * vb, "in", wrap_align(vb), values))
        if R:
            specs.append(Spec("gather_out", R * W * vb, "out", wrap_align(vb)))
            expect["gather_out"], refuse["gather_out"] = as_bytes(values[mask]), vb
    if scatter:
        specs.append(Spec("scatter_input", n * W * vb, "in", wrap_align(vb), s_input))
        if R:
            specs.append(Spec("scatter_source", R * W * vb, "in", wrap_align(vb), s_source[:R]))
        specs.append(Spec("scatter_out", n * W * vb, "out", wrap_align(vb)))
        merged = s_input.clone()
        merged[mask] = s_source[:R]
        expect["scatter_out"], refuse["scatter_out"] = as_bytes(merged), vb

    def call(c, h):
        rc = count(c, h)
        return rc if rc != capi.VRS_OK else emit(c, h)

    def count(c, h):
        return c.lib.vrs_compact_count(c.handle, h["flags"], n, COMPACT_CODES[flags_dtype], h["scratch"], h["count"], None)

    def emit(c, h):
        def value(name):
            return h[name].value if h[name] is not None else None
        code = COMPACT_CODES[flags_dtype]
        o = capi.CompactOutputs()
        o.num_selected, o.flat, o.coords = R, value("flat"), value("coords")
        o.coords_layout, o.ndim, o.shape = coords or 0, len(dims), (ctypes.c_uint32 * 8)(*dims)
        o.gather_values, o.gather_out, o.value_bytes, o.row_elems = value("gather_values"), value("gather_out"), vb, W if W > 1 else 0
        o.scatter_input, o.scatter_source, o.scatter_out = value("scatter_input"), value("scatter_source"), value("scatter_out")
        return c.lib.vrs_compact_emit(c.handle, h["flags"], n, code, h["scratch"], ctypes.byref(o))

    def ran(before, after):
        return after["count_calls"] - before["count_calls"] == 1 and after["emit_calls"] - before["emit_calls"] == 1

    late = tuple(k for k in refuse if k not in ("scratch", "count"))
    return Case(specs, call, expect, vrs.compact_stats, ran, refuse, first=count, second=emit, late=late, misalign={"scratch": 8})


@pytest.mark.parametrize("mask_name", ["none", "all", "half"])
@pytest.mark.parametrize("form", COMPACT_FORMS)
def test_compact(ctx, dev, form, mask_name):
    run_case(ctx, dev, f"compact {form} {mask_name}", compact_case(ctx, form, mask_name))


def test_compact_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "compact", compact_case(ctx, "all-4", "half"))


# ---------------------------------------------------------------------------------------------- vrs_run_length_encode, vrs_unique

N_RLE = 2 * capi.RLE_TILE + 77  # three tiles of the look-back, a tail that is no multiple of 64
RLE_OUTPUTS = ("keys", "offsets", "counts", "run_ids")
# every combination of optional outputs that changes the scratch flag (counts without offsets keeps the offsets in the scratch), none, all
RLE_COMBOS = {"none": (), "all": RLE_OUTPUTS, "counts-alone": ("counts",), "counts-and-offsets": ("counts", "offsets"),
              "keys-and-run-ids": ("keys", "run_ids")}


def rle_case(ctx, width, combo, kind="tile_edges"):
    n = N_RLE
    a = rle_input(kind, n, width, 5)
    keys, offsets, counts, ids = ref_runs(a)
    R = keys.size
    outputs = RLE_COMBOS[combo]
    flags = capi.VRS_RLE_COUNTS if "counts" in outputs and "offsets" not in outputs else 0
    need = capi.query_u64("vrs_run_length_encode_scratch_bytes", n, width, flags)
    specs = [Spec("keys", n * width, "in", wrap_align(width), a), Spec("num_runs", 4, "out", 4), Spec("scratch", need, "scratch", 8)]
    expect, refuse = {"num_runs": np.uint32(R).tobytes()}, {"scratch": 1, "num_runs": 1}
    # outputs of n (n + 1) entries, writable only up to R (R + 1)
    for name, entries, live, want, item in (("out_keys", n, R, keys, width), ("out_offsets", n + 1, R + 1, offsets, 4),
                                            ("out_counts", n, R, counts, 4), ("out_run_ids", n, n, ids, 4)):
        if name[4:] in outputs:
            specs.append(Spec(name, entries * item, "out", wrap_align(item), writable=[(0, live * item)]))
            expect[name], refuse[name] = as_bytes(want), item

    def call(c, h):
        return c.lib.vrs_run_length_encode(c.handle, h["keys"], n, width, h["out_keys"], h["out_offsets"], h["out_counts"], h["out_run_ids"],
                                           h["num_runs"], h["scratch"])

    return Case(specs, call, expect, refuse=refuse, misalign={"scratch": 4})


@pytest.mark.parametrize("combo", list(RLE_COMBOS))
@pytest.mark.parametrize("width", [4, 8])
def test_run_length_encode(ctx, dev, width, combo):
    run_case(ctx, dev, f"run_length_encode {width}-byte keys, {combo}", rle_case(ctx, width, combo))


def test_run_length_encode_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "run_length_encode", rle_case(ctx, 4, "all"))
    run_refusals(ctx, dev, "run_length_encode, the offsets in the scratch", rle_case(ctx, 8, "counts-alone"))


def unique_case(ctx, kt, inverse, counts):
    n = N_RLE
    a = unique_input(kt, n, 300, 9)
    width = a.dtype.itemsize
    u, first, inv, cnt = np.unique(unique_rank(a, kt), return_index=True, return_inverse=True, return_counts=True)
    R = u.size
    flags = (capi.VRS_UNIQUE_INVERSE if inverse else 0) | (capi.VRS_UNIQUE_COUNTS if counts else 0)
    need = capi.query_u64("vrs_unique_scratch_bytes", n, KT[kt], flags)
    specs = [Spec("keys", n * width, "in", wrap_align(width), a), Spec("num_runs", 4, "out", 4), Spec("scratch", need, "scratch", 8),
             Spec("out_keys", n * width, "out", wrap_align(width), writable=[(0, R * width)])]
    expect, refuse = {"num_runs": np.uint32(R).tobytes(), "out_keys": as_bytes(a[first])}, {"scratch": 1, "num_runs": 1, "out_keys": width}
    if counts:
        specs.append(Spec("out_counts", n * 4, "out", 4, writable=[(0, R * 4)]))
        expect["out_counts"], refuse["out_counts"] = as_bytes(cnt.astype(np.uint32)), 4
    if inverse:
        specs.append(Spec("out_inverse", n * 4, "out", 4))
        expect["out_inverse"], refuse["out_inverse"] = as_bytes(inv.astype(np.uint32)), 4

    def call(c, h):
        return c.lib.vrs_unique(c.handle, h["keys"], n, KT[kt], h["out_keys"], h["out_counts"], h["out_inverse"], h["num_runs"], h["scratch"])

    return Case(specs, call, expect, refuse=refuse, misalign={"scratch": 4})


@pytest.mark.parametrize("outputs", ["keys-only", "inverse", "counts", "inverse-and-counts"])
@pytest.mark.parametrize("kt", list(KT))
def test_unique(ctx, dev, kt, outputs):
    run_case(ctx, dev, f"unique {kt} {outputs}", unique_case(ctx, kt, "inverse" in outputs, "counts" in outputs))


def test_unique_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "unique", unique_case(ctx, "f64", True, True))


# ---------------------------------------------------------------------------------------------- the one-call sorts

POOL_FLOOR = 1 << 22  # the floor of the counted and the pool form (tests/test_gpu_pool.py)
# entry point -> (key bytes, pairs); form -> (num_elements, VRS_TUNE_MSD_POOL): no length a multiple of 4, 64 or a tile; the capacity
# edge of the single launch and the edge + 1, the last contract size and the first look-back size, the floor + 3 of the two big forms
SORTS = {"keys_u32": (4, False), "pairs_u32": (4, True), "keys_u64": (8, False), "pairs_u64": (8, True)}
FORMS = {"single": (4096, 0), "contract-first": (4097, 0), "contract": (8191, 0), "lsd": (8193, 0), "counted": (POOL_FLOOR + 3, 0),
         "pool": (POOL_FLOOR + 3, 2)}
KERNELS = {name: kid for kid, name in capi.KERNEL_NAMES.items()}


def sort_form_for(lib, n, key_bytes, pairs, pool):
    knobs = (ctypes.c_int64 * 7)(-1, -1, POOL_FLOOR, POOL_FLOOR, -1, pool, -1)
    form = ctypes.c_int()
    assert lib.vrs_sort_form_for(n, key_bytes, int(pairs), knobs, 7, ctypes.byref(form), None) == capi.VRS_OK
    return capi.FORM_NAMES[form.value]


def sort_keys_for(n, key_bytes, seed):
    """keys with many ties (so that a pairs sort shows whether it is stable) whose top bits are uniform (so that the big forms take them)"""
    rs = np.random.RandomState(seed)
    k = rs.randint(0, 2 ** 32, size=n, dtype=np.uint32) & np.uint32(0xFFFF00FF)
    if key_bytes == 4:
        return k
    return (k.astype(np.uint64) << np.uint64(32)) | np.uint64(rs.randint(0, 4)) << np.uint64(7)


_sort_inputs = {}


def sort_input(n, key_bytes):
    """(keys, their stable order): made once per size and width, shared, never written"""
    if (n, key_bytes) not in _sort_inputs:
        keys = sort_keys_for(n, key_bytes, n % 1000)
        _sort_inputs[n, key_bytes] = (keys, np.argsort(keys, kind="stable"))
    return _sort_inputs[n, key_bytes]


def one_call_case(ctx, entry, form):
    key_bytes, pairs = SORTS[entry]
    n, pool = FORMS[form]
    tune(ctx, capi.VRS_TUNE_HYBRID_MIN_KEYS, POOL_FLOOR)
    tune(ctx, capi.VRS_TUNE_MSD_POOL_MIN_KEYS, POOL_FLOOR)
    tune(ctx, capi.VRS_TUNE_MSD_POOL, pool)
    keys, order = sort_input(n, key_bytes)
    specs = [Spec("keys", n * key_bytes, "inout", wrap_align(key_bytes), keys), Spec("keys_tmp", n * key_bytes, "scratch", wrap_align(key_bytes))]
    expect, refuse = {"keys": as_bytes(keys[order])}, {"keys": key_bytes, "keys_tmp": 1}
    if pairs:
        specs += [Spec("values", n * 4, "inout", 4, np.arange(n, dtype=np.uint32)), Spec("values_tmp", n * 4, "scratch", 4)]
        expect["values"] = as_bytes(order.astype(np.uint32))  # stable: equal keys keep their input order
        refuse.update(values=4, values_tmp=1)
    fn = getattr(ctx.lib, f"vrs_sort_{entry}")
    seen = {}

    def call(c, h):
        c.profileReset()
        c.profileEnable(True)
        try:
            args = (h["keys"], h["keys_tmp"], h["values"], h["values_tmp"]) if pairs else (h["keys"], h["keys_tmp"])
            rc = fn(c.handle, *args, n)
            if rc == capi.VRS_OK:
                rc = c.lib.vrs_sort_settle(c.handle)
            seen.update({name: c.profileQuery(kid)[0] for name, kid in KERNELS.items()})
        finally:
            c.profileEnable(False)
        return rc

    def counters(c):
        took, refused, hybrid = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        c.check(c.lib.vrs_one_call_pool_sorts(c.handle, ctypes.byref(took), ctypes.byref(refused)))
        c.check(c.lib.vrs_one_call_hybrid_sorts(c.handle, ctypes.byref(hybrid)))
        reused = ctypes.c_uint64()
        c.check(c.lib.vrs_one_call_pool_layouts(c.handle, ctypes.byref(reused), None))
        return took.value, hybrid.value, reused.value

    def ran(before, after):
        pool_sorts, hybrid_sorts = after[0] - before[0], after[1] - before[1]
        big = seen["local_sort"] + seen["pool_sample"] + seen["digit_tables"] + seen["lookback_scatter"]
        return {"single": seen["single"] == 1 and big == 0 and seen["scatter"] == 0,
                "contract": 1 <= seen["histogram"] == seen["scatter"] <= key_bytes and big == 0 and seen["single"] == 0,
                "lsd": seen["digit_tables"] >= 1 and seen["lookback_scatter"] >= 1 and seen["local_sort"] == 0 and pool_sorts == 0,
                "counted": seen["local_sort"] >= 1 and seen["pool_sample"] == 0 and pool_sorts == 0 and hybrid_sorts == 1,
                # (a pool sort of the size of the context's last one starts in that sort's regions and samples nothing: the second
                # seed's run takes that path, the first one samples)
                "pool": (seen["pool_sample"] >= 1 or after[2] - before[2] == 1) and seen["local_sort"] >= 1 and pool_sorts == 1}[form.split("-")[0]]

    return Case(specs, call, expect, counters, ran, refuse)


# the forms each entry point takes at these sizes: the single launch is for bare 32-bit keys, the pool form for 32-bit keys and their pairs
ONE_CALL_PARAMS = [(entry, form) for entry in SORTS for form in FORMS
                   if not (form == "single" and entry != "keys_u32") and not (form == "pool" and entry.endswith("u64"))]


@pytest.mark.parametrize("entry,form", ONE_CALL_PARAMS)
def test_one_call_sorts(ctx, dev, entry, form):
    run_case(ctx, dev, f"sort_{entry} {form}", one_call_case(ctx, entry, form))


def test_the_forms_every_one_call_sort_takes():
    """the cases above are exactly what vrs_sort_form_for says each entry point takes"""
    lib = capi.load_library()
    said = [(entry, form) for entry, (kb, pairs) in SORTS.items() for form, (n, pool) in FORMS.items()
            if sort_form_for(lib, n, kb, pairs, pool) == form.split("-")[0]]
    assert said == ONE_CALL_PARAMS


@pytest.mark.parametrize("entry", list(SORTS))
def test_one_call_sorts_refuse_short_buffers(ctx, dev, entry):
    run_refusals(ctx, dev, f"sort_{entry}", one_call_case(ctx, entry, "lsd"))


# ---------------------------------------------------------------------------------------------- the reference's stages and its single launch

N_STAGE = 3 * 8192 + 77  # B = 32: four workgroups, the last with a few blocks and a ragged end


def stage_case(ctx, pairs):
    n, B, shift = N_STAGE, 32, 8
    W = ctx.lib.vrs_workgroup_count(n, B)
    assert W == 4
    keys = np.random.RandomState(3).randint(0, 2 ** 32, size=n, dtype=np.uint32)
    order = np.argsort((keys >> np.uint32(shift)) & np.uint32(0xFF), kind="stable")
    pc = capi.PushConstants(n, shift, W, B)
    # the table: written by the histogram stage, read by the sort stage -- the call's own working memory between its two stages
    specs = [Spec("keys_in", 4 * n, "in", 4, keys), Spec("keys_out", 4 * n, "out", 4), Spec("histograms", W * 256 * 4, "scratch", 4)]
    expect, refuse = {"keys_out": as_bytes(keys[order])}, {"keys_out": 4, "histograms": 1}
    if pairs:
        specs += [Spec("values_in", 4 * n, "in", 4, np.arange(n, dtype=np.uint32)), Spec("values_out", 4 * n, "out", 4)]
        expect["values_out"], refuse["values_out"] = as_bytes(order.astype(np.uint32)), 4
    seen = {}

    def histograms(c, h):
        return c.lib.vrs_multi_radixsort_histograms(c.handle, h["keys_in"], h["histograms"], ctypes.byref(pc))

    def sort(c, h):
        if pairs:
            return c.lib.vrs_multi_radixsort_pairs(c.handle, h["keys_in"], h["keys_out"], h["values_in"], h["values_out"], h["histograms"], ctypes.byref(pc))
        return c.lib.vrs_multi_radixsort(c.handle, h["keys_in"], h["keys_out"], h["histograms"], ctypes.byref(pc))

    def call(c, h):
        c.profileReset()
        c.profileEnable(True)
        try:
            rc = histograms(c, h)
            rc = sort(c, h) if rc == capi.VRS_OK else rc
            seen.update({name: c.profileQuery(kid)[0] for name, kid in KERNELS.items()})
        finally:
            c.profileEnable(False)
        return rc

    # (the table is refused by the histogram stage already; the outputs by the sort stage, after the histogram stage has run)
    return Case(specs, call, expect, lambda c: 0, lambda before, after: seen["histogram"] == 1 and seen["scatter"] == 1, refuse,
                first=histograms, second=sort, late=tuple(k for k in refuse if k != "histograms"))


@pytest.mark.parametrize("pairs", [False, True], ids=["multi_radixsort", "multi_radixsort_pairs"])
def test_reference_stages(ctx, dev, pairs):
    case = stage_case(ctx, pairs)
    run_case(ctx, dev, "multi_radixsort" + ("_pairs" if pairs else ""), case)
    run_refusals(ctx, dev, "multi_radixsort" + ("_pairs" if pairs else ""), case)


def test_single_radixsort(ctx, dev):
    n = 4093
    keys = np.random.RandomState(4).randint(0, 2 ** 32, size=n, dtype=np.uint32)
    specs = [Spec("buffer0", 4 * n, "inout", 4, keys), Spec("buffer1", 4 * n, "scratch", 4)]
    seen = {}

    def call(c, h):
        c.profileReset()
        c.profileEnable(True)
        try:
            rc = c.lib.vrs_single_radixsort(c.handle, h["buffer0"], h["buffer1"], n)
            seen["single"] = c.profileQuery(capi.VRS_KERNEL_SINGLE)[0]
        finally:
            c.profileEnable(False)
        return rc

    case = Case(specs, call, {"buffer0": as_bytes(np.sort(keys))}, lambda c: 0, lambda before, after: seen["single"] == 1, {"buffer0": 4, "buffer1": 1})
    run_case(ctx, dev, "single_radixsort", case)
    run_refusals(ctx, dev, "single_radixsort", case)


# ---------------------------------------------------------------------------------------------- the segmented sorts

SEG_THR = 1 << 16  # VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS as the per-op tests set it: the one-call tier at a size a test can afford
SEGMENTED = {"u32": (4, False), "pairs_u32": (4, True), "u64": (8, False), "pairs_u64": (8, True)}


def segment_layout():
    """(n, offsets): all four tiers in one call.  The offsets first walk a high part of the buffer (a GLOBAL and a ONE_CALL segment), then
    drop to a low part (a WAVE segment, an empty one, one of one element, one at the wave tier's capacity and one past it): the drop itself clamps to an empty segment,
    and the elements between the two parts are a gap no segment covers.  The low part starts above 0, the high part ends below n."""
    low = np.cumsum([7, 77, 0, 1, capi.SEGMENT_WAVE_MAX, capi.SEGMENT_WAVE_MAX + 1])  # (32-bit keys: the wave tier's last length, the block tier's first)
    high = np.cumsum([low[-1] + 13, 14341, SEG_THR + 3])  # a gap of 13 elements
    return int(high[-1]) + 9, np.concatenate([high, low]).astype(np.uint32)


def segments_of(lib, offsets, n, key_bytes, pairs):
    """[(tier, clamped begin, clamped end)] by the library's own classification"""
    fn = lib.vrs_segment_tier_for if key_bytes == 4 else lib.vrs_segment_tier_for_u64
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    out = []
    for b, e in zip(offsets[:-1], offsets[1:]):
        assert fn(int(b), int(e), n, int(pairs), SEG_THR, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
        out.append((t.value, cb.value, ce.value))
    return out


def segmented_case(ctx, entry):
    key_bytes, pairs = SEGMENTED[entry]
    tune(ctx, capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, SEG_THR)
    n, offsets = segment_layout()
    S = offsets.size - 1
    segments = segments_of(ctx.lib, offsets, n, key_bytes, pairs)
    tiers = np.bincount([t for t, _, _ in segments], minlength=4)
    assert (tiers > 0).all() and any(e == b for _, b, e in segments) and any(e - b == 1 for _, b, e in segments)
    keys = sort_keys_for(n, key_bytes, 21)
    vals = np.arange(n, dtype=np.uint32)[::-1].copy()
    want_k, want_v = keys.copy(), vals.copy()
    for _, b, e in segments:
        order = np.argsort(keys[b:e], kind="stable")
        want_k[b:e], want_v[b:e] = keys[b:e][order], vals[b:e][order]
    spans = sorted((b, e) for _, b, e in segments if e > b)
    merged = []  # only the clamped segments are writable: not the gap, nothing before the first and nothing behind the last
    for b, e in spans:
        if merged and merged[-1][1] == b:
            merged[-1][1] = e
        else:
            merged.append([b, e])
    assert len(merged) == 2 and merged[0][0] > 0 and merged[1][1] < n and merged[0][1] < merged[1][0]

    def live(item, arr):
        return b"".join(arr[b:e].tobytes() for b, e in merged), [(b * item, e * item) for b, e in merged]

    kbytes, kspans = live(key_bytes, want_k)
    specs = [Spec("keys", n * key_bytes, "inout", wrap_align(key_bytes), keys, kspans), Spec("keys_tmp", n * key_bytes, "scratch", wrap_align(key_bytes)),
             Spec("offsets", 4 * (S + 1), "in", 4, offsets)]
    expect, refuse = {"keys": kbytes}, {"keys": key_bytes, "keys_tmp": 1}
    if pairs:
        vbytes, vspans = live(4, want_v)
        specs += [Spec("values", 4 * n, "inout", 4, vals, vspans), Spec("values_tmp", 4 * n, "scratch", 4)]
        expect["values"] = vbytes
        refuse.update(values=4, values_tmp=1)
    fn = getattr(ctx.lib, f"vrs_sort_segments_{entry}")

    def call(c, h):
        if pairs:
            return fn(c.handle, h["keys"], h["keys_tmp"], h["values"], h["values_tmp"], n, h["offsets"], S)
        return fn(c.handle, h["keys"], h["keys_tmp"], n, h["offsets"], S)

    def ran(before, after):
        return [after[k] - before[k] for k in ("wave", "block", "global", "one_call")] == list(tiers)

    return Case(specs, call, expect, vrs.segmented_stats, ran, refuse)


@pytest.mark.parametrize("entry", list(SEGMENTED))
def test_sort_segments(ctx, dev, entry):
    run_case(ctx, dev, f"sort_segments_{entry}", segmented_case(ctx, entry))


@pytest.mark.parametrize("entry", list(SEGMENTED))
def test_sort_segments_refuse_short_buffers(ctx, dev, entry):
    run_refusals(ctx, dev, f"sort_segments_{entry}", segmented_case(ctx, entry))


# ---------------------------------------------------------------------------------------------- vrs_sort_rank_keys, vrs_sort_restore

# dtype code -> (storage, bits, float?, signed?, the bits of +inf)
RANK_DTYPES = {capi.VRS_SORT_INT8: (np.uint8, 8, False, True, 0), capi.VRS_SORT_UINT8: (np.uint8, 8, False, False, 0),
               capi.VRS_SORT_INT16: (np.uint16, 16, False, True, 0), capi.VRS_SORT_INT32: (np.uint32, 32, False, True, 0),
               capi.VRS_SORT_INT64: (np.uint64, 64, False, True, 0), capi.VRS_SORT_FLOAT16: (np.uint16, 16, True, False, 0x7C00),
               capi.VRS_SORT_BFLOAT16: (np.uint16, 16, True, False, 0x7F80), capi.VRS_SORT_FLOAT32: (np.uint32, 32, True, False, 0x7F800000),
               capi.VRS_SORT_FLOAT64: (np.uint64, 64, True, False, 0x7FF0000000000000)}
RANK_NAMES = {0: "int8", 1: "uint8", 2: "int16", 3: "int32", 4: "int64", 5: "float16", 6: "bfloat16", 7: "float32", 8: "float64"}
ROW_LEN, ROWS = 1031, 3  # an odd row, three of them: more than one tile of either kernel, no multiple of anything


def rank_of(u, dtype, descending):
    """the header's r in numpy: unsigned as is, signed with the sign bit flipped, floats by the total order with -0.0 at +0.0's rank and
    every NaN at the largest rank of its width; zero-extended to the rank's width; descending: the complement over that width"""
    storage, B, is_float, signed, inf = RANK_DTYPES[dtype]
    R = np.uint64 if B == 64 else np.uint32
    u = u.astype(R)
    sign = R(1 << (B - 1))
    ones = R((1 << B) - 1)
    if is_float:
        mag = u & (sign - R(1))
        r = np.where(mag > R(inf), ones, np.where(mag == 0, sign, np.where(u & sign != 0, ~u & ones, u | sign)))
    else:
        r = u ^ sign if signed else u
    return (~r if descending else r).astype(R)


def rank_input(dtype):
    storage, B, is_float, _, inf = RANK_DTYPES[dtype]
    rng = np.random.default_rng(B + dtype)
    u = rng.integers(0, 1 << 63, ROWS * ROW_LEN, dtype=np.uint64).astype(storage) if B < 64 else rng.integers(0, 1 << 63, ROWS * ROW_LEN, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if is_float:  # both zeros, both infinities, NaNs of both signs and several payloads, in every row
        top = 1 << (B - 1)
        special = np.array([0, top, inf, inf | top, inf | 1, inf | top | 1, (top - 1), (2 * top - 1)], dtype=np.uint64).astype(storage)
        u[rng.integers(0, u.size, 200)] = special[rng.integers(0, special.size, 200)]
        u[:special.size] = special
    return u


def rank_case(ctx, dtype, descending, positions):
    storage, B, *_ = RANK_DTYPES[dtype]
    n, eb, rb = ROWS * ROW_LEN, B // 8, 8 if B == 64 else 4
    u = rank_input(dtype)
    want = rank_of(u, dtype, descending)
    specs = [Spec("src", n * eb, "in", wrap_align(eb), u), Spec("out_ranks", n * rb, "out", wrap_align(rb))]
    expect, refuse = {"out_ranks": as_bytes(want)}, {"out_ranks": rb}
    if positions:
        specs.append(Spec("out_positions", 4 * n, "out", 4))
        expect["out_positions"], refuse["out_positions"] = as_bytes((np.arange(n) % ROW_LEN).astype(np.uint32)), 4

    def call(c, h):
        return c.lib.vrs_sort_rank_keys(c.handle, h["src"], n, ROW_LEN, dtype, capi.VRS_SORT_DESCENDING if descending else 0, h["out_ranks"], h["out_positions"])

    return Case(specs, call, expect, refuse=refuse)


def restore_case(ctx, dtype, descending, with_positions):
    """the ranks and positions as the stable sort of every row leaves them; out_values and out_indices from them.  Without positions (an
    integer dtype only) the values alone."""
    storage, B, is_float, *_ = RANK_DTYPES[dtype]
    n, eb, rb = ROWS * ROW_LEN, B // 8, 8 if B == 64 else 4
    u = rank_input(dtype)
    r = rank_of(u, dtype, descending).reshape(ROWS, ROW_LEN)
    order = np.argsort(r, axis=1, kind="stable")
    ranks = np.take_along_axis(r, order, axis=1).reshape(-1)
    values = np.take_along_axis(u.reshape(ROWS, ROW_LEN), order, axis=1).reshape(-1)
    specs = [Spec("src", n * eb, "in", wrap_align(eb), u), Spec("ranks", n * rb, "in", wrap_align(rb), ranks),
             Spec("out_values", n * eb, "out", wrap_align(eb))]
    expect, refuse = {"out_values": as_bytes(values)}, {"out_values": eb}
    if with_positions:
        specs += [Spec("positions", 4 * n, "in", 4, order.reshape(-1).astype(np.uint32)), Spec("out_indices", 8 * n, "out", 8)]
        expect["out_indices"], refuse["out_indices"] = as_bytes(order.reshape(-1).astype(np.int64)), 8
    else:
        assert not is_float

    def call(c, h):
        return c.lib.vrs_sort_restore(c.handle, h["src"], h["ranks"], h["positions"], n, ROW_LEN, dtype, capi.VRS_SORT_DESCENDING if descending else 0,
                                      h["out_values"], h["out_indices"])

    return Case(specs, call, expect, refuse=refuse)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("dtype", list(RANK_DTYPES), ids=lambda d: RANK_NAMES[d])
def test_sort_rank_keys(ctx, dev, dtype, descending):
    run_case(ctx, dev, f"sort_rank_keys {RANK_NAMES[dtype]}", rank_case(ctx, dtype, descending, positions=True))
    if not descending:
        run_case(ctx, dev, f"sort_rank_keys {RANK_NAMES[dtype]}, no positions", rank_case(ctx, dtype, descending, positions=False))


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("dtype", list(RANK_DTYPES), ids=lambda d: RANK_NAMES[d])
def test_sort_restore(ctx, dev, dtype, descending):
    run_case(ctx, dev, f"sort_restore {RANK_NAMES[dtype]}", restore_case(ctx, dtype, descending, with_positions=True))
    if not RANK_DTYPES[dtype][2] and descending:
        run_case(ctx, dev, f"sort_restore {RANK_NAMES[dtype]}, no positions", restore_case(ctx, dtype, descending, with_positions=False))


def test_sort_rank_and_restore_refuse_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "sort_rank_keys", rank_case(ctx, capi.VRS_SORT_FLOAT16, True, positions=True))
    run_refusals(ctx, dev, "sort_rank_keys, 64-bit ranks", rank_case(ctx, capi.VRS_SORT_FLOAT64, False, positions=True))
    run_refusals(ctx, dev, "sort_restore", restore_case(ctx, capi.VRS_SORT_BFLOAT16, False, with_positions=True))


# ---------------------------------------------------------------------------------------------- vrs_topk_segments

TOPK_GRID = 20000  # VRS_TUNE_TOPK_GRID_MIN_KEYS as tests/test_gpu_topk.py sets it
# lengths of the segments (the first offset is 3, five elements follow the last), k, key type, largest, sorted, with indices.
# Every case has a segment shorter than k, whose slots from its length on take 0xFFFFFFFF.
TOPK_CASES = {
    "lds-sorted": ([5, 300, capi.TOPK_LDS_MAX], 500, "f32", True, True, True),
    "block-sorted-no-indices": ([capi.TOPK_LDS_MAX + 1, 9001, 70], 77, "i32", False, True, False),
    "grid-sorted": ([TOPK_GRID, TOPK_GRID + 3, 100], 300, "u32", False, True, True),
    "all-tiers-unsorted": ([100, 9001, TOPK_GRID + 3], 200, "f32", False, False, True),
    "all-tiers-unsorted-no-indices": ([100, 9001, TOPK_GRID + 3], 200, "u32", True, False, False),
    "inner-segmented-sort-of-pairs": ([TOPK_GRID + 3, 5000, 4100, 7], capi.TOPK_SORT_IN_LDS_MAX_K + 3, "i32", True, True, True),
    "inner-segmented-sort-of-keys": ([TOPK_GRID + 3, 5000, 4100, 7], capi.TOPK_SORT_IN_LDS_MAX_K + 3, "f32", False, True, False),
}


def ragged(lengths, lead=3, tail=5):
    offsets = np.concatenate([[lead], lead + np.cumsum(lengths)]).astype(np.uint32)
    return int(offsets[-1]) + tail, offsets


def topk_case(ctx, key):
    from .test_gpu_topk import KT as TOPK_KT
    from .test_gpu_topk import rank as topk_rank
    from .test_gpu_topk import reference as topk_reference

    lengths, k, kt, largest, in_order, indices = TOPK_CASES[key]
    tune(ctx, capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, TOPK_GRID)
    n, offsets = ragged(lengths)
    S = len(lengths)
    rs = np.random.RandomState(k)
    keys = rs.randint(0, 2 ** 32, size=n, dtype=np.uint32) & np.uint32(0xFFF000FF)  # many ties: the lowest index wins
    if kt == "f32":
        keys[rs.randint(0, n, 50)] = np.array([0x7FC00000, 0xFFC00001, 0x80000000, 0, 0x7F800000], np.uint32)[rs.randint(0, 5, 50)]
    want_k, want_i = topk_reference(keys, offsets, k, kt, largest)
    assert (want_k.reshape(S, k)[:, -1] == 0xFFFFFFFF).any() and (want_i == 0xFFFFFFFF).any()
    flags = (capi.VRS_TOPK_LARGEST if largest else 0) | (capi.VRS_TOPK_SORTED if in_order else 0)
    need = capi.query_u64("vrs_topk_scratch_bytes", n, S, k, flags)
    specs = [Spec("keys", 4 * n, "in", 4, keys), Spec("offsets", 4 * (S + 1), "in", 4, offsets), Spec("out_keys", 4 * S * k, "out", 4),
             Spec("scratch", need, "scratch", 8)]
    expect, refuse = {"out_keys": as_bytes(want_k)}, {"out_keys": 4, "scratch": 1}
    if indices:
        specs.append(Spec("out_indices", 4 * S * k, "out", 4))
        expect["out_indices"], refuse["out_indices"] = as_bytes(want_i), 4
    tiers = {"lds": 0, "block": 0, "grid": 0}
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    for b, e in zip(offsets[:-1], offsets[1:]):
        assert ctx.lib.vrs_topk_tier_for(int(b), int(e), n, TOPK_GRID, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
        tiers[("lds", "block", "grid")[t.value]] += 1

    def call(c, h):
        return c.lib.vrs_topk_segments(c.handle, h["keys"], n, h["offsets"], S, k, TOPK_KT[kt], flags, h["out_keys"], h["out_indices"], h["scratch"])

    def canon(got):
        """without VRS_TOPK_SORTED a segment's m entries come in some order: ordered here by (rank, index) -- with the indices that is
        the stable order itself, without them the order of the ranks (equal ranks are equal bits)"""
        if in_order:
            return got
        ok = np.frombuffer(got["out_keys"], np.uint32).reshape(S, k).copy()
        oi = np.frombuffer(got["out_indices"], np.uint32).reshape(S, k).copy() if indices else None
        for s in range(S):
            m = min(k, lengths[s])
            r = topk_rank(ok[s, :m], kt, largest).astype(np.uint64) << np.uint64(32)
            o = np.argsort(r | oi[s, :m] if indices else r, kind="stable")
            ok[s, :m] = ok[s, :m][o]
            if indices:
                oi[s, :m] = oi[s, :m][o]
        return {"out_keys": ok.tobytes(), **({"out_indices": oi.tobytes()} if indices else {})}

    return Case(specs, call, expect, vrs.topk_stats, lambda before, after: {t_: after[t_] - before[t_] for t_ in tiers} == tiers, refuse,
                misalign={"scratch": 4}, canon=canon)


@pytest.mark.parametrize("key", list(TOPK_CASES))
def test_topk_segments(ctx, dev, key):
    run_case(ctx, dev, f"topk_segments {key}", topk_case(ctx, key))


def test_topk_segments_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "topk_segments", topk_case(ctx, "grid-sorted"))


# ---------------------------------------------------------------------------------------------- vrs_select_segments, vrs_quantile_segments

SELECT_GRID = 8193  # VRS_TUNE_SELECT_GRID_MIN_KEYS of the per-op tests' grid cases
# segment lengths, dtype, (mode, k, descending), with indices, grid threshold (0: never), compaction divisor (0: never), the tiers
SELECT_CASES = {
    "lds-int8": ([5, 0, 1, 4099], "int8", ("kth", 3, False), True, 0, 0, (4, 0, 0)),
    "lds-float32-at-capacity": ([8192, 2], "float32", ("nanmedian", 0, True), True, SELECT_GRID, 0, (2, 0, 0)),
    "block-float16": ([9001, 70], "float16", ("median", 0, True), False, 0, 0, (1, 1, 0)),
    "block-int64-past-capacity": ([4097, 4096], "int64", ("kth", 4000, False), True, 0, 0, (1, 1, 0)),
    "grid-int32": ([8193, 12001, 100], "int32", ("kth", 77, True), True, SELECT_GRID, 0, (1, 0, 2)),
    "grid-bfloat16": ([16385, 3], "bfloat16", ("nanmedian", 0, False), False, SELECT_GRID, 0, (1, 0, 1)),
    "grid-compacting-float64": ([40003, 9001], "float64", ("kth", 20000, False), True, SELECT_GRID, 16, (0, 0, 2)),
}


def select_case(ctx, key):
    from . import test_gpu_select as sel

    lengths, name, (mode, k, descending), indices, grid_min, divisor, tiers = SELECT_CASES[key]
    dtype = getattr(torch, name)
    tune(ctx, capi.VRS_TUNE_SELECT_GRID_MIN_KEYS, grid_min)
    tune(ctx, capi.VRS_TUNE_SELECT_COMPACT_DIVISOR, divisor)
    n, offsets = ragged(lengths)
    S, code, eb = len(lengths), sel.CODES[dtype], torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g, dtype=torch.float64) if divisor else sel.make(dtype, (1, n), g).reshape(-1)
    mode_code = {"kth": capi.VRS_SELECT_KTH, "median": capi.VRS_SELECT_MEDIAN, "nanmedian": capi.VRS_SELECT_NANMEDIAN}[mode]
    vals, idx = sel.Oracle(x, [int(o) for o in offsets]).answer(mode_code, k, descending)
    assert tuple(sel.predicted_tiers([int(o) for o in offsets], n, code, grid_min).values()) == tiers
    need = capi.query_u64("vrs_select_scratch_bytes", n, S, code)
    specs = [Spec("src", n * eb, "in", wrap_align(eb), x), Spec("offsets", 4 * (S + 1), "in", 4, offsets),
             Spec("out_values", S * eb, "out", wrap_align(eb)), Spec("scratch", need, "scratch", 8)]
    expect, refuse = {"out_values": as_bytes(vals)}, {"out_values": eb, "scratch": 1}
    if indices:
        specs.append(Spec("out_indices", 4 * S, "out", 4))
        expect["out_indices"], refuse["out_indices"] = as_bytes(idx.numpy().astype(np.uint32)), 4

    def call(c, h):
        return c.lib.vrs_select_segments(c.handle, h["src"], n, h["offsets"], S, code, mode_code, k, capi.VRS_SELECT_DESCENDING if descending else 0,
                                         h["out_values"], h["out_indices"], h["scratch"])

    def ran(before, after):
        d = {t: after[t] - before[t] for t in after}
        return (d["lds"], d["block"], d["grid"]) == tiers and (d["compacted"] > 0) == (divisor > 0)

    return Case(specs, call, expect, vrs.select_stats, ran, refuse, misalign={"scratch": 4})


@pytest.mark.parametrize("key", list(SELECT_CASES))
def test_select_segments(ctx, dev, key):
    run_case(ctx, dev, f"select_segments {key}", select_case(ctx, key))


def test_select_segments_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "select_segments", select_case(ctx, "grid-int32"))


# segment lengths, dtype, qs, interpolation, ignore NaNs, grid threshold, divisor, the tiers, whether the grid segments sieve
QUANTILE_CASES = {
    "lds-float32": ([7, 0, 1, 1001], "float32", [0.0, 0.37, 1.0], "linear", True, 0, 0, (4, 0, 0), False),
    "block-float64": ([4097, 333], "float64", [0.5, 0.9], "midpoint", False, 0, 0, (1, 1, 0), False),
    "grid-float32": ([8193, 9001, 5], "float32", [0.1, 0.5, 0.75], "nearest", True, SELECT_GRID, 0, (1, 0, 2), False),
    "grid-sieve-float64": ([20003, 8193], "float64", [0.25, 0.5], "linear", False, SELECT_GRID, 16, (0, 0, 2), True),
    "grid-sieve-float32": ([40003], "float32", [0.999], "lower", True, SELECT_GRID, 16, (0, 0, 1), True),
}
QUANTILE_OUTPUTS = ("out_values", "out_lower", "out_upper", "out_weight")


def quantile_case(ctx, key, only_values):
    from vkradixsort_amd.quantile import INTERPOLATIONS as INTERPOLATION_CODES

    from . import test_gpu_quantile as qt

    lengths, name, qs, interpolation, ignore_nan, grid_min, divisor, tiers, sieves = QUANTILE_CASES[key]
    dtype = getattr(torch, name)
    tune(ctx, capi.VRS_TUNE_SELECT_GRID_MIN_KEYS, grid_min)
    tune(ctx, capi.VRS_TUNE_SELECT_COMPACT_DIVISOR, divisor)
    n, offsets = ragged(lengths)
    S, Q, code, eb = len(lengths), len(qs), qt.CODES[dtype], 4 if dtype == torch.float32 else 8
    g = torch.Generator().manual_seed(n)
    x = (qt.uniform_bits(dtype, (1, n), g) if sieves else qt.make(dtype, (1, n), g, nans=not sieves)).reshape(-1).contiguous()
    want = qt.host(x, [int(o) for o in offsets], qs, interpolation, ignore_nan)
    assert tuple(qt.predicted_tiers([int(o) for o in offsets], n, code, grid_min).values()) == tiers
    need = capi.query_u64("vrs_quantile_scratch_bytes", n, S, code)
    specs = [Spec("src", n * eb, "in", wrap_align(eb), x), Spec("offsets", 4 * (S + 1), "in", 4, offsets), Spec("scratch", need, "scratch", 8)]
    expect, refuse = {}, {"scratch": 1}
    for out, w in list(zip(QUANTILE_OUTPUTS, want))[:1 if only_values else 4]:
        specs.append(Spec(out, S * Q * eb, "out", wrap_align(eb)))
        expect[out], refuse[out] = as_bytes(w), eb
    q = (ctypes.c_double * Q)(*qs)
    flags = capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0

    def call(c, h):
        return c.lib.vrs_quantile_segments(c.handle, h["src"], n, h["offsets"], S, code, q, Q, INTERPOLATION_CODES[interpolation], flags,
                                           h["out_values"], h["out_lower"], h["out_upper"], h["out_weight"], h["scratch"])

    def ran(before, after):
        d = {t: after[t] - before[t] for t in after}
        return (d["lds"], d["block"], d["grid"]) == tiers and d["sieved"] == (tiers[2] if sieves else 0)

    return Case(specs, call, expect, vrs.quantile_stats, ran, refuse, misalign={"scratch": 4})


@pytest.mark.parametrize("only_values", [False, True], ids=["all-four-outputs", "values-only"])
@pytest.mark.parametrize("key", list(QUANTILE_CASES))
def test_quantile_segments(ctx, dev, key, only_values):
    run_case(ctx, dev, f"quantile_segments {key}", quantile_case(ctx, key, only_values))


def test_quantile_segments_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "quantile_segments", quantile_case(ctx, "grid-sieve-float64", False))


# ---------------------------------------------------------------------------------------------- vrs_search_sorted

SEARCH_KEYS = (capi.VRS_TUNE_SEARCH_LDS_BYTES, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES)
# forced tier (tests/test_gpu_searchsorted.py: FORCE), dtype, boundary rows x row length, query rows x row length, sorter, int64 out, right
SEARCH_CASES = {
    "lds-float32": ("lds", "float32", (1, 1001), (1, 5003), False, False, False),
    "lds-rows-int16-int64": ("lds", "int16", (3, 67), (3, 101), False, True, True),
    "table-int16-int64": ("table", "int16", (1, 4001), (1, 5003), False, True, True),
    "table-uint8": ("table", "uint8", (1, 77), (1, 4099), False, False, False),
    "direct-float64": ("direct", "float64", (1, 4099), (1, 301), False, False, True),
    "direct-sorter-int32-int64": ("direct", "int32", (1, 4099), (1, 301), True, True, False),
    "indexed-int32-int64": ("indexed", "int32", (1, 4099), (1, 5003), False, True, False),
    "indexed-float64": ("indexed", "float64", (1, 4099), (1, 5003), False, False, True),
    "indexed-sorter-bfloat16": ("indexed", "bfloat16", (1, 8197), (1, 5003), True, False, False),
}


def force_search(ctx, tier):
    from .test_gpu_searchsorted import DEFAULTS as SEARCH_DEFAULTS
    from .test_gpu_searchsorted import FORCE

    for key in SEARCH_KEYS:
        tune(ctx, key, FORCE[tier].get(key, SEARCH_DEFAULTS[key]))


def search_case(ctx, key, member=None):
    """member: None for the counting form, else whether the membership bytes are inverted"""
    from .test_gpu_searchsorted import sorted_seq, values

    tier, name, (b_rows, m), (q_rows, q_len), with_sorter, out64, right = SEARCH_CASES[key]
    force_search(ctx, tier)
    dtype = getattr(torch, name)
    code, eb = CODES[dtype], torch.empty(0, dtype=dtype).element_size()
    rng = np.random.default_rng(m + q_len)
    seq = torch.stack([sorted_seq(name, m, rng) for _ in range(b_rows)])
    x = torch.stack([values(name, q_len, rng, nan=True) for _ in range(q_rows)])
    nb, nq = b_rows * m, q_rows * q_len
    sorter = None
    if with_sorter:  # the boundaries lie shuffled; sorter[j] says where the j-th smallest is
        perm = torch.from_numpy(rng.permutation(m))
        shuffled = torch.empty_like(seq)
        shuffled[0, perm] = seq[0]
        sorter, stored = perm.to(torch.int64), shuffled
    else:
        stored = seq
    wide = seq.float() if eb == 2 else seq  # (float16 and bfloat16 widen exactly)
    xw = x.float() if eb == 2 else x
    if member is None:
        want = torch.searchsorted(wide, xw, right=right)
        want = want if out64 else want.to(torch.int32)
        flags = (capi.VRS_SEARCH_RIGHT if right else 0) | (capi.VRS_SEARCH_OUT_INT64 if out64 else 0)
        ob = 8 if out64 else 4
    else:
        want = torch.stack([torch.isin(xw[r], wide[r if b_rows > 1 else 0]) for r in range(q_rows)])
        want = (want ^ member).to(torch.uint8)
        flags = capi.VRS_SEARCH_MEMBER | (capi.VRS_SEARCH_MEMBER_INVERT if member else 0)
        ob = 1
    plan_tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(ctx.lib.vrs_search_plan(ctx.handle, nb, m, nq, q_len, code, int(with_sorter), ctypes.byref(plan_tier), ctypes.byref(need)))
    assert plan_tier.value == ("lds", "table", "direct", "indexed").index(tier)
    assert (need.value > 0) == (tier in ("table", "indexed"))
    specs = [Spec("boundaries", nb * eb, "in", wrap_align(eb), stored), Spec("queries", nq * eb, "in", wrap_align(eb), x),
             Spec("out", nq * ob, "out", wrap_align(ob))]
    expect, refuse = {"out": as_bytes(want)}, {"out": ob}
    if with_sorter:
        specs.append(Spec("sorter", 8 * nb, "in", 8, sorter))
    if need.value:
        specs.append(Spec("scratch", need.value, "scratch", 8 if eb == 8 else 4))
        refuse["scratch"] = 1

    def call(c, h):
        return c.lib.vrs_search_sorted(c.handle, h["boundaries"], nb, m, h["queries"], nq, q_len, code, flags, h["sorter"], h["out"], h["scratch"])

    return Case(specs, call, expect, vrs.search_stats, delta({tier}), refuse)


@pytest.mark.parametrize("key", list(SEARCH_CASES))
def test_search_sorted_counting(ctx, dev, key):
    run_case(ctx, dev, f"search_sorted {key}", search_case(ctx, key))


@pytest.mark.parametrize("key", ["lds-float32", "lds-rows-int16-int64", "table-int16-int64", "direct-float64", "direct-sorter-int32-int64",
                                 "indexed-float64", "indexed-sorter-bfloat16"])
def test_search_sorted_membership(ctx, dev, key):
    """the existing canaries sit around `out` only: here the scratch, the boundaries, the queries and the sorter are under guard too"""
    run_case(ctx, dev, f"search_sorted membership {key}", search_case(ctx, key, member=key.startswith("direct")))


@pytest.mark.parametrize("out64", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("name", ["int32", "int64"])
def test_search_sorted_identity_queries(ctx, dev, name, out64):
    """queries == NULL: run-length decode by one merge pass, no tier and no scratch"""
    rng = np.random.default_rng(3)
    m, rows = 4099, 2
    counts = rng.integers(0, 6, (rows, m))
    ends = np.cumsum(counts, axis=1)
    q_len = int(ends[:, -1].min()) + 3  # (a few outputs past the shorter row's last run: they answer m)
    dtype = np.int32 if name == "int32" else np.int64
    ob = 8 if out64 else 4
    want = np.stack([np.searchsorted(ends[r], np.arange(q_len), side="right") for r in range(rows)])
    flags = capi.VRS_SEARCH_RIGHT | (capi.VRS_SEARCH_OUT_INT64 if out64 else 0)
    eb = np.dtype(dtype).itemsize
    specs = [Spec("boundaries", rows * m * eb, "in", wrap_align(eb), ends.astype(dtype)), Spec("out", rows * q_len * ob, "out", wrap_align(ob))]
    code = CODES[getattr(torch, name)]

    def call(c, h):
        return c.lib.vrs_search_sorted(c.handle, h["boundaries"], rows * m, m, None, rows * q_len, q_len, code, flags, None, h["out"], None)

    case = Case(specs, call, {"out": as_bytes(want.astype(np.int64 if out64 else np.int32))}, vrs.search_stats, delta(set()), {"out": ob})
    run_case(ctx, dev, f"search_sorted identity {name}", case)
    run_refusals(ctx, dev, f"search_sorted identity {name}", case)


def test_search_sorted_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "search_sorted, the index", search_case(ctx, "indexed-sorter-bfloat16"))
    run_refusals(ctx, dev, "search_sorted, the table", search_case(ctx, "table-int16-int64"))
    run_refusals(ctx, dev, "search_sorted membership", search_case(ctx, "indexed-float64", member=False))


# ---------------------------------------------------------------------------------------------- vrs_bin_count

# tier, values dtype, mode, num_bins, weight dtype, out dtype, with skipped
I8, U8, I16, I32, I64, F16, BF16, F32, F64 = range(9)
NO_W = capi.VRS_BIN_NO_WEIGHTS
BINCOUNT_CASES = {
    "lds-index-int64-counts": ("lds", I32, capi.VRS_BIN_INDEX, 1000, NO_W, I64, True),
    "global-index-int64-counts": ("global", I16, capi.VRS_BIN_INDEX, 1000, NO_W, I64, False),
    "lds-index-float32-counts": ("lds", U8, capi.VRS_BIN_INDEX, 200, NO_W, F32, True),
    "global-index-float16-counts": ("global", I64, capi.VRS_BIN_INDEX, 77, NO_W, F16, False),
    "lds-index-float32-weights": ("lds", I32, capi.VRS_BIN_INDEX, 333, F32, F32, False),
    "global-index-float64-weights": ("global", I8, capi.VRS_BIN_INDEX, 100, F64, F64, True),
    "lds-linear-int64-counts": ("lds", F32, capi.VRS_BIN_LINEAR, 101, NO_W, I64, True),
    "global-linear-float64-weights": ("global", F64, capi.VRS_BIN_LINEAR, 101, F64, F64, True),
    "lds-linear-bfloat16-float32-weights": ("lds", BF16, capi.VRS_BIN_LINEAR, 50, F32, F32, False),
}
N_BINCOUNT = 20011  # more than one tile of every element width, a ragged end


def bincount_case(ctx, key):
    from .test_bincount_cpu import host_bins, to_bits

    tier, dtype, mode, num_bins, wd, od, with_skipped = BINCOUNT_CASES[key]
    tune(ctx, capi.VRS_TUNE_BINCOUNT_LDS_BYTES, capi.BINCOUNT_LDS_BYTES_DEFAULT if tier == "lds" else 0)
    n = N_BINCOUNT
    rng = np.random.default_rng(num_bins)
    lo, hi = (0.0, 0.0) if mode == capi.VRS_BIN_INDEX else (-2.5, 3.0)
    if mode == capi.VRS_BIN_INDEX:
        storage = {I8: np.int8, U8: np.uint8, I16: np.int16, I32: np.int32, I64: np.int64}[dtype]
        info = np.iinfo(storage)
        raw = rng.integers(max(info.min, -num_bins // 8), min(info.max, num_bins + num_bins // 8), n, endpoint=True).astype(storage)
        bins = np.where((raw >= 0) & (raw < num_bins), raw.astype(np.int64), -1)
        below, beyond = int((raw < 0).sum()), int((raw.astype(np.int64) >= num_bins).sum())
    else:
        x = (rng.standard_normal(n) * 2).astype(np.float32)
        x[rng.integers(0, n, 20)] = np.array([np.nan, lo, hi, np.inf, -np.inf], np.float32)[rng.integers(0, 5, 20)]
        raw = x.astype(np.float64) if dtype == F64 else x if dtype == F32 else to_bits(x, dtype)
        bins = host_bins(ctx.lib, raw, dtype, lo, hi, num_bins)
        wide = raw if dtype in (F32, F64) else (raw.astype(np.uint32) << 16).view(np.float32)
        below, beyond = int((wide < lo).sum()), int((wide > hi).sum())
    assert beyond > 0 and (below > 0 or dtype == U8) and (bins >= 0).sum() > n // 2
    ok = bins >= 0
    out_np = {I64: np.int64, F16: np.float16, F32: np.float32, F64: np.float64}[od]
    if wd == NO_W:
        weights = None
        want = np.bincount(bins[ok], minlength=num_bins).astype(out_np)  # (counts below 2^11: exact in float16 too)
    else:  # integer-valued weights whose partial sums stay below 2^24: every order of the float atomics gives the same bits
        weights = rng.integers(-8, 9, n).astype(np.float32 if wd == F32 else np.float64)
        want = np.bincount(bins[ok], weights=weights[ok], minlength=num_bins).astype(out_np)
        assert np.abs(weights).sum() < 2 ** 24
    plan_tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(ctx.lib.vrs_bin_count_plan(ctx.handle, num_bins, wd, od, ctypes.byref(plan_tier), ctypes.byref(need)))
    assert plan_tier.value == ("lds", "global").index(tier)
    eb, ob = raw.itemsize, np.dtype(out_np).itemsize
    specs = [Spec("values", n * eb, "in", wrap_align(eb), raw), Spec("out", num_bins * ob, "out", wrap_align(ob)),
             Spec("scratch", need.value, "scratch", 4)]
    expect, refuse = {"out": as_bytes(want)}, {"out": ob, "scratch": 1}
    if weights is not None:
        specs.append(Spec("weights", n * weights.itemsize, "in", wrap_align(weights.itemsize), weights))
    if with_skipped:
        specs.append(Spec("skipped", 16, "out", 8))
        expect["skipped"], refuse["skipped"] = as_bytes(np.array([below, beyond], np.uint64)), 8

    def call(c, h):
        return c.lib.vrs_bin_count(c.handle, h["values"], n, dtype, mode, lo, hi, num_bins, h["weights"], wd, od, h["out"], h["skipped"], h["scratch"])

    return Case(specs, call, expect, vrs.bincount_stats, delta({tier}), refuse)


@pytest.mark.parametrize("key", list(BINCOUNT_CASES))
def test_bin_count(ctx, dev, key):
    run_case(ctx, dev, f"bin_count {key}", bincount_case(ctx, key))


def test_bin_count_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "bin_count, counters in the scratch", bincount_case(ctx, "lds-index-float32-counts"))
    run_refusals(ctx, dev, "bin_count, weighted", bincount_case(ctx, "global-linear-float64-weights"))


# ---------------------------------------------------------------------------------------------- vrs_segment_reduce

REDUCE_CH = 64  # VRS_TUNE_REDUCE_CHUNK_ROWS: two levels from 65 rows on, three from 4097
# segment lengths, row width, dtype, op, with order, with init, out == init, the map of the first level's chunks, the most levels
REDUCE_CASES = {
    "lane-float32-sum": ([5, 0, 16, 1], 3, "F32", "SUM", False, False, False, "lane", 1),
    "rows-int32-sum-order": ([17, 64, 30], 3, "I32", "SUM", True, False, False, "rows", 1),
    "columns-float16-max-init": ([10, 3, 0], 65, "F16", "MAX", False, True, False, "columns", 1),
    "rows-two-levels-float64-order-init": ([200, 4096, 7], 5, "F64", "SUM", True, True, False, "rows", 2),
    "columns-two-levels-bfloat16": ([65, 130], 64, "BF16", "SUM", False, False, False, "columns", 2),
    "rows-three-levels-int64-prod": ([4097, 3], 2, "I64", "PROD", False, False, False, "rows", 3),
    "rows-three-levels-float32-out-is-init": ([4097, 66, 0], 1, "F32", "SUM", True, True, True, "rows", 3),
}


def reduce_case(ctx, key):
    from . import test_segreduce_cpu as sr

    lengths, C, dname, opname, with_order, with_init, out_is_init, first_map, levels = REDUCE_CASES[key]
    dtype, op = getattr(sr, dname), getattr(sr, opname)
    tune(ctx, capi.VRS_TUNE_REDUCE_CHUNK_ROWS, REDUCE_CH)
    tune(ctx, capi.VRS_TUNE_REDUCE_LANE_ROWS, sr.LR)
    n, offsets = ragged(lengths, lead=2, tail=3)  # offsets index reduction rows: two rows in front and three behind belong to no segment
    S = len(lengths)
    rng = np.random.default_rng(n + C)
    if dtype in (sr.I32, sr.I64):
        info = np.iinfo(sr.STORAGE[dtype])
        make = lambda shape: rng.integers(info.min, info.max, shape, dtype=sr.STORAGE[dtype], endpoint=True) | (1 if op == sr.PROD else 0)  # noqa: E731
    else:
        make = lambda shape: sr.to_storage(rng.standard_normal(shape), dtype)  # noqa: E731  (no NaN: which NaN a sum keeps is the processor's choice)
    raw, init = make((n, C)), make((S, C)) if with_init else None
    order = rng.permutation(n).astype(np.uint32) if with_order else None
    want = sr.host(ctx.lib, raw, dtype, offsets, op, init, order, ch=REDUCE_CH)
    assert max(sr.levels_for(ctx.lib, int(length), REDUCE_CH)[1] for length in lengths) == levels
    assert sr.map_for(ctx.lib, min(max(lengths), REDUCE_CH), C)[1] == getattr(sr, {"lane": "LANE", "rows": "ROWS", "columns": "COLUMNS"}[first_map])
    eb = raw.itemsize
    need = capi.query_u64("vrs_segment_reduce_scratch_bytes", n, C, S, dtype, REDUCE_CH)
    specs = [Spec("values", n * C * eb, "in", wrap_align(eb), raw), Spec("offsets", 4 * (S + 1), "in", 4, offsets),
             Spec("scratch", need, "scratch", wrap_align(eb))]
    if with_order:
        specs.append(Spec("order", 4 * n, "in", 4, order))
    if out_is_init:  # allowed: init is then the range that is written
        specs.append(Spec("init", S * C * eb, "inout", wrap_align(eb), init))
        expect, refuse = {"init": as_bytes(want)}, {"init": eb, "scratch": 1}
    else:
        specs.append(Spec("out", S * C * eb, "out", wrap_align(eb)))
        expect, refuse = {"out": as_bytes(want)}, {"out": eb, "scratch": 1}
        if with_init:
            specs.append(Spec("init", S * C * eb, "in", wrap_align(eb), init))

    def call(c, h):
        return c.lib.vrs_segment_reduce(c.handle, h["values"], n, C, dtype, h["order"], h["offsets"], S, op, h["init"],
                                        h["init"] if out_is_init else h["out"], h["scratch"])

    def ran(before, after):
        d = {k: after[k] - before[k] for k in ("lane", "rows", "columns")}
        others = "columns" if C < 64 else ("lane", "rows")
        return d[first_map] > 0 and all(d[k] == 0 for k in ([others] if isinstance(others, str) else others)) and after["max_levels"] >= levels

    return Case(specs, call, expect, vrs.reduce_stats, ran, refuse)


@pytest.mark.parametrize("key", list(REDUCE_CASES))
def test_segment_reduce(ctx, dev, key):
    run_case(ctx, dev, f"segment_reduce {key}", reduce_case(ctx, key))


def test_segment_reduce_refuses_short_buffers(ctx, dev):
    run_refusals(ctx, dev, "segment_reduce", reduce_case(ctx, "rows-two-levels-float64-order-init"))
    run_refusals(ctx, dev, "segment_reduce, out == init", reduce_case(ctx, "rows-three-levels-float32-out-is-init"))
