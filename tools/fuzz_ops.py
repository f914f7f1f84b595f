"""Differential fuzz of the torch-level entry points, interleaved on the contexts `_torch.context_for` hands out.

Two halves.  `cases(seed, count)` is a pure generator of case descriptions (plain dicts, no tensors, numpy's Generator only, no device):
op, dtype, shapes, layouts, flags, value distribution and a data seed per case, sizes drawn around the thresholds the library exports
(found by bisecting its pure functions, never written down here).  `run(seed, count, device)` executes them through the public
functions of vkradixsort_amd -- a window's inputs are all uploaded first, then its `window` calls go out back to back with no copy
and no host synchronisation between them, every fifth window on a second stream -- and compares every element of every output
with references written on torch's CPU functions and numpy alone.  It stops at the first mismatch or error, prints the seed, the
case index, the last eight descriptions, the first differing position and a replay line, and starts nothing more on the GPU.
   python tools/fuzz_ops.py SECONDS SEED            (soak: the same runner with a time budget)
   python tools/fuzz_ops.py 0 SEED --count N        (replay the first N cases of a seed)
Three decks of ops, never folded into one (`--deck`, `cases(..., deck=)`, `run(..., deck=)`).  "first": sort, sort_values, argsort, sort_rows,
topk, unique, unique_consecutive, searchsorted, bucketize; its stream of descriptions is pinned by a hash in tests/test_ops_fuzz_cpu.py.
"newer": the selections (kthvalue, median, nanmedian, quantile, nanquantile), the counts (bincount, histc, histogram), the reductions
(segment_reduce, index_add, index_reduce, scatter_reduce), the scans (cumsum, cumprod, cummax, cummin) and the compactions (nonzero,
argwhere, count_nonzero, masked_select, masked_scatter, mask_index, mask_index_put).  Every window of the newer deck holds a case of the
first deck's ops, and every second window opens with a 1-D sort / sort_values / unique of the one-call minimum or more, so that a
deferred sort is pending when the next op's settle_pending runs.  Its outputs are held to torch's CPU functions and numpy bit for bit
wherever the result is defined exactly; float sums, products and means come in two value classes that the description names: "exact"
(small integers, +-1 factors, lengths capped so that every partial result is representable: == against torch) and "general" (random
finite values against the same operation in float64, within (t + 1) u sum|x| for a sum of t terms, t u / (1 - t u) relative for a
product, one u more for a mean's division, u the dtype's epsilon, t u < 0.1 kept by the generator).
"third": repeat_interleave, isin, mode and the dim= forms of unique / unique_consecutive (as ops "unique_dim" / "unique_consecutive_dim"), in
the newer deck's windows: a neighbour from the first or the newer deck's ops in every window, a pending sort in front of every second one.
All of its outputs are defined exactly and held bit for bit: repeat_interleave and isin to torch's CPU functions, mode and the dim= forms
to numpy restatements of their documented rules (mode: the smallest of the most frequent values, -0.0 and +0.0 one value, all NaNs one
value, the largest, the index of the LAST occurrence, the value with that element's bits; rows: words by the IEEE total order, equal when
bit-identical) and, where torch defines the same answer (NaN-free mode values; integer rows and float rows without NaN and -0.0), to
torch.mode / torch.unique(dim=) / torch.unique_consecutive(dim=) as well.
tools/fuzz_gpu.py covers the raw key and pair sorts on a context of its own."""
from __future__ import annotations

import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

DTYPES = ["int8", "uint8", "int16", "int32", "int64", "float16", "bfloat16", "float32", "float64"]
DTYPE_BYTES = {"bool": 1, "int8": 1, "uint8": 1, "int16": 2, "int32": 4, "int64": 8, "float16": 2, "bfloat16": 2, "float32": 4, "float64": 8}
FLOATS = ("float16", "bfloat16", "float32", "float64")
KEY32, KEY3264 = ["int32", "float32"], ["int32", "int64", "float32", "float64"]
# what each wrapper accepts (tests/test_ops_fuzz_cpu.py reads the same lists out of the wrappers' refusals)
OP_DTYPES = {"sort": DTYPES, "sort_values": DTYPES, "argsort": DTYPES, "sort_rows": KEY32, "topk": KEY32, "unique": KEY3264,
             "unique_consecutive": KEY3264, "searchsorted": DTYPES, "bucketize": DTYPES}
FIRST_OPS = tuple(OP_DTYPES)  # the first deck's ops; the newer deck's follow
TEN, SIX = ["bool"] + DTYPES, ["int32", "int64", "float16", "bfloat16", "float32", "float64"]
INDEX_DTYPES = ["uint8", "int8", "int16", "int32", "int64"]
OP_DTYPES.update({"kthvalue": DTYPES, "median": DTYPES, "nanmedian": DTYPES, "quantile": ["float32", "float64"], "nanquantile": ["float32", "float64"],
                  "bincount": INDEX_DTYPES, "histc": list(FLOATS), "histogram": ["float32", "float64"],
                  "segment_reduce": SIX, "index_add": SIX, "index_reduce": SIX, "scatter_reduce": SIX,
                  "cumsum": TEN, "cumprod": TEN, "cummax": TEN, "cummin": TEN,
                  "nonzero": TEN, "argwhere": TEN, "count_nonzero": TEN, "masked_select": TEN, "masked_scatter": TEN, "mask_index": TEN, "mask_index_put": TEN})
NEWER_OPS = tuple(op for op in OP_DTYPES if op not in FIRST_OPS)  # (OP_DTYPES ends here: the first and the newer deck's ops, nothing joins it)
# the third deck's ops; the dim= forms of unique / unique_consecutive under names of their own (the first deck's entries stay what they are)
THIRD_OPS = ("repeat_interleave", "isin", "mode", "unique_dim", "unique_consecutive_dim")
# what the third deck's wrappers accept: a table of its own, so that OP_DTYPES and NEWER_OPS stay what the two older decks and their tests read
THIRD_OP_DTYPES = {"repeat_interleave": TEN, "isin": DTYPES, "mode": DTYPES, "unique_dim": KEY3264, "unique_consecutive_dim": KEY3264}
THIRD_OP_TURNS = {"repeat_interleave": 5, "isin": 5, "mode": 6, "unique_dim": 4, "unique_consecutive_dim": 3}  # turns per round of the third deck's op deck
OP_WEIGHT = {"searchsorted": 3, "bucketize": 2, "topk": 4, "sort_rows": 3, "unique": 2, "unique_consecutive": 2}  # (turns per round of the op x dtype deck: one unless named)
CONTIGUOUS_ONLY = ("sort_rows", "topk", "unique", "unique_consecutive")  # these refuse a non-contiguous tensor
LAYOUTS = ["contiguous", "transposed", "strided", "offset", "expanded"]
DISTS_FLOAT = ["uniform", "few", "ascending", "descending", "constant", "onebyte", "hot", "specials"]
DISTS_INT = ["uniform", "few", "ascending", "descending", "constant", "onebyte", "hot", "extremes"]
SEARCH_VARIANTS = ["1d_nd", "rows", "mixed", "scalar", "dependent"]
# (sequence dtype, input dtype, what torch promotes the two to: one of the nine)
MIXED_PAIRS = [("int32", "int64", "int64"), ("uint8", "int8", "int16"), ("float16", "float32", "float32"), ("int32", "float32", "float32"),
               ("bfloat16", "float32", "float32"), ("int64", "float64", "float64")]
SMALL_ELEMENTS = 100_000     # most cases stay below this many elements
LARGE_ELEMENTS = 1 << 23     # the fixed minority reaches up to here
LARGE_EVERY, LARGE_AT = 8, 5  # case i is of the large minority when i % LARGE_EVERY == LARGE_AT
EDGE_EVERY, EDGE_AT = 16, 2    # case i is a bare-key sort at an edge of the one-call sort's small forms when i % EDGE_EVERY == EDGE_AT
LARGE_KINDS = ["pool_keys", "pool_keys", "pool_pairs", "pool_pairs", "segment_one_call", "segment_one_call_u64", "unique_large", "topk_large"]
SECOND_STREAM_EVERY = 5      # every fifth window runs on a second stream
PENDING_BYTES_CAP = 1 << 30
# (seed, count) of the runs tests/test_gpu_ops_fuzz.py makes; tests/test_ops_fuzz_cpu.py holds them to what the generator claims to reach
COMMITTED_RUNS = [(104, 256)]
COMMITTED_RUNS_NEWER = [(491, 256)]  # the same for the newer deck
COMMITTED_RUNS_THIRD = [(7, 256)]    # and for the third


# ------------------------------------------------------------------------------------------------------------------------------
# thresholds: bisected out of the library's pure functions (no device)

def _first(pred, lo: int, hi: int) -> int:
    """The smallest v in (lo, hi] with pred(v), pred monotone, pred(lo) false and pred(hi) true."""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


class Thresholds:
    """Every size the generator straddles, read once from the library."""

    def __init__(self):
        from vkradixsort_amd import capi
        self.capi = capi
        self.lib = capi.load_library()
        top = LARGE_ELEMENTS * 4
        self.segment = {}  # (wide, pairs) -> [first block length, first global length, first one-call length]
        for wide in (False, True):
            for pairs in (False, True):
                tier = lambda L, w=wide, p=pairs: self.segment_tier(L, w, p)
                self.segment[wide, pairs] = [_first(lambda L, t=t: tier(L) >= t, 1, top) for t in (capi.VRS_SEGMENT_BLOCK, capi.VRS_SEGMENT_GLOBAL,
                                                                                                    capi.VRS_SEGMENT_ONE_CALL)]
        self.segment_one_call_min = self.segment[False, False][2]
        self.topk = [_first(lambda L, t=t: self.topk_tier(L) >= t, 1, top) for t in (capi.VRS_TOPK_BLOCK, capi.VRS_TOPK_GRID)]
        self.form_cuts = {}  # (key bytes, pairs) -> the element counts up to LARGE_ELEMENTS at which the one-call sort changes form
        for kb in (4, 8):
            for pairs in (0, 1):
                cuts, n = [], 1
                while n < LARGE_ELEMENTS:
                    hi = min(n * 2, LARGE_ELEMENTS)
                    f0 = self.sort_form(n, kb, pairs)
                    if f0 != self.sort_form(hi, kb, pairs):
                        n = _first(lambda v: self.sort_form(v, kb, pairs) != f0, n, hi)
                        cuts.append(n)
                    else:
                        n = hi
                self.form_cuts[kb, pairs] = cuts
        pool = [n for n in self.form_cuts[4, 0] if self.sort_form(n, 4, 0) == "pool"]
        self.pool_min = pool[0]  # bare 4-byte keys: the only kind whose pool form starts below LARGE_ELEMENTS
        self.search = {}  # dtype -> (first row length outside LDS, table minimum or None, index minimum)
        for name in DTYPES:
            code = getattr(capi, "VRS_SORT_" + name.upper())
            out = _first(lambda m: self.search_tier(m, m, 1, 1, code) != capi.VRS_SEARCH_LDS, 1, top)
            table = None
            if DTYPE_BYTES[name] <= 2:
                table = _first(lambda q: self.search_tier(out, out, q, q, code) == capi.VRS_SEARCH_TABLE, 0, top)
            index = _first(lambda q: self.search_tier(2 * out, out, 2 * q, q, code) == capi.VRS_SEARCH_INDEXED, 0, top)
            self.search[name] = (out, table, index)
        # -- what the newer deck straddles
        self.select = {}  # dtype -> [first block-tier row length, first grid-tier row length]
        for name in DTYPES:
            self.select[name] = [_first(lambda L, t=t: self.select_tier(L, name) >= t, 1, top) for t in (capi.VRS_SELECT_BLOCK, capi.VRS_SELECT_GRID)]
        self.bincount = {cb: _first(lambda b: self.bincount_tier(b, cb) == capi.VRS_BINCOUNT_GLOBAL, 1, top) for cb in (4, 8)}  # counter bytes -> first global bins
        self.reduce_levels = [_first(lambda L, k=k: self.reduce_levels_of(L) >= k, 1, top) for k in (2, 3)]
        self.scan_levels = [_first(lambda L, k=k: self.scan_levels_of(L) >= k, 1, top) for k in (1, 2)]
        self._scan_cuts = {}
        # the first count up to the cap at which key + payload pairs take the pool form (None: only above the cap, or never): a walk over the
        # form's changes up to the cap, as form_cuts is, so that a minimum that comes within the cap is found wherever it lies
        pairs_pool = [n for n in self.form_cuts[4, 1] if self.sort_form(n, 4, 1) == "pool"]
        self.pool_min_pairs = pairs_pool[0] if pairs_pool else None
        self.compact_tile = capi.COMPACT_TILE_ELEMS_DEFAULT

    def select_tier(self, length: int, dtype: str) -> int:
        lo, hi, tier = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
        assert self.lib.vrs_select_tier_for(0, length, length, getattr(self.capi, "VRS_SORT_" + dtype.upper()), self.capi.SELECT_GRID_MIN_KEYS_DEFAULT,
                                            ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(tier)) == 0
        return tier.value

    def bincount_tier(self, bins: int, counter_bytes: int) -> int:
        tier = ctypes.c_int()
        assert self.lib.vrs_bin_count_tier_for(bins, counter_bytes, self.capi.BINCOUNT_LDS_BYTES_DEFAULT, ctypes.byref(tier)) == 0
        return tier.value

    def reduce_levels_of(self, length: int) -> int:
        levels = ctypes.c_uint32()
        assert self.lib.vrs_segment_reduce_levels_for(length, self.capi.REDUCE_CHUNK_ROWS_DEFAULT, ctypes.byref(levels)) == 0
        return levels.value

    def scan_levels_of(self, length: int) -> int:
        levels = ctypes.c_uint32()
        assert self.lib.vrs_scan_levels_for(length, self.capi.SCAN_TILE_ROWS_DEFAULT, ctypes.byref(levels)) == 0
        return levels.value

    def scan_tier(self, S: int, L: int, C: int, dtype: str, out_dtype: str, op: str) -> int:
        c, tier = self.capi, ctypes.c_int()
        code = lambda name: getattr(c, "VRS_SORT_" + name.upper())  # noqa: E731
        assert self.lib.vrs_scan_tier_for(S, L, C, code(dtype), code(out_dtype), getattr(c, "VRS_SCAN_" + SCAN_KERNEL_OP[op]), c.SCAN_TILE_ROWS_DEFAULT,
                                          c.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT, ctypes.byref(tier)) == 0
        return tier.value

    def scan_cuts(self, dtype: str, out_dtype: str, op: str):
        """[first three-launch length, first single-pass length or None] of one segment of one column of this kernel dtype pair and op."""
        key = (dtype, out_dtype, op)
        if key not in self._scan_cuts:
            top, cuts = LARGE_ELEMENTS * 4, []
            for tier in (self.capi.VRS_SCAN_THREE_LAUNCH, self.capi.VRS_SCAN_SINGLE_PASS):
                reached = self.scan_tier(1, top, 1, dtype, out_dtype, op) >= tier
                cuts.append(_first(lambda L: self.scan_tier(1, L, 1, dtype, out_dtype, op) >= tier, 1, top) if reached else None)
            self._scan_cuts[key] = cuts
        return self._scan_cuts[key]

    def segment_tier(self, length: int, wide: bool, pairs: bool) -> int:
        fn = self.lib.vrs_segment_tier_for_u64 if wide else self.lib.vrs_segment_tier_for
        tier, lo, hi = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
        assert fn(0, length, length, int(pairs), self.capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT, ctypes.byref(tier), ctypes.byref(lo), ctypes.byref(hi)) == 0
        return tier.value

    def topk_tier(self, length: int) -> int:
        tier, lo, hi = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
        assert self.lib.vrs_topk_tier_for(0, length, length, self.capi.TOPK_GRID_MIN_KEYS_DEFAULT, ctypes.byref(tier), ctypes.byref(lo), ctypes.byref(hi)) == 0
        return tier.value

    def search_tier(self, nb: int, m: int, nq: int, q_len: int, code: int) -> int:
        c, tier = self.capi, ctypes.c_int()
        assert self.lib.vrs_search_tier_for(nb, m, nq, q_len, code, c.SEARCH_LDS_BYTES_DEFAULT, c.SEARCH_TABLE_MIN_QUERIES_DEFAULT,
                                            c.SEARCH_INDEX_MIN_QUERIES_DEFAULT, ctypes.byref(tier)) == 0
        return tier.value

    def sort_form(self, n: int, key_bytes: int, pairs: int) -> str:
        form = ctypes.c_int()
        assert self.lib.vrs_sort_form_for(n, key_bytes, pairs, None, 0, ctypes.byref(form), None) == 0
        return self.capi.FORM_NAMES[form.value]


_thresholds = None


def thresholds() -> Thresholds:
    global _thresholds
    if _thresholds is None:
        _thresholds = Thresholds()
    return _thresholds


# ------------------------------------------------------------------------------------------------------------------------------
# the case generator

class _Deck:
    """Draws without replacement and reshuffles when empty: every item comes up once per len(items) draws."""

    def __init__(self, rng, items):
        self.rng, self.items, self.left = rng, list(items), []

    def draw(self, where=None):
        """The next item (where: the next one that satisfies it; the others keep their turn)."""
        for _ in range(2):
            for i in range(len(self.left) - 1, -1, -1):
                if where is None or where(self.left[i]):
                    return self.left.pop(i)
            self.left = [self.items[i] for i in self.rng.permutation(len(self.items))] + self.left
        raise ValueError("no item of the deck satisfies the condition")


def _around(gen, cuts, cap: int):
    """One length of the class built on `cuts`: cut - 1, cut, cut + 1 for every cut below the cap, and a random point between
    neighbouring cuts (below the first, 2 is the lower neighbour).  One deck per class: every edge comes up once per round."""
    rng = gen.rng
    cuts = sorted(c for c in set(cuts) if c + 1 <= cap)
    key = (tuple(cuts), cap)
    if key not in gen.around:
        bounds = [2] + cuts + [cap]
        gen.around[key] = _Deck(rng, [c + d for c in cuts for d in (-1, 0, 1)] + list(zip(bounds[:-1], bounds[1:])))
    pick = gen.around[key].draw()
    if isinstance(pick, tuple):
        lo, hi = pick
        return int(rng.integers(lo + 1, hi)) if hi - lo > 2 else int(lo)
    return int(pick)


class _Gen:
    def __init__(self, seed: int, count: int, window: int):
        self.t = thresholds()
        self.rng = rng = np.random.Generator(np.random.PCG64(seed))
        self.count, self.window = count, window
        pairs = [(op, dt) for op in FIRST_OPS for dt in OP_DTYPES[op] for _ in range(OP_WEIGHT.get(op, 1))]
        self.op_dtype = _Deck(rng, pairs)
        self.layout = _Deck(rng, LAYOUTS)
        self.layout_contiguous = _Deck(rng, ["contiguous", "offset"])
        self.dist = {True: _Deck(rng, DISTS_FLOAT), False: _Deck(rng, DISTS_INT)}
        self.large = _Deck(rng, LARGE_KINDS)
        self.variant = _Deck(rng, SEARCH_VARIANTS + ["mixed"])
        self.search_tier = {dt: _Deck(rng, ["lds", "direct", "indexed"] + (["table"] if DTYPE_BYTES[dt] <= 2 else [])) for dt in DTYPES}
        self.mixed = _Deck(rng, MIXED_PAIRS)
        self.sort_size = _Deck(rng, ["tiny", "rows", "rows", "rows", "one_row", "many_short"])
        self.topk_k = _Deck(rng, ["one", "two", "small", "half", "all_but_one", "all"])
        self.flags4 = _Deck(rng, [(a, b) for a in (False, True) for b in (False, True)])
        self.side = _Deck(rng, [(False, None), (True, None), (False, "left"), (False, "right")])
        self.twin_n = {}
        self.bare_edge = _Deck(rng, [c + d for c in self.t.form_cuts[4, 0] if c < SMALL_ELEMENTS for d in (-1, 0, 1)])
        self.around = {}
        self.one_call_edge = _Deck(rng, [-1, 0, 1])
        self.pool_n = _Deck(rng, [self.t.pool_min - 1, self.t.pool_min, self.t.pool_min + 1, None])
        self.queue = []

    # -- pieces ---------------------------------------------------------------------------------------------------------------
    def _seed(self) -> int:
        return int(self.rng.integers(1 << 31))

    def _dist(self, dtype: str) -> str:
        return self.dist[dtype in FLOATS].draw()

    def _layout(self, shape, contiguous_only: bool = False) -> dict:
        rng = self.rng
        for _ in range(8):
            kind = (self.layout_contiguous if contiguous_only else self.layout).draw()
            if kind == "transposed" and len(shape) >= 2:
                d0 = int(rng.integers(len(shape) - 1))
                return {"kind": kind, "dims": [d0, int(rng.integers(d0 + 1, len(shape)))]}
            if kind == "strided" and len(shape) >= 1:
                return {"kind": kind, "step": int(rng.integers(2, 4))}
            if kind == "offset" and len(shape) >= 1:
                return {"kind": kind, "by": int(rng.integers(1, 4))}
            if kind == "expanded" and len(shape) >= 2:
                return {"kind": kind, "dim": int(rng.integers(len(shape)))}
            if kind == "contiguous":
                break
        return {"kind": "contiguous"}

    def _rows_for(self, length: int, cap: int = SMALL_ELEMENTS) -> int:
        most = max(1, cap // max(length, 1))
        return int(self.rng.integers(1, min(most, 2000) + 1))

    def _shape_with(self, rows: int, length: int):
        """A 1-D to 3-D shape of `rows` rows of `length` elements, the rows' dimension at a random place: (shape, dim)."""
        rng = self.rng
        if rows == 1 and rng.integers(2):
            return [length], 0
        other = [rows]
        if rows > 1 and rng.integers(2):
            a = int(rng.integers(1, 5))
            other = [a, -(-rows // a)]
        dim = int(rng.integers(len(other) + 1))
        return other[:dim] + [length] + other[dim:], dim

    # -- ops ------------------------------------------------------------------------------------------------------------------
    def _sort(self, op: str, dtype: str, size=None) -> dict:
        rng, t = self.rng, self.t
        wide = DTYPE_BYTES[dtype] == 8
        pairs = op != "sort_values" or dtype in FLOATS
        dist = self._dist(dtype)
        size = size or self.sort_size.draw()
        if DTYPE_BYTES[dtype] == 2 and size != "tiny" and rng.integers(6) == 0:
            dist, shape, dim = "allbits", [1 << 16], 0  # every bit pattern of a 2-byte dtype exactly once
        elif size == "tiny":
            shape, dim = [([0], 0), ([1], 0), ([], 0), ([3, 0], 1), ([3, 0], 0), ([1, 5], 0), ([4, 1, 3], 1), ([2, 1], 1)][int(rng.integers(8))]
        elif size == "one_row":
            shape, dim = [_around(self, t.form_cuts[8 if wide else 4, int(pairs)], SMALL_ELEMENTS)], 0
        elif size == "many_short":
            length = int(rng.integers(2, 65))
            shape, dim = self._shape_with(self._rows_for(length), length)
        else:
            length = _around(self, t.segment[wide, pairs][:2], SMALL_ELEMENTS // 2)
            shape, dim = self._shape_with(int(rng.integers(2, max(3, SMALL_ELEMENTS // length + 1))), length)
        if len(shape) and rng.integers(2):
            dim -= len(shape)  # (a negative dim)
        return {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "descending": bool(rng.integers(2)), "layout": self._layout(shape),
                "dist": dist, "data_seed": self._seed()}

    def _sort_rows(self, dtype: str) -> dict:
        rng = self.rng
        indices = bool(rng.integers(2))
        kind = int(rng.integers(8))
        if kind == 0:
            shape = [[0, 5], [3, 0], [1, 1], [7, 1]][int(rng.integers(4))]
        elif kind <= 2:
            length = int(rng.integers(2, 65))
            shape = [self._rows_for(length), length]
        else:
            length = _around(self, self.t.segment[False, indices][:2], SMALL_ELEMENTS // 2)
            shape = [int(rng.integers(1, max(2, SMALL_ELEMENTS // length + 1))), length]
        return {"op": "sort_rows", "dtype": dtype, "shape": shape, "return_indices": indices, "layout": self._layout(shape, True),
                "dist": self._dist(dtype), "data_seed": self._seed()}

    def _topk(self, dtype: str, length=None) -> dict:
        rng = self.rng
        if length is None:
            kind = int(rng.integers(8))
            if kind == 0:
                length = int(rng.integers(0, 3))
            elif kind == 1:
                length = int(rng.integers(2, 65))
            else:
                length = _around(self, self.t.topk, 2 * self.t.topk[1])
            rows = self._rows_for(length, max(SMALL_ELEMENTS, 2 * length))
        else:
            rows = 1
        shape = [length] if rows == 1 and rng.integers(2) else [rows, length]
        which = self.topk_k.draw()
        k = {"one": 1, "two": 2, "small": int(rng.integers(3, 40)), "half": length // 2, "all_but_one": length - 1, "all": length}[which]
        k = max(min(k, length), min(1, length))
        return {"op": "topk", "dtype": dtype, "shape": shape, "k": k, "largest": bool(rng.integers(2)), "sorted": bool(rng.integers(2)),
                "layout": self._layout(shape, True), "dist": self._dist(dtype), "data_seed": self._seed()}

    def _unique(self, op: str, dtype: str, n=None, dist=None, flags=None) -> dict:
        rng, t = self.rng, self.t
        inverse, counts = flags if flags is not None else self.flags4.draw()
        if n is None:
            kind = int(rng.integers(8))
            if kind == 0:
                n = int(rng.integers(0, 3))
            elif op == "unique":
                n = _around(self, t.form_cuts[DTYPE_BYTES[dtype], 1] + t.form_cuts[DTYPE_BYTES[dtype], 0], SMALL_ELEMENTS)
            else:
                tile = t.capi.RLE_TILE
                n = _around(self, [tile, 2 * tile, 8 * tile], SMALL_ELEMENTS)
        shape = [n]
        if n > 1 and rng.integers(3) == 0:
            a = int(rng.integers(1, 5))
            shape = [a, n // a] if rng.integers(2) else [a, 1, n // a]
        return {"op": op, "dtype": dtype, "shape": shape, "return_inverse": inverse, "return_counts": counts,
                "layout": self._layout(shape, True), "dist": dist or self._dist(dtype), "data_seed": self._seed()}

    def _search_sizes(self, dtype: str, tier: str, rows_allowed: bool):
        """(rows, boundary row length m, queries per row) that land in `tier` (rows == 0: a 1-D sequence)."""
        rng = self.rng
        out, table, index = self.t.search[dtype]
        one_byte = DTYPE_BYTES[dtype] == 1
        few = int(rng.integers(0, 200)) if not one_byte else int(rng.integers(0, max(table - 1, 1)))
        if table is not None and not rows_allowed and rng.integers(2) == 0:
            few = table - 1
        if tier == "lds":
            m = [0, 1, out - 2, out - 1][int(rng.integers(4))] if rng.integers(2) else int(rng.integers(2, out - 1))
            rows = int(rng.integers(2, 40)) if rows_allowed and m < 2000 and rng.integers(2) else (1 if rows_allowed else 0)
            return rows, m, few
        if tier == "table":
            m = _around(self, [out], 3 * out)
            return 0, m, [table, table + 1, int(rng.integers(table + 1, 2 * table + 2))][int(rng.integers(3))]
        m = [out, out + 1][int(rng.integers(2))] if rng.integers(2) else int(rng.integers(out + 1, 3 * out))
        if tier == "direct":
            if rows_allowed:  # (two rows of a 1- or 2-byte dtype: one row with many queries takes the table)
                return (2 if table is not None else int(rng.integers(1, 3))), m, [index - 1, max(few, 1)][int(rng.integers(2))]
            return 0, m, few if table is not None else [index - 1, few][int(rng.integers(2))]
        q = [index, index + 1, int(rng.integers(index + 1, index + index // 2))][int(rng.integers(3))]
        if table is not None:
            return 2, m, q  # (one boundary row of a 1- or 2-byte dtype with this many queries takes the table)
        return (int(rng.integers(1, 3)) if rows_allowed else 0), m, q

    def _search(self, op: str, dtype: str, variant=None) -> list:
        rng = self.rng
        right, side = self.side.draw()
        base = {"op": op, "dtype": dtype, "right": right, "side": side, "out_int32": bool(rng.integers(2)), "sorter": bool(rng.integers(2)),
                "data_seed": self._seed()}
        if op == "bucketize":
            base.pop("side"), base.pop("sorter")
            base["right"] = right or side == "right"
            variant = "1d_nd"
        variant = variant or self.variant.draw()
        if variant == "dependent" and (self._index % self.window == self.window - 1 or self._index + 2 > self.count):
            variant = "1d_nd"  # (the source and its search share a window)
        if variant == "dependent":
            sdt = KEY3264[int(rng.integers(4))] if rng.integers(2) else dtype
            dist = [d for d in (DISTS_FLOAT if sdt in FLOATS else DISTS_INT) if d != "specials"][int(rng.integers(7))]
            n = _around(self, [self.t.search[sdt][0]], SMALL_ELEMENTS // 2)
            if sdt in KEY3264 and rng.integers(2):
                source = self._unique("unique", sdt, n=n, dist=dist)
                source["shape"], source["layout"] = [n], self._layout([n], True)
            else:
                source = {"op": ["sort", "sort_values"][int(rng.integers(2))], "dtype": sdt, "shape": [n], "dim": 0, "descending": False,
                          "layout": self._layout([n]), "dist": dist, "data_seed": self._seed()}
            nq = int(rng.integers(1, 3000))
            base.update(op="searchsorted", dtype=sdt, variant=variant, source=self._index, in_dtype=sdt, in_shape=[nq],
                        in_layout=self._layout([nq]), in_dist=self._dist(sdt), sorter=False)
            return [source, base]
        in_dtype = tier_dtype = dtype
        if variant == "mixed":
            dtype, in_dtype, tier_dtype = self.mixed.draw()
            base["dtype"] = dtype
        rows_ok = variant in ("rows", "mixed") or (op == "searchsorted" and variant == "1d_nd")
        if variant == "scalar":  # (one query)
            tier = self.search_tier[dtype].draw(lambda t: t in ("lds", "direct"))
        else:  # (the promoted dtype's turn; one boundary row of a 1- or 2-byte dtype with an index's queries takes the table)
            tier = self.search_tier[tier_dtype].draw(lambda t: rows_ok or t != "indexed" or DTYPE_BYTES[tier_dtype] > 2)
        rows, m, q = self._search_sizes(tier_dtype, tier, rows_allowed=variant in ("rows", "mixed") or (rows_ok and tier == "indexed"))
        if rows == 0:
            variant = "1d_nd" if variant == "rows" else variant
            seq_shape = [m]
            in_shape = [[q], [1, q], [q, 1, 1]][int(rng.integers(3))]
            if q > 3 and rng.integers(2) and tier in ("lds", "direct"):
                a = int(rng.integers(2, 5))
                in_shape = [a, q // a] if rng.integers(2) else [q // a, 1, a]
        else:
            lead = [rows] if rng.integers(2) else [rows, 1]
            seq_shape, in_shape = lead + [m], lead + [q]
            variant = "rows" if variant == "1d_nd" else variant
        base.update(variant=variant, in_dtype=in_dtype, seq_shape=seq_shape, seq_layout=self._layout(seq_shape), seq_dist=self._dist(dtype))
        if base["seq_layout"]["kind"] == "expanded":
            base["seq_layout"] = {"kind": "contiguous"}  # (a sorted row cannot be written through an expanded view)
        if variant == "scalar":
            base.update(seq_shape=[m], number_is_float=dtype in FLOATS)
            base["seq_layout"] = self._layout([m])
            if base["seq_layout"]["kind"] == "expanded":
                base["seq_layout"] = {"kind": "contiguous"}
            return [base]
        base.update(in_shape=in_shape, in_layout=self._layout(in_shape), in_dist=self._dist(in_dtype))
        return [base]

    def _large(self) -> dict:
        rng, t = self.rng, self.t
        kind = self.large.draw()
        if kind.startswith("pool_"):
            group = kind.split("_")[1]
            twin = group in self.twin_n
            if twin:
                n = self.twin_n.pop(group)  # the same element count again, another distribution: the kept-layout case
            else:
                n = self.twin_n[group] = self.pool_n.draw()
                if n is None:
                    n = self.twin_n[group] = int(rng.integers(t.pool_min + 2, LARGE_ELEMENTS + 1 if rng.integers(4) == 0 else t.pool_min * 5 // 4))
            dist = ["few", "hot", "onebyte", "ascending"][int(rng.integers(4))] if twin else "uniform"
            if group == "keys":
                if rng.integers(2):
                    return {"op": "sort_values", "dtype": ["int32", "int16", "uint8"][int(rng.integers(3))], "shape": [n], "dim": 0,
                            "descending": bool(rng.integers(2)), "layout": self._layout([n]), "dist": dist, "data_seed": self._seed()}
                return self._unique("unique", "int32", n=n, dist="few" if not twin else "hot", flags=(False, False)) | {"shape": [n]}
            return {"op": ["sort", "argsort"][int(rng.integers(2))], "dtype": "float32", "shape": [n], "dim": -1, "descending": bool(rng.integers(2)),
                    "layout": self._layout([n]), "dist": dist, "data_seed": self._seed()}
        if kind.startswith("segment_one_call"):
            wide = kind.endswith("u64")
            dtype = (["int64", "float64"] if wide else ["int32", "float32", "bfloat16", "int8"])[int(rng.integers(2 if wide else 4))]
            op = ["sort", "sort_values", "argsort"][int(rng.integers(3))]
            cut = t.segment[wide, op != "sort_values" or dtype in FLOATS][2]
            length = cut + self.one_call_edge.draw()
            shape, dim = ([2, length], 1) if rng.integers(2) else ([length, 2], 0)
            return {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "descending": bool(rng.integers(2)), "layout": self._layout(shape),
                    "dist": self._dist(dtype), "data_seed": self._seed()}
        if kind == "unique_large":
            dtype = KEY3264[int(rng.integers(4))]
            n = int(rng.integers(SMALL_ELEMENTS, LARGE_ELEMENTS // 4))
            return self._unique("unique", dtype, n=n)
        return self._topk(KEY32[int(rng.integers(2))], length=int(rng.integers(2 * t.topk[1], LARGE_ELEMENTS // 2)))

    def _bare_keys_edge(self) -> dict:
        """Bare 4-byte keys (an integer sort_values, a unique without the inverse) at an edge of the one-call sort's small forms: the
        only kind of sort that has them, and too rare among the drawn cases to meet all six."""
        rng, n = self.rng, self.bare_edge.draw()
        if rng.integers(2):
            dtype = KEY32[int(rng.integers(2))]
            return self._unique("unique", dtype, n=n, flags=(False, bool(rng.integers(2)))) | {"shape": [n]}
        dtype = ["int8", "uint8", "int16", "int32"][int(rng.integers(4))]
        return {"op": "sort_values", "dtype": dtype, "shape": [n], "dim": 0, "descending": bool(rng.integers(2)), "layout": self._layout([n]),
                "dist": self._dist(dtype), "data_seed": self._seed()}

    def _next(self) -> list:
        if self._index % LARGE_EVERY == LARGE_AT:
            return [self._large()]
        if self._index % EDGE_EVERY == EDGE_AT:
            return [self._bare_keys_edge()]
        op, dtype = self.op_dtype.draw()
        if op in ("sort", "sort_values", "argsort"):
            return [self._sort(op, dtype)]
        if op == "sort_rows":
            return [self._sort_rows(dtype)]
        if op == "topk":
            return [self._topk(dtype)]
        if op in ("unique", "unique_consecutive"):
            return [self._unique(op, dtype)]
        return self._search(op, dtype)

    def __iter__(self):
        self._index = 0
        while self._index < self.count:
            for case in self._next():
                window = self._index // self.window
                case.update(index=self._index, window=window, stream="second" if window % SECOND_STREAM_EVERY == SECOND_STREAM_EVERY - 1 else "current")
                yield case
                self._index += 1


def cases(seed: int, count: int, window: int = 4, deck: str = "first"):
    """`count` case descriptions of `seed`: plain dicts of numbers, strings and lists.  The same everywhere; needs no device.
    deck "first": sort, topk, unique and the searches; "newer": the selections, counts, reductions, scans and compactions, every window with
    a neighbour from the first deck's ops; "third": repeat_interleave, isin, mode and unique / unique_consecutive along a dim, every window
    with a neighbour from the first or the newer deck's ops."""
    if deck not in ("first", "newer", "third"):
        raise ValueError(f"unknown deck {deck!r}")
    return iter({"first": _Gen, "newer": _GenNewer, "third": _GenThird}[deck](seed, count, window))


# ------------------------------------------------------------------------------------------------------------------------------
# values and layouts (torch on the CPU and numpy; nothing of the library)

_BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
_EXPONENT = {"float16": (0x7C00, 10), "bfloat16": (0x7F80, 7), "float32": (0x7F800000, 23), "float64": (0x7FF0000000000000, 52)}


def torch_dtype(name: str):
    import torch
    return getattr(torch, name)


def from_bits(bits, name: str):
    """A CPU tensor of dtype `name` over the unsigned bit patterns `bits` (a numpy array)."""
    import torch
    signed = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[bits.dtype.itemsize]
    t = torch.from_numpy(np.ascontiguousarray(bits).view(signed))
    return t.view(torch_dtype(name)) if name != "int" + str(8 * bits.dtype.itemsize) else t


def to_bits(t):
    """The unsigned bit patterns of a CPU tensor, as a numpy array of its shape."""
    import torch
    signed = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    t = t.contiguous()
    return (t if t.dtype == signed else t.view(signed)).numpy().view(_BITS[t.element_size()])


def special_bits(name: str):
    """±0, ±inf, quiet and signalling NaNs of both signs, the smallest and the largest denormal, the largest finite value."""
    em, mant = _EXPONENT[name]
    sign = 1 << (8 * DTYPE_BYTES[name] - 1)
    quiet = 1 << (mant - 1)
    full = (1 << (8 * DTYPE_BYTES[name])) - 1
    return [0, sign, em, sign | em, em | quiet, sign | em | quiet | 1, em | 1, full, 1, sign | 1, (1 << mant) - 1, em - 1, sign | (em - 1)]


def make_values(name: str, shape, dist: str, seed: int):
    """A contiguous CPU tensor of `shape` drawn from `dist`."""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    nbytes = DTYPE_BYTES[name]
    ut = _BITS[nbytes]
    n = int(np.prod(shape)) if len(shape) else 1
    is_float = name in FLOATS

    def uniform(count):
        b = rng.integers(0, 1 << (8 * nbytes), size=count, dtype=ut)
        if is_float:  # finite values only: an all-ones exponent loses its lowest bit
            em = ut(_EXPONENT[name][0])
            b = np.where((b & em) == em, b & ~ut(int(em) & -int(em)), b)
        return b.astype(ut)

    if dist == "allbits":
        assert nbytes == 2 and n == 1 << 16
        bits = rng.permutation(1 << 16).astype(ut)
    elif dist in ("uniform", "ascending", "descending"):
        bits = uniform(n)
    elif dist == "few":
        pool = uniform(int(rng.integers(2, 51)))
        bits = pool[rng.integers(0, pool.size, size=n)]
    elif dist == "constant":
        bits = np.full(n, uniform(1)[0], dtype=ut)
    elif dist == "onebyte":
        at = 8 * int(rng.integers(nbytes))
        fixed = uniform(1)[0] & ~ut(0xFF << at)
        bits = fixed | (rng.integers(0, 256, size=n).astype(ut) << ut(at))
        if is_float:
            em = ut(_EXPONENT[name][0])
            bits = np.where((bits & em) == em, bits & ~ut(int(em) & -int(em)), bits).astype(ut)
    elif dist == "hot":
        bits = uniform(n)
        bits[rng.random(n) < rng.uniform(0.6, 0.9)] = uniform(1)[0]
    elif dist == "specials":
        t = (torch.from_numpy(rng.integers(-40, 40, size=n)).to(torch.float64) / 4).to(torch_dtype(name))
        bits = to_bits(t).copy()
        sp = np.array(special_bits(name), dtype=ut)
        if n:
            at = rng.integers(0, n, size=min(n, 3 * sp.size))
            bits[at] = np.tile(sp, 3)[:at.size]
    elif dist == "extremes":
        info = torch.iinfo(torch_dtype(name))
        lo, hi = max(info.min, -40), min(info.max, 40)
        t = torch.from_numpy(rng.integers(lo, hi + 1, size=n)).to(torch_dtype(name))
        if n:
            ext = torch.tensor([info.min, info.max, info.min + 1, info.max - 1, 0], dtype=torch_dtype(name))
            at = torch.from_numpy(rng.integers(0, n, size=min(n, 15)))
            t[at] = ext.repeat(3)[:at.numel()]
        bits = to_bits(t)
    else:
        raise ValueError(f"unknown distribution {dist!r}")
    t = from_bits(np.asarray(bits, dtype=ut).reshape(-1), name)
    if dist in ("ascending", "descending"):
        t = torch.sort(t, descending=dist == "descending").values
    return t.reshape(shape)


def lay_out(shape, layout: dict, fill):
    """(base, view): a contiguous CPU allocation and the function that views it -- or a copy of it on a GPU -- as a tensor of `shape`
    in `layout`, holding fill(shape) (an expanded view: fill of the shape with that dimension 1, repeated)."""
    import torch
    kind = layout["kind"]
    shape = list(shape)
    if kind == "contiguous":
        return fill(shape), lambda t: t
    if kind == "expanded":
        small = shape[:layout["dim"]] + [1] + shape[layout["dim"] + 1:]
        return fill(small), lambda t: t.expand(shape)
    logical = fill(shape)
    if kind == "transposed":
        d0, d1 = layout["dims"]
        return logical.transpose(d0, d1).contiguous(), lambda t: t.transpose(d0, d1)
    if kind == "offset":  # the view starts 1 to 3 elements into its allocation: not 16-byte aligned
        by = layout["by"]
        base = torch.zeros(logical.numel() + by, dtype=logical.dtype)
        base[by:] = logical.reshape(-1)
        return base, lambda t: t[by:].view(shape)
    if kind == "strided":
        step = layout["step"]
        base = torch.zeros(shape[:-1] + [shape[-1] * step], dtype=logical.dtype)
        base[..., ::step] = logical
        return base, lambda t: t[..., ::step]
    raise ValueError(f"unknown layout {kind!r}")


# ------------------------------------------------------------------------------------------------------------------------------
# references: torch's CPU functions and numpy only

def order_key(t):
    """The unsigned integer whose order is the IEEE-754 total order of a float tensor's bit patterns (negative: all bits flipped, else the
    sign bit flipped) or the numeric order of a signed integer tensor (sign bit flipped)."""
    bits = to_bits(t)
    sign = bits.dtype.type(1 << (8 * bits.dtype.itemsize - 1))
    if t.dtype.is_floating_point:
        return np.where(bits & sign, ~bits, bits ^ sign).astype(bits.dtype)
    return bits ^ sign


def values_of_key(key, name: str):
    sign = key.dtype.type(1 << (8 * key.dtype.itemsize - 1))
    bits = np.where(key & sign, key ^ sign, ~key).astype(key.dtype) if name in FLOATS else key ^ sign
    return from_bits(bits, name)


def plain_values(t) -> bool:
    """No NaN and no -0.0: where the bit-pattern operations and torch's own agree."""
    import torch
    if not t.dtype.is_floating_point:
        return True
    return not bool(torch.isnan(t).any()) and not bool(((t == 0) & torch.signbit(t)).any())


def ref_sort(x, dim: int, descending: bool):
    import torch
    return torch.sort(x, dim=dim, descending=descending, stable=True)


def ref_sort_rows(x):
    """Each row by a stable sort of the order key; torch.sort itself for values where the two orders agree."""
    import torch
    if plain_values(x):
        r = torch.sort(x, dim=-1, stable=True)
        return r.values, r.indices
    order = torch.from_numpy(np.argsort(order_key(x), axis=-1, kind="stable"))
    return torch.gather(x, -1, order), order


def ref_topk(x, k: int, largest: bool):
    """The first k of a stable argsort of the order key per row (largest: of the reversed key, so ties stay lowest index first)."""
    import torch
    key = order_key(x)
    order = torch.from_numpy(np.argsort(~key if largest else key, axis=-1, kind="stable")[..., :k].copy())
    return torch.gather(x, -1, order), order


def ref_unique(x):
    import torch
    uk, inv, cnt = np.unique(order_key(x).reshape(-1), return_inverse=True, return_counts=True)
    return (values_of_key(uk, str(x.dtype).split(".")[1]), torch.from_numpy(inv.astype(np.int64)).reshape(x.shape),
            torch.from_numpy(cnt.astype(np.int64)))


def ref_unique_consecutive(x):
    import torch
    bits = to_bits(x).reshape(-1)
    heads = np.ones(bits.size, dtype=bool)
    heads[1:] = bits[1:] != bits[:-1]
    starts = np.flatnonzero(heads)
    counts = np.diff(np.append(starts, bits.size))
    return (from_bits(bits[heads], str(x.dtype).split(".")[1]), torch.from_numpy(np.cumsum(heads) - 1).to(torch.int64).reshape(x.shape),
            torch.from_numpy(counts.astype(np.int64)))


def ref_searchsorted(seq, values, right: bool, out_int32: bool, sorter=None):
    """torch.searchsorted on the CPU when the sequence has no NaN, numpy.searchsorted on float32 / float64 upcasts when it has.
    `values`: a tensor or a Python number; promoted with the sequence by torch.result_type."""
    import torch
    common = torch.result_type(seq, values)
    v = values.to(common) if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=common)
    s = seq.to(common)
    if common in (torch.float16, torch.bfloat16):  # (exact, and keeps the order)
        s, v = s.float(), v.float()
    s, v = s.contiguous(), v.contiguous()
    out = torch.int32 if out_int32 else torch.int64
    if not (s.is_floating_point() and bool(torch.isnan(s).any())):
        if s.dim() == 1 and v.dim() == 0:
            return torch.searchsorted(s, v.reshape(1), right=right, sorter=sorter, out_int32=out_int32).reshape(())
        return torch.searchsorted(s, v, right=right, sorter=sorter, out_int32=out_int32)
    m = s.shape[-1]
    sn, vn = s.reshape(-1, m).numpy(), (v.reshape(1, -1) if s.dim() == 1 else v.reshape(-1, v.shape[-1])).numpy()
    so = sorter.reshape(-1, m).numpy() if sorter is not None else None
    rows = [np.searchsorted(sn[i], vn[i], side="right" if right else "left", sorter=None if so is None else so[i]) for i in range(sn.shape[0])]
    return torch.from_numpy(np.stack(rows).astype(np.int64)).reshape(v.shape).to(out)


# ------------------------------------------------------------------------------------------------------------------------------
# the newer deck: its generator

SCAN_KERNEL_OP = {"cumsum": "SUM", "cumprod": "PROD", "cummax": "MAX", "cummin": "MIN"}
SELECT_OPS, QUANTILE_OPS, COUNT_OPS = ("kthvalue", "median", "nanmedian"), ("quantile", "nanquantile"), ("bincount", "histc", "histogram")
REDUCE_OPS, SCAN_OPS = ("segment_reduce", "index_add", "index_reduce", "scatter_reduce"), tuple(SCAN_KERNEL_OP)
COMPACT_OPS = ("nonzero", "argwhere", "count_nonzero", "masked_select", "masked_scatter", "mask_index", "mask_index_put")
K_CLASSES = ["one", "two", "middle", "all_but_one", "all"]
Q_KINDS = ["float", "0d", "t1", "t8", "t9", "t17"]  # a Python float, a 0-d tensor, a tensor of so many values
INTERPOLATIONS = ["linear", "lower", "higher", "midpoint", "nearest"]
NAN_KINDS = ["none", "some", "row"]                 # no NaN put in, NaNs in some rows, and one row of NaNs alone besides
DESTINATIONS = ["equal", "distinct", "zipf"]
MASK_CLASSES = ["none", "all", "sparse", "half", "one_tile"]
ROW_WIDTHS = [1, 3, 4, 1025]
BINCOUNT_WEIGHTS = [None, "float32", "float64", "int32", "float16"]  # (the last two: "another dtype", which the wrapper .double()s)
SCAN_TARGETS = {"bool": [None, "int32", "float32"], "int8": [None, "int32", "int64", "float32"], "uint8": [None, "int32", "float64"],
                "int16": [None, "int32", "float32"], "int32": [None, "int32", "int64", "float64"], "int64": [None, "float64"],
                "float16": [None, "float32"], "bfloat16": [None, "float32", "float64"], "float32": [None, "float64"], "float64": [None]}
# turns per round beyond one: the (op, dtype) pairs that alone can draw the edges of a cut (a bincount whose dtype reaches the cut, the
# histogram whose edge tensor straddles the search's LDS cut)
PAIR_WEIGHT_NEWER = {("bincount", "int32"): 3, ("bincount", "int64"): 2, ("histogram", "float32"): 3, ("quantile", "float32"): 2}  # (and six kinds of q, five interpolations for four pairs)
LARGE_KINDS_NEWER = ["index_add_skewed", "index_add_pool_edge", "cumsum_single_pass", "reduce_three_levels", "kthvalue_grid", "quantile_grid",
                     "bincount_global", "masked_select_large", "nonzero_large"]
EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7, "float32": 2.0 ** -23, "float64": 2.0 ** -52}  # u of the bounds: the dtype's epsilon
EXACT_LIMIT = {"float16": 2048, "bfloat16": 256, "float32": 1 << 24, "float64": 1 << 53}  # every integer up to here is held


def terms_cap(dtype: str, value_class: str, per_term: int = 1, start: int = 0) -> int:
    """The most terms a float sum or product of this class may have.  exact: terms of at most `per_term` on top of `start` stay within
    the integers the dtype holds, in any order.  general: t * u < 0.1, the condition of the bound (one term kept for an input or initial)."""
    if dtype not in FLOATS:
        return 1 << 40
    if value_class == "exact":
        return (EXACT_LIMIT[dtype] - start) // per_term
    return int(0.1 / EPS[dtype]) - 2


def segment_lengths(num_segments: int, longest: int, seed: int):
    """The lengths of a segment_reduce case: one segment of `longest` rows among short ones, about one in five of them empty."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = rng.integers(1, min(longest, 64) + 1, size=num_segments)
    lengths[rng.random(num_segments) < 0.2] = 0
    lengths[int(rng.integers(num_segments))] = longest
    return lengths.astype(np.int64)


class _GenNewer(_Gen):
    """The newer deck.  Window w of four holds: w even, a 1-D sort / sort_values / unique of the one-call minimum or more first (a deferred
    sort is pending when the next op's settle_pending runs); w odd, a case of the first deck's ops last; case i with i % LARGE_EVERY ==
    LARGE_AT is of the large minority; every other case is the next (op, dtype) of the newer ops' deck."""

    def __init__(self, seed: int, count: int, window: int):
        super().__init__(seed, count, window)
        if window < 4:
            raise ValueError("the newer deck takes windows of four cases or more")
        rng = self.rng
        self.new_op_dtype = _Deck(rng, [(op, dt) for op in NEWER_OPS for dt in OP_DTYPES[op] for _ in range(PAIR_WEIGHT_NEWER.get((op, dt), 1))])
        self.pending = _Deck(rng, [(op, dt) for op in ("sort", "sort_values", "unique") for dt in OP_DTYPES[op]])
        self.large_newer = _Deck(rng, LARGE_KINDS_NEWER)
        self.named, self.turns = {}, {}

    def _pick(self, name: str, items):
        """The next item of the deck `name` (made of `items` at its first use)."""
        if name not in self.named:
            self.named[name] = _Deck(self.rng, items)
        return self.named[name].draw()

    def _turn(self, name: str, items):
        """The items of `name` in their order, round and round: for the ops with so few cases a round that the order has to be planned."""
        self.turns[name] = self.turns.get(name, -1) + 1
        return items[self.turns[name] % len(items)]

    def _preferred(self, op: str, first, then=None) -> str:
        """A dtype for a large case of `op`: the deck's next one of `first` while the round still holds one, else its next one of `then`;
        when the round holds neither, any of them, and the deck keeps its turn (the case adds no pair to the round then)."""
        for allowed in (first, then or ()):
            if any(p[0] == op and p[1] in allowed for p in self.new_op_dtype.left):
                return self.new_op_dtype.draw(lambda p: p[0] == op and p[1] in allowed)[1]
        allowed = tuple(first) + tuple(then or ())
        return allowed[int(self.rng.integers(len(allowed)))]

    def _done(self, case: dict, role: str = "newer") -> list:
        case.update(deck="newer", role=role, data_seed=self._seed())
        return [case]

    def _value_dist(self, dtype: str) -> str:
        return "uniform" if dtype == "bool" else self._dist(dtype)

    def _rows_shape(self, length: int, cap: int = SMALL_ELEMENTS):
        shape, dim = self._shape_with(self._rows_for(length, cap), length)
        return shape, (dim - len(shape) if self.rng.integers(2) else dim)

    def _short_or(self, name: str, cuts, cap: int) -> int:
        """A length for `name`: 1 to 3, 2 to 64, or (three times in four) one of the class built on `cuts`."""
        kind = int(self.rng.integers(8))
        if kind == 0:
            return int(self.rng.integers(1, 4))
        if kind == 1:
            return int(self.rng.integers(2, 65))
        return _around(self, cuts, cap)

    # -- the neighbours from the first deck -------------------------------------------------------------------------------------
    def _pending_sort(self) -> list:
        rng = self.rng
        op, dtype = self.pending.draw()
        low = self.t.capi.ONE_CALL_MIN_KEYS_DEFAULT
        n = int(rng.integers(low, SMALL_ELEMENTS + 1)) if rng.integers(4) else low + int(rng.integers(2))
        if op == "unique":
            case = self._unique("unique", dtype, n=n)
            case["shape"], case["layout"] = [n], self._layout([n], True)
        else:
            case = {"op": op, "dtype": dtype, "shape": [n], "dim": 0, "descending": bool(rng.integers(2)), "layout": self._layout([n]),
                    "dist": self._dist(dtype), "data_seed": self._seed()}
        case.update(deck="newer", role="pending_sort")
        return [case]

    def _neighbour(self) -> list:
        op, dtype = self.op_dtype.draw()
        if op in ("sort", "sort_values", "argsort"):
            case = self._sort(op, dtype)
        elif op == "sort_rows":
            case = self._sort_rows(dtype)
        elif op == "topk":
            case = self._topk(dtype)
        elif op in ("unique", "unique_consecutive"):
            case = self._unique(op, dtype)
        else:
            case = self._search(op, dtype, variant=self.variant.draw(lambda v: v != "dependent"))[0]
        case.update(deck="newer", role="neighbour")
        return [case]

    # -- selection --------------------------------------------------------------------------------------------------------------
    def _select_length(self, dtype: str, family: str = "select") -> int:
        """A row length: the block tier's cut for this dtype's rank width - 1, + 0, + 1, each once in four draws of that width, else short
        or anywhere up to half the small cap."""
        cut = self.t.select[dtype][0]
        step = self._pick(f"{family}_length_{cut}", [-1, 0, 1, None])
        if step is not None:
            return cut + step
        return int(self.rng.integers(1, 200)) if self.rng.integers(2) else int(self.rng.integers(200, SMALL_ELEMENTS // 2))

    def _select(self, op: str, dtype: str, length=None) -> dict:
        rng = self.rng
        if length is None:
            length = self._select_length(dtype)
            shape, dim = self._rows_shape(length)
        else:
            shape, dim = ([length], 0) if rng.integers(2) else ([2, length], -1)
        case = {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "keepdim": self._pick("keepdim", [False, True]), "layout": self._layout(shape),
                "dist": self._dist(dtype), "nans": self._pick("nans_" + op, NAN_KINDS) if dtype in FLOATS else "none"}
        if op == "kthvalue":
            which = self._pick("k", K_CLASSES)
            k = {"one": 1, "two": 2, "middle": (length + 1) // 2, "all_but_one": length - 1, "all": length}[which]
            case.update(k=max(1, min(k, length)), k_class=which)
        elif self._pick("dim_none", [True, False, False]):
            case.update(dim=None, keepdim=False)
            if _numel(shape) != length:  # (all elements are one row: the drawn length is the row's)
                case.update(shape=[length], layout=self._layout([length]))
        return case

    def _quantile(self, op: str, dtype: str, length=None) -> dict:
        rng = self.rng
        if length is None:
            length = self._select_length(dtype, "quantile")
            shape, dim = self._rows_shape(length)
        else:
            shape, dim = ([length], 0) if rng.integers(2) else ([2, length], -1)
        kind = self._pick("q", Q_KINDS)
        count = int(kind[1:]) if kind.startswith("t") else 1
        qs = [[0.0, 1.0, 0.5, 0.25][int(rng.integers(4))] if rng.integers(3) == 0 else float(np.float32(rng.random())) for _ in range(count)]
        case = {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "keepdim": self._pick("keepdim", [False, True]), "layout": self._layout(shape),
                "dist": self._pick("quantile_dist", ["normal", "small_ints", "near_one"]), "nans": self._pick("nans_quantile", NAN_KINDS), "q_kind": kind, "qs": qs,
                "interpolation": self._pick("interpolation", INTERPOLATIONS)}
        if self._pick("dim_none", [True, False, False]):
            case["dim"] = None
            if _numel(shape) != length:  # (all elements are one row: the drawn length is the row's)
                case.update(shape=[length], layout=self._layout([length]))
        return case

    # -- counting ---------------------------------------------------------------------------------------------------------------
    def _edge_or(self, name: str, cut: int, cap: int) -> int:
        """cut - 1, cut, cut + 1 or a random length up to the cap, each once in four draws of `name`: for the ops with few cases a round."""
        step = self._pick(name, [-1, 0, 1, None])
        return cut + step if step is not None else int(self.rng.integers(1, cap + 1))

    def _bins(self, counter: int) -> int:
        """A number of bins: the LDS tier's cut for this counter width - 1, + 0, + 1 (4-byte counters: or anywhere, once in four)."""
        cut = self.t.bincount[counter]
        step = self._pick(f"bins{counter}", [-1, 0, 1] + ([None] if counter == 4 else []))
        return cut + step if step is not None else int(self.rng.integers(1, 3 * self.t.bincount[4] + 1))

    def _bincount(self, dtype: str, bins=None, n=None) -> dict:
        rng = self.rng
        wide = dtype in ("int32", "int64")  # (the largest element is bins - 1: the cuts lie within these dtypes' range only)
        wide = "large" if bins is not None else wide
        weights = self._pick(f"bincount_weights_{wide}", BINCOUNT_WEIGHTS)
        counter = 8 if weights not in (None, "float32") else 4
        most = {"uint8": 256, "int8": 128, "int16": 32768}.get(dtype, 1 << 40)
        how = self._pick(f"minlength_{wide}", ["zero", "below", "above"])
        if bins is None:
            bins = self._bins(counter) if wide else int(rng.integers(1, min(most, 300) + 1))  # (the bins the call counts into)
            n = 0 if not wide and self._pick("bincount_empty", [False] * 5 + [True]) else int(rng.integers(1, SMALL_ELEMENTS // 2))
            if how == "above" and n:  # (a minlength above the maximum: the data stays 17 below the drawn number of bins)
                bins = max(bins - 17, 1)
        minlength = {"zero": 0, "below": bins // 2, "above": bins + 17}[how]
        return {"op": "bincount", "dtype": dtype, "n": n, "bins": bins, "minlength": minlength, "num_bins": max(bins, minlength) if n else minlength,
                "weights": weights, "value_class": self._pick("class", ["exact", "general"]) if weights else "count", "layout": self._layout([n]),
                "w_layout": self._layout([n])}

    def _histc(self, dtype: str) -> dict:
        rng = self.rng
        rule = self._pick("histc_range", ["exact", "explicit", "data", "constant"])
        shape = self._any_shape(int(rng.integers(1, SMALL_ELEMENTS // 2)) if rule in ("data", "constant") or rng.integers(6) else 0)
        case = {"op": "histc", "dtype": dtype, "shape": shape, "layout": self._layout(shape), "value_class": "general"}
        if rule == "exact":  # integer-valued data, lo = 0, hi = 2^k, a power of two of bins: every operation of the rule is exact
            k = int(rng.integers(3, 8))
            case.update(bins=1 << int(rng.integers(0, k + 1)), lo=0.0, hi=float(1 << k), range="explicit", nans="none", value_class="exact")
            return case
        lo = round(float(rng.uniform(-3, 0)), 3)
        lo, hi = (lo, lo + round(float(rng.uniform(0.5, 4)), 3)) if rule == "explicit" else (0.0, 0.0)
        case.update(bins=self._bins(4), lo=lo, hi=hi, range=rule,
                    nans=self._pick("nans", NAN_KINDS) if rule == "explicit" else "none")
        return case

    def _histogram(self, dtype: str) -> dict:
        rng = self.rng
        weight = self._turn("histogram_weight", [True, False])
        # the edge tensor's length bins + 1 on both sides of where a sequence leaves the search's LDS tier: the cut - 1, + 0, + 1
        step = self._pick("histogram_edges_" + dtype, [-2, -1, 0] + ([None] if dtype == "float64" else []))
        bins = self.t.search[dtype][0] + step if step is not None else int(rng.integers(1, 3 * self.t.bincount[4]))
        n = self.t.search[dtype][2] + int(rng.integers(-1, 2)) if rng.integers(3) == 0 else int(rng.integers(1, SMALL_ELEMENTS))
        if dtype == "float64" and rng.integers(6) == 0:
            n = 0
        shape = self._any_shape(n)
        kind = self._pick("histogram_bins", ["int", "int_range", "edges"])
        case = {"op": "histogram", "dtype": dtype, "shape": shape, "layout": self._layout(shape), "bins": bins, "bins_kind": kind, "weight": weight,
                "w_layout": self._layout(shape), "value_class": self._turn("class_histogram", ["general", "exact"]) if weight else "count"}
        if kind == "int_range":
            lo = round(float(rng.uniform(-2, 0)), 2)
            case["range"] = [lo, lo + round(float(rng.uniform(0.5, 3)), 2)]
        return case

    def _any_shape(self, n: int) -> list:
        """A 1-D to 3-D shape of n elements (about: n rounded down to a multiple of the leading sizes)."""
        rng = self.rng
        if n < 2 or rng.integers(2):
            return [n]
        a = int(rng.integers(1, 5))
        return [a, n // a] if rng.integers(2) else [a, 1, n // a]

    # -- reductions -------------------------------------------------------------------------------------------------------------
    def _reduce_class(self, op: str, dtype: str, reduce: str) -> str:
        if reduce in ("max", "min", "amax", "amin"):
            return "any"
        return "wrap" if dtype not in FLOATS else self._turn("class_" + op, ["general", "exact"])

    def _segment_reduce(self, dtype: str, longest=None) -> dict:
        rng = self.rng
        large = longest is not None
        # (planned, not shuffled: a round has two regular float cases -- the large ones take float16 and bfloat16 --, two integer ones and
        # three or four large ones: sum and prod, mean and max, min)
        if large:
            reduce = self._turn("segment_reduce_large", ["min", "max"])
        elif dtype in FLOATS:
            reduce = self._turn("segment_reduce_float", ["sum", "prod", "mean", "max", "min"])
        else:
            reduce = self._turn("segment_reduce_int", ["mean", "max", "sum", "min", "prod"])
        if large and dtype in ("float16", "bfloat16") and reduce in ("sum", "mean"):
            reduce = "prod"  # (no sum of so many 16-bit terms is in either value class)
        cls = self._reduce_class("segment_reduce", dtype, reduce)
        if large and dtype in ("float16", "bfloat16") and reduce == "prod":
            cls = "exact"
        initial = self._pick("initial", [None, 2])
        capped = cls in ("exact", "general") and not (cls == "exact" and reduce == "prod")
        cap = terms_cap(dtype, cls, 1, 2) if capped else 1 << 40
        if longest is None:  # (the cut's edges are drawn only where the value class of this dtype holds so many terms)
            longest = int(rng.integers(1, min(cap, 20000) + 1))
            if cap > self.t.reduce_levels[0] + 1 and rng.integers(8):
                longest = self.t.reduce_levels[0] + self._pick("segment_edge", [-1, 0, 1])
        longest = min(longest, cap)
        num_segments = int(rng.integers(1, 5 if large else 200))
        seed = self._seed()
        n = int(segment_lengths(num_segments, longest, seed).sum())
        width = max(1, min(40, SMALL_ELEMENTS // n)) if not large else 1
        tail = [[], [1], [int(rng.integers(2, width + 1))] if width >= 2 else [], [2, 2] if width >= 4 else []][int(rng.integers(4))]
        shape = [n] + tail
        return {"op": "segment_reduce", "dtype": dtype, "shape": shape, "layout": self._layout(shape), "reduce": reduce, "initial": initial,
                "bounds": self._pick("bounds", ["lengths", "offsets"]), "bounds_dtype": self._pick("index_dtype", ["int32", "int64"]), "num_segments": num_segments,
                "longest": longest, "lengths_seed": seed, "value_class": cls}

    def _by_destination(self, op: str, dtype: str, n=None, M=None, dest=None) -> dict:
        rng, t = self.rng, self.t
        reduce = "sum"
        if op != "index_add":
            names = (["sum"] if op == "scatter_reduce" else []) + ["prod", "mean", "amax", "amin"]
            reduce = self._turn(op + "_float", names) if dtype in FLOATS else self._turn(op + "_int", names[::-1])
        cls = self._reduce_class(op, dtype, reduce)
        alpha = self._pick("alpha", [1, 2]) if op == "index_add" else 1
        include_self = True if op == "index_add" else self._pick("include_self", [True, False])
        large = n is not None
        if large:
            if dtype == "float32":
                cls = "exact"  # (millions of float32 terms to one destination: t * u < 0.1 does not hold)
            shape, dim = [M], 0
        else:
            # (a general sum or product: several terms to one destination, which is what its bound is about)
            dest = self._pick("destinations_general", ["equal", "zipf"]) if cls == "general" else self._pick("destinations", DESTINATIONS)
            n = self._short_or("contributions", t.form_cuts[4, 1] + [t.search["int32"][0]], SMALL_ELEMENTS // 2)
            size = self._pick("destination_count", ["few", "some", "index_edge"])
            M = {"few": int(rng.integers(1, 51)), "some": int(rng.integers(51, 5000)), "index_edge": t.search["int32"][2] + self._pick("index_edge", [-1, 0, 1]) - 1}[size]
            if dest != "distinct" and cls in ("exact", "general") and not (cls == "exact" and reduce == "prod") and n > terms_cap(dtype, cls, 2, 4):
                # more terms to one destination than the value class of this dtype holds: in turn, as many as it holds, or distinct destinations
                if self._pick("too_many_terms", ["fewer", "distinct"]) == "fewer":
                    n = max(2, terms_cap(dtype, cls, 2, 4))
                else:
                    dest = "distinct"
            if dest == "distinct":
                M = max(M, n)
            width = max(1, min(8, SMALL_ELEMENTS // max(M, n)))
            other = [] if op == "scatter_reduce" or width < 2 else [[], [int(rng.integers(1, width + 1))], [2, width // 2] if width >= 4 else [1]][int(rng.integers(3))]
            dim = int(rng.integers(len(other) + 1))
            shape = other[:dim] + [M] + other[dim:]
        source_shape = shape[:dim] + [n + (self._pick("src_extra", [0, 3]) if op == "scatter_reduce" else 0)] + shape[dim + 1:]
        return {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "layout": self._layout(shape), "source_shape": source_shape,
                "source_layout": self._layout(source_shape), "n": n, "M": M, "destinations": dest, "index_dtype": self._pick("index_dtype", ["int32", "int64"]),
                "index_layout": self._layout([n]), "reduce": reduce, "include_self": include_self, "alpha": alpha, "value_class": cls}

    # -- scans ------------------------------------------------------------------------------------------------------------------
    def _scan(self, op: str, dtype: str, length=None, target="draw") -> dict:
        rng = self.rng
        arith = op in ("cumsum", "cumprod")
        if target == "draw":
            target = self._pick("target_" + dtype, SCAN_TARGETS[dtype]) if arith else None
        out = target or (dtype if dtype in FLOATS or not arith else "int64")
        cls = "any" if not arith else "wrap" if out not in FLOATS else self._pick("class_" + op, ["general", "exact"])
        if length is None:
            kernel_in = dtype if dtype != "bool" else "uint8"
            cuts = self.t.scan_cuts("int32", "int64", op)[:1] if arith else self.t.scan_cuts(kernel_in, kernel_in, op)[:1]
            length = self._short_or("scan", cuts + [self.t.scan_levels[0]], SMALL_ELEMENTS // 2)
            if cls in ("exact", "general") and not (cls == "exact" and op == "cumprod"):
                length = min(length, terms_cap(out, cls, 1, 1))
            shape, dim = self._rows_shape(length)
            if rng.integers(16) == 0:
                shape, dim = [[0], [3, 0], [0, 4]][int(rng.integers(3))], 0
        else:
            shape, dim = [length], 0
        return {"op": op, "dtype": dtype, "shape": shape, "dim": dim, "layout": self._layout(shape), "out_dtype": target, "value_class": cls,
                "dist": self._value_dist(dtype)}

    # -- compaction -------------------------------------------------------------------------------------------------------------
    def _tiles(self, cap: int = SMALL_ELEMENTS) -> int:
        tile = self.t.compact_tile
        return self._short_or("compact", [tile, 2 * tile, 5 * tile], cap)

    def _compact(self, op: str, dtype: str, n=None) -> dict:
        rng = self.rng
        case = {"op": op, "dtype": dtype, "mask_class": self._pick("mask", MASK_CLASSES), "dist": self._value_dist(dtype)}
        large = n is not None
        if op in ("nonzero", "argwhere", "count_nonzero"):
            shape = [n] if large else self._any_shape(self._tiles()) if rng.integers(12) else [[], [0], [2, 0]][int(rng.integers(3))]
            case.update(shape=shape, layout=self._layout(shape))
            if op == "nonzero":
                case["as_tuple"] = self._pick("as_tuple", [False, True])
        elif op in ("masked_select", "masked_scatter"):
            n = n or self._tiles()
            a = 1 if large else int(rng.integers(1, 5))
            full = [a, max(n // a, 1)]
            how = "same" if large else self._pick("broadcast", ["same", "mask", "x", "same"])
            lower = [1, full[1]] if rng.integers(2) else [full[0], 1]
            case.update(shape=lower if how == "x" else full, mask_shape=lower if how == "mask" else full, broadcast=how)
            case.update(layout=self._layout(case["shape"]), mask_layout=self._layout(case["mask_shape"]))
        else:
            width = self._pick("row_width", ROW_WIDTHS)
            rows = max(1, min(self._tiles(), SMALL_ELEMENTS // width))
            lead = [rows] if self._pick("mask_dims", [1, 2]) == 1 else [int(rng.integers(1, 4)), max(rows // 3, 1)]
            tail = {1: [[], [1]], 3: [[3]], 4: [[4], [2, 2]], 1025: [[1025], [5, 205]]}[width]
            shape = lead + tail[int(rng.integers(len(tail)))]
            case.update(shape=shape, mask_shape=lead, row_width=width, layout=self._layout(shape), mask_layout=self._layout(lead))
            if op == "mask_index_put":
                case["values"] = self._pick("put_values", ["exact", "broadcast", "scalar"])
        return case

    # -- the large minority -----------------------------------------------------------------------------------------------------
    def _large_newer(self) -> list:
        rng, t = self.rng, self.t
        kind = self.large_newer.draw()
        draw = lambda op, dtypes=None: self.new_op_dtype.draw(lambda p: p[0] == op and (dtypes is None or p[1] in dtypes))[1]  # noqa: E731
        pool_min = t.pool_min_pairs or t.pool_min  # (pairs reach the pool form only above the cap: the bare keys' minimum stands in)
        if kind == "index_add_skewed":
            n = int(rng.integers(pool_min + 2, min(pool_min * 5 // 4, LARGE_ELEMENTS)))
            dtype = self._preferred("index_add", ("int32", "int64"), ("int32", "int64", "float32", "float64"))
            case = self._by_destination("index_add", dtype, n=n, M=int(rng.integers(2, 51)), dest="zipf")
        elif kind == "index_add_pool_edge":
            n = pool_min + self._pick("pool_edge", [-1, 0, 1])
            # (one term and the input to a destination: every dtype's sum is in its value class; float32 and float64 are left to the regular cases)
            dtype = self._preferred("index_add", ("float16", "bfloat16"), ("float16", "bfloat16", "int32", "int64"))
            case = self._by_destination("index_add", dtype, n=n, M=n + int(rng.integers(0, 100)), dest="distinct")
        elif kind == "cumsum_single_pass":
            dtype = self._preferred("cumsum", ("int32", "float32"))
            length = t.scan_cuts(dtype, dtype, "cumsum")[1] + self._pick("single_pass_edge", [-1, 0, 1])
            case = self._scan("cumsum", dtype, length=length, target="int32" if dtype == "int32" else None)
            if dtype == "float32":
                case["value_class"] = "exact"
        elif kind == "reduce_three_levels":
            # (float16 / bfloat16 first: no sum of so many of their terms is in a value class, so their regular cases cannot draw the cut's edges)
            case = self._segment_reduce(self._preferred("segment_reduce", ("float16", "bfloat16"), ("int32", "int64")), longest=t.reduce_levels[1] + self._pick("level_edge", [-1, 0, 1]))
        elif kind == "kthvalue_grid":
            dtype = draw("kthvalue")
            case = self._select("kthvalue", dtype, length=t.select[dtype][1] + self._pick("grid_edge", [-1, 0, 1, 1000]))
        elif kind == "quantile_grid":
            op = self._pick("quantile_grid", list(QUANTILE_OPS))
            dtype = draw(op)
            case = self._quantile(op, dtype, length=t.select[dtype][1] + self._pick("grid_edge", [-1, 0, 1, 1000]))
        elif kind == "bincount_global":
            case = self._bincount(["int32", "int64"][int(rng.integers(2))], bins=1 << 20, n=int(rng.integers(1 << 20, 1 << 21)))
        elif kind == "masked_select_large":
            case = self._compact("masked_select", draw("masked_select"), n=LARGE_ELEMENTS)
        else:
            case = self._compact("nonzero", draw("nonzero"), n=LARGE_ELEMENTS)
        return self._done(case, "large:" + kind)

    def _next(self) -> list:
        window, at = divmod(self._index, self.window)
        if self._index % LARGE_EVERY == LARGE_AT:
            return self._large_newer()
        if window % 2 == 0 and at == 0:
            return self._pending_sort()
        if window % 2 == 1 and at == self.window - 1:
            return self._neighbour()
        return self._regular()

    def _regular(self) -> list:
        """The next (op, dtype) of the newer ops' deck as a case."""
        op, dtype = self.new_op_dtype.draw()
        if op in SELECT_OPS:
            case = self._select(op, dtype)
        elif op in QUANTILE_OPS:
            case = self._quantile(op, dtype)
        elif op in COUNT_OPS:
            case = {"bincount": self._bincount, "histc": self._histc, "histogram": self._histogram}[op](dtype)
        elif op == "segment_reduce":
            case = self._segment_reduce(dtype)
        elif op in REDUCE_OPS:
            case = self._by_destination(op, dtype)
        elif op in SCAN_OPS:
            case = self._scan(op, dtype)
        else:
            case = self._compact(op, dtype)
        return self._done(case)


def _numel(shape) -> int:
    out = 1
    for v in shape:
        out *= v
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the newer deck: its inputs (torch on the CPU and numpy; nothing of the library)

def newer_values(name: str, shape, kind: str, seed: int):
    """A contiguous CPU tensor of `shape`: a distribution of make_values, or "small_ints" (-1, 0, 1: exact sums), "signs" (+-1: exact
    products), "normal" (finite, general sums), "near_one" (general products), "counts" (0 .. 100).  bool: random bits whatever the kind."""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = list(shape)
    unsigned = name in ("uint8", "bool")
    if name == "bool":
        return torch.from_numpy(rng.integers(0, 2, size=shape).astype(np.bool_))
    if kind == "small_ints":
        return torch.from_numpy(rng.integers(0 if unsigned else -1, 2, size=shape)).to(torch_dtype(name))
    if kind == "signs":
        return torch.from_numpy(np.ones(shape, dtype=np.int64) if unsigned else rng.integers(0, 2, size=shape) * 2 - 1).to(torch_dtype(name))
    if kind == "normal":
        if name in FLOATS:
            return torch.from_numpy(rng.standard_normal(shape)).to(torch_dtype(name))
        return torch.from_numpy(rng.integers(0 if unsigned else -50, 51, size=shape)).to(torch_dtype(name))
    if kind.startswith("near_one"):
        if name in FLOATS:
            terms = int(kind.split(":")[1]) if ":" in kind else 20
            return torch.from_numpy(1.0 + np.clip(rng.standard_normal(shape), -5, 5) / terms).to(torch_dtype(name))
        return torch.from_numpy(rng.integers(0, 2, size=shape) * 2 + (1 if unsigned else -1)).to(torch_dtype(name))  # (odd: a wrapping product is never 0)
    return make_values(name, shape, kind, seed)


def put_nans(t, dim, kind: str, seed: int):
    """NaNs of `kind` (NAN_KINDS) into the float tensor t, whose rows run along dim (None: all of it one row)."""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    if kind == "none" or not t.dtype.is_floating_point or t.numel() == 0:
        return t
    rows = t.reshape(1, -1) if dim is None or t.dim() == 0 else t.movedim(dim, -1).reshape(-1, t.shape[dim])
    rows = rows.clone()
    R, L = rows.shape
    for r in rng.integers(0, R, size=max(1, R // 3)):
        rows[int(r), torch.from_numpy(rng.integers(0, L, size=int(rng.integers(1, 4))))] = float("nan")
    if kind == "row" and R > 1:
        rows[int(rng.integers(R))] = float("nan")
    if dim is None or t.dim() == 0:
        return rows.reshape(t.shape)
    moved = t.movedim(dim, -1)
    return rows.reshape(moved.shape).movedim(-1, dim).contiguous()


def make_mask(shape, cls: str, seed: int, tile: int):
    """A bool CPU tensor of `shape` of one of MASK_CLASSES."""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed + 11))
    n = _numel(shape)
    if cls in ("none", "all"):
        flat = np.full(n, cls == "all")
    elif cls in ("sparse", "half"):
        flat = rng.random(n) < (1 / 64 if cls == "sparse" else 0.5)
    else:  # set in one tile only
        flat = np.zeros(n, dtype=bool)
        first = int(rng.integers(0, max(-(-n // tile), 1))) * tile
        flat[first:first + tile] = rng.random(len(flat[first:first + tile])) < 0.5
    return torch.from_numpy(flat.astype(np.bool_)).reshape(list(shape))


def _sum_kind(case: dict, product: bool) -> str:
    cls = case["value_class"]
    if product:  # (general: factors 1 + z / t for a product of up to t terms, so that it stays within e^+-5 whatever the layout repeats)
        if case["op"] == "segment_reduce":
            most = case["longest"]
        elif case["op"] in SCAN_OPS:
            most = case["shape"][case["dim"]] if _numel(case["shape"]) else 1
        else:
            most = case["n"]
        return {"exact": "signs", "general": f"near_one:{most + 1}", "wrap": "near_one"}.get(cls, "uniform")
    return {"exact": "small_ints", "general": "normal", "wrap": "uniform"}.get(cls, "uniform")


def destinations(kind: str, n: int, M: int, seed: int):
    """n destinations in [0, M): all equal, distinct, or Zipf-like (destination 0 takes most, the far ones stay untouched)."""
    rng = np.random.Generator(np.random.PCG64(seed + 13))
    if kind == "equal":
        return np.full(n, M // 3, dtype=np.int64)
    if kind == "distinct":
        return rng.permutation(M)[:n].astype(np.int64)
    return np.minimum(rng.zipf(1.3, n) - 1, M - 1).astype(np.int64)


def newer_inputs(case: dict) -> dict:
    """name -> (base, view) as lay_out gives them, or a plain Python value: the inputs of a case of the newer ops, on the CPU."""
    import torch
    op, dtype, seed = case["op"], case["dtype"], case["data_seed"]
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    tile = thresholds().compact_tile
    out = {}

    def laid(name, shape, layout, fill):
        out[name] = lay_out(shape, layout, fill)

    if op in SELECT_OPS or op in QUANTILE_OPS:
        dim = case["dim"]
        laid("x", case["shape"], case["layout"], lambda s: put_nans(newer_values(dtype, s, case["dist"], seed), dim, case["nans"], seed))
        if op in QUANTILE_OPS and case["q_kind"] != "float":
            q = torch.tensor(case["qs"], dtype=torch_dtype(dtype))
            out["q"] = (q.reshape(()) if case["q_kind"] == "0d" else q, lambda t: t)
    elif op == "bincount":
        n, bins = case["n"], case["bins"]

        def index(s):
            x = rng.integers(0, bins, size=s[0])
            x[rng.random(s[0]) < 0.3] = int(rng.integers(bins))  # (one hot bin)
            if s[0]:
                x[int(rng.integers(s[0]))] = bins - 1
            return torch.from_numpy(x).to(torch_dtype(dtype))

        laid("x", [n], case["layout"], index)
        if case["weights"]:
            laid("w", [n], case["w_layout"], lambda s: newer_values(case["weights"], s, _sum_kind(case, False), seed + 1))
    elif op == "histc":
        def data(s):
            if case["value_class"] == "exact":
                return torch.from_numpy(rng.integers(-2, int(case["hi"]) + 3, size=s)).to(torch_dtype(dtype))
            if case["range"] == "constant":
                return torch.full(s, 1.5, dtype=torch_dtype(dtype))
            return put_nans(newer_values(dtype, s, "normal", seed), None, case["nans"], seed)

        laid("x", case["shape"], case["layout"], data)
    elif op == "histogram":
        kind = case["bins_kind"]
        edges = None
        if kind == "edges":
            steps = torch.from_numpy(np.abs(rng.standard_normal(case["bins"] + 1)) + 0.01)
            edges = ((torch.cumsum(steps, 0) - steps.sum() / 2) * (6.0 / steps.sum())).to(torch_dtype(dtype))
            out["edges"] = (edges, lambda t: t)

        def data(s):
            x = newer_values(dtype, s, "normal", seed)
            marks = edges if edges is not None else torch.tensor(case["range"], dtype=x.dtype) if kind == "int_range" else None
            if marks is not None and x.numel():  # a quarter of the elements exactly on an edge, the first and the last edge among them
                hits = marks[torch.from_numpy(rng.integers(0, marks.numel(), size=x.numel()))].reshape(x.shape)
                hits.reshape(-1)[:2] = marks[[0, -1]][:x.numel()]
                x = torch.where(torch.from_numpy(rng.random(x.numel()) < 0.25).reshape(x.shape) | (torch.arange(x.numel()).reshape(x.shape) < 2), hits, x)
            return x

        laid("x", case["shape"], case["layout"], data)
        if case["weight"]:
            laid("w", case["shape"], case["w_layout"], lambda s: newer_values(dtype, s, _sum_kind(case, False), seed + 1))
    elif op == "segment_reduce":
        laid("x", case["shape"], case["layout"], lambda s: newer_values(dtype, s, _sum_kind(case, case["reduce"] == "prod"), seed))
        lengths = torch.from_numpy(segment_lengths(case["num_segments"], case["longest"], case["lengths_seed"]))
        bounds = lengths if case["bounds"] == "lengths" else torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)))
        out["bounds"] = (bounds.to(torch_dtype(case["bounds_dtype"])), lambda t: t)
    elif op in REDUCE_OPS:
        product = case["reduce"] == "prod"
        base_kind = "signs" if product and case["value_class"] == "exact" else "counts4" if case["value_class"] == "exact" else _sum_kind(case, product)

        def base(s):
            if base_kind == "counts4":
                return torch.from_numpy(rng.integers(0 if dtype == "uint8" else -4, 5, size=s)).to(torch_dtype(dtype))
            return newer_values(dtype, s, base_kind, seed + 2)

        laid("x", case["shape"], case["layout"], base)
        laid("source", case["source_shape"], case["source_layout"], lambda s: newer_values(dtype, s, _sum_kind(case, product), seed))
        laid("index", [case["n"]], case["index_layout"],
             lambda s: torch.from_numpy(destinations(case["destinations"], case["n"], case["M"], seed)).to(torch_dtype(case["index_dtype"])))
    elif op in SCAN_OPS:
        kind = case["dist"] if case["value_class"] == "any" else _sum_kind(case, op == "cumprod")
        laid("x", case["shape"], case["layout"], lambda s: newer_values(dtype, s, kind, seed))
    elif op in ("nonzero", "argwhere", "count_nonzero"):
        def flags(s):
            x = newer_values(dtype, s, case["dist"], seed)
            keep = make_mask(s, case["mask_class"], seed, tile)
            x = torch.where(keep, x, torch.zeros((), dtype=x.dtype))
            if x.dtype.is_floating_point:  # (-0.0 is zero)
                x = torch.where(~keep & torch.from_numpy(rng.random(_numel(s)) < 0.1).reshape(s), torch.full((), -0.0, dtype=x.dtype), x)
            return x

        laid("x", case["shape"], case["layout"], flags)
    else:
        laid("x", case["shape"], case["layout"], lambda s: newer_values(dtype, s, case["dist"], seed))
        laid("mask", case["mask_shape"], case["mask_layout"], lambda s: make_mask(s, case["mask_class"], seed, tile))
        base, view = out["mask"]
        mask = view(base)
        if op == "masked_scatter":
            R = int(torch.broadcast_tensors(mask, torch.empty(case["shape"]))[0].sum())
            out["source"] = (newer_values(dtype, [R + int(rng.integers(0, 3))], case["dist"], seed + 1), lambda t: t)
        elif op == "mask_index_put":
            tail = case["shape"][len(case["mask_shape"]):]
            shape = {"exact": [int(mask.sum())] + tail, "broadcast": [[1] + tail, tail][int(rng.integers(2))], "scalar": []}[case["values"]]
            out["values"] = (newer_values(dtype, shape, case["dist"], seed + 1), lambda t: t)
    return out


def call_newer(api, case: dict, t: dict):
    """The one public call of a case of the newer ops on `api`: this library, or anything with the same functions."""
    op = case["op"]
    if op == "kthvalue":
        return api.kthvalue(t["x"], case["k"], case["dim"], case["keepdim"])
    if op in ("median", "nanmedian"):
        return getattr(api, op)(t["x"]) if case["dim"] is None else getattr(api, op)(t["x"], case["dim"], case["keepdim"])
    if op in QUANTILE_OPS:
        q = case["qs"][0] if case["q_kind"] == "float" else t["q"]
        return getattr(api, op)(t["x"], q, case["dim"], case["keepdim"], interpolation=case["interpolation"])
    if op == "bincount":
        return api.bincount(t["x"], weights=t.get("w"), minlength=case["minlength"])
    if op == "histc":
        return api.histc(t["x"], bins=case["bins"], min=case["lo"], max=case["hi"])
    if op == "histogram":
        bins = t["edges"] if case["bins_kind"] == "edges" else case["bins"]
        return api.histogram(t["x"], bins, range=tuple(case["range"]) if "range" in case else None, weight=t.get("w"))
    if op == "segment_reduce":
        return api.segment_reduce(t["x"], case["reduce"], **{case["bounds"]: t["bounds"]}, initial=case["initial"])
    if op == "index_add":
        return api.index_add(t["x"], case["dim"], t["index"], t["source"], alpha=case["alpha"])
    if op == "index_reduce":
        return api.index_reduce(t["x"], case["dim"], t["index"], t["source"], case["reduce"], include_self=case["include_self"])
    if op == "scatter_reduce":
        return api.scatter_reduce(t["x"], 0, t["index"], t["source"], case["reduce"], include_self=case["include_self"])
    if op in ("cumsum", "cumprod"):
        return getattr(api, op)(t["x"], case["dim"], dtype=torch_dtype(case["out_dtype"]) if case["out_dtype"] else None)
    if op in ("cummax", "cummin"):
        return getattr(api, op)(t["x"], case["dim"])
    if op == "nonzero":
        return api.nonzero(t["x"], as_tuple=case["as_tuple"])
    if op in ("argwhere", "count_nonzero"):
        return getattr(api, op)(t["x"])
    if op == "masked_select":
        return api.masked_select(t["x"], t["mask"])
    if op == "masked_scatter":
        return api.masked_scatter(t["x"], t["mask"], t["source"])
    if op == "mask_index":
        return api.mask_index(t["x"], t["mask"])
    return api.mask_index_put(t["x"], t["mask"], t["values"])


# ------------------------------------------------------------------------------------------------------------------------------
# the newer deck: its references (torch's CPU functions and numpy only) and the rules they are compared by

class Want:
    """One expected output: `rule` says how the returned tensor is held to `want`.
       bits      the same dtype, shape and bits; for floats a NaN on both sides counts as equal
       value     the same dtype and shape, == or NaN on both sides, and the same bits wherever `want` is neither zero nor NaN (the sign
                 of a zero that an order leaves open: kthvalue's tie of -0.0 and +0.0, a maximum of the two, quantile's +0.0)
       bound     the same dtype and shape, NaN where `want` (float64) is, and |returned - want| <= bound
       index     int64 positions into `rows` along `dim`, in range, at which `rows` holds the returned values' bits (`values_at`: which output)"""

    def __init__(self, name, want, rule="bits", **more):
        self.name, self.want, self.rule = name, want, rule
        self.__dict__.update(more)


def as_count(counts, dtype):
    """Integer counts (numpy) as a CPU tensor of the dtype, each the correctly rounded count."""
    import torch
    counts = np.asarray(counts, dtype=np.int64)
    if dtype == torch.int64:
        return torch.from_numpy(counts)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return torch.from_numpy(counts.astype(np.float64).astype(np.float16))  # (exact in float64, then one rounding)
    if dtype == torch.bfloat16:
        assert counts.max(initial=0) < 1 << 24  # (exact in float32, then one rounding)
        return torch.from_numpy(counts.astype(np.float32)).to(torch.bfloat16)
    return torch.from_numpy(counts.astype(np.float32 if dtype == torch.float32 else np.float64))


def _signed_view(t):
    import torch
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _sum_wants(name, exact64, mass64, terms, dtype, value_class, same_dtype, divisor=None):
    """A float sum as a Want: exact class `same_dtype` (torch's own result in the dtype) under ==; general class the float64 sum within
    (t + 1) u sum|x| (a mean: that over the divisor, and one more u)."""
    import torch
    if value_class != "general":
        return Want(name, same_dtype, "value")
    u = EPS[str(dtype).split(".")[1]]
    bound = (terms.double() + 1) * u * mass64
    if divisor is not None:
        d = divisor.double().clamp(min=1)
        bound = (terms.double() + 2) * u * mass64 / d
    return Want(name, exact64, "bound", bound=bound, dtype=dtype)


def _select_reference(case, x):
    import torch
    op, dim = case["op"], case["dim"]
    flat = x.reshape(-1) if dim is None else x
    d = 0 if dim is None else dim
    order = torch.sort(flat, dim=d, stable=True)
    L = flat.shape[d]
    nans = torch.isnan(flat).sum(d, keepdim=True) if flat.dtype.is_floating_point else torch.zeros_like(order.indices.narrow(d, 0, 1))
    if op == "kthvalue":
        j = torch.full_like(nans, case["k"] - 1)
    elif op == "median":
        j = torch.where(nans > 0, L - nans, torch.full_like(nans, (L - 1) // 2))
    else:
        j = torch.where(nans < L, (L - nans - 1) // 2, torch.zeros_like(nans))
    idx = order.indices.gather(d, j)
    val = _signed_view(flat).gather(d, idx).view(flat.dtype)
    srt = order.values
    free = ((srt.narrow(d, 1, L - 1) != srt.narrow(d, 0, L - 1)).all(d, keepdim=True) if L > 1 else torch.ones_like(nans, dtype=torch.bool)) & (nans == 0)
    if dim is None:
        return [Want("values", val.reshape(()), "value")]
    keep = (lambda t: t) if case["keepdim"] else (lambda t: t.squeeze(d))
    theirs = getattr(torch, op)(flat, *((case["k"],) if op == "kthvalue" else ()), d, True).indices
    return [Want("values", keep(val), "value"),
            Want("indices", keep(idx), "index", rows=flat, dim=d, keepdim=case["keepdim"], values_at=0, free=keep(free), theirs=keep(theirs))]


def _histc_rule(x, bins: int, lo: float, hi: float):
    """The rule of histc's docstring in numpy: bin = (int)((x - lo) * bins / (hi - lo)), each operation rounded on its own, in float32
    (float64 for float64); bin == bins goes to the last bin; x < lo, x > hi and NaN are not counted."""
    import torch
    F = np.float64 if x.dtype == torch.float64 else np.float32
    xs = x.to(torch.float64 if F is np.float64 else torch.float32).reshape(-1).numpy()
    lo, hi = F(lo), F(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = xs[(xs >= lo) & (xs <= hi)]
        q = ((xs - lo) * F(bins)) / (hi - lo)
        at = np.where(q < F(4294967296.0), q, F(0)).astype(np.int64)
        at = np.where(q < F(4294967296.0), np.minimum(at, bins - 1), bins - 1)
    return np.bincount(at, minlength=bins)


def _bin_sums(at, bins: int, w, case, dtype, name):
    """Counts (no weights) or weighted sums per bin as a Want; `at`: numpy bin numbers, already filtered, w: the matching weights."""
    import torch
    counts = np.bincount(at, minlength=bins)
    if w is None:
        return Want(name, as_count(counts, dtype), "bits")
    w64 = w.double().numpy()
    exact = torch.from_numpy(np.bincount(at, weights=w64, minlength=bins))
    mass = torch.from_numpy(np.bincount(at, weights=np.abs(w64), minlength=bins))
    return _sum_wants(name, exact, mass, torch.from_numpy(counts), dtype, case["value_class"], exact.to(dtype))


def _segment_ints(x, lengths, reduce: str, initial):
    """segment_reduce of int32 / int64 rows in numpy, as the wrapper documents it: sums and products wrap, an empty max / min answers the
    type's minimum / maximum, the mean is floored and 0 for an empty segment."""
    import torch
    info = np.iinfo(np.int32 if x.dtype == torch.int32 else np.int64)
    rows = x.reshape(x.shape[0], -1).numpy()
    out = np.empty((len(lengths), rows.shape[1]), dtype=rows.dtype)
    at = 0
    with np.errstate(over="ignore"):
        for i, n in enumerate(lengths):
            part = rows[at:at + n]
            at += n
            if reduce in ("sum", "mean"):
                v = part.sum(0, dtype=rows.dtype) + rows.dtype.type(initial or 0)
                out[i] = v // max(n, 1) if reduce == "mean" else v
            elif reduce == "prod":
                out[i] = part.prod(0, dtype=rows.dtype) * rows.dtype.type(1 if initial is None else initial)
            else:
                start = (info.min if reduce == "max" else info.max) if initial is None else initial
                out[i] = (np.maximum if reduce == "max" else np.minimum)(part.max(0, initial=info.min) if reduce == "max" else part.min(0, initial=info.max), start)
    return torch.from_numpy(out).reshape((len(lengths),) + tuple(x.shape[1:]))


def reference_newer(case: dict, cpu: dict, got=None) -> list:
    """The expected outputs of a case of the newer ops, in the order the call returns them: a list of Want.  `got` (the returned CPU
    tensors) is read only where the expectation hangs on an output that is torch's and not a kernel's: histogram's linspace edges."""
    import torch
    op = case["op"]
    x = cpu["x"].contiguous()
    dtype = x.dtype
    if op in SELECT_OPS:
        return _select_reference(case, x)
    if op in QUANTILE_OPS:
        fn, q = getattr(torch, op), (case["qs"][0] if case["q_kind"] == "float" else cpu["q"])
        want = fn(x, q, case["dim"], case["keepdim"], interpolation=case["interpolation"])
        if case["interpolation"] in ("lower", "higher", "nearest"):
            return [Want("quantiles", want, "value")]
        lo, hi = (fn(x, q, case["dim"], case["keepdim"], interpolation=i) for i in ("lower", "higher"))
        bound = 4 * EPS[case["dtype"]] * torch.maximum(lo.abs(), hi.abs()).double()
        return [Want("quantiles", want.double(), "bound", bound=torch.where(torch.isnan(bound), torch.zeros_like(bound), bound), dtype=dtype, nan_as=want)]
    if op == "bincount":
        w = cpu.get("w")
        if w is not None and w.dtype not in (torch.float32, torch.float64):
            w = w.double()
        out = torch.int64 if w is None else w.dtype
        return [_bin_sums(x.numpy().astype(np.int64), case["num_bins"], w.contiguous() if w is not None else None, case, out, "counts")]
    if op == "histc":
        lo, hi = case["lo"], case["hi"]
        if lo == hi and x.numel():
            lo, hi = float(x.min()), float(x.max())
        if lo == hi:
            lo, hi = lo - 1.0, hi + 1.0
        return [Want("counts", as_count(_histc_rule(x, case["bins"], lo, hi), dtype), "bits")]
    if op == "histogram":
        bins = case["bins"]
        if case["bins_kind"] == "edges":
            edges, edge_want = cpu["edges"], Want("bin_edges", cpu["edges"], "bits")
        else:
            lo, hi = case["range"] if "range" in case else ((float(x.min()), float(x.max())) if x.numel() else (0.0, 1.0))
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            exact = torch.linspace(lo, hi, bins + 1, dtype=torch.float64)
            # (the edges are torch.linspace's on the device, not a kernel's: a step, a product and a sum, each rounded once)
            edge_want = Want("bin_edges", exact, "bound", bound=torch.full_like(exact, 4 * EPS[case["dtype"]] * max(abs(lo), abs(hi))), dtype=dtype)
            edges = got[1] if got is not None and len(got) > 1 and got[1].shape == exact.shape and got[1].dtype == dtype else exact.to(dtype)
        e, xs = edges.numpy(), x.reshape(-1).numpy()
        at = np.searchsorted(e, xs, side="right") - 1
        at = np.where(xs == e[-1], bins - 1, at)
        ok = (at >= 0) & (at < bins) & ~np.isnan(xs)
        w = cpu["w"].contiguous().reshape(-1)[torch.from_numpy(ok)] if "w" in cpu else None
        return [_bin_sums(at[ok], bins, w, case, dtype, "hist"), edge_want]
    if op == "segment_reduce":
        lengths = segment_lengths(case["num_segments"], case["longest"], case["lengths_seed"])
        reduce, initial, cls = case["reduce"], case["initial"], case["value_class"]
        kw = {case["bounds"]: cpu["bounds"].long()}
        if not dtype.is_floating_point:
            return [Want("out", _segment_ints(x, lengths, reduce, initial), "bits")]
        same = torch.segment_reduce(x, reduce, initial=initial, **kw)
        if cls != "general":
            return [Want("out", same, "value")]
        exact = torch.segment_reduce(x.double(), reduce, initial=initial, **kw)
        terms = torch.from_numpy(lengths + (initial is not None)).reshape((-1,) + (1,) * (x.dim() - 1))
        if reduce == "prod":
            return [_product_want("out", exact, terms, dtype)]
        mass = torch.segment_reduce(x.double().abs(), "sum", initial=abs(initial) if initial is not None else None, **kw)
        want = _sum_wants("out", exact, mass, terms, dtype, cls, same, torch.from_numpy(lengths).reshape(terms.shape) if reduce == "mean" else None)
        want.nan_as = same  # (a mean of no rows without an initial: NaN)
        return [want]
    if op in REDUCE_OPS:
        return [_by_destination_reference(case, x, cpu["index"].contiguous().long(), cpu["source"].contiguous())]
    if op in ("cumsum", "cumprod"):
        target = torch_dtype(case["out_dtype"]) if case["out_dtype"] else None
        same = getattr(torch, op)(x, case["dim"], dtype=target)
        if case["value_class"] != "general":
            return [Want("out", same, "value" if same.dtype.is_floating_point else "bits")]
        xt = x.to(same.dtype).double()
        exact = getattr(torch, op)(xt, case["dim"])
        terms = (torch.arange(x.shape[case["dim"]]) + 1).reshape([-1 if d == case["dim"] % x.dim() else 1 for d in range(x.dim())]).expand(x.shape)
        if op == "cumprod":
            return [_product_want("out", exact, terms, same.dtype)]
        return [_sum_wants("out", exact, torch.cumsum(xt.abs(), case["dim"]), terms, same.dtype, "general", same)]
    if op in ("cummax", "cummin"):
        values, indices = getattr(torch, op)(x, case["dim"])
        return [Want("values", values, "bits"), Want("indices", indices, "bits")]
    if op == "nonzero":
        r = torch.nonzero(x, as_tuple=case["as_tuple"])
        return [Want(f"dim {i}", c.contiguous(), "bits") for i, c in enumerate(r)] if case["as_tuple"] else [Want("coordinates", r, "bits")]
    if op == "argwhere":
        return [Want("coordinates", torch.argwhere(x), "bits")]
    if op == "count_nonzero":
        return [Want("count", torch.count_nonzero(x), "bits")]
    mask = cpu["mask"]
    if op == "masked_select":
        return [Want("selected", torch.masked_select(x, mask), "bits")]
    if op == "masked_scatter":
        full = torch.broadcast_tensors(x, mask)[0].contiguous()
        return [Want("out", full.masked_scatter(mask, cpu["source"]), "bits")]
    if op == "mask_index":
        return [Want("rows", x[mask], "bits")]
    return [Want("out", torch.index_put(x, (mask,), cpu["values"]), "bits")]


def _product_want(name, exact64, terms, dtype):
    """A float product of t terms: relative error at most t u / (1 - t u).  (The generator keeps a general product of t factors within
    e^+-5 of the first one, far from the dtype's denormals and from its largest value, where this bound would not hold.)"""
    tu = terms.double() * EPS[str(dtype).split(".")[1]]
    return Want(name, exact64, "bound", bound=(tu / (1 - tu)) * exact64.abs(), dtype=dtype)


def _by_destination_reference(case, x, index, source):
    import torch
    op, dim, reduce, cls = case["op"], case["dim"], case["reduce"], case["value_class"]
    include_self, alpha, M = case["include_self"], case["alpha"], case["M"]

    def run(base, src):
        if op == "index_add":
            return torch.index_add(base, dim, index, src, alpha=alpha)
        if op == "index_reduce":
            return torch.index_reduce(base, dim, index, src, reduce, include_self=include_self)
        return torch.scatter_reduce(base, 0, index, src[:index.numel()], reduce, include_self=include_self)

    if cls != "general":
        if reduce == "prod" and x.dtype in (torch.float16, torch.bfloat16):
            # (torch's CPU index_reduce fails an internal assertion on some 16-bit shapes; products of +-1 are exact in float32 as well)
            return Want("out", run(x.float(), source.float()).to(x.dtype), "value")
        return Want("out", run(x, source), "value" if x.dtype.is_floating_point else "bits")
    exact = run(x.double(), source.double())
    count = torch.bincount(index, minlength=M).reshape([-1 if d == dim else 1 for d in range(x.dim())])
    terms = (count + (1 if include_self else 0)).expand(x.shape)
    if reduce == "prod":
        return _product_want("out", exact, terms, x.dtype)
    src_abs = source.double().abs() * alpha
    if op == "scatter_reduce":
        mass = torch.scatter_reduce(x.double().abs(), 0, index, src_abs[:index.numel()], "sum", include_self=include_self)
    else:
        mass = torch.index_add(x.double().abs() if include_self else torch.where(count.expand(x.shape) > 0, 0.0, x.double().abs()), dim, index, src_abs)
    return _sum_wants("out", exact, mass, terms, x.dtype, cls, None, terms if reduce == "mean" else None)


def _hold(w: Want, g, got: list):
    """None when the returned tensor g meets the Want, else the line that says where it does not."""
    import torch
    want, rule = w.want, w.rule
    dtype = getattr(w, "dtype", want.dtype)
    if g.dtype != dtype or g.shape != want.shape:
        return f"{w.name}: {g.dtype} {tuple(g.shape)} returned, {dtype} {tuple(want.shape)} expected"
    if g.numel() == 0:
        return None

    def at(bad, what):
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        pos = tuple(int(i) for i in np.unravel_index(flat, tuple(g.shape))) if g.dim() else ()
        return (f"{w.name}: {what} at {pos} (flat {flat}) of {g.numel()}: returned {g.reshape(-1)[flat].item()!r}, expected "
                f"{want.reshape(-1)[flat].item()!r}; {int(bad.sum())} elements differ")

    if rule == "bits":
        if g.dtype.is_floating_point:
            both = torch.isnan(g) & torch.isnan(want)
            g = torch.where(both, torch.zeros_like(g), g)
            want = torch.where(both, torch.zeros_like(want), want)
        return _first_difference(w.name, g, want)
    if rule == "value":
        if not g.dtype.is_floating_point:
            return _first_difference(w.name, g, want)
        both = torch.isnan(g) & torch.isnan(want)
        bad = ~both & ~(g == want)
        plain = ~torch.isnan(want) & (want != 0)
        bad |= plain & (_signed_view(g) != _signed_view(want))
        return at(bad, "another value") if bool(bad.any()) else None
    if rule == "bound":
        nan_as = getattr(w, "nan_as", None)
        expect_nan = torch.isnan(nan_as) if nan_as is not None else torch.isnan(want)
        bad = torch.isnan(g) != expect_nan
        err = (g.double() - want).abs()
        inf = torch.isinf(want)
        bad |= ~expect_nan & torch.where(inf, g.double() != want, ~(err <= w.bound))
        if bool(bad.any()):
            flat = int(torch.nonzero(bad.reshape(-1))[0])
            return at(bad, f"beyond the bound {w.bound.reshape(-1)[flat].item():.3e}")
        return None
    if rule == "index":
        L = w.rows.shape[w.dim]
        if g.dtype != torch.int64:
            return f"{w.name}: {g.dtype} returned, int64 expected"
        bad = (g < 0) | (g >= L)
        if bool(bad.any()):
            return at(bad, "out of range")
        values = got[w.values_at]
        gi, gv = (g, values) if w.keepdim else (g.unsqueeze(w.dim), values.unsqueeze(w.dim))
        bad = _signed_view(w.rows).gather(w.dim, gi) != _signed_view(gv)
        if bool(bad.any()):
            return f"{w.name}: the row does not hold the returned value at {int(bad.sum())} returned positions"
        bad = w.free & (g != w.theirs)  # (torch's own index, where no tie leaves it open)
        return at(bad, "another index than torch's on a row without ties") if bool(bad.any()) else None
    raise ValueError(rule)


def check_newer(case: dict, cpu: dict, got: list) -> list:
    import torch
    wants = reference_newer(case, cpu, got)
    if len(got) != len(wants):
        return [f"{len(got)} outputs returned, {len(wants)} expected"]
    bad = [line for line in (_hold(w, g, got) for w, g in zip(wants, got)) if line]
    if not bad and case["op"] == "histc" and case["value_class"] == "exact":  # torch's own, where its arithmetic is exact too
        x = cpu["x"]
        theirs = torch.histc(x.double() if x.dtype == torch.float64 else x.float(), case["bins"], case["lo"], case["hi"])
        line = _first_difference("counts against torch.histc", got[0], as_count(theirs.long().numpy(), x.dtype))
        bad += [line] if line else []
    return bad


# ------------------------------------------------------------------------------------------------------------------------------
# the third deck: repeat_interleave, isin, mode and the dim= forms of unique / unique_consecutive

MODE_CLASSES = ["alphabet", "constant", "distinct", "hot", "row_edges", "specials"]  # (specials: floats; NaNs of several payloads, both zeros)
MODE_SHORT = [1, 2, 3, 63, 64, 65]           # row lengths given enough rows for three full tiles of the run tables and more
ISIN_VARIANTS = ["same", "same", "same", "mixed", "mixed", "mixed", "number_elements", "number_tests"]
ISIN_SHARES = ["none", "half", "all"]        # about which share of the elements is a member
ISIN_NANS = ["none", "elements", "tests", "both"]
REPEAT_FORMS = ["one_arg", "one_arg", "tensor", "tensor", "tensor", "tensor_strided", "zero_d", "one_element", "int"]
REPEAT_CLASSES = ["uniform_small", "mostly_zeros", "giant", "ones", "zeros", "zero_ends"]
OUTPUT_SIZES = ["absent", "exact", "too_large"]
REPEAT_CHUNK = 4096                          # the identity search writes its output in chunks of this many (vrs_search.hip)
UNIQUE_COLUMNS = [1, 2, 3, 4, 5, 9]
UNIQUE_REST = {1: [1, 1], 2: [2, 1], 3: [1, 3], 4: [2, 2], 5: [5, 1], 9: [3, 3]}  # the two trailing sizes of a 3-D shape with so many columns
ROW_CLASSES = ["few", "equal", "distinct", "sorted", "last_column", "behind_top", "specials"]  # (specials: floats; NaN and -0.0 columns)
# turns per round: once the last, whose reference, torch.unique(dim=) of 2^21 rows on the CPU, takes seconds; twice the others;
# (three times a round what has three edges to draw)
LARGE_KINDS_THIRD = (3 * ["mode_pool_skewed", "mode_pool_uniform", "mode_segment_one_call", "isin_pool"]
                     + 2 * ["mode_rows_of_3", "mode_int64_row", "isin_int16", "repeat_few_runs", "repeat_many_runs"] + ["unique_dim_large"])


def _wide(dtype: str) -> bool:
    return DTYPE_BYTES[dtype] == 8


def _promoted_name(a: str, b: str) -> str:
    import torch
    return str(torch.result_type(torch.empty(0, dtype=torch_dtype(a)), torch.empty(0, dtype=torch_dtype(b)))).split(".")[1]


def make_repeats(runs: int, cls: str, total, seed: int):
    """`runs` non-negative int64 repeats of class `cls` (REPEAT_CLASSES); total: their sum, where the class leaves it open (None: as drawn)."""
    rng = np.random.Generator(np.random.PCG64(seed + 17))
    if cls == "ones":
        return np.ones(runs, dtype=np.int64)
    if cls == "zeros" or runs == 0:
        return np.zeros(runs, dtype=np.int64)
    mean = max(1, -(-(total if total is not None else 3 * runs) // runs))
    if cls == "uniform_small":
        r = rng.integers(0, 2 * mean + 1, size=runs)
    elif cls == "mostly_zeros":
        r = np.where(rng.random(runs) < 0.9, 0, rng.integers(0, 20 * mean + 1, size=runs))
    elif cls == "giant":
        r = rng.integers(0, 2, size=runs)
        r[int(rng.integers(runs))] = (total if total is not None else 20 * runs)
    else:  # zero_ends
        r = rng.integers(0, 2 * mean + 1, size=runs)
    r = r.astype(np.int64)
    ends = max(1, runs // 8) if cls == "zero_ends" and runs >= 3 else 0
    if ends:
        r[:ends] = 0
        r[-ends:] = 0
    if total is not None:  # (what is missing goes to the middle run; what is too much is cut off the end)
        r[runs // 2] += max(0, total - int(r.sum()))
        c = np.minimum(np.cumsum(r), total)
        r = np.diff(c, prepend=0)
    return r


class _GenThird(_GenNewer):
    """The third deck, in the newer deck's window structure.  Window w of four holds: w even, a pending 1-D sort / sort_values / unique of the
    one-call minimum or more first; w odd, a neighbour last, from the first deck's ops and the newer deck's in turn; case i with
    i % LARGE_EVERY == LARGE_AT is of the large minority; every other case is the next op of the third deck's op deck.  An op draws its
    size plan first -- one deck per op, every edge of every cut one item of it -- and then a dtype that the plan's item allows."""

    def __init__(self, seed: int, count: int, window: int):
        super().__init__(seed, count, window)
        rng = self.rng
        self.third_op = _Deck(rng, [op for op in THIRD_OPS for _ in range(THIRD_OP_TURNS[op])])
        self.third_dtype = {op: _Deck(rng, THIRD_OP_DTYPES[op]) for op in THIRD_OPS}
        self.large_third = _Deck(rng, LARGE_KINDS_THIRD)
        self.third_mixed = _Deck(rng, MIXED_PAIRS)

    def _third_done(self, case: dict, role: str = "third") -> list:
        case.update(deck="third", role=role, data_seed=self._seed())
        return [case]

    def _dtype_of(self, op: str, ok=None) -> str:
        return self.third_dtype[op].draw(ok)

    @staticmethod
    def _edges(cuts) -> list:
        return [c + d for c in sorted(set(cuts)) for d in (-1, 0, 1)]

    def _exact_shape(self, n: int) -> list:
        """A 1-D to 3-D shape of exactly n elements."""
        rng = self.rng
        kind = int(rng.integers(4))
        if kind == 0 and n % 2 == 0 and n:
            return [2, n // 2]
        return [[n], [n], [1, n], [n, 1, 1]][kind]

    # -- mode -------------------------------------------------------------------------------------------------------------------
    def _mode(self) -> dict:
        rng, t = self.rng, self.t
        tile = t.capi.RLE_TILE  # (kModeTile of vrs_sort_mode.hip: the same 4096, and the constant the package exports)
        cap = SMALL_ELEMENTS
        plan = ([("one_row", kb, L) for kb in (4, 8) for L in self._edges(c for c in t.form_cuts[kb, 0] if c < cap) + [None]]
                + [("many_rows", 8 if w else 4, L) for w in (False, True) for L in self._edges(t.segment[w, False][:2]) + [None]]
                + [("short", 0, L) for L in MODE_SHORT] + [("tile_len", 0, tile + d) for d in (-1, 0, 1)] + [("tiny", 0, i) for i in range(2)])
        kind, kb, L = self._pick("mode_plan", plan)
        dtype = self._dtype_of("mode", None if not kb else (lambda d: _wide(d) == (kb == 8)))
        if kind == "one_row":
            L = L or int(rng.integers(2, cap + 1))
            shape, dim = self._shape_with(1, L)
        elif kind == "many_rows":
            L = L or int(rng.integers(2, 1000))
            shape, dim = self._shape_with(int(rng.integers(2, max(3, min(cap // L, 2000) + 1))), L)
        elif kind == "short":
            shape, dim = self._shape_with(-(-3 * tile // L) + int(rng.integers(1, 200)), L)
        elif kind == "tile_len":
            shape, dim = self._shape_with(int(rng.integers(1, 9)), L)
        else:
            shape, dim = ([], 0) if L == 0 else [([1], 0), ([2, 1], 1), ([1, 3], 0), ([4, 1, 2], 1)][int(rng.integers(4))]
        if shape and rng.integers(2):
            dim -= len(shape)
        classes = MODE_CLASSES if dtype in FLOATS else MODE_CLASSES[:-1]
        return {"op": "mode", "dtype": dtype, "shape": shape, "dim": dim, "keepdim": self._pick("keepdim", [False, True]), "layout": self._layout(shape),
                "values": self._pick("mode_class_" + str(dtype in FLOATS), classes), "size": kind}

    # -- isin -------------------------------------------------------------------------------------------------------------------
    def _isin(self) -> dict:
        rng, t = self.rng, self.t
        low = t.capi.ONE_CALL_MIN_KEYS_DEFAULT
        narrow, cuts4 = (lambda d: not _wide(d)), [c for c in t.form_cuts[4, 0] if c < SMALL_ELEMENTS and c != low]
        bare4 = lambda d: not _wide(d) and d not in FLOATS  # noqa: E731  (the test set's sort is one of bare 4-byte keys)
        plan = ([("out", d, narrow) for d in (-1, 0, 1)] + [("out", 0, _wide)]
                + [("table", d, lambda n: DTYPE_BYTES[n] == 1) for d in (-1, 0, 1)] + [("table", 0, lambda n: DTYPE_BYTES[n] == 2)]
                + [("index", d, lambda n: DTYPE_BYTES[n] >= 4) for d in (-1, 0, 1)]
                + [("cut", m, bare4) for m in self._edges(cuts4)] + [("cut", m, bare4) for m in self._edges([low])]
                + [("cut", m, ok) for ok in ((lambda n: n == "int64"), (lambda n: n == "float64"), (lambda n: n in FLOATS and not _wide(n))) for m in self._edges([low])]
                + [("lds", 0, None), ("lds", 0, None), ("few", 0, None), ("empty_elements", 0, None), ("empty_tests", 0, None), ("zero_d", 0, None)])
        variant = self._pick("isin_variant", ISIN_VARIANTS)
        if "isin_plan" not in self.named:
            self.named["isin_plan"] = _Deck(rng, plan)

        def fits(item):  # (a number as elements is one query, a number as the test set one test element: the sizes that are about neither)
            if variant == "mixed":
                return any(item[2] is None or item[2](p[2]) for p in MIXED_PAIRS)
            if variant == "number_elements":
                return item[0] in ("out", "cut", "lds", "few")
            return variant == "same" or item[0] in ("lds", "few", "zero_d")

        kind, arg, ok = self.named["isin_plan"].draw(fits)
        ok = ok or (lambda n: True)
        if variant == "mixed":
            test_dtype, dtype, common = self.third_mixed.draw(lambda p: ok(p[2]))
        else:
            dtype = test_dtype = common = self._dtype_of("isin", ok)
        out, table, index = t.search[common]
        q = int(rng.integers(1, 3000))
        if kind == "out":
            m, q = out + arg, int(rng.integers(1, 200))
        elif kind == "table":
            m, q = int(rng.integers(out, 2 * out)), table + arg
        elif kind == "index":
            m, q = int(rng.integers(out, 2 * out)), index + arg
        elif kind == "cut":
            m = arg
        elif kind == "lds":
            m = int(rng.integers(2, out - 1))
        else:
            m, q = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        shape = [] if kind == "zero_d" else [0] if kind == "empty_elements" else self._exact_shape(q)
        test_shape = [[0], [2, 0]][int(rng.integers(2))] if kind == "empty_tests" else self._exact_shape(m)
        case = {"op": "isin", "dtype": dtype, "test_dtype": test_dtype, "variant": variant, "shape": shape, "layout": self._layout(shape),
                "test_shape": test_shape, "test_layout": self._layout(test_shape), "invert": self._pick("invert", [False, True]),
                "assume_unique": self._pick("assume_unique", [False, False, True]), "share": self._pick("isin_share", ISIN_SHARES),
                "dist": self._dist(dtype), "test_dist": self._dist(test_dtype), "size": kind,
                "nans": self._pick("isin_nans", ISIN_NANS) if common in FLOATS else "none", "signed_zero": common in FLOATS and bool(rng.integers(2))}
        if variant == "number_elements":
            case.update(shape=[], layout={"kind": "contiguous"})
        elif variant == "number_tests":
            case.update(test_shape=[], test_layout={"kind": "contiguous"})
        return case

    # -- repeat_interleave --------------------------------------------------------------------------------------------------------
    def _repeat(self) -> dict:
        rng, t = self.rng, self.t
        form = self._pick("repeat_form", REPEAT_FORMS)
        rdt = self._pick("repeats_dtype", ["int32", "int64"])
        how = self._pick("output_size", OUTPUT_SIZES)
        case = {"op": "repeat_interleave", "form": form, "repeats_dtype": rdt, "repeats_layout": {"kind": "contiguous"}, "rep_seed": self._seed()}
        if form in ("one_arg", "tensor", "tensor_strided"):
            cuts = [c for c in t.scan_cuts(rdt, "int64", "cumsum") if c and c < SMALL_ELEMENTS // 2]
            plan = [("runs", m) for m in self._edges(cuts)] + [("total", v) for v in self._edges(k * REPEAT_CHUNK for k in (1, 2, 5))] + [("free", 0), ("free", 0), ("empty", 0)]
            cls = self._pick("repeat_class", REPEAT_CLASSES)
            if "repeat_plan" not in self.named:  # (one plan for both dtypes of repeats: the scan's cuts are those of its int64 output)
                self.named["repeat_plan"] = _Deck(rng, plan)
            kind, arg = self.named["repeat_plan"].draw(lambda item: item[0] != "total" or cls != "zeros")
            if kind == "empty":
                runs, total = 0, None
            elif kind == "runs":
                runs, total = arg, None if cls in ("ones", "zeros") else int(rng.integers(arg, 4 * arg))
            elif kind == "total":
                runs, total = (arg if cls == "ones" else int(rng.integers(3, arg))), arg
            else:
                runs = int(rng.integers(0, 3)) if rng.integers(4) == 0 else int(rng.integers(3, 3000))
                total = None if cls in ("ones", "zeros") or runs == 0 else int(rng.integers(runs, 4 * runs + 2))
            true_total = int(make_repeats(runs, cls, total, case["rep_seed"]).sum())
            case.update(runs=runs, rep_class=cls, total_target=total, total=true_total, size=kind)
            if form == "tensor_strided":
                case["repeats_layout"] = {"kind": "strided", "step": int(rng.integers(2, 4))} if self._pick("repeats_layout", [True, False]) else {"kind": "offset", "by": int(rng.integers(1, 4))}
        else:
            runs, k = int(rng.integers(1, 3000)), int(rng.integers(0, 5))
            case.update(runs=runs, rep_class="equal", k=k, total_target=None, total=runs * k, size="free")
            if form == "int" and how == "too_large":
                how = "exact"  # (a Python int's total is known to the wrapper: another output_size is refused, as torch refuses it)
        if case["runs"] == 0 and how == "too_large":
            how = "exact"  # (no last element to repeat)
        case.update(output_size=how, extra=int(rng.integers(1, 100)) if how == "too_large" else 0)
        if form == "one_arg":
            case.update(dtype=rdt, shape=[case["runs"]], dim=None, layout={"kind": "contiguous"})
            return case
        dtype = self._dtype_of("repeat_interleave")
        runs = case["runs"]
        width = max(1, min(4, SMALL_ELEMENTS // max(case["total"] + case["extra"], runs, 1)))
        other = [[], [int(rng.integers(1, width + 1))], [2, width // 2] if width >= 4 else [1, 1]][self._pick("repeat_other", [0, 1, 2, 2])]
        if self._pick("repeat_dim_none", [True, False, False]):
            a = 2 if runs % 2 == 0 and runs and rng.integers(2) else 1
            shape, dim = ([a, runs // a] if a == 2 else [runs]), None  # (the flattened input: runs elements)
        else:
            dim = self._pick("repeat_dim3", [0, 1, 2]) if len(other) == 2 else int(rng.integers(len(other) + 1))
            shape = other[:dim] + [runs] + other[dim:]
            dim = dim - len(shape) if rng.integers(2) else dim
        case.update(dtype=dtype, shape=shape, dim=dim, layout=self._layout(shape), dist=self._value_dist(dtype))
        return case

    # -- unique(dim=) and unique_consecutive(dim=) ----------------------------------------------------------------------------------
    def _unique_dim(self, op: str, N=None, C=None, dtype=None, rows=None) -> dict:
        rng, t = self.rng, self.t
        dtype = dtype or self._dtype_of(op)
        cuts = {t.capi.RLE_TILE, t.capi.ONE_CALL_MIN_KEYS_DEFAULT, *t.form_cuts[4, 1], *t.form_cuts[8, 1]}
        classes = ROW_CLASSES if dtype in FLOATS else ROW_CLASSES[:-1]
        rows = rows or self._pick(f"rows_{op}_{dtype in FLOATS}", classes)
        C = C or self._pick("columns_" + op, UNIQUE_COLUMNS)
        if rows == "behind_top" and C * DTYPE_BYTES[dtype] <= 8:
            C = [3, 4, 5, 9][int(rng.integers(4))]  # (something behind the first 8 bytes)
        if N is None:
            N = self._pick("rows_plan_" + op, self._edges(c for c in cuts if c < SMALL_ELEMENTS // 9) + [None, None, "tiny", "above"])
            if N is None:
                N = int(rng.integers(2, 3000))
            elif N == "tiny":
                N = int(rng.integers(1, 3))
            elif N == "above":
                N = int(rng.integers(t.capi.RLE_TILE + 2, min(20000, SMALL_ELEMENTS // C)))
        rest = [C] if self._pick("unique_nd", [2, 3]) == 2 else UNIQUE_REST[C]
        dim = int(rng.integers(len(rest) + 1))
        shape = rest[:dim] + [N] + rest[dim:]
        inverse, counts = self.flags4.draw()
        return {"op": op, "dtype": dtype, "shape": shape, "dim": dim - len(shape) if rng.integers(2) else dim, "N": N, "C": C,
                "layout": self._layout(shape), "return_inverse": inverse, "return_counts": counts, "rows": rows}

    # -- the large minority -----------------------------------------------------------------------------------------------------
    def _large_third(self) -> list:
        rng, t = self.rng, self.t
        kind = self.large_third.draw()
        plain = {"kind": "contiguous"}
        if kind in ("mode_pool_skewed", "mode_pool_uniform"):
            n = t.pool_min + self._pick(kind + "_edge", [-1, 0, 1])
            case = {"op": "mode", "dtype": self._turn(kind, ["int32", "float32"]), "shape": [n], "dim": 0, "keepdim": False, "layout": self._layout([n]),
                    "values": "thousand" if kind == "mode_pool_skewed" else "uniform", "size": "large"}
        elif kind == "mode_rows_of_3":
            dtype = self._dtype_of("mode")
            shape, dim = (([1 << 20, 3], -1) if rng.integers(2) else ([3, 1 << 20], 0))
            case = {"op": "mode", "dtype": dtype, "shape": shape, "dim": dim, "keepdim": bool(rng.integers(2)), "layout": plain, "values": "alphabet", "size": "large"}
        elif kind == "mode_int64_row":
            case = {"op": "mode", "dtype": "int64", "shape": [1 << 22], "dim": -1, "keepdim": False, "layout": plain,
                    "values": self._turn(kind, ["thousand", "hot", "uniform"]), "size": "large"}
        elif kind == "mode_segment_one_call":
            wide = self._turn(kind, [False, True])
            length = t.segment[wide, False][2] + self._pick(kind + "_edge", [-1, 0, 1])
            dtype = self._dtype_of("mode", lambda d: _wide(d) == wide)
            shape, dim = (([2, length], 1) if rng.integers(2) else ([length, 2], 0))
            case = {"op": "mode", "dtype": dtype, "shape": shape, "dim": dim, "keepdim": False, "layout": plain,
                    "values": self._pick("mode_class_large", ["alphabet", "hot", "thousand", "row_edges"]), "size": "large"}
        elif kind == "isin_pool":
            m = t.pool_min + self._pick("isin_pool_edge", [-1, 0, 1])
            dtype = self._turn(kind, ["int32", "int32", "int32", "float32"])  # (bare keys: the pool form; float32's test set sorts as pairs)
            case = {"op": "isin", "dtype": dtype, "test_dtype": dtype, "variant": "same", "shape": [1 << 20], "layout": plain, "test_shape": [m], "test_layout": plain,
                    "invert": bool(rng.integers(2)), "assume_unique": False, "share": "half", "dist": "uniform", "test_dist": "uniform", "size": "large",
                    "nans": "none", "signed_zero": False}
        elif kind == "isin_int16":
            case = {"op": "isin", "dtype": "int16", "test_dtype": "int16", "variant": "same", "shape": [LARGE_ELEMENTS], "layout": plain, "test_shape": [10_000],
                    "test_layout": plain, "invert": bool(rng.integers(2)), "assume_unique": False, "share": "none", "dist": "uniform", "test_dist": "uniform",
                    "size": "large", "nans": "none", "signed_zero": False}
        elif kind in ("repeat_few_runs", "repeat_many_runs"):
            runs = 1 << 10 if kind == "repeat_few_runs" else 1 << 22
            rdt = self._turn("large_repeats_dtype", ["int64", "int32"])
            case = {"op": "repeat_interleave", "form": self._turn(kind, ["tensor", "one_arg"]), "repeats_dtype": rdt, "repeats_layout": plain, "rep_seed": self._seed(),
                    "runs": runs, "rep_class": self._turn(kind + "_class", ["uniform_small", "mostly_zeros", "zero_ends"]), "total_target": LARGE_ELEMENTS,
                    "total": LARGE_ELEMENTS, "size": "large", "output_size": self._turn(kind + "_size", ["exact", "absent"]), "extra": 0}
            if case["form"] == "one_arg":
                case.update(dtype=rdt, shape=[runs], dim=None, layout=plain)
            else:
                dtype = self._dtype_of("repeat_interleave", lambda d: DTYPE_BYTES[d] <= 4)
                case.update(dtype=dtype, shape=[runs], dim=0, layout=plain, dist=self._value_dist(dtype))
        else:
            case = self._unique_dim("unique_dim", N=1 << 21, C=3, dtype="int32", rows="thousand")
            case.update(shape=[1 << 21, 3], dim=0, layout=plain)
        return self._third_done(case, "large:" + kind)

    def _next(self) -> list:
        window, at = divmod(self._index, self.window)
        if self._index % LARGE_EVERY == LARGE_AT:
            return self._large_third()
        if window % 2 == 0 and at == 0:
            case = self._pending_sort()[0]
        elif window % 2 == 1 and at == self.window - 1:
            case = (self._neighbour() if self._turn("neighbour_from", ["first", "newer"]) == "first" else self._regular())[0]
            case["role"] = "neighbour"
        else:
            op = self.third_op.draw()
            case = {"mode": self._mode, "isin": self._isin, "repeat_interleave": self._repeat}[op]() if not op.startswith("unique") else self._unique_dim(op)
            return self._third_done(case)
        case["deck"] = "third"
        return [case]


# -- the third deck's inputs (torch on the CPU and numpy; nothing of the library) ------------------------------------------------------

def _finite_bits(rng, name: str, count):
    """`count` random bit patterns of the dtype (a shape or a number), finite where it is a float."""
    nbytes = DTYPE_BYTES[name]
    ut = _BITS[nbytes]
    b = rng.integers(0, 1 << (8 * nbytes), size=count, dtype=ut)
    if name in FLOATS:
        em = ut(_EXPONENT[name][0])
        b = np.where((b & em) == em, b & ~ut(int(em) & -int(em)), b).astype(ut)
    return b


def _numbers_as_bits(numbers, name: str):
    """Small integers (a numpy array) as the dtype's bit patterns."""
    import torch
    return to_bits(torch.from_numpy(np.ascontiguousarray(numbers, dtype=np.int64)).to(torch_dtype(name)))


def _special_pool(name: str):
    """NaNs of three payloads and both signs, both zeros, and a few numbers: the values of the "specials" classes, as bit patterns."""
    em, mant = _EXPONENT[name]
    sign, quiet = 1 << (8 * DTYPE_BYTES[name] - 1), 1 << (mant - 1)
    ut = _BITS[DTYPE_BYTES[name]]
    return np.concatenate((np.array([em | quiet, em | quiet | 1, sign | em | quiet | 2, 0, sign], dtype=ut), _numbers_as_bits(np.array([1, -1, 2]), name)))


def _row_permuted(rng, a):
    return rng.permuted(a, axis=1) if a.shape[1] > 1 else a


def mode_values(name: str, shape, dim: int, cls: str, seed: int):
    """A contiguous CPU tensor of `shape` whose rows along `dim` are of class `cls` (MODE_CLASSES, or "thousand" / "uniform" of the large kinds)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = list(shape)
    ut = _BITS[DTYPE_BYTES[name]]
    if not shape:
        return from_bits(_finite_bits(rng, name, 1), name).reshape(())
    dim %= len(shape)
    L = shape[dim]
    moved = shape[:dim] + shape[dim + 1:] + [L]
    R = _numel(moved) // max(L, 1)
    if cls == "alphabet":
        k = int(rng.integers(2, 8))
        pool = _finite_bits(rng, name, k)
        idx = _row_permuted(rng, np.tile(np.arange(L) % k, (R, 1)))  # every value as often as the others (L a multiple of k: all tied)
        free = rng.random(R) < 0.5
        idx[free] = rng.integers(0, k, size=(int(free.sum()), L))
        bits = pool[idx]
    elif cls == "constant":
        bits = np.full((R, L), _finite_bits(rng, name, 1)[0], dtype=ut)
    elif cls == "distinct":
        span = int(_EXPONENT[name][0]) if name in FLOATS else 1 << (8 * DTYPE_BYTES[name])  # (floats: the non-negative finite patterns)
        span = min(span, 1 << 62)
        start = int(rng.integers(span))
        bits = _row_permuted(rng, ((start + np.arange(L, dtype=np.int64)[None, :] + 7 * np.arange(R, dtype=np.int64)[:, None]) % span)).astype(ut)
    elif cls == "hot":
        bits = _finite_bits(rng, name, (R, L))
        hot = _row_permuted(rng, np.tile(np.arange(L) < (L + 1) // 2, (R, 1)))
        bits = np.where(hot, _finite_bits(rng, name, (R, 1)), bits)
    elif cls == "row_edges":  # row r holds r % 100 and r % 100 + 1: its largest value is the next row's smallest, and that run is the longest
        lo = (np.arange(R) % 100)[:, None]
        a = rng.integers(L // 3, 2 * L // 3 + 1, size=(R, 1)) if L >= 2 else np.ones((R, 1), dtype=np.int64)
        bits = _numbers_as_bits(_row_permuted(rng, np.where(np.arange(L)[None, :] < a, lo, lo + 1)), name)
    elif cls == "specials":
        pool = _special_pool(name)
        bits = pool[rng.integers(0, pool.size, size=(R, L))]
    elif cls == "thousand":
        pool = _finite_bits(rng, name, 1000)
        bits = pool[rng.integers(0, 1000, size=(R, L))]
    elif cls == "uniform":
        bits = _finite_bits(rng, name, (R, L))
    else:
        raise ValueError(f"unknown class {cls!r}")
    return from_bits(np.ascontiguousarray(bits, dtype=ut).reshape(-1), name).reshape(moved).movedim(-1, dim).contiguous()


def row_values(name: str, N: int, C: int, cls: str, consecutive: bool, seed: int):
    """A contiguous [N, C] CPU tensor of rows of class `cls` (ROW_CLASSES, or "thousand"); consecutive: every row repeated a few times."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ut = _BITS[DTYPE_BYTES[name]]
    cols = np.arange(C)[None, :]

    def alphabet(k):
        return _finite_bits(rng, name, (C, k))[cols, rng.integers(0, k, size=(N, C))]

    if cls == "few":
        bits = alphabet(2)
    elif cls == "thousand":
        bits = alphabet(10)
    elif cls == "equal":
        bits = np.tile(_finite_bits(rng, name, (1, C)), (N, 1))
    elif cls == "distinct":
        bits = alphabet(2)
        bits[:, 0] = _numbers_as_bits(rng.permutation(N) - N // 2, name)
    elif cls == "sorted":
        small = rng.integers(-1, 2, size=(N, C))
        bits = _numbers_as_bits(small[np.lexsort(small.T[::-1])], name)
    elif cls == "last_column":
        bits = np.tile(_finite_bits(rng, name, (1, C)), (N, 1))
        bits[:, -1] = _numbers_as_bits(rng.integers(-max(N // 4, 2), max(N // 4, 2), size=N), name)
    elif cls == "behind_top":  # equal in the first 8 bytes, different behind them
        top = 8 // DTYPE_BYTES[name]
        bits = np.tile(_finite_bits(rng, name, (1, C)), (N, 1))
        bits[:, top:] = alphabet(3)[:, top:]
    elif cls == "specials":
        pool = _special_pool(name)
        bits = pool[rng.integers(0, pool.size, size=(N, C))]
    else:
        raise ValueError(f"unknown class {cls!r}")
    if consecutive and cls not in ("equal", "distinct") and N:
        bits = bits[np.minimum(np.cumsum(rng.random(N) < 0.4), N - 1)]
    return from_bits(np.ascontiguousarray(bits, dtype=ut).reshape(-1), name).reshape(N, C)


def _order_key_any(t):
    """order_key, and an unsigned tensor's own bits (order_key is about signed integers and floats)."""
    import torch
    return to_bits(t) if t.dtype == torch.uint8 else order_key(t)


def _neighbours_of(tests, name: str):
    """Two values of the dtype `name`: just below the smallest and just above the largest of `tests` (as that dtype) in its order."""
    key = _order_key_any(tests.to(torch_dtype(name)).reshape(-1))
    top = int(np.iinfo(key.dtype).max)
    pair = np.array([max(int(key.min()), 1) - 1, min(int(key.max()), top - 1) + 1], dtype=key.dtype)
    return from_bits(pair, name) if name == "uint8" else values_of_key(pair, name)


def third_inputs(case: dict) -> dict:
    """name -> (base, view) as lay_out gives them, or a plain Python number: the inputs of a case of the third deck's ops, on the CPU."""
    import torch
    op, dtype, seed = case["op"], case["dtype"], case["data_seed"]
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    out = {}
    if op == "mode":
        shape, dim = case["shape"], case["dim"]
        out["x"] = lay_out(shape, case["layout"], lambda s: mode_values(dtype, s, dim, case["values"], seed))
    elif op in ("unique_dim", "unique_consecutive_dim"):
        dim = case["dim"] % len(case["shape"])

        def rows(s):
            rest = s[:dim] + s[dim + 1:]
            return row_values(dtype, s[dim], _numel(rest), case["rows"], op == "unique_consecutive_dim", seed).reshape([s[dim]] + rest).movedim(0, dim).contiguous()

        out["x"] = lay_out(case["shape"], case["layout"], rows)
    elif op == "repeat_interleave":
        rdt = torch_dtype(case["repeats_dtype"])
        if case["rep_class"] == "equal":
            repeats = {"zero_d": torch.tensor(case["k"], dtype=rdt), "one_element": torch.tensor([case["k"]], dtype=rdt), "int": case["k"]}[case["form"]]
            out["repeats"] = repeats if case["form"] == "int" else (repeats, lambda t: t)
        else:
            r = torch.from_numpy(make_repeats(case["runs"], case["rep_class"], case["total_target"], case["rep_seed"])).to(rdt)
            out["repeats"] = lay_out([case["runs"]], case["repeats_layout"], lambda s: r)
        if case["form"] != "one_arg":
            out["x"] = lay_out(case["shape"], case["layout"], lambda s: newer_values(dtype, s, case["dist"], seed))
    else:  # isin
        el, te = case["dtype"], case["test_dtype"]
        m, q = _numel(case["test_shape"]), _numel(case["shape"])
        tests = make_values(te, [m], case["test_dist"], seed)
        if m and case["share"] != "none":  # duplicates: about a third of the test elements repeat another one
            again = torch.from_numpy(rng.random(m) < 0.3)
            tests = torch.where(again, tests[torch.from_numpy(rng.integers(0, m, size=m))], tests)
        elements = make_values(el, [q], case["dist"], seed + 1)
        if m and q and case["share"] != "none":
            hits = tests[torch.from_numpy(rng.integers(0, m, size=q))].to(elements.dtype)
            take = torch.ones(q, dtype=torch.bool) if case["share"] == "all" else torch.from_numpy(rng.random(q) < 0.5)
            elements = torch.where(take, hits, elements)
        if m and q >= 2 and case["share"] != "all":
            elements[:2] = _neighbours_of(tests, el)
        if case["signed_zero"] and m and q >= 3:
            tests[0], elements[2] = 0.0, -0.0
        if case["nans"] in ("tests", "both") and m >= 2 and te in FLOATS:
            tests[1] = float("nan")
        if case["nans"] in ("elements", "both") and q >= 4 and el in FLOATS:
            elements[3] = float("nan")
        as_number = lambda t: t.reshape(-1)[0].item()  # noqa: E731
        out["elements"] = as_number(elements) if case["variant"] == "number_elements" else lay_out(case["shape"], case["layout"], lambda s: _fit(elements, s))
        out["tests"] = as_number(tests) if case["variant"] == "number_tests" else lay_out(case["test_shape"], case["test_layout"], lambda s: _fit(tests, s))
    return out


def _fit(flat, shape):
    """The first elements of a 1-D tensor as `shape` (an expanded layout asks for fewer than were made)."""
    import torch
    if flat.numel() < _numel(shape):  # (an empty shape expanded along its empty dimension: one element a row, none of them seen)
        return torch.zeros(list(shape), dtype=flat.dtype)
    return flat[:_numel(shape)].reshape(list(shape)).clone()


def call_third(api, case: dict, t: dict):
    """The one public call of a case of the third deck's ops on `api`: this library, or anything with the same functions."""
    op = case["op"]
    if op == "mode":
        return api.mode(t["x"], case["dim"], case["keepdim"])
    if op == "isin":
        return api.isin(t["elements"], t["tests"], assume_unique=case["assume_unique"], invert=case["invert"])
    if op == "repeat_interleave":
        size = {"absent": None, "exact": case["total"], "too_large": case["total"] + case["extra"]}[case["output_size"]]
        if case["form"] == "one_arg":
            return api.repeat_interleave(t["repeats"], output_size=size)
        return api.repeat_interleave(t["x"], t["repeats"], case["dim"], output_size=size)
    fn = api.unique if op == "unique_dim" else api.unique_consecutive
    return fn(t["x"], return_inverse=case["return_inverse"], return_counts=case["return_counts"], dim=case["dim"])


# -- the third deck's references (torch's CPU functions and numpy only) ----------------------------------------------------------------

def ref_mode(x, dim: int):
    """The documented rule in numpy: per row along dim the smallest of the most frequent values, -0.0 and +0.0 one value and all NaNs one
    value, the largest; the index of its LAST occurrence; the value with the bits of the element there.  -> (values, indices), dim kept."""
    import torch
    if x.dim() == 0:
        return x.clone(), torch.zeros((), dtype=torch.int64)
    rows = x.movedim(dim, -1).contiguous()
    L = rows.shape[-1]
    flat = rows.reshape(-1, L)
    R = flat.shape[0]
    canon = flat
    if flat.dtype.is_floating_point:
        canon = torch.where(torch.isnan(flat), torch.full((), float("nan"), dtype=flat.dtype), torch.where(flat == 0, torch.zeros((), dtype=flat.dtype), flat))
    key = _order_key_any(canon)                  # (a positive quiet NaN: above +inf)
    ks = np.sort(key, axis=1).reshape(-1)
    heads = np.ones(R * L, dtype=bool)
    heads[1:] = ks[1:] != ks[:-1]
    heads[::L] = True                            # a run ends with its row
    starts = np.flatnonzero(heads)
    counts = np.diff(np.append(starts, R * L))
    run_row = starts // L
    first_run = np.flatnonzero(np.diff(run_row, prepend=-1))  # (every row has a run: L >= 1)
    most = np.maximum.reduceat(counts, first_run)
    cand = np.flatnonzero(counts == most[run_row])
    _, first = np.unique(run_row[cand], return_index=True)  # the first of them: the smallest value
    mode_key = ks[starts[cand[first]]]
    last = L - 1 - np.argmax((key == mode_key[:, None])[:, ::-1], axis=1)
    idx = torch.from_numpy(last.astype(np.int64)).reshape(-1, 1)
    values = _signed_view(flat).gather(1, idx).view(flat.dtype)
    shape = list(rows.shape[:-1]) + [1]
    return values.reshape(shape).movedim(-1, dim), idx.reshape(shape).movedim(-1, dim)


def ref_unique_rows(x, dim: int, consecutive: bool):
    """unique(dim=) / unique_consecutive(dim=) on bit patterns: the slices along dim as rows of words, ordered word by word by the IEEE
    total order (signed integers numerically), equal when bit-identical.  -> (values, inverse, counts)."""
    import torch
    rows = x.movedim(dim, 0).contiguous()
    N = rows.shape[0]
    flat = rows.reshape(N, -1)
    key = order_key(flat)
    order = np.arange(N) if consecutive else np.lexsort(key.T[::-1])  # (the first column decides first; stable)
    ks = key[order]
    heads = np.ones(N, dtype=bool)
    heads[1:] = (ks[1:] != ks[:-1]).any(axis=1)
    starts = np.flatnonzero(heads)
    inverse = np.empty(N, dtype=np.int64)
    inverse[order] = np.cumsum(heads) - 1
    counts = np.diff(np.append(starts, N)).astype(np.int64)
    values = rows[torch.from_numpy(order[starts])]
    return values.movedim(0, dim), torch.from_numpy(inverse), torch.from_numpy(counts)


def ref_isin(elements, tests, invert: bool):
    """torch.isin on the CPU after torch's own promotion (float16 / bfloat16 as float32, which is exact).  assume_unique is not passed on:
    the library documents that duplicates never change membership, and torch leaves the result open for them."""
    import torch
    common = torch.result_type(elements, tests)
    e = elements.to(common) if isinstance(elements, torch.Tensor) else torch.tensor(elements, dtype=common)
    t = tests.to(common) if isinstance(tests, torch.Tensor) else torch.tensor(tests, dtype=common)
    if common in (torch.float16, torch.bfloat16):
        e, t = e.float(), t.float()
    return torch.isin(e.contiguous(), t.contiguous().reshape(-1), invert=invert)


def ref_repeat_interleave(case: dict, cpu: dict):
    """torch.repeat_interleave on the CPU; a too-large output_size: the documented answer, the last element repeated."""
    import torch
    total = None if case["output_size"] == "absent" else case["total"]
    if case["form"] == "one_arg":
        out, d = torch.repeat_interleave(cpu["repeats"].contiguous(), output_size=total), 0
    else:
        x = cpu["x"].contiguous()
        rep = cpu["repeats"].contiguous() if isinstance(cpu["repeats"], torch.Tensor) else cpu["repeats"]
        out = torch.repeat_interleave(x, rep, case["dim"], output_size=total)
        d = 0 if case["dim"] is None else case["dim"] % max(x.dim(), 1)
        last = (x.reshape(-1) if case["dim"] is None else x).narrow(d, (x.numel() if case["dim"] is None else x.shape[d]) - 1, 1) if case["extra"] else None
    if case["extra"]:
        if case["form"] == "one_arg":
            last = torch.full((1,), case["runs"] - 1, dtype=out.dtype)
        out = torch.cat((out, last.expand(*out.shape[:d], case["extra"], *out.shape[d + 1:])), dim=d)
    return out


def check_third(case: dict, cpu: dict, got: list) -> list:
    import torch
    op, bad = case["op"], []

    def same(name, g, w):
        line = _first_difference(name, g, w)
        if line:
            bad.append(line)

    if op == "isin":
        if len(got) != 1:
            return [f"{len(got)} outputs returned, 1 expected"]
        same("result", got[0], ref_isin(cpu["elements"], cpu["tests"], case["invert"]))
    elif op == "repeat_interleave":
        if len(got) != 1:
            return [f"{len(got)} outputs returned, 1 expected"]
        same("out", got[0], ref_repeat_interleave(case, cpu))
    elif op == "mode":
        if len(got) != 2:
            return [f"{len(got)} outputs returned, 2 expected"]
        x = cpu["x"]
        dim = case["dim"] % max(x.dim(), 1)
        values, indices = ref_mode(x, dim)
        if not case["keepdim"] and x.dim():
            values, indices = values.squeeze(dim), indices.squeeze(dim)
        same("values", got[0], values)
        same("indices", got[1], indices)
        if not bad and not (x.dtype.is_floating_point and bool(torch.isnan(x).any())):  # torch's own values, where they are defined
            exact = x.double() if x.dtype.is_floating_point else x.long()
            theirs = torch.mode(exact, dim, case["keepdim"]).values if x.dim() else exact
            if not bool((got[0].to(theirs.dtype) == theirs).all()):
                at = int(torch.nonzero((got[0].to(theirs.dtype) != theirs).reshape(-1))[0])
                bad.append(f"values against torch.mode: another value at flat {at}: returned {got[0].reshape(-1)[at].item()!r}, torch {theirs.reshape(-1)[at].item()!r}")
    else:
        x = cpu["x"]
        dim = case["dim"] % x.dim()
        want = ref_unique_rows(x, dim, op == "unique_consecutive_dim")
        names = ["values"] + (["inverse"] if case["return_inverse"] else []) + (["counts"] if case["return_counts"] else [])
        if len(got) != len(names):
            return [f"{len(got)} outputs returned, {len(names)} expected"]
        picked = {"values": want[0], "inverse": want[1], "counts": want[2]}
        for name, g in zip(names, got):
            same(name, g, picked[name])
        if not bad and plain_values(x):
            fn = torch.unique if op == "unique_dim" else torch.unique_consecutive
            tw = _as_tuple(fn(x, return_inverse=case["return_inverse"], return_counts=case["return_counts"], dim=dim))
            for name, g, w in zip(names, got, tw):
                same(f"{name} against torch.{fn.__name__}(dim=)", g, w)
    return bad


# ------------------------------------------------------------------------------------------------------------------------------
# the runner

class Mismatch(AssertionError):
    pass


def _first_difference(name: str, got, want):
    """None when got and want are the same tensor (dtype, shape, every bit), else a line that names the first differing position."""
    import torch
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{name}: {got.dtype} {tuple(got.shape)} returned, {want.dtype} {tuple(want.shape)} expected"
    if got.numel() == 0:
        return None
    g, w = to_bits(got).reshape(-1), to_bits(want).reshape(-1)
    if np.array_equal(g, w):
        return None
    at = int(np.flatnonzero(g != w)[0])
    pos = tuple(int(i) for i in np.unravel_index(at, tuple(got.shape))) if got.dim() else ()
    return (f"{name}: first difference at {pos} (flat {at}) of {g.size}: returned {got.reshape(-1)[at].item()!r} (bits {int(g[at]):#x}), "
            f"expected {want.reshape(-1)[at].item()!r} (bits {int(w[at]):#x}); {int((g != w).sum())} elements differ")


class _Pending:
    def __init__(self, case, stream, inputs, outputs, nbytes):
        self.case, self.stream, self.inputs, self.outputs, self.nbytes = case, stream, inputs, outputs, nbytes


def _nbytes(*tensors) -> int:
    import torch
    total = 0
    for t in tensors:
        if isinstance(t, torch.Tensor):
            total += t.numel() * t.element_size()
        elif isinstance(t, (tuple, list)):
            total += _nbytes(*t)
    return total


def prepare(case: dict, device):
    """The case's inputs: CPU tensors in their layout (for the references) and the same on the device, uploaded on torch's current
    stream.  A dependent searchsorted gets its queries only: its sequence is a library result that launch() picks up."""
    import torch
    op = case["op"]
    if op in NEWER_OPS or op in THIRD_OPS:
        cpu, gpu = {}, {}
        for name, item in (newer_inputs if op in NEWER_OPS else third_inputs)(case).items():
            if not isinstance(item, tuple):  # (a Python number)
                cpu[name] = gpu[name] = item
                continue
            base, view = item
            cpu[name] = view(base)
            if device is not None:
                gpu[name] = view(base.to(device))
        return cpu, gpu
    if op not in ("searchsorted", "bucketize"):
        base, view = lay_out(case["shape"], case["layout"], lambda s: make_values(case["dtype"], s, case["dist"], case["data_seed"]))
        return {"x": view(base)}, {"x": view(base.to(device))}
    rng = np.random.Generator(np.random.PCG64(case["data_seed"]))
    cpu, gpu = {}, {}
    if case["variant"] == "dependent":
        seq_values = None  # (on the device, not looked at yet; its CPU copy is taken when the window is checked)
    else:
        raw = {}

        def fill(shape):
            t = make_values(case["dtype"], shape, case["seq_dist"], case["data_seed"])
            if case.get("sorter"):
                raw["t"] = t
                return t
            return torch.sort(t, dim=-1).values

        base, view = lay_out(case["seq_shape"], case["seq_layout"], fill)
        cpu["seq"], gpu["seq"] = view(base), view(base.to(device))
        seq_values = cpu["seq"]
        if case.get("sorter"):
            so = torch.argsort(cpu["seq"].float() if cpu["seq"].dtype in (torch.float16, torch.bfloat16) else cpu["seq"], dim=-1, stable=True)
            cpu["sorter"], gpu["sorter"] = so, so.to(device)
    if case["variant"] == "scalar":
        m = case["seq_shape"][0]
        number = cpu["seq"].reshape(-1)[int(rng.integers(m))].item() if m and rng.integers(3) else int(rng.integers(-50, 50))
        if isinstance(number, float) and number != number:
            number = 0.5
        cpu["input"] = gpu["input"] = float(number) if case["number_is_float"] else (abs(int(number)) if case["dtype"] == "uint8" else int(number))
        return cpu, gpu

    def fill_input(shape):
        t = make_values(case["in_dtype"], shape, case["in_dist"], case["data_seed"] + 1)
        if seq_values is not None and seq_values.numel() and t.numel():  # half of the queries hit a boundary exactly
            flat = seq_values.reshape(-1)
            hits = flat[torch.from_numpy(rng.integers(0, flat.numel(), size=t.numel()))].to(t.dtype).reshape(t.shape)
            t = torch.where(torch.from_numpy(rng.random(t.numel()) < 0.5).reshape(t.shape), hits, t)
        return t

    base, view = lay_out(case["in_shape"], case["in_layout"], fill_input)
    cpu["input"], gpu["input"] = view(base), view(base.to(device))
    return cpu, gpu


def launch(case: dict, gpu: dict, results: dict):
    """One call of the public API; returns its result as it came.  No copy between host and device is made here."""
    import vkradixsort_amd as vrs
    op = case["op"]
    if op in NEWER_OPS:
        return call_newer(vrs, case, gpu)
    if op in THIRD_OPS:
        return call_third(vrs, case, gpu)
    if case.get("variant") == "dependent":
        gpu["seq"] = results[case["source"]]  # what an earlier sort / unique of this window returned, possibly still being computed
    if op == "sort":
        return vrs.sort(gpu["x"], dim=case["dim"], descending=case["descending"])
    if op == "sort_values":
        return vrs.sort_values(gpu["x"], dim=case["dim"], descending=case["descending"])
    if op == "argsort":
        return vrs.argsort(gpu["x"], dim=case["dim"], descending=case["descending"])
    if op == "sort_rows":
        return vrs.sort_rows(gpu["x"], return_indices=case["return_indices"])
    if op == "topk":
        return vrs.topk(gpu["x"], case["k"], largest=case["largest"], sorted=case["sorted"])
    if op == "unique":
        return vrs.unique(gpu["x"], return_inverse=case["return_inverse"], return_counts=case["return_counts"])
    if op == "unique_consecutive":
        return vrs.unique_consecutive(gpu["x"], return_inverse=case["return_inverse"], return_counts=case["return_counts"])
    if op == "bucketize":
        return vrs.bucketize(gpu["input"], gpu["seq"], out_int32=case["out_int32"], right=case["right"])
    kw = {"out_int32": case["out_int32"], "right": case["right"], "sorter": gpu.get("sorter")}
    if case["side"] is not None:
        kw["side"] = case["side"]
    return vrs.searchsorted(gpu["seq"], gpu["input"], **kw)


def _as_tuple(result):
    return tuple(result) if isinstance(result, (tuple, list)) else (result,)


def check(case: dict, cpu: dict, result) -> list:
    """Every output against its reference; returns the lines of what differs (none: the case passed)."""
    import torch
    op = case["op"]
    got = [t.cpu() for t in _as_tuple(result)]
    if op in NEWER_OPS:
        return check_newer(case, cpu, got)
    if op in THIRD_OPS:
        return check_third(case, cpu, got)
    bad = []

    def same(name, g, w):
        line = _first_difference(name, g, w)
        if line:
            bad.append(line)

    if op in ("sort", "sort_values", "argsort"):
        x = cpu["x"]
        ref = ref_sort(x, case["dim"], case["descending"])
        want = {"sort": (ref.values, ref.indices), "sort_values": (ref.values,), "argsort": (ref.indices,)}[op]
        for name, g, w in zip(("values", "indices") if op != "argsort" else ("indices",), got, want):
            same(name, g, w)
    elif op == "sort_rows":
        values, indices = ref_sort_rows(cpu["x"])
        same("values", got[0], values)
        if case["return_indices"]:
            same("indices", got[1], indices)
    elif op == "topk":
        x, k = cpu["x"], case["k"]
        values, indices = ref_topk(x, k, case["largest"])
        gv, gi = got
        if not case["sorted"] and gi.dtype == torch.int64 and gi.shape == indices.shape and gi.numel():
            # as sorted multisets of (key, index): positions are distinct within a row, so ordering both sides by position does it
            same("values at the returned indices", gv, torch.gather(x, -1, gi.clamp(0, max(x.shape[-1] - 1, 0))))
            order = torch.argsort(gi, dim=-1, stable=True)
            gv, gi = torch.gather(gv, -1, order), torch.gather(gi, -1, order)
            order = torch.argsort(indices, dim=-1, stable=True)
            values, indices = torch.gather(values, -1, order), torch.gather(indices, -1, order)
        same("values", gv, values)
        same("indices", gi, indices)
        if not bad and plain_values(x) and k:
            rows = x.reshape(-1, x.shape[-1])
            free = torch.tensor([bool(np.unique(r).size == r.size) for r in order_key(rows)])  # tie-free rows: torch.topk is defined there
            if bool(free.any()):
                tv, ti = torch.topk(rows[free], k, dim=-1, largest=case["largest"], sorted=True)
                rv, ri = ref_topk(rows[free], k, case["largest"])
                same("values against torch.topk", rv, tv)
                same("indices against torch.topk", ri, ti)
    elif op in ("unique", "unique_consecutive"):
        x = cpu["x"]
        want = (ref_unique if op == "unique" else ref_unique_consecutive)(x)
        names = ["values"] + (["inverse"] if case["return_inverse"] else []) + (["counts"] if case["return_counts"] else [])
        if len(got) != len(names):
            bad.append(f"{len(got)} outputs returned, {len(names)} expected")
        picked = {"values": want[0], "inverse": want[1], "counts": want[2]}
        for name, g in zip(names, got):
            same(name, g, picked[name])
        if not bad and plain_values(x):
            fn = torch.unique if op == "unique" else torch.unique_consecutive
            tw = _as_tuple(fn(x, return_inverse=case["return_inverse"], return_counts=case["return_counts"]))
            for name, g, w in zip(names, got, tw):
                same(f"{name} against torch.{op}", g, w)
    else:
        seq = cpu["seq"]
        right = case["right"] or case.get("side") == "right"
        same("positions", got[0], ref_searchsorted(seq, cpu["input"], right, case["out_int32"], cpu.get("sorter")))
    return bad


def replay_line(seed: int, index: int, deck: str = "first") -> str:
    return f"python tools/fuzz_ops.py 0 {seed} --count {index + 1}" + ("" if deck == "first" else f" --deck {deck}")


def _report(seed: int, index: int, recent: list, what: list) -> str:
    lines = [f"fuzz_ops: seed {seed}, case {index} FAILED"] + [f"  {w}" for w in what]
    lines += ["the last cases (the failing one last):"] + ["  " + json.dumps(c, sort_keys=True) for c in recent[-8:]]
    lines.append("replay: " + replay_line(seed, index, recent[-1].get("deck", "first") if recent else "first"))
    return "\n".join(lines)


def run(seed: int, count: int, device=None, window: int = 4, seconds=None, quiet: bool = True, deck: str = "first") -> int:
    """Runs the first `count` cases of `seed` in `deck` (or as many as `seconds` allow) and returns how many ran and passed.  The inputs of a
    whole window are made and uploaded first, on a stream of their own, so that nothing waits for the streams the library works on;
    then the window's calls go out back to back on torch's current stream -- every fifth window on a second stream -- with no copy and
    no synchronisation between them, while the window before has not been looked at yet; that one is checked afterwards.  The first
    mismatch raises Mismatch, the first error is raised as it is; either way the report is printed first and nothing more is started
    on the GPU."""
    import itertools

    import torch

    device = torch.device(device if device is not None else "cuda:0")
    second, upload = torch.cuda.Stream(device), torch.cuda.Stream(device)
    started = time.monotonic()
    history, pending, results = [], [], {}
    done = 0

    def stop(case, error):
        print(_report(seed, case["index"], [c for c in history if c["index"] <= case["index"]], [f"{type(error).__name__}: {error}"]), flush=True)

    def settle(upto: int):
        """Checks the oldest `upto` pending cases, in order."""
        nonlocal done
        for rec in pending[:upto]:
            try:
                with torch.cuda.stream(rec.stream):
                    cpu = rec.inputs
                    if rec.case.get("variant") == "dependent":
                        cpu = dict(cpu, seq=results[rec.case["source"]].cpu())
                    bad = check(rec.case, cpu, rec.outputs)
            except Exception as e:  # (an asynchronous HIP error shows when the outputs are fetched)
                stop(rec.case, e)
                raise
            if bad:
                upto_here = [c for c in history if c["index"] <= rec.case["index"]]
                text = _report(seed, rec.case["index"], upto_here, bad)
                print(text, flush=True)
                raise Mismatch(text)
            done += 1
            if not quiet:
                print(f"ok {rec.case['index']} {rec.case['op']} {rec.case['dtype']}", flush=True)
        del pending[:upto]

    def launch_all(ready: list, stream):
        """The prepared cases' calls, one after the other: nothing here waits for the device (but unique, inside the library)."""
        with torch.cuda.stream(stream):
            for case, cpu, gpu in ready:
                try:
                    for t in gpu.values():
                        if isinstance(t, torch.Tensor):
                            t.record_stream(stream)  # (allocated on the upload stream)
                    out = launch(case, gpu, results)
                except Exception as e:
                    stop(case, e)
                    raise
                if case["op"] in ("sort", "sort_values", "unique"):
                    results[case["index"]] = _as_tuple(out)[0]  # what a dependent searchsorted of this window may search
                pending.append(_Pending(case, stream, cpu, out, _nbytes(list(gpu.values()), _as_tuple(out))))

    for _, group in itertools.groupby(cases(seed, count, window, deck), key=lambda c: c["window"]):
        if seconds is not None and time.monotonic() - started > seconds:
            break
        group = list(group)
        for index in [i for i in results if not any(i in (p.case["index"], p.case.get("source")) for p in pending)]:
            del results[index]
        history.extend(group)
        del history[:-(8 + 2 * window)]
        stream = second if group[0]["stream"] == "second" else torch.cuda.current_stream(device)
        before = len(pending)  # (the window launched last: still unchecked while this one goes out)
        ready, held = [], sum(p.nbytes for p in pending)
        for case in group:
            try:
                with torch.cuda.stream(upload):
                    cpu, gpu = prepare(case, device)
            except Exception as e:
                stop(case, e)
                raise
            ready.append((case, cpu, gpu))
            held += 2 * _nbytes(list(gpu.values()))  # (inputs and, about, as much again for the outputs)
            if held > PENDING_BYTES_CAP:  # the window closes early
                launch_all(ready, stream)
                settle(len(pending))
                ready, held, before = [], 0, 0
        launch_all(ready, stream)
        settle(before)
    settle(len(pending))
    torch.cuda.synchronize(device)
    return done


def main(argv) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="differential fuzz of the torch-level entry points")
    ap.add_argument("seconds", type=float, help="time budget of a soak (0 with --count)")
    ap.add_argument("seed", type=int)
    ap.add_argument("--count", type=int, default=None, help="run exactly the first COUNT cases instead of a time budget")
    ap.add_argument("--deck", default="first", choices=["first", "newer", "third"], help="which ops: the first deck's, the newer ops among them, or the third deck's")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    t0 = time.monotonic()
    if args.count is not None:
        done = run(args.seed, args.count, args.device, quiet=not args.verbose, deck=args.deck)
    else:
        done = run(args.seed, 1 << 30, args.device, seconds=args.seconds, quiet=not args.verbose, deck=args.deck)
    print(f"fuzz_ops: seed {args.seed}, deck {args.deck}: {done} cases passed in {time.monotonic() - t0:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
