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
DTYPE_BYTES = {"int8": 1, "uint8": 1, "int16": 2, "int32": 4, "int64": 8, "float16": 2, "bfloat16": 2, "float32": 4, "float64": 8}
FLOATS = ("float16", "bfloat16", "float32", "float64")
KEY32, KEY3264 = ["int32", "float32"], ["int32", "int64", "float32", "float64"]
# what each wrapper accepts (tests/test_ops_fuzz_cpu.py reads the same lists out of the wrappers' refusals)
OP_DTYPES = {"sort": DTYPES, "sort_values": DTYPES, "argsort": DTYPES, "sort_rows": KEY32, "topk": KEY32, "unique": KEY3264,
             "unique_consecutive": KEY3264, "searchsorted": DTYPES, "bucketize": DTYPES}
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
        pairs = [(op, dt) for op, dts in OP_DTYPES.items() for dt in dts for _ in range(OP_WEIGHT.get(op, 1))]
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


def cases(seed: int, count: int, window: int = 4):
    """`count` case descriptions of `seed`: plain dicts of numbers, strings and lists.  The same everywhere; needs no device."""
    return iter(_Gen(seed, count, window))


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


def replay_line(seed: int, index: int) -> str:
    return f"python tools/fuzz_ops.py 0 {seed} --count {index + 1}"


def _report(seed: int, index: int, recent: list, what: list) -> str:
    lines = [f"fuzz_ops: seed {seed}, case {index} FAILED"] + [f"  {w}" for w in what]
    lines += ["the last cases (the failing one last):"] + ["  " + json.dumps(c, sort_keys=True) for c in recent[-8:]]
    lines.append("replay: " + replay_line(seed, index))
    return "\n".join(lines)


def run(seed: int, count: int, device=None, window: int = 4, seconds=None, quiet: bool = True) -> int:
    """Runs the first `count` cases of `seed` (or as many as `seconds` allow) and returns how many ran and passed.  The inputs of a
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

    for _, group in itertools.groupby(cases(seed, count, window), key=lambda c: c["window"]):
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
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    t0 = time.monotonic()
    if args.count is not None:
        done = run(args.seed, args.count, args.device, quiet=not args.verbose)
    else:
        done = run(args.seed, 1 << 30, args.device, seconds=args.seconds, quiet=not args.verbose)
    print(f"fuzz_ops: seed {args.seed}: {done} cases passed in {time.monotonic() - t0:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
