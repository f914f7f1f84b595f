"""The case generator of tools/fuzz_ops.py reaches what it claims (no device): every case of the committed runs is classified with the
library's pure functions, and every op x dtype, tier, sort form, layout, distribution, flag and threshold edge has to occur.  This is
what keeps tests/test_gpu_ops_fuzz.py from quietly covering less after the generator is edited."""
import ctypes
import importlib
import importlib.util
import inspect
import math
import re
from pathlib import Path

import pytest
import torch

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

# (the package's functions sort, topk and unique shadow their modules' names)
search_mod, segmented_mod, sort_mod, topk_mod, unique_mod = (importlib.import_module("vkradixsort_amd." + name)
                                                             for name in ("search", "segmented", "sort", "topk", "unique"))

ROOT = Path(__file__).resolve().parent.parent


def _load():
    spec = importlib.util.spec_from_file_location("fuzz_ops", ROOT / "tools" / "fuzz_ops.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fuzz = _load()
NINE = {torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64}


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def all_cases():
    return [c for seed, count in fuzz.COMMITTED_RUNS for c in fuzz.cases(seed, count)]


def _refusal_dtypes(fn) -> set:
    """The dtypes a wrapper's own refusal names: '... takes int32, int64, float32 or float64, not {dtype}'."""
    found = re.search(r"takes ((?:\w+,\s+)*\w+\s+or\s+\w+), not", re.sub(r'"\s*f?"', "", inspect.getsource(fn)))
    assert found, fn
    return set(re.split(r",\s+|\s+or\s+", found.group(1)))


def accepted_dtypes() -> dict:
    nine = {str(d).split(".")[1] for d in NINE if _accepts_sort(d)}
    assert nine == _refusal_dtypes(sort_mod._dtype_code)
    return {"sort": nine, "sort_values": nine, "argsort": nine, "searchsorted": nine, "bucketize": nine,
            "sort_rows": _refusal_dtypes(segmented_mod.sort_rows), "topk": _refusal_dtypes(topk_mod.topk),
            "unique": _refusal_dtypes(unique_mod._check_tensor), "unique_consecutive": _refusal_dtypes(unique_mod._check_tensor)}


def _accepts_sort(dtype) -> bool:
    try:
        sort_mod._dtype_code(torch, dtype)
        return True
    except vrs.VrsError:
        return False


# ---- the classification of a description, by the wrappers' own rules and the library's pure functions -------------------------

def _numel(shape) -> int:
    return math.prod(shape)


def _segment_tier(lib, length, wide, pairs) -> str:
    fn = lib.vrs_segment_tier_for_u64 if wide else lib.vrs_segment_tier_for
    t, b, e = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    assert fn(0, length, length, int(pairs), capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT, ctypes.byref(t), ctypes.byref(b), ctypes.byref(e)) == 0
    return {capi.VRS_SEGMENT_WAVE: "wave", capi.VRS_SEGMENT_BLOCK: "block", capi.VRS_SEGMENT_GLOBAL: "global", capi.VRS_SEGMENT_ONE_CALL: "one_call"}[t.value]


def _topk_tier(lib, length) -> str:
    t, b, e = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_topk_tier_for(0, length, length, capi.TOPK_GRID_MIN_KEYS_DEFAULT, ctypes.byref(t), ctypes.byref(b), ctypes.byref(e)) == 0
    return {capi.VRS_TOPK_LDS: "lds", capi.VRS_TOPK_BLOCK: "block", capi.VRS_TOPK_GRID: "grid"}[t.value]


def _form(lib, n, key_bytes, pairs) -> str:
    form = ctypes.c_int()
    assert lib.vrs_sort_form_for(n, key_bytes, int(pairs), None, 0, ctypes.byref(form), None) == 0
    return capi.FORM_NAMES[form.value]


def _search_tier(lib, nb, m, nq, q_len, dtype) -> str:
    t = ctypes.c_int()
    code = sort_mod._dtype_code(torch, dtype)
    assert lib.vrs_search_tier_for(nb, m, nq, q_len, code, capi.SEARCH_LDS_BYTES_DEFAULT, capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT,
                                   capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT, ctypes.byref(t)) == 0
    return search_mod.TIER_NAMES[t.value]


def _promoted(case):
    seq = torch.empty(0, dtype=getattr(torch, case["dtype"]))
    if case["variant"] == "scalar":
        return torch.result_type(seq, 1.5 if case["number_is_float"] else 1)
    return torch.result_type(seq, torch.empty(0, dtype=getattr(torch, case["in_dtype"])))


def classify(lib, case) -> dict:
    """What the call of this description runs: {"segment": (wide, tier, length)}, {"form": (key bytes, pairs, form, n)},
    {"topk": (tier, length)}, {"search": (dtype name, tier, m, queries per row)}."""
    op, out = case["op"], {}
    if op in ("sort", "sort_values", "argsort"):
        shape = case["shape"]
        n = _numel(shape)
        if shape and n:
            length = shape[case["dim"] % len(shape)]
            wide = fuzz.DTYPE_BYTES[case["dtype"]] == 8
            pairs = op != "sort_values" or case["dtype"] in fuzz.FLOATS
            if length > 1 and n == length:
                out["form"] = (8 if wide else 4, pairs, _form(lib, n, 8 if wide else 4, pairs), n)
            elif length > 1:
                out["segment"] = (wide, _segment_tier(lib, length, wide, pairs), length)
    elif op == "sort_rows":
        rows, length = case["shape"]
        if rows * length:
            out["segment"] = (False, _segment_tier(lib, length, False, case["return_indices"]), length)
    elif op == "topk":
        if case["k"] and _numel(case["shape"]):
            out["topk"] = (_topk_tier(lib, case["shape"][-1]), case["shape"][-1])
    elif op == "unique":
        n = _numel(case["shape"])
        if n:
            kb = fuzz.DTYPE_BYTES[case["dtype"]]
            out["form"] = (kb, case["return_inverse"], _form(lib, n, kb, case["return_inverse"]), n)
    elif op in ("searchsorted", "bucketize") and case["variant"] != "dependent":
        seq = case["seq_shape"]
        nq = 1 if case["variant"] == "scalar" else _numel(case["in_shape"])
        if nq:
            q_len = nq if len(seq) == 1 else case["in_shape"][-1]
            dtype = _promoted(case)
            out["search"] = (str(dtype).split(".")[1], _search_tier(lib, _numel(seq), seq[-1], nq, q_len, dtype), seq[-1], q_len)
    return out


@pytest.fixture(scope="module")
def classes(lib, all_cases):
    return [classify(lib, c) for c in all_cases]


def _tensor_layouts(case):
    return [case[k]["kind"] for k in ("layout", "seq_layout", "in_layout") if k in case]


def _tensor_dists(case):
    return [case[k] for k in ("dist", "seq_dist", "in_dist") if k in case]


# ---- the assertions ------------------------------------------------------------------------------------------------------------

def test_the_generator_is_deterministic_and_plain():
    for seed, count in fuzz.COMMITTED_RUNS:
        a, b = list(fuzz.cases(seed, count)), list(fuzz.cases(seed, count))
        assert a == b and len(a) == count and [c["index"] for c in a] == list(range(count))
        import json
        assert json.loads(json.dumps(a)) == a  # plain descriptions: numbers, strings, lists, dicts
    first = [c for c in fuzz.cases(fuzz.COMMITTED_RUNS[0][0], 40)]
    other = [c for c in fuzz.cases(fuzz.COMMITTED_RUNS[0][0] + 1000, 40)]
    assert first != other
    assert len({seed for seed, _ in fuzz.COMMITTED_RUNS}) == len(fuzz.COMMITTED_RUNS)


def test_every_op_and_dtype_the_wrappers_accept_occurs(all_cases):
    accepted = accepted_dtypes()
    assert {op: set(d) for op, d in fuzz.OP_DTYPES.items()} == accepted
    seen = {(c["op"], c["dtype"]) for c in all_cases if c.get("variant") not in ("mixed", "dependent")}
    missing = {(op, dt) for op, dts in accepted.items() for dt in dts} - seen
    assert not missing, sorted(missing)


def test_every_search_tier_occurs_for_every_dtype_that_can_take_it(classes):
    seen = {c["search"][:2] for c in classes if "search" in c}
    for name in accepted_dtypes()["searchsorted"]:
        want = {"lds", "direct", "indexed"} | ({"table"} if fuzz.DTYPE_BYTES[name] <= 2 else set())
        assert {t for d, t in seen if d == name} == want, (name, sorted(seen))


def test_every_segmented_tier_of_both_key_widths_occurs(classes):
    seen = {c["segment"][:2] for c in classes if "segment" in c}
    assert seen == {(w, t) for w in (False, True) for t in ("wave", "block", "global", "one_call")}, sorted(seen)


def test_every_topk_tier_and_k_class_occurs(all_cases, classes):
    assert {c["topk"][0] for c in classes if "topk" in c} == {"lds", "block", "grid"}
    topk = [c for c in all_cases if c["op"] == "topk"]
    lengths = lambda c: c["shape"][-1]
    assert any(c["k"] == 1 for c in topk) and any(c["k"] == 2 for c in topk) and any(2 < c["k"] < 40 for c in topk)
    assert any(c["k"] == lengths(c) // 2 and c["k"] > 2 for c in topk) and any(c["k"] == lengths(c) - 1 and c["k"] > 2 for c in topk)
    assert any(c["k"] == lengths(c) and c["k"] > 2 for c in topk)
    assert any(c["k"] > capi.TOPK_SORT_IN_LDS_MAX_K and c["sorted"] for c in topk)  # the survivors' sort outside LDS
    assert {(c["largest"], c["sorted"]) for c in topk} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {len(c["shape"]) for c in topk} == {1, 2} and {c["dtype"] for c in topk} == {"int32", "float32"}


def test_the_one_call_sort_occurs_in_every_form_and_twice_at_a_pool_size(lib, all_cases, classes):
    grid = sorted({v for e in range(24) for v in (1 << e, (1 << e) + 1, 3 << e >> 1) if 0 < v <= fuzz.LARGE_ELEMENTS})
    seen = {c["form"][:3] for c in classes if "form" in c}
    for kb in (4, 8):
        for pairs in (False, True):
            reachable = {_form(lib, n, kb, pairs) for n in grid}
            if not pairs and kb == 4:
                assert "pool" in reachable  # (what the large minority is sized for)
            if pairs or kb == 8:
                reachable.discard("single")  # (one element: nothing any wrapper sorts)
            assert {f for k, p, f in seen if (k, p) == (kb, pairs)} >= reachable, (kb, pairs, sorted(seen))
    pool_min = min(n for n in grid if _form(lib, n, 4, False) == "pool")
    while _form(lib, pool_min - 1, 4, False) == "pool":
        pool_min -= 1
    # the kept-layout case: the same element count from the pool-form minimum on at least twice, with different values.  Bare keys are
    # in the pool form there, so these twins do meet a kept layout.  Key + payload pairs take the pool form only from the hybrid form's
    # minimum on, which lies above LARGE_ELEMENTS: the twins of pairs are drawn as the issue asks, at the bare keys' minimum or above,
    # but run the counted form and keep no layout.  Pairs in the pool form are covered by the scenario that
    # tests/test_gpu_ops_fuzz.py spells out, not by the generator.
    for pairs in (False, True):
        dists = {}
        for case, cls in zip(all_cases, classes):
            if "form" in cls and cls["form"][0] == 4 and cls["form"][1] == pairs and cls["form"][3] >= pool_min:
                dists.setdefault((cls["form"][3], cls["form"][2]), set()).add((case["dist"], case["data_seed"]))
        assert any(len({d for d, _ in v}) >= 2 for v in dists.values()), (pairs, dists)
        if not pairs:
            assert any(len({d for d, _ in v}) >= 2 for (_, form), v in dists.items() if form == "pool"), dists
        else:
            assert all(_form(lib, n, 4, True) != "pool" for n in grid), "pairs reach the pool form within LARGE_ELEMENTS now: have the generator draw them"


def test_every_threshold_has_its_three_edges(lib, all_cases, classes):
    t = fuzz.thresholds()

    def edges(values, cut, what):
        assert {cut - 1, cut, cut + 1} <= set(values), (what, cut, sorted(v for v in set(values) if abs(v - cut) < 3))

    assert all(cuts[2] == t.segment_one_call_min for cuts in t.segment.values())
    for which in (0, 1):  # the wave / block and block / global cuts: all three edges of one key width and kind at least
        assert any({cuts[which] - 1, cuts[which], cuts[which] + 1} <= {c["segment"][2] for c in classes if "segment" in c and c["segment"][0] == wide}
                   for (wide, _), cuts in t.segment.items()), ("segment", which)
    edges([c["segment"][2] for c in classes if "segment" in c], t.segment_one_call_min, "the one-call segment minimum")
    for cut in t.topk:
        edges([c["topk"][1] for c in classes if "topk" in c], cut, "top-k")
    one_row = [c["form"][3] for c in classes if "form" in c]
    for cut in t.form_cuts[4, False]:
        edges(one_row, cut, "one-call form")
    assert t.pool_min in t.form_cuts[4, False]
    rows = [c["search"] for c in classes if "search" in c]
    # (one threshold, VRS_TUNE_SEARCH_LDS_BYTES; the row length it allows depends on the rank's width: the edges of one width at least)
    assert any({cap - 2, cap - 1, cap} <= {m for d, _, m, _ in rows if t.search[d][0] == cap} for cap in {t.search[d][0] for d in fuzz.DTYPES})
    # (one threshold again, VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, of which a 1-byte dtype takes 1/256: the edges for one width at least)
    assert any({v - 1, v, v + 1} <= {q for d, _, _, q in rows if t.search[d][1] == v} for v in {t.search[d][1] for d in fuzz.DTYPES} - {None})
    index_min = {t.search[d][2] for d in fuzz.DTYPES}
    assert len(index_min) == 1
    edges([q for _, _, _, q in rows], index_min.pop(), "index minimum")
    sizes = [_numel(c[k]) for c in all_cases for k in ("shape", "seq_shape", "in_shape") if k in c]
    assert 0 in sizes and 1 in sizes
    shapes = [c[k] for c in all_cases for k in ("shape", "seq_shape", "in_shape") if k in c]
    assert any(1 in s and _numel(s) > 1 for s in shapes) and any(0 in s and len(s) > 1 for s in shapes) and [] in shapes
    small = sum(1 for c in all_cases if max(_numel(c[k]) for k in ("shape", "seq_shape", "in_shape") if k in c) <= fuzz.SMALL_ELEMENTS)
    assert small >= 0.7 * len(all_cases) and max(sizes) <= fuzz.LARGE_ELEMENTS
    # rows x length both ways: few long rows and many short rows
    sorts = [c for c in all_cases if c["op"] in ("sort", "sort_values", "argsort") and len(c["shape"]) >= 2 and _numel(c["shape"])]
    ratio = [(c["shape"][c["dim"] % len(c["shape"])], _numel(c["shape"]) // c["shape"][c["dim"] % len(c["shape"])]) for c in sorts]
    assert any(length >= 50 * rows for length, rows in ratio) and any(rows >= 50 * length for length, rows in ratio)


def test_every_layout_distribution_flag_and_stream_occurs(all_cases):
    assert {k for c in all_cases for k in _tensor_layouts(c)} == set(fuzz.LAYOUTS)
    assert {d for c in all_cases for d in _tensor_dists(c)} == set(fuzz.DISTS_FLOAT) | set(fuzz.DISTS_INT) | {"allbits"}
    steps = {c[k]["step"] for c in all_cases for k in ("layout", "seq_layout", "in_layout") if k in c and c[k]["kind"] == "strided"}
    assert steps == {2, 3}
    assert {c["stream"] for c in all_cases} == {"current", "second"}
    windows = {c["window"]: c["stream"] for c in all_cases}
    assert all((s == "second") == (w % 5 == 4) for w, s in windows.items())
    sorts = [c for c in all_cases if c["op"] in ("sort", "sort_values", "argsort")]
    assert {c["descending"] for c in sorts} == {False, True}
    assert any(c["dim"] < 0 for c in sorts) and any(c["dim"] == 0 and len(c["shape"]) >= 2 for c in sorts)
    assert any(len(c["shape"]) == 3 and c["layout"]["kind"] in ("strided", "transposed") for c in sorts)
    assert {c["return_indices"] for c in all_cases if c["op"] == "sort_rows"} == {False, True}
    for op in ("unique", "unique_consecutive"):
        assert {(c["return_inverse"], c["return_counts"]) for c in all_cases if c["op"] == op} == {(a, b) for a in (False, True) for b in (False, True)}
    search = [c for c in all_cases if c["op"] == "searchsorted"]
    assert {c["variant"] for c in search} == set(fuzz.SEARCH_VARIANTS)
    assert {(c["right"], c["side"]) for c in search} == {(False, None), (True, None), (False, "left"), (False, "right")}
    assert {c["sorter"] for c in search} == {False, True} and {c["out_int32"] for c in search} == {False, True}
    assert any(c["sorter"] and len(c["seq_shape"]) > 1 for c in search)
    assert {(c["dtype"], c["in_dtype"]) for c in search if c["variant"] == "mixed"} == {tuple(p[:2]) for p in fuzz.MIXED_PAIRS}
    for seq, inp, promoted in fuzz.MIXED_PAIRS:
        assert seq != inp and torch.result_type(torch.empty(0, dtype=getattr(torch, seq)), torch.empty(0, dtype=getattr(torch, inp))) == getattr(torch, promoted)
    bucket = [c for c in all_cases if c["op"] == "bucketize"]
    assert {c["right"] for c in bucket} == {False, True} and {c["out_int32"] for c in bucket} == {False, True}
    # the dependent case searches what an earlier sort or unique of its own window returned
    by_index = {(seed, c["index"]): c for seed, count in fuzz.COMMITTED_RUNS for c in fuzz.cases(seed, count)}
    sources = set()
    for (seed, index), c in by_index.items():
        if c.get("variant") == "dependent":
            src = by_index[seed, c["source"]]
            assert src["index"] < index and src["window"] == c["window"] and src["dtype"] == c["dtype"] and len(src["shape"]) == 1
            assert src["op"] in ("sort", "sort_values", "unique") and not src.get("descending") and src["dist"] != "specials"
            sources.add(src["op"])
    assert "unique" in sources and sources & {"sort", "sort_values"}


def test_no_case_leaves_an_ops_documented_domain(all_cases):
    accepted = accepted_dtypes()
    for c in all_cases:
        op = c["op"]
        assert c["dtype"] in accepted[op], c
        for key in ("shape", "seq_shape", "in_shape"):
            if key in c:
                assert _numel(c[key]) <= fuzz.LARGE_ELEMENTS < 1 << 32 and all(isinstance(v, int) and v >= 0 for v in c[key]), c
        for key in ("layout", "seq_layout", "in_layout"):
            if key in c:
                lay, shape = c[key], c[key.replace("layout", "shape")]
                assert lay["kind"] in fuzz.LAYOUTS
                if lay["kind"] == "transposed":
                    assert 0 <= lay["dims"][0] < lay["dims"][1] < len(shape), c
                if lay["kind"] == "expanded":
                    assert 0 <= lay["dim"] < len(shape), c
                if lay["kind"] == "offset":
                    assert 1 <= lay["by"] <= 3 and len(shape) >= 1, c
        if op in fuzz.CONTIGUOUS_ONLY:  # these wrappers refuse a non-contiguous tensor
            assert c["layout"]["kind"] in ("contiguous", "offset"), c
        if op in ("sort", "sort_values", "argsort"):
            nd = max(len(c["shape"]), 1)
            assert -nd <= c["dim"] < nd, c
        if op == "sort_rows":
            assert len(c["shape"]) == 2, c
        if op == "topk":
            assert len(c["shape"]) in (1, 2) and 0 <= c["k"] <= c["shape"][-1], c
        if op in ("searchsorted", "bucketize"):
            promoted = _promoted(c)
            assert promoted in NINE, c
            if c["variant"] == "dependent":
                continue
            assert c["seq_layout"]["kind"] != "expanded" and len(c["seq_shape"]) >= 1, c
            if c["variant"] == "scalar":
                assert len(c["seq_shape"]) == 1 and op == "searchsorted", c
            elif len(c["seq_shape"]) != 1:
                assert len(c["seq_shape"]) == len(c["in_shape"]) and c["seq_shape"][:-1] == c["in_shape"][:-1], c
            if op == "bucketize":
                assert len(c["seq_shape"]) == 1 and "sorter" not in c and "side" not in c and c["dtype"] == c["in_dtype"], c
            else:
                assert not (c["side"] == "left" and c["right"]), c
