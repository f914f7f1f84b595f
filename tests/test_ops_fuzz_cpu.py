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
    return {**{op: {name for name in fuzz.TEN if _wrapper_takes(op, name)} for op in fuzz.NEWER_OPS}, "sort": nine, "sort_values": nine, "argsort": nine, "searchsorted": nine, "bucketize": nine,
            "sort_rows": _refusal_dtypes(segmented_mod.sort_rows), "topk": _refusal_dtypes(topk_mod.topk),
            "unique": _refusal_dtypes(unique_mod._check_tensor), "unique_consecutive": _refusal_dtypes(unique_mod._check_tensor)}


def _wrapper_takes(op: str, name: str) -> bool:
    """Whether a newer wrapper takes the dtype, by its own refusals: called with small CPU tensors of the dtype, a wrapper that takes it
    gets as far as refusing tensors that are not on a GPU; one that does not refuses the dtype first, in whatever words it has for that.
    cumsum and cumprod take every real dtype (what the kernel does not write is converted first), so among the ten candidates their
    set is the ten; that the probe can say no there too is asserted with a complex dtype and, for cummax / cummin, a dtype without a code."""
    x = torch.zeros(4, dtype=getattr(torch, name))
    index, mask = torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.bool)
    calls = {"kthvalue": lambda: vrs.kthvalue(x, 1), "median": lambda: vrs.median(x, 0), "nanmedian": lambda: vrs.nanmedian(x, 0),
             "quantile": lambda: vrs.quantile(x, 0.5), "nanquantile": lambda: vrs.nanquantile(x, 0.5), "bincount": lambda: vrs.bincount(x),
             "histc": lambda: vrs.histc(x), "histogram": lambda: vrs.histogram(x, 2),
             "segment_reduce": lambda: vrs.segment_reduce(x, "max", lengths=torch.tensor([4])), "index_add": lambda: vrs.index_add(x, 0, index, x),
             "index_reduce": lambda: vrs.index_reduce(x, 0, index, x, "amax"), "scatter_reduce": lambda: vrs.scatter_reduce(x, 0, index, x, "amax"),
             "cumsum": lambda: vrs.cumsum(x, 0), "cumprod": lambda: vrs.cumprod(x, 0), "cummax": lambda: vrs.cummax(x, 0), "cummin": lambda: vrs.cummin(x, 0),
             "nonzero": lambda: vrs.nonzero(x), "argwhere": lambda: vrs.argwhere(x), "count_nonzero": lambda: vrs.count_nonzero(x),
             "masked_select": lambda: vrs.masked_select(x, mask), "masked_scatter": lambda: vrs.masked_scatter(x, mask, x),
             "mask_index": lambda: vrs.mask_index(x, mask), "mask_index_put": lambda: vrs.mask_index_put(x, mask, x)}
    try:
        calls[op]()
    except vrs.VrsError as e:
        return "on a GPU" in str(e)
    except RuntimeError:
        return False
    raise AssertionError(f"{op} took CPU tensors")


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
    missing = {(op, dt) for op in fuzz.FIRST_OPS for dt in accepted[op]} - seen  # (the newer ops: the newer deck's run, below)
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


# ==== the newer deck ==============================================================================================================
# the same claims for the committed run of deck "newer", and two that need no device either: torch's own CPU functions pass the fuzz's
# checks (the references and their bounds are right), and one changed element does not (they would notice).

scan_mod = importlib.import_module("vkradixsort_amd.scan")
FIRST_DECK_SHA256 = "8be40a9da0caad19ab49ab6ad19f6cd2b2add9c492a6b967ef1872ca5c491b6f"  # json.dumps(list(cases(104, 256)), sort_keys=True)


@pytest.fixture(scope="module")
def newer_cases():
    return [c for seed, count in fuzz.COMMITTED_RUNS_NEWER for c in fuzz.cases(seed, count, deck="newer")]


def test_the_first_decks_stream_is_what_it_was_before_the_newer_deck():
    import hashlib
    import json
    assert hashlib.sha256(json.dumps(list(fuzz.cases(104, 256)), sort_keys=True).encode()).hexdigest() == FIRST_DECK_SHA256
    assert fuzz.COMMITTED_RUNS == [(104, 256)]


def _scan_kernel_dtypes(case):
    """(what the kernel reads, what it writes) for a scan case, by scan._arith's own rule."""
    name = case["dtype"]
    if case["op"] in ("cummax", "cummin"):
        name = "uint8" if name == "bool" else name
        return name, name
    target = case["out_dtype"] or (name if name in fuzz.FLOATS else "int64")
    if target in scan_mod._KERNEL_OUT:
        direct = name == target or (target == "int64" and name in scan_mod._WIDENED)
        return (name if direct else target), target
    if target in fuzz.FLOATS:
        return "float32", "float32"
    return (target if target in scan_mod._WIDENED else "int64"), "int64"


def _sizes(case):
    return [_numel(case[k]) for k in ("shape", "seq_shape", "in_shape", "mask_shape", "source_shape") if k in case] + [case.get("n", 0), case.get("num_bins", 0)]


def classify_newer(lib, case) -> dict:
    """What a case of the newer ops runs, by the library's pure functions on the description alone."""
    t = fuzz.thresholds()
    op, out = case["op"], {}
    if op in fuzz.SELECT_OPS + fuzz.QUANTILE_OPS:
        shape = case["shape"]
        length = _numel(shape) if case["dim"] is None else shape[case["dim"] % len(shape)]
        out["select"] = (selection_names[t.select_tier(length, case["dtype"])], length)
        if op in fuzz.QUANTILE_OPS:
            sides = 2 if case["interpolation"] in ("linear", "midpoint") else 1
            out["quantile_path"] = "sort" if len(case["qs"]) * sides > capi.VRS_QUANTILE_MAX_TARGETS else "select"
    elif op in fuzz.COUNT_OPS:
        bins = case["num_bins"] if op == "bincount" else case["bins"]
        if op == "bincount":
            counter = 8 if case["weights"] not in (None, "float32") else 4
        else:
            counter = 8 if case.get("weight") and case["dtype"] == "float64" else 4
        if bins and (_numel(case["shape"]) if op != "bincount" else case["n"]):
            out["bincount"] = (counter, "global" if t.bincount_tier(bins, counter) == capi.VRS_BINCOUNT_GLOBAL else "lds", bins)
        if op == "histogram" and _numel(case["shape"]):
            n = _numel(case["shape"])
            out["search"] = (_search_tier(lib, bins + 1, bins + 1, n, n, getattr(torch, case["dtype"])), bins + 1, n)
    elif op == "segment_reduce":
        out["reduce_levels"] = (t.reduce_levels_of(case["longest"]), case["longest"])
    elif op in fuzz.REDUCE_OPS:
        n, M = case["n"], case["M"]
        out["form"] = (_form(lib, n, 4, True), n)
        out["search"] = (_search_tier(lib, n, n, M + 1, M + 1, torch.int32), n, M + 1)
    elif op in fuzz.SCAN_OPS:
        shape = case["shape"]
        if _numel(shape):
            dim = case["dim"] % len(shape)
            S, L, C = _numel(shape[:dim]), shape[dim], _numel(shape[dim + 1:])
            src, dst = _scan_kernel_dtypes(case)
            out["scan"] = (scan_mod.TIER_NAMES[t.scan_tier(S, L, C, src, dst, case["op"])], t.scan_levels_of(L), L)
    else:
        flags = _numel(case["mask_shape"] if "mask_shape" in case and case["op"] in ("mask_index", "mask_index_put") else
                       [max(a, b) for a, b in zip(case["shape"], case["mask_shape"])] if "mask_shape" in case else case["shape"])
        out["compact"] = (-(-flags // t.compact_tile), flags)
    return out


selection_names = importlib.import_module("vkradixsort_amd.selection").TIER_NAMES


@pytest.fixture(scope="module")
def newer_classes(lib, newer_cases):
    return [classify_newer(lib, c) if c["op"] in fuzz.NEWER_OPS else classify(lib, c) for c in newer_cases]


def test_the_newer_deck_is_deterministic_and_plain_and_leaves_the_first_alone():
    import json
    for seed, count in fuzz.COMMITTED_RUNS_NEWER:
        a, b = list(fuzz.cases(seed, count, deck="newer")), list(fuzz.cases(seed, count, deck="newer"))
        assert a == b and len(a) == count and [c["index"] for c in a] == list(range(count))
        assert json.loads(json.dumps(a)) == a
        assert a[:40] != list(fuzz.cases(seed + 1000, 40, deck="newer"))
    assert len(fuzz.COMMITTED_RUNS_NEWER) == 1 and fuzz.COMMITTED_RUNS_NEWER[0][1] == 256
    assert list(fuzz.cases(104, 32)) == list(fuzz.cases(104, 32, deck="first"))
    with pytest.raises(ValueError):
        fuzz.cases(1, 1, deck="both")


def test_every_newer_op_and_dtype_the_wrappers_accept_occurs(newer_cases):
    accepted = accepted_dtypes()
    assert set(fuzz.NEWER_OPS) == {"kthvalue", "median", "nanmedian", "quantile", "nanquantile", "bincount", "histc", "histogram", "segment_reduce",
                                   "index_add", "index_reduce", "scatter_reduce", "cumsum", "cumprod", "cummax", "cummin", "nonzero", "argwhere",
                                   "count_nonzero", "masked_select", "masked_scatter", "mask_index", "mask_index_put"}
    for op in fuzz.SCAN_OPS:  # (the scans refuse a dtype before the device too)
        assert not _wrapper_takes(op, "complex64"), op
    assert not _wrapper_takes("cummax", "uint16") and not _wrapper_takes("cummin", "uint16") and _wrapper_takes("cumsum", "uint16")
    seen = {(c["op"], c["dtype"]) for c in newer_cases}
    missing = {(op, dt) for op in fuzz.NEWER_OPS for dt in accepted[op]} - seen
    assert not missing, sorted(missing)


def test_every_newer_tier_occurs(newer_cases, newer_classes):
    assert {c["select"][0] for c in newer_classes if "select" in c} == {"lds", "block", "grid"}
    for ops in (fuzz.SELECT_OPS, fuzz.QUANTILE_OPS):
        assert {k["select"][0] for c, k in zip(newer_cases, newer_classes) if c["op"] in ops} == {"lds", "block", "grid"}, ops
    assert {c["quantile_path"] for c in newer_classes if "quantile_path" in c} == {"select", "sort"}
    assert {c["bincount"][:2] for c in newer_classes if "bincount" in c} == {(w, t) for w in (4, 8) for t in ("lds", "global")}
    assert {c["reduce_levels"][0] for c in newer_classes if "reduce_levels" in c} == {1, 2, 3}
    assert {c["scan"][0] for c in newer_classes if "scan" in c} == {"tile", "three_launch", "single_pass"}
    assert {c["scan"][1] for c in newer_classes if "scan" in c} >= {0, 1}
    searches = [k["search"][0] for c, k in zip(newer_cases, newer_classes) if "search" in k and c["op"] in fuzz.REDUCE_OPS]
    assert set(searches) == {"lds", "direct", "indexed"}, set(searches)
    assert len({k["search"][0] for c, k in zip(newer_cases, newer_classes) if c["op"] == "histogram" and "search" in k}) >= 2  # (bucketize over the edges)
    assert {c["compact"][0] for c in newer_classes if "compact" in c} >= {1, 2, 3, 5, 6}


def test_every_newer_threshold_has_its_three_edges(newer_cases, newer_classes):
    t = fuzz.thresholds()

    def edges(values, cut, what):
        assert {cut - 1, cut, cut + 1} <= set(values), (what, cut, sorted(v for v in set(values) if abs(v - cut) < 3))

    lengths = {}
    for c, k in zip(newer_cases, newer_classes):
        if "select" in k:
            lengths.setdefault(c["dtype"], []).append(k["select"][1])
    # the block tier begins where a row's ranks leave LDS, which the tier function decides from the rank's width alone: 4-byte ranks for
    # the seven dtypes of up to 4 bytes, 8-byte ranks for int64 and float64.  Three edges for each width's cut.
    widths = {}
    for d in fuzz.DTYPES:
        widths.setdefault(t.select[d][0], []).append(d)
    assert sorted(len(v) for v in widths.values()) == [2, 7] and sorted(widths[min(widths)]) == ["float64", "int64"]
    for cut, names in widths.items():
        edges([v for d in names for v in lengths.get(d, [])], cut, f"select block tier, {names}")
    assert len({t.select[d][1] for d in fuzz.DTYPES}) == 1
    edges([v for vs in lengths.values() for v in vs], t.select["float32"][1], "select grid tier")  # (the large minority)
    for counter in (4, 8):
        edges([k["bincount"][2] for k in newer_classes if "bincount" in k and k["bincount"][0] == counter], t.bincount[counter],
              f"bincount LDS tier, {counter}-byte counters")
    # histogram's bucketize over its bins + 1 edges: where that sequence leaves the search's LDS tier (float32's cut; float64's edge
    # tensors are drawn around theirs too, two cases a round)
    edges([k["search"][1] for c, k in zip(newer_cases, newer_classes) if c["op"] == "histogram" and c["dtype"] == "float32" and "search" in k],
          t.search["float32"][0], "histogram: the edges leave LDS")
    edges([k["reduce_levels"][1] for k in newer_classes if "reduce_levels" in k], t.reduce_levels[0], "two reduce levels")
    edges([k["reduce_levels"][1] for k in newer_classes if "reduce_levels" in k], t.reduce_levels[1], "three reduce levels")
    scans = [k["scan"][2] for k in newer_classes if "scan" in k]
    assert t.scan_cuts("float32", "float32", "cumsum")[0] == t.scan_levels[0]  # (one tile: where the three-launch tier and the first level begin)
    edges(scans, t.scan_levels[0], "scan tile")
    single = t.scan_cuts("float32", "float32", "cumsum")[1]
    assert single == t.scan_cuts("int32", "int32", "cumsum")[1] and single is not None
    edges(scans, single, "scan single pass")
    contributions = [c["n"] for c in newer_cases if c["op"] in fuzz.REDUCE_OPS and c["op"] != "segment_reduce"]
    for cut in t.form_cuts[4, 1]:
        edges(contributions, cut, "pair sort form")
    edges(contributions, t.search["int32"][0], "sorted indices leave LDS")
    edges([c["M"] + 1 for c in newer_cases if "M" in c], t.search["int32"][2], "destinations: the search index minimum")
    flags = [k["compact"][1] for k in newer_classes if "compact" in k]
    for tiles in (1, 2, 5):
        edges(flags, tiles * t.compact_tile, "compaction tiles")
    sizes = [v for c in newer_cases for v in _sizes(c)]
    assert max(sizes) == fuzz.LARGE_ELEMENTS and 0 in sizes
    small = sum(1 for c in newer_cases if max(_sizes(c)) <= fuzz.SMALL_ELEMENTS)
    assert small >= 0.7 * len(newer_cases)


def test_every_newer_class_of_argument_occurs(newer_cases):
    by_op = {}
    for c in newer_cases:
        by_op.setdefault(c["op"], []).append(c)
    newer = [c for c in newer_cases if c["op"] in fuzz.NEWER_OPS]
    assert {c["k_class"] for c in by_op["kthvalue"]} == set(fuzz.K_CLASSES)
    for c in by_op["kthvalue"]:
        L = c["shape"][c["dim"] % len(c["shape"])]
        assert c["k"] == max(1, min({"one": 1, "two": 2, "middle": (L + 1) // 2, "all_but_one": L - 1, "all": L}[c["k_class"]], L))
    select = [c for c in newer if c["op"] in fuzz.SELECT_OPS + fuzz.QUANTILE_OPS]
    assert {c["dim"] is None for c in select if c["op"] != "kthvalue"} == {False, True}
    assert any(c["dim"] is not None and c["dim"] < 0 for c in select) and any(c["dim"] == 0 and len(c["shape"]) > 1 for c in select)
    assert {c["keepdim"] for c in select} == {False, True}
    for ops in (("median", "nanmedian"), fuzz.QUANTILE_OPS):
        assert {c["nans"] for c in select if c["op"] in ops} == set(fuzz.NAN_KINDS), ops
    quant = [c for c in newer if c["op"] in fuzz.QUANTILE_OPS]
    assert {c["q_kind"] for c in quant} == set(fuzz.Q_KINDS) and {len(c["qs"]) for c in quant} == {1, 8, 9, 17}
    assert {c["interpolation"] for c in quant} == set(fuzz.INTERPOLATIONS)
    assert all(0.0 <= q <= 1.0 and float(torch.tensor(q, dtype=torch.float32)) == q for c in quant for q in c["qs"])
    assert {c["weights"] for c in by_op["bincount"]} == set(fuzz.BINCOUNT_WEIGHTS)
    assert any(0 < c["minlength"] < c["bins"] for c in by_op["bincount"]) and any(c["minlength"] > c["bins"] for c in by_op["bincount"])
    assert {c["range"] for c in by_op["histc"]} == {"explicit", "data", "constant"} and {c["value_class"] for c in by_op["histc"]} == {"exact", "general"}
    assert {(c["bins_kind"]) for c in by_op["histogram"]} == {"int", "int_range", "edges"} and {c["weight"] for c in by_op["histogram"]} == {False, True}
    seg = by_op["segment_reduce"]
    assert {c["reduce"] for c in seg} == {"sum", "mean", "max", "min", "prod"} and {c["initial"] for c in seg} == {None, 2}
    assert {c["bounds"] for c in seg} == {"lengths", "offsets"}
    assert any(0 in fuzz.segment_lengths(c["num_segments"], c["longest"], c["lengths_seed"]) for c in seg)
    assert {c["reduce"] for c in by_op["index_reduce"]} == {"prod", "mean", "amax", "amin"}
    assert {c["reduce"] for c in by_op["scatter_reduce"]} == {"sum", "prod", "mean", "amax", "amin"}
    index_forms = by_op["index_add"] + by_op["index_reduce"] + by_op["scatter_reduce"]
    assert {c["include_self"] for c in index_forms} == {False, True} and {c["alpha"] for c in by_op["index_add"]} == {1, 2}
    assert {c["destinations"] for c in index_forms} == set(fuzz.DESTINATIONS) and {c["index_dtype"] for c in index_forms} == {"int32", "int64"}
    assert {c["value_class"] for c in newer if "value_class" in c} == {"exact", "general", "wrap", "any", "count"}
    for op in ("segment_reduce", "index_add", "index_reduce", "scatter_reduce", "cumsum", "cumprod", "histogram", "bincount"):
        assert {"exact", "general"} <= {c["value_class"] for c in by_op[op]}, op
    for op in ("index_add", "index_reduce", "scatter_reduce"):  # the bound over several contributions to one destination
        assert any(c["value_class"] == "general" and c["destinations"] != "distinct" and c["n"] > 1 for c in by_op[op]), op
    assert any(c["value_class"] == "general" and c["longest"] > 1 for c in seg)
    assert sum(1 for c in by_op["bincount"] if c["weights"] is None and c["n"]) >= 2
    assert sum(1 for c in by_op["histogram"] if not c["weight"] and _numel(c["shape"])) >= 2
    scans = by_op["cumsum"] + by_op["cumprod"]
    assert any(c["out_dtype"] is not None and c["out_dtype"] != c["dtype"] for c in scans) and any(c["out_dtype"] is None for c in scans)
    masked = [c for c in newer if "mask_class" in c]
    assert {c["mask_class"] for c in masked} == set(fuzz.MASK_CLASSES)
    assert {c["broadcast"] for c in by_op["masked_select"] + by_op["masked_scatter"]} == {"same", "mask", "x"}
    rows = by_op["mask_index"] + by_op["mask_index_put"]
    assert {c["row_width"] for c in rows} == set(fuzz.ROW_WIDTHS) and {len(c["mask_shape"]) for c in rows} == {1, 2}
    assert {c["values"] for c in by_op["mask_index_put"]} == {"exact", "broadcast", "scalar"}
    assert {c["as_tuple"] for c in by_op["nonzero"]} == {False, True}
    layouts = {k for c in newer for k in _newer_layouts(c)}
    assert layouts == set(fuzz.LAYOUTS)
    assert any(fuzz.DTYPE_BYTES[c["dtype"]] <= 2 and c["layout"]["kind"] == "offset" for c in newer)  # 1 to 3 bytes into a word: what aligned() is for
    assert {c["stream"] for c in newer_cases} == {"current", "second"}
    assert all((c["stream"] == "second") == (c["window"] % 5 == 4) for c in newer_cases)


def _newer_layouts(case):
    return [case[k]["kind"] for k in ("layout", "mask_layout", "source_layout", "index_layout", "w_layout") if k in case]


def test_the_large_minority_and_both_pair_sort_kinds_occur(lib, newer_cases):
    t = fuzz.thresholds()
    large = [c for c in newer_cases if c["role"].startswith("large:")]
    assert [c["index"] for c in large] == [i for i in range(len(newer_cases)) if i % fuzz.LARGE_EVERY == fuzz.LARGE_AT]
    assert {c["role"].split(":")[1] for c in large} == set(fuzz.LARGE_KINDS_NEWER)
    # Key + payload pairs take the pool form only above LARGE_ELEMENTS with the default tunings (the first deck's test says the same of
    # its twins), and nothing here goes above that cap: the two kinds are drawn from the bare keys' pool minimum on, where the pair sort
    # behind index_add is the counted form's deferred sort.  If pairs reach the pool form within the cap, the generator draws them there.
    # (bisected up to a count where pairs are in the pool form, as tests/test_gpu_ops_fuzz.py's scenario finds it)
    assert _form(lib, 1 << 27, 4, True) == "pool" and _form(lib, 1, 4, True) != "pool"
    pairs_pool = fuzz._first(lambda v: _form(lib, v, 4, True) == "pool", 1, 1 << 27)
    assert _form(lib, pairs_pool, 4, True) == "pool" and _form(lib, pairs_pool - 1, 4, True) != "pool"
    assert pairs_pool > fuzz.LARGE_ELEMENTS and t.pool_min_pairs is None, "pairs reach the pool form within LARGE_ELEMENTS now: the two kinds move there"
    assert all(_form(lib, n, 4, True) != "pool" for n in t.form_cuts[4, True] + [fuzz.LARGE_ELEMENTS, fuzz.LARGE_ELEMENTS - 1])
    pool_min = t.pool_min_pairs or t.pool_min
    skewed = [c for c in large if c["role"] == "large:index_add_skewed"]
    assert skewed and all(c["op"] == "index_add" and c["M"] <= 50 and pool_min < c["n"] <= fuzz.LARGE_ELEMENTS for c in skewed)
    edge = [c for c in large if c["role"] == "large:index_add_pool_edge"]
    assert {c["n"] - pool_min for c in edge} <= {-1, 0, 1} and len({c["n"] for c in edge}) >= 2
    assert all(c["destinations"] == "distinct" and c["M"] >= c["n"] for c in edge)
    assert {c["shape"][-1] for c in large if c["role"] in ("large:masked_select_large", "large:nonzero_large")} == {fuzz.LARGE_ELEMENTS}
    assert all(c["num_bins"] >= 1 << 20 for c in large if c["role"] == "large:bincount_global")


def test_every_window_has_its_neighbour_and_a_sort_is_pending_before_a_newer_op(lib, newer_cases):
    windows = {}
    for c in newer_cases:
        windows.setdefault(c["window"], []).append(c)
    pending_windows = 0
    for w, group in windows.items():
        assert len(group) == 4
        old = [c for c in group if c["op"] in fuzz.FIRST_OPS]
        assert old, w
        first = group[0]
        if first["role"] == "pending_sort":
            assert first["op"] in ("sort", "sort_values", "unique") and len(first["shape"]) == 1 and first["shape"][0] >= capi.ONE_CALL_MIN_KEYS_DEFAULT
            assert "form" in classify(lib, first)  # (a one-call sort)
            assert any(c["op"] in fuzz.NEWER_OPS for c in group[1:])
            pending_windows += 1
    assert all(sum(1 for v in range(w0, w0 + 8) if windows[v][0]["role"] == "pending_sort") >= 1 for w0 in range(0, len(windows) - 7))
    assert pending_windows * 2 >= len(windows)  # every second neighbour


def test_no_newer_case_leaves_an_ops_documented_domain(newer_cases):
    accepted = accepted_dtypes()
    for c in newer_cases:
        op = c["op"]
        assert c["dtype"] in accepted[op], c
        assert max(_sizes(c)) <= fuzz.LARGE_ELEMENTS, c
        if op not in fuzz.NEWER_OPS:
            continue
        cls = c.get("value_class")
        if op in fuzz.SELECT_OPS + fuzz.QUANTILE_OPS:
            nd = len(c["shape"])
            assert nd >= 1 and _numel(c["shape"]) > 0 and (c["dim"] is None or -nd <= c["dim"] < nd), c
        if op == "bincount":
            assert c["bins"] - 1 <= {"uint8": 255, "int8": 127, "int16": 32767}.get(c["dtype"], 1 << 62) and c["minlength"] >= 0, c
        if op in ("histc", "histogram"):
            assert c["bins"] >= 1 and (op == "histogram" or c["lo"] <= c["hi"]), c
        if op == "segment_reduce":
            lengths = fuzz.segment_lengths(c["num_segments"], c["longest"], c["lengths_seed"])
            assert lengths.sum() == c["shape"][0] and lengths.max() == c["longest"] and lengths.min() >= 0, c
            terms, start, per_term = c["longest"], 2, 1
        if op in ("index_add", "index_reduce", "scatter_reduce"):
            assert c["shape"][c["dim"]] == c["M"] and c["source_shape"][c["dim"]] >= c["n"] and (c["destinations"] != "distinct" or c["M"] >= c["n"]), c
            assert op != "scatter_reduce" or len(c["shape"]) == 1, c
            terms, start, per_term = 1 if c["destinations"] == "distinct" else c["n"], 4, 2
        if op in ("cumsum", "cumprod") and _numel(c["shape"]):
            terms, start, per_term = c["shape"][c["dim"] % len(c["shape"])], 0, 1
        if op in fuzz.REDUCE_OPS + ("cumsum", "cumprod") and cls in ("exact", "general") and _numel(c["shape"]):
            out = (c.get("out_dtype") or c["dtype"]) if op in ("cumsum", "cumprod") else c["dtype"]
            if cls == "general":  # the condition of the bound: t * u < 0.1, the input or initial counted as a term
                assert (terms + 1) * fuzz.EPS[out] < 0.1, c
            elif c.get("reduce", "sum") != "prod" and op != "cumprod":  # every partial sum, in any order, is an integer the dtype holds
                assert start + terms * per_term <= fuzz.EXACT_LIMIT[out], c
        if op in ("mask_index", "mask_index_put"):
            assert c["shape"][:len(c["mask_shape"])] == c["mask_shape"], c


# ---- torch's own functions through check(): the references and their bounds are right ---------------------------------------------

class _Torch:
    """torch's CPU functions under the library's names and calling conventions."""

    def __getattr__(self, name):
        return getattr(torch, name)

    index_add = staticmethod(lambda x, d, i, s, alpha=1: torch.index_add(x, d, i.long(), s, alpha=alpha))
    index_reduce = staticmethod(lambda x, d, i, s, r, include_self=True: torch.index_reduce(x, d, i.long(), s, r, include_self=include_self))
    scatter_reduce = staticmethod(lambda x, d, i, s, r, include_self=True: torch.scatter_reduce(x, d, i.long(), s[:i.numel()], r, include_self=include_self))
    mask_index = staticmethod(lambda x, m: x[m])
    mask_index_put = staticmethod(lambda x, m, v: torch.index_put(x, (m,), v))
    masked_scatter = staticmethod(lambda x, m, s: torch.broadcast_tensors(x, m)[0].contiguous().masked_scatter(m, s))

    @staticmethod
    def histc(x, bins, min, max):
        """(float16 / bfloat16: torch sums float ones in the dtype and stops growing; its float32 counts of the same values, which the
        upcast keeps exactly, rounded to the dtype once as the op defines its counts)"""
        if x.dtype in (torch.float16, torch.bfloat16):
            return fuzz.as_count(torch.histc(x.float(), bins, min=min, max=max).long().numpy(), x.dtype)
        return torch.histc(x, bins, min=min, max=max)

    @staticmethod
    def segment_reduce(x, reduce, lengths=None, offsets=None, initial=None):
        kw = {"lengths": lengths.long()} if lengths is not None else {"offsets": offsets.long()}
        return torch.segment_reduce(x, reduce, initial=initial, **kw)

    @staticmethod
    def histogram(x, bins, range=None, weight=None):
        return torch.histogram(x, bins, weight=weight) if range is None else torch.histogram(x, bins, range=range, weight=weight)


# where torch has no such function on the CPU or defines the answer differently: by name, not computed
TORCH_SKIPS = {
    "segment_reduce of int32 / int64": lambda c: c["op"] == "segment_reduce" and c["dtype"] in ("int32", "int64"),                # torch has none
    "bincount of an empty input with weights": lambda c: c["op"] == "bincount" and c["n"] == 0 and c["weights"] is not None,      # torch: int64
    "histc outside the exact class": lambda c: c["op"] == "histc" and c["value_class"] != "exact",                                # another formula on the CPU
}
THROUGH_TORCH_ELEMENTS = fuzz.SMALL_ELEMENTS


def test_torchs_own_cpu_functions_pass_the_fuzzs_checks(newer_cases):
    """Every newer-op case of the committed run below SMALL_ELEMENTS: its inputs built on the CPU, the corresponding torch function run
    on them (on contiguous copies: this is about the references, and torch.median reads an expanded view wrongly), and torch's result
    handed to check() as if it were the library's.  It reports nothing: the references agree with torch bit for bit where they claim
    bits, and torch's own rounding stays within the bounds where they claim bounds."""
    ran = {}
    for c in newer_cases:
        if c["op"] not in fuzz.NEWER_OPS or max(_sizes(c)) > THROUGH_TORCH_ELEMENTS:
            continue
        if any(applies(c) for applies in TORCH_SKIPS.values()):
            continue
        cpu, _ = fuzz.prepare(c, None)
        result = fuzz.call_newer(_Torch(), c, {k: v.contiguous() for k, v in cpu.items()})
        assert fuzz.check(c, cpu, result) == [], c
        ran[c["op"]] = ran.get(c["op"], 0) + 1
    assert set(ran) == set(fuzz.NEWER_OPS), sorted(set(fuzz.NEWER_OPS) - set(ran))


# ---- one changed element: the references would notice ------------------------------------------------------------------------------

def _ulp_step(t, flat):
    """t with element `flat` moved to the next representable value (floats) or changed by one (integers, bool flipped)."""
    out = t.clone().reshape(-1)
    if t.dtype == torch.bool:
        out[flat] = ~out[flat]
    elif t.dtype.is_floating_point:
        bits = out.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
        bits[flat] += 1 if out[flat] >= 0 else -1  # (away from zero; of a finite value)
    else:
        out[flat] += 1
    return out.reshape(t.shape)


def _beyond(want, bound, flat, dtype):
    """The reference `want` (float64) as the dtype, element `flat` moved just beyond its bound."""
    out = want.to(dtype).reshape(-1).clone()
    target = want.reshape(-1)[flat] + 1.05 * bound.reshape(-1)[flat] + torch.finfo(dtype).tiny
    out[flat] = target.to(dtype)
    while (out[flat].double() - want.reshape(-1)[flat]).abs() <= bound.reshape(-1)[flat]:
        out = _ulp_step(out, flat) if out[flat] > 0 else out.index_fill(0, torch.tensor([flat]), torch.finfo(dtype).tiny)
    return out.reshape(want.shape)


def _as_returned(wants):
    return [w.want.to(w.dtype) if w.rule == "bound" else w.want for w in wants]


def test_one_changed_element_is_reported_by_name(newer_cases):
    """For one case per op (the first of the run below SMALL_ELEMENTS whose output has an element to change): the reference's own outputs
    pass check(), and with one element changed -- the last, or one in the second tile where there is one; 1 ulp where the rule is exact,
    just beyond the bound where it is a bound -- check() reports that output by its name."""
    tile = fuzz.thresholds().compact_tile
    seen, rules = {}, set()  # op -> the value classes done (a float sum or product: one case per class that occurs)
    for c in newer_cases:
        op, cls = c["op"], c.get("value_class")
        if op not in fuzz.NEWER_OPS or max(_sizes(c)) > fuzz.SMALL_ELEMENTS:
            continue
        if cls in seen.get(op, ()) or (op in seen and cls not in ("exact", "general")):
            continue
        cpu, _ = fuzz.prepare(c, None)
        wants = fuzz.reference_newer(c, cpu)
        if any(w.want.numel() == 0 or (w.rule in ("value", "bits") and w.want.dtype.is_floating_point and not torch.isfinite(w.want.reshape(-1)[-1]))
               for w in wants):
            continue
        outputs = _as_returned(wants)
        assert fuzz.check(c, cpu, tuple(outputs)) == [], c
        for which, w in enumerate(wants):
            n = w.want.numel()
            flat = tile + 1 if n > tile + 1 else n - 1
            changed = list(outputs)
            if w.rule == "index":  # (on a row without ties where there is one: a tie leaves the index open; else out of range)
                free = torch.nonzero(w.free.reshape(-1))
                changed[which] = outputs[which].clone()
                if free.numel():
                    changed[which].view(-1)[int(free[-1])] += 1
                else:
                    changed[which].view(-1)[flat] = w.rows.shape[w.dim]
            elif w.rule == "bound":
                if not torch.isfinite(w.want.reshape(-1)[flat]):
                    continue
                changed[which] = _beyond(w.want, w.bound, flat, w.dtype)
            else:
                changed[which] = _ulp_step(outputs[which], flat)
            lines = fuzz.check(c, cpu, tuple(changed))
            assert lines and any(line.startswith(w.name) for line in lines), (c, w.name, lines)
            rules.add(w.rule)
        seen.setdefault(op, set()).add(cls)
    assert set(seen) == set(fuzz.NEWER_OPS), sorted(set(fuzz.NEWER_OPS) - set(seen))
    assert {"exact", "general"} <= seen["cumsum"] | seen["cumprod"]
    assert {"exact", "general"} <= seen["index_add"] | seen["index_reduce"] | seen["scatter_reduce"] | seen["segment_reduce"]
    assert rules == {"bits", "value", "bound", "index"}


def test_a_swapped_pair_of_tied_indices_and_a_dropped_row_are_reported(newer_cases):
    x = torch.tensor([3, 5, 5, 1, 5], dtype=torch.int32)
    case = {"op": "cummax", "dtype": "int32", "dim": 0}
    values, indices = torch.cummax(x, 0)
    assert fuzz.check(case, {"x": x}, (values, indices)) == []
    swapped = indices.clone()
    swapped[2], swapped[4] = indices[1], indices[2]  # (the earlier of two equal values: still a position of the maximum)
    assert bool((x[swapped] == values).all())
    lines = fuzz.check(case, {"x": x}, (values, swapped))
    assert lines and lines[0].startswith("indices")
    c = next(c for c in newer_cases if c["op"] == "mask_index" and c["mask_class"] in ("half", "all") and max(_sizes(c)) <= fuzz.SMALL_ELEMENTS)
    cpu, _ = fuzz.prepare(c, None)
    rows = cpu["x"][cpu["mask"]]
    assert rows.shape[0] > 1 and fuzz.check(c, cpu, rows) == []
    lines = fuzz.check(c, cpu, rows[:-1])
    assert lines and lines[0].startswith("rows")


# ==== the third deck ==============================================================================================================
# repeat_interleave, isin, mode and the dim= forms of unique / unique_consecutive: the same claims for the committed run of deck "third".

NEWER_DECK_SHA256 = "6b27afadb6e94739b9f0755aab7ebd232b140dcdd7dd7e1947c800bd86bbd772"  # json.dumps(list(cases(491, 256, deck="newer")), sort_keys=True)
SEGMENT_TIERS = ("wave", "block", "global", "one_call")


@pytest.fixture(scope="module")
def third_cases():
    return [c for seed, count in fuzz.COMMITTED_RUNS_THIRD for c in fuzz.cases(seed, count, deck="third")]


def _third_takes(op: str, name: str) -> bool:
    """_wrapper_takes for repeat_interleave, isin and mode: with small CPU tensors of the dtype, a wrapper that takes it gets as far as
    refusing tensors that are not on a GPU; one that does not refuses the dtype first."""
    x, index = torch.zeros(4, dtype=getattr(torch, name)), torch.zeros(4, dtype=torch.int64)
    calls = {"repeat_interleave": lambda: vrs.repeat_interleave(x, index), "isin": lambda: vrs.isin(x, x), "mode": lambda: vrs.mode(x, 0)}
    try:
        calls[op]()
    except vrs.VrsError as e:
        return "on a GPU" in str(e)
    except RuntimeError:
        return False
    raise AssertionError(f"{op} took CPU tensors")


def accepted_third() -> dict:
    """What the third deck's wrappers accept, by their own refusals (the dim= forms look at the device before the dtype: their refusal's
    own list, as for the word forms)."""
    return {**{op: {name for name in fuzz.TEN if _third_takes(op, name)} for op in ("repeat_interleave", "isin", "mode")},
            "unique_dim": _refusal_dtypes(unique_mod._check_tensor), "unique_consecutive_dim": _refusal_dtypes(unique_mod._check_tensor)}


def _own(cases, op=None):
    return [c for c in cases if c["op"] in fuzz.THIRD_OPS and (op is None or c["op"] == op)]


def _sizes_third(case):
    return [_numel(case[k]) for k in ("shape", "test_shape") if k in case] + [case.get("total", 0) + case.get("extra", 0)]


def _isin_promoted(case) -> str:
    return fuzz._promoted_name(case["dtype"], case["test_dtype"])


def classify_third(lib, case) -> dict:
    """What a case of the third deck's ops runs, by the wrappers' own rules and the library's pure functions on the description alone:
    {"form": (key bytes, pairs, form, n)} of the one-call sort inside, {"segment": (wide, tier, length)}, {"search": (dtype, tier, m, q)},
    {"scan": (tier, runs)}, {"tiles": (row length, rows)}."""
    t = fuzz.thresholds()
    op, out = case["op"], {}
    if op == "mode":
        shape, n = case["shape"], _numel(case["shape"])
        if shape:
            length = shape[case["dim"] % len(shape)]
            wide = fuzz.DTYPE_BYTES[case["dtype"]] == 8
            out["tiles"] = (length, n // length)
            if length > 1 and n == length:   # vrs_sort_keys_u32 / _u64 of the ranks
                out["form"] = (8 if wide else 4, False, _form(lib, n, 8 if wide else 4, False), n)
            elif length > 1:                 # vrs_sort_segments_u32 / _u64 of the ranks
                out["segment"] = (wide, _segment_tier(lib, length, wide, False), length)
    elif op == "isin":
        m, q = _numel(case["test_shape"]), _numel(case["shape"])
        name = _isin_promoted(case)
        if m and q:
            out["search"] = (name, _search_tier(lib, m, m, q, q, getattr(torch, name)), m, q)
            if m > 1:  # sort_values of the test set: bare keys for the integers, key + position pairs for the floats
                kb, pairs = (8 if fuzz.DTYPE_BYTES[name] == 8 else 4), name in fuzz.FLOATS
                out["form"] = (kb, pairs, _form(lib, m, kb, pairs), m)
    elif op == "repeat_interleave":
        if case["form"] in ("one_arg", "tensor", "tensor_strided") and case["runs"]:
            out["scan"] = (scan_mod.TIER_NAMES[t.scan_tier(1, case["runs"], 1, case["repeats_dtype"], "int64", "cumsum")], case["runs"])
    else:
        N, C, word = case["N"], case["C"], fuzz.DTYPE_BYTES[case["dtype"]]
        if op == "unique_dim" and N > 1:  # one column: the word form's sort; more: a stable pair sort per 8 bytes of row
            kb, pairs = (word, case["return_inverse"]) if C == 1 else (8 if (C * word) % 8 == 0 or word == 8 else 4, True)
            out["form"] = (kb, pairs, _form(lib, N, kb, pairs), N)
    return out


@pytest.fixture(scope="module")
def third_classes(lib, third_cases):
    return [classify_third(lib, c) if c["op"] in fuzz.THIRD_OPS else {} for c in third_cases]


def test_both_older_decks_streams_are_what_they_were_before_the_third_deck():
    import hashlib
    import json
    assert hashlib.sha256(json.dumps(list(fuzz.cases(104, 256)), sort_keys=True).encode()).hexdigest() == FIRST_DECK_SHA256
    assert hashlib.sha256(json.dumps(list(fuzz.cases(491, 256, deck="newer")), sort_keys=True).encode()).hexdigest() == NEWER_DECK_SHA256
    assert fuzz.COMMITTED_RUNS == [(104, 256)] and fuzz.COMMITTED_RUNS_NEWER == [(491, 256)]
    assert not set(fuzz.THIRD_OPS) & set(fuzz.NEWER_OPS) and not set(fuzz.THIRD_OPS) & set(fuzz.FIRST_OPS)
    assert set(fuzz.OP_DTYPES) == set(fuzz.FIRST_OPS) | set(fuzz.NEWER_OPS) and set(fuzz.THIRD_OP_DTYPES) == set(fuzz.THIRD_OPS)


def test_the_third_deck_is_deterministic_and_plain():
    import json
    for seed, count in fuzz.COMMITTED_RUNS_THIRD:
        a, b = list(fuzz.cases(seed, count, deck="third")), list(fuzz.cases(seed, count, deck="third"))
        assert a == b and len(a) == count and [c["index"] for c in a] == list(range(count))
        assert json.loads(json.dumps(a)) == a
        assert a[:40] != list(fuzz.cases(seed + 1000, 40, deck="third"))
        assert all(c["deck"] == "third" for c in a)
    assert len(fuzz.COMMITTED_RUNS_THIRD) == 1 and fuzz.COMMITTED_RUNS_THIRD[0][1] == 256
    assert fuzz.replay_line(7, 3, "third").endswith("--deck third")


def test_every_third_op_and_dtype_the_wrappers_accept_occurs(third_cases):
    accepted = accepted_third()
    assert fuzz.THIRD_OPS == ("repeat_interleave", "isin", "mode", "unique_dim", "unique_consecutive_dim")
    assert {op: set(d) for op, d in fuzz.THIRD_OP_DTYPES.items()} == accepted
    assert not _third_takes("isin", "bool") and not _third_takes("mode", "bool") and _third_takes("repeat_interleave", "bool")
    seen = {(c["op"], c["dtype"]) for c in _own(third_cases)} | {("isin", c["test_dtype"]) for c in _own(third_cases, "isin")}
    missing = {(op, dt) for op in fuzz.THIRD_OPS for dt in accepted[op]} - seen
    assert not missing, sorted(missing)
    isin = _own(third_cases, "isin")
    for dt in accepted["isin"]:  # the nine dtypes on both sides
        assert any(c["dtype"] == dt for c in isin) and any(c["test_dtype"] == dt for c in isin), dt
    assert {(c["test_dtype"], c["dtype"]) for c in isin if c["variant"] == "mixed"} == {tuple(p[:2]) for p in fuzz.MIXED_PAIRS}
    assert all(_isin_promoted(c) == p for c in isin if c["variant"] == "mixed" for p in [dict((tuple(q[:2]), q[2]) for q in fuzz.MIXED_PAIRS)[c["test_dtype"], c["dtype"]]])
    assert {c["repeats_dtype"] for c in _own(third_cases, "repeat_interleave")} == {"int32", "int64"}


def test_every_third_tier_and_form_occurs(lib, third_cases, third_classes):
    assert {k["search"][1] for k in third_classes if "search" in k} == {"lds", "direct", "table", "indexed"}
    segments = {k["segment"][:2] for k in third_classes if "segment" in k}
    assert segments == {(w, t) for w in (False, True) for t in SEGMENT_TIERS}, sorted(segments)
    grid = sorted({v for e in range(24) for v in (1 << e, (1 << e) + 1, 3 << e >> 1) if 1 < v <= fuzz.LARGE_ELEMENTS})
    for op, kinds in (("mode", [(4, False), (8, False)]), ("isin", [(4, False), (4, True), (8, False), (8, True)]), ("unique_dim", [(4, True), (8, True)])):
        seen = {k["form"][:3] for c, k in zip(third_cases, third_classes) if c["op"] == op and "form" in k}
        for kb, pairs in kinds:  # every form of the one-call sort up to the cap, the pool form of bare 4-byte keys among them
            reachable = {_form(lib, n, kb, pairs) for n in grid}
            assert {f for b, p, f in seen if (b, p) == (kb, pairs)} >= reachable, (op, kb, pairs, sorted(seen))
    assert "pool" in {_form(lib, n, 4, False) for n in grid}
    assert {k["scan"][0] for k in third_classes if "scan" in k} >= {"tile", "three_launch"}


def test_every_third_threshold_has_its_three_edges(third_cases, third_classes):
    t = fuzz.thresholds()
    low, tile = capi.ONE_CALL_MIN_KEYS_DEFAULT, capi.RLE_TILE

    def edges(values, cut, what):
        assert {cut - 1, cut, cut + 1} <= set(values), (what, cut, sorted(v for v in set(values) if abs(v - cut) < 3))

    own = list(zip(third_cases, third_classes))
    # mode: one row around the one-call sort's form cuts of either rank width, the pool minimum among them; many rows around the segmented
    # sort's three cuts of either rank width (the third one, the one-call tier's, is one setting for both widths)
    for kb in (4, 8):
        for cut in t.form_cuts[kb, 0]:
            edges([k["form"][3] for c, k in own if c["op"] == "mode" and "form" in k and k["form"][0] == kb], cut, f"mode, one row, {kb}-byte ranks")
    assert t.pool_min in t.form_cuts[4, 0]
    for wide in (False, True):
        for cut in t.segment[wide, False][:2]:
            edges([k["segment"][2] for c, k in own if "segment" in k and k["segment"][0] == wide], cut, f"mode, many rows, wide {wide}")
    edges([k["segment"][2] for c, k in own if "segment" in k], t.segment_one_call_min, "mode, many rows, the one-call tier")
    for kind in ("mode_pool_skewed", "mode_pool_uniform"):
        edges([c["shape"][0] for c in third_cases if c["role"] == "large:" + kind], t.pool_min, kind)
    tiles = [k["tiles"] for c, k in own if "tiles" in k]
    for length in fuzz.MODE_SHORT:  # at least three full tiles of the run tables
        assert any(L == length and rows * L >= 3 * tile for L, rows in tiles), length
    assert {tile - 1, tile, tile + 1} <= {L for L, _ in tiles}
    # isin: the search's three cuts for the promoted dtype, the one-call minimum and the sort's form cuts for the test set
    searches = [k["search"] for c, k in own if "search" in k]
    out4 = t.search["int32"][0]
    assert {t.search[d][0] for d in fuzz.DTYPES} == {out4, t.search["int64"][0]}
    edges([m for d, _, m, _ in searches if t.search[d][0] == out4], out4, "isin: the test set leaves LDS")
    assert t.search["int64"][0] in [m for d, _, m, _ in searches if fuzz.DTYPE_BYTES[d] == 8]
    edges([q for d, _, _, q in searches if fuzz.DTYPE_BYTES[d] == 1], t.search["int8"][1], "isin: the table's minimum of queries")
    assert t.search["int16"][1] in [q for d, _, _, q in searches if fuzz.DTYPE_BYTES[d] == 2]
    edges([q for d, _, _, q in searches if fuzz.DTYPE_BYTES[d] >= 4], t.search["int32"][2], "isin: the index's minimum of queries")
    bare = [k["form"][3] for c, k in own if c["op"] == "isin" and "form" in k and k["form"][:2] == (4, False)]
    for cut in t.form_cuts[4, 0]:
        edges(bare, cut, "isin: the test set's sort of bare 4-byte keys")
    edges(bare, low, "isin: the one-call minimum, bare keys")
    edges([k["form"][3] for c, k in own if c["op"] == "isin" and "form" in k and k["form"][:2] != (4, False)], low, "isin: the one-call minimum, pairs or 8-byte keys")
    # repeat_interleave: runs around the scan's cuts for repeats -> int64, totals around 1, 2 and 5 chunks
    repeats = _own(third_cases, "repeat_interleave")
    cuts = [c for c in t.scan_cuts("int32", "int64", "cumsum") if c and c < fuzz.SMALL_ELEMENTS // 2]
    assert cuts == [c for c in t.scan_cuts("int64", "int64", "cumsum") if c and c < fuzz.SMALL_ELEMENTS // 2] == [t.scan_levels[0]]  # (the int64 output's tile)
    for cut in cuts:
        edges([c["runs"] for c in repeats if c["rep_class"] != "equal"], cut, "repeat_interleave: runs")
        assert {c["repeats_dtype"] for c in repeats if c["rep_class"] != "equal" and abs(c["runs"] - cut) <= 1} == {"int32", "int64"}
    for chunks in (1, 2, 5):
        edges([c["total"] for c in repeats], chunks * fuzz.REPEAT_CHUNK, "repeat_interleave: total")
    # unique(dim=) / unique_consecutive(dim=): N around the encode's tile, the one-call minimum and the pair sort's form cuts
    for op in ("unique_dim", "unique_consecutive_dim"):
        rows = [c["N"] for c in _own(third_cases, op)]
        for cut in {tile, low, *t.form_cuts[4, 1], *t.form_cuts[8, 1]}:
            edges(rows, cut, op)
        assert max(rows) > tile + 1 and any(tile + 1 < n < low - 1 or low + 1 < n for n in rows)
    sizes = [v for c in _own(third_cases) for v in _sizes_third(c)]
    assert max(sizes) == fuzz.LARGE_ELEMENTS and 0 in sizes
    small = sum(1 for c in third_cases if c["op"] not in fuzz.THIRD_OPS or max(_sizes_third(c)) <= fuzz.SMALL_ELEMENTS)
    assert small >= 0.7 * len(third_cases)


def test_every_third_class_of_argument_occurs(third_cases):
    both = {False, True}
    mode = _own(third_cases, "mode")
    assert {c["values"] for c in mode if c["dtype"] in fuzz.FLOATS} >= set(fuzz.MODE_CLASSES)
    assert {c["values"] for c in mode if c["dtype"] not in fuzz.FLOATS} >= set(fuzz.MODE_CLASSES[:-1])
    assert {c["keepdim"] for c in mode} == both and {c["layout"]["kind"] for c in mode} == set(fuzz.LAYOUTS)
    assert any(c["dim"] < 0 for c in mode) and {c["dim"] % len(c["shape"]) for c in mode if len(c["shape"]) == 3} == {0, 1, 2}
    assert [] in [c["shape"] for c in mode] and {c["size"] for c in mode} == {"one_row", "many_rows", "short", "tile_len", "tiny", "large"}
    isin = _own(third_cases, "isin")
    assert {c["variant"] for c in isin} == set(fuzz.ISIN_VARIANTS)
    assert {c["invert"] for c in isin} == both and {c["assume_unique"] for c in isin} == both
    assert {c["share"] for c in isin} == set(fuzz.ISIN_SHARES) and {c["nans"] for c in isin} == set(fuzz.ISIN_NANS)
    assert {c["signed_zero"] for c in isin if _isin_promoted(c) in fuzz.FLOATS} == both
    assert {c["layout"]["kind"] for c in isin} == set(fuzz.LAYOUTS) and {c["test_layout"]["kind"] for c in isin} == set(fuzz.LAYOUTS)
    assert any(c["shape"] == [] and c["variant"] != "number_elements" for c in isin) and any(_numel(c["shape"]) == 0 for c in isin)
    assert any(_numel(c["test_shape"]) == 0 for c in isin) and any(len(c["test_shape"]) >= 2 and _numel(c["test_shape"]) > 1 for c in isin)
    assert any(len(c["shape"]) >= 2 and _numel(c["shape"]) > 1 for c in isin)
    repeats = _own(third_cases, "repeat_interleave")
    assert {c["form"] for c in repeats} == set(fuzz.REPEAT_FORMS) and {c["rep_class"] for c in repeats} == set(fuzz.REPEAT_CLASSES) | {"equal"}
    assert {c["output_size"] for c in repeats} == set(fuzz.OUTPUT_SIZES)
    for form in ("one_arg", "tensor"):
        assert {c["output_size"] for c in repeats if c["form"] == form} == set(fuzz.OUTPUT_SIZES), form
    assert {c["repeats_layout"]["kind"] for c in repeats} == {"contiguous", "strided", "offset"}
    with_input = [c for c in repeats if c["form"] != "one_arg"]
    assert {c["dim"] is None for c in with_input} == both and any(c["dim"] is not None and c["dim"] < 0 for c in with_input)
    assert {c["dim"] % len(c["shape"]) for c in with_input if c["dim"] is not None and len(c["shape"]) == 3} == {0, 1, 2}
    assert {c["layout"]["kind"] for c in with_input} == set(fuzz.LAYOUTS)
    assert any(c["total"] == 0 for c in repeats) and any(c["runs"] == 0 for c in repeats)
    for op in ("unique_dim", "unique_consecutive_dim"):
        rows = _own(third_cases, op)
        assert {(c["return_inverse"], c["return_counts"]) for c in rows} == {(a, b) for a in both for b in both}, op
        assert {c["C"] for c in rows} == set(fuzz.UNIQUE_COLUMNS) and {c["layout"]["kind"] for c in rows} == set(fuzz.LAYOUTS), op
        assert {c["rows"] for c in rows if c["dtype"] in fuzz.FLOATS} >= set(fuzz.ROW_CLASSES), op
        assert {c["rows"] for c in rows if c["dtype"] not in fuzz.FLOATS} >= set(fuzz.ROW_CLASSES[:-1]), op
        assert {len(c["shape"]) for c in rows} == {2, 3} and {(len(c["shape"]), c["dim"] % len(c["shape"])) for c in rows} == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}, op
        assert any(c["dim"] < 0 for c in rows), op
        assert all(c["C"] * fuzz.DTYPE_BYTES[c["dtype"]] > 8 for c in rows if c["rows"] == "behind_top"), op
    assert {c["stream"] for c in third_cases} == {"current", "second"}
    assert all((c["stream"] == "second") == (c["window"] % 5 == 4) for c in third_cases)
    assert {c["stream"] for c in _own(third_cases, "isin")} == {"current", "second"}


def test_the_third_decks_large_minority_occurs(third_cases):
    t = fuzz.thresholds()
    large = [c for c in third_cases if c["role"].startswith("large:")]
    assert [c["index"] for c in large] == [i for i in range(len(third_cases)) if i % fuzz.LARGE_EVERY == fuzz.LARGE_AT]
    kinds = {}
    for c in large:
        kinds.setdefault(c["role"].split(":")[1], []).append(c)
    assert set(kinds) == set(fuzz.LARGE_KINDS_THIRD) and len(set(fuzz.LARGE_KINDS_THIRD)) == 10
    for kind in ("mode_pool_skewed", "mode_pool_uniform"):
        assert all(c["op"] == "mode" and c["dtype"] in ("int32", "float32") and len(c["shape"]) == 1 and abs(c["shape"][0] - t.pool_min) <= 1 for c in kinds[kind])
        assert {c["values"] for c in kinds[kind]} == {"thousand" if kind == "mode_pool_skewed" else "uniform"}
    assert {c["dtype"] for c in kinds["mode_pool_skewed"]} == {"int32", "float32"}
    assert all(sorted(c["shape"]) == [3, 1 << 20] and c["shape"][c["dim"]] == 3 for c in kinds["mode_rows_of_3"])
    assert all(c["dtype"] == "int64" and c["shape"] == [1 << 22] for c in kinds["mode_int64_row"])
    assert all(abs(_numel(c["test_shape"]) - t.pool_min) <= 1 and c["shape"] == [1 << 20] and fuzz.DTYPE_BYTES[c["dtype"]] == 4 for c in kinds["isin_pool"])
    assert "int32" in {c["dtype"] for c in kinds["isin_pool"]}  # (bare keys: the pool form)
    assert len({_numel(c["test_shape"]) for c in kinds["isin_pool"]}) >= 2
    assert all(c["dtype"] == "int16" and c["shape"] == [1 << 23] and c["test_shape"] == [10_000] for c in kinds["isin_int16"])
    assert all(c["runs"] == 1 << 10 and c["total"] == 1 << 23 for c in kinds["repeat_few_runs"])
    assert all(c["runs"] == 1 << 22 and c["total"] == 1 << 23 for c in kinds["repeat_many_runs"])
    assert all(c["shape"] == [1 << 21, 3] and c["dtype"] == "int32" and c["rows"] == "thousand" for c in kinds["unique_dim_large"])


def test_every_third_window_has_its_neighbour_and_every_second_its_pending_sort(lib, third_cases):
    windows = {}
    for c in third_cases:
        windows.setdefault(c["window"], []).append(c)
    origins = set()
    for w, group in windows.items():
        assert len(group) == 4
        old = [c for c in group if c["op"] not in fuzz.THIRD_OPS]
        assert old and any(c["op"] in fuzz.THIRD_OPS for c in group), w
        origins |= {"first" if c["op"] in fuzz.FIRST_OPS else "newer" for c in old}
        first = group[0]
        assert (first["role"] == "pending_sort") == (w % 2 == 0), w
        if w % 2 == 0:
            assert first["op"] in ("sort", "sort_values", "unique") and len(first["shape"]) == 1 and first["shape"][0] >= capi.ONE_CALL_MIN_KEYS_DEFAULT
            assert "form" in classify(lib, first) and group[1]["op"] in fuzz.THIRD_OPS  # (the next op's settle_pending meets it)
        else:
            assert group[-1]["role"] == "neighbour"
    assert origins == {"first", "newer"}
    behind = {windows[w][1]["op"] for w in windows if w % 2 == 0}
    assert behind == set(fuzz.THIRD_OPS), behind  # each of the five ops runs straight behind someone else's pending sort


def test_no_third_case_leaves_an_ops_documented_domain(third_cases):
    accepted = {**accepted_dtypes(), **accepted_third()}
    for c in third_cases:
        op = c["op"]
        assert c["dtype"] in accepted[op], c
        if op not in fuzz.THIRD_OPS:
            continue
        assert max(_sizes_third(c)) <= fuzz.LARGE_ELEMENTS < 1 << 32, c
        nd = max(len(c["shape"]), 1)
        if op == "mode":
            assert -nd <= c["dim"] < nd and _numel(c["shape"]) > 0, c
        elif op == "isin":
            assert c["test_dtype"] in accepted[op] and getattr(torch, _isin_promoted(c)) in NINE, c
            assert not (c["variant"] == "number_elements" and c["variant"] == "number_tests"), c
        elif op == "repeat_interleave":
            r = fuzz.make_repeats(c["runs"], c["rep_class"], c["total_target"], c["rep_seed"]) if c["rep_class"] != "equal" else fuzz.np.full(c["runs"], c["k"])
            assert len(r) == c["runs"] and int(r.min(initial=0)) >= 0 and int(r.sum()) == c["total"] < 1 << 32, c
            assert c["extra"] >= 0 and (c["extra"] > 0) == (c["output_size"] == "too_large"), c  # output_size is never below the true total
            assert c["total_target"] is None or c["total"] == c["total_target"], c
            assert c["repeats_dtype"] in ("int32", "int64") and c["total"] <= torch.iinfo(torch.int32).max, c
            if c["form"] == "one_arg":
                assert c["dtype"] == c["repeats_dtype"] and c["dim"] is None, c
            else:
                assert c["dim"] is None or -nd <= c["dim"] < nd, c
                assert (_numel(c["shape"]) if c["dim"] is None else c["shape"][c["dim"]]) == c["runs"], c
            assert not (c["output_size"] == "too_large" and (c["runs"] == 0 or c["form"] == "int")), c
        else:
            assert -nd <= c["dim"] < nd and c["shape"][c["dim"]] == c["N"] and _numel(c["shape"]) == c["N"] * c["C"], c
            assert 1 <= c["C"] < 1 << 23 and c["N"] >= 1 and len(c["shape"]) in (2, 3), c


# ---- torch's and numpy's own functions through check(): the third deck's references are right -------------------------------------------

def _has_nan(cpu) -> bool:
    x = cpu["x"]
    return x.dtype.is_floating_point and bool(torch.isnan(x).any())


# what is not handed to check(), by name (the first one leaves the values in: only the index is the reference's own)
THIRD_SKIPS = {
    "mode's index, where torch's choice is unspecified": lambda c, cpu: False,
    "mode with NaNs": lambda c, cpu: c["op"] == "mode" and _has_nan(cpu),
    "unique*_dim of floats with NaN or -0.0": lambda c, cpu: c["op"].endswith("_dim") and not fuzz.plain_values(cpu["x"]),
    "a too-large output_size": lambda c, cpu: c["op"] == "repeat_interleave" and c["output_size"] == "too_large",
}


class _Independent:
    """The third deck's ops by other means than the references take: torch.mode's values (the index is the reference's), numpy's isin and
    repeat, torch.unique(dim=) / torch.unique_consecutive(dim=)."""

    @staticmethod
    def mode(x, dim, keepdim):
        d = dim % max(x.dim(), 1)
        index = fuzz.ref_mode(x, d)[1]
        index = index if keepdim or not x.dim() else index.squeeze(d)
        exact = x.double() if x.dtype.is_floating_point else x.long()
        return (torch.mode(exact, dim, keepdim).values.to(x.dtype) if x.dim() else x.clone()), index

    @staticmethod
    def isin(elements, tests, assume_unique=False, invert=False):
        common = torch.result_type(elements, tests)
        up = torch.float32 if common in (torch.float16, torch.bfloat16) else common
        e, t = (v.to(up) if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=up) for v in (elements, tests))
        return torch.from_numpy(fuzz.np.asarray(fuzz.np.isin(e.contiguous().numpy(), t.contiguous().numpy(), invert=invert)))

    @staticmethod
    def repeat_interleave(x, repeats=None, dim=None, output_size=None):
        np = fuzz.np
        if repeats is None:
            return torch.from_numpy(np.repeat(np.arange(x.numel()), x.numpy())).to(x.dtype)
        r = repeats.reshape(-1).numpy() if isinstance(repeats, torch.Tensor) else repeats
        r = int(r[0]) if not isinstance(r, int) and r.size == 1 else r
        bits = fuzz.to_bits(x.view(torch.uint8) if x.dtype == torch.bool else x)
        out = np.repeat(bits.reshape(-1) if dim is None else bits, r, axis=0 if dim is None else dim)
        return fuzz.from_bits(out.reshape(-1), "uint8" if x.dtype == torch.bool else str(x.dtype).split(".")[1]).reshape(out.shape).view(x.dtype)

    unique = staticmethod(lambda x, **kw: torch.unique(x, **kw))
    unique_consecutive = staticmethod(lambda x, **kw: torch.unique_consecutive(x, **kw))


def test_torchs_and_numpys_own_functions_pass_the_third_decks_checks(third_cases):
    """Every case of the third deck's ops in the committed run below SMALL_ELEMENTS, but those THIRD_SKIPS names: the op by other means
    (contiguous copies: this is about the references) handed to check() as if it were the library's result.  It reports nothing.  And the
    conditions on the run: no case is without its numpy / torch reference, and at least half of the float cases of mode and of the two dim=
    forms are plain, so that torch's own answer is compared as well."""
    ran, skipped, plain, floats = {}, {}, {}, {}
    for c in _own(third_cases):
        if max(_sizes_third(c)) > THROUGH_TORCH_ELEMENTS:
            continue
        cpu, _ = fuzz.prepare(c, None)
        op = c["op"]
        if op != "isin" and c["dtype"] in fuzz.FLOATS and "x" in cpu and op != "repeat_interleave":
            floats[op] = floats.get(op, 0) + 1
            plain[op] = plain.get(op, 0) + (not _has_nan(cpu) if op == "mode" else fuzz.plain_values(cpu["x"]))
        named = [name for name, applies in THIRD_SKIPS.items() if applies(c, cpu)]
        if named:
            skipped[named[0]] = skipped.get(named[0], 0) + 1
            continue
        result = fuzz.call_third(_Independent(), c, {k: v.contiguous() if isinstance(v, torch.Tensor) else v for k, v in cpu.items()})
        assert fuzz.check(c, cpu, result) == [], c
        ran[op] = ran.get(op, 0) + 1
    assert set(ran) == set(fuzz.THIRD_OPS)
    print(f"through torch / numpy: {sum(ran.values())} cases ran, skipped by name: {skipped}; plain float cases: {plain} of {floats}")
    for op in ("mode", "unique_dim", "unique_consecutive_dim"):
        assert 2 * plain[op] >= floats[op] > 0, (op, plain, floats)
    assert sum(skipped.values()) * 4 <= sum(ran.values())


# ---- one changed element: the third deck's references would notice --------------------------------------------------------------------

def _first_case(cases, op, ok):
    for c in _own(cases, op):
        if max(_sizes_third(c)) <= 20_000:
            cpu, _ = fuzz.prepare(c, None)
            found = ok(c, cpu)
            if found is not None and found is not False:
                return c, cpu, found
    raise AssertionError(f"no {op} case of the committed run fits")


def _named(c, cpu, outputs, name):
    lines = fuzz.check(c, cpu, tuple(outputs))
    assert lines and lines[0].startswith(name), (c, name, lines)


def test_one_changed_element_of_a_third_deck_output_is_reported_by_name(third_cases):
    np = fuzz.np
    # isin: a flipped bool
    c, cpu, _ = _first_case(third_cases, "isin", lambda c, cpu: _numel(c["shape"]) > 5 and _numel(c["test_shape"]) > 0)
    want = fuzz.ref_isin(cpu["elements"], cpu["tests"], c["invert"])
    assert fuzz.check(c, cpu, want) == []
    flipped = want.clone().reshape(-1)
    flipped[5] = ~flipped[5]
    _named(c, cpu, [flipped.reshape(want.shape)], "result")
    # repeat_interleave: an index off by one
    c, cpu, _ = _first_case(third_cases, "repeat_interleave", lambda c, cpu: c["form"] == "one_arg" and c["total"] > 3)
    want = fuzz.ref_repeat_interleave(c, cpu)
    assert fuzz.check(c, cpu, want) == []
    off = want.clone()
    off[want.numel() // 2] += 1
    _named(c, cpu, [off], "out")

    # mode: the index moved to an earlier occurrence; the value swapped for the other value of a tie
    def tied_row(c, cpu):
        x = cpu["x"]
        if x.dim() == 0 or c["values"] not in ("alphabet", "row_edges") or c["dtype"] in fuzz.FLOATS:
            return None
        rows = x.movedim(c["dim"], -1).reshape(-1, x.shape[c["dim"]]).numpy()
        for r in range(min(rows.shape[0], 300)):
            values, counts = np.unique(rows[r], return_counts=True)
            top = values[counts == counts.max()]
            if top.size >= 2 and counts.max() >= 2:
                return r, top[1], int(np.flatnonzero(rows[r] == top[1])[-1]), int(np.flatnonzero(rows[r] == top[0])[0])
        return None

    c, cpu, (row, other, other_at, earlier) = _first_case(third_cases, "mode", tied_row)
    x = cpu["x"]
    d = c["dim"] % x.dim()
    values, indices = fuzz.ref_mode(x, d)
    outputs = [values, indices] if c["keepdim"] else [values.squeeze(d), indices.squeeze(d)]
    assert fuzz.check(c, cpu, tuple(outputs)) == []
    flat_values, flat_indices = values.movedim(d, -1).reshape(-1).clone(), indices.movedim(d, -1).reshape(-1).clone()
    back = lambda flat: flat.reshape(values.movedim(d, -1).shape).movedim(-1, d) if c["keepdim"] else flat.reshape(values.movedim(d, -1).shape).squeeze(-1)  # noqa: E731
    moved = flat_indices.clone()
    moved[row] = earlier  # (an occurrence of the same value, not the last)
    assert earlier < int(flat_indices[row])
    _named(c, cpu, [outputs[0], back(moved)], "indices")
    swapped_values, swapped_indices = flat_values.clone(), flat_indices.clone()
    swapped_values[row], swapped_indices[row] = int(other), other_at  # (as frequent, at its own last occurrence, but not the smallest)
    _named(c, cpu, [back(swapped_values), back(swapped_indices)], "values")
    # unique(dim=): two adjacent rows of the values swapped, one inverse entry changed, one count changed, the last row dropped
    for op in ("unique_dim", "unique_consecutive_dim"):
        c, cpu, _ = _first_case(third_cases, op, lambda c, cpu: c["return_inverse"] and c["return_counts"] and c["N"] > 8
                                and fuzz.ref_unique_rows(cpu["x"], c["dim"] % 2 if len(c["shape"]) == 2 else c["dim"] % 3, op != "unique_dim")[0].shape[c["dim"]] > 2)
        d = c["dim"] % len(c["shape"])
        values, inverse, counts = fuzz.ref_unique_rows(cpu["x"], d, op != "unique_dim")
        assert fuzz.check(c, cpu, (values, inverse, counts)) == []
        rows = values.movedim(d, 0).clone()
        rows[[0, 1]] = rows[[1, 0]]
        _named(c, cpu, [rows.movedim(0, d), inverse, counts], "values")
        changed = inverse.clone()
        changed[3] = (changed[3] + 1) % values.shape[d]
        _named(c, cpu, [values, changed, counts], "inverse")
        changed = counts.clone()
        changed[-1] += 1
        _named(c, cpu, [values, inverse, changed], "counts")
        _named(c, cpu, [values.narrow(d, 0, values.shape[d] - 1), inverse, counts], "values")
        assert fuzz.check(c, cpu, (values, inverse))[0].startswith("2 outputs returned")  # the tuple's arity
