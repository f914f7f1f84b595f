"""The torch drop-ins interleaved on the contexts `_torch.context_for` hands out, default tunings (kept pool layouts included):
tools/fuzz_ops.py's committed runs of both decks -- every element of every output against torch on the CPU and numpy, no tolerance but
the stated bound of the newer deck's float sums and products --, and the kept-layout scenario spelled out.  tests/test_ops_fuzz_cpu.py (no
device) holds the same runs to what the generator claims to reach."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import vkradixsort_amd as vrs
from vkradixsort_amd import _torch as vrs_torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _load():
    spec = importlib.util.spec_from_file_location("fuzz_ops", ROOT / "tools" / "fuzz_ops.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fuzz = _load()


def pool_layouts(ctx):
    """(sorts that started in a kept layout, those of them it did not fit): what tests/test_gpu_pool.py's kept-layout tests read."""
    reused, stale = ctypes.c_uint64(), ctypes.c_uint64()
    ctx.check(ctx.lib.vrs_one_call_pool_layouts(ctx.handle, ctypes.byref(reused), ctypes.byref(stale)))
    return reused.value, stale.value


@pytest.mark.parametrize("seed,count", fuzz.COMMITTED_RUNS)
def test_the_committed_runs_pass(seed, count):
    assert fuzz.run(seed, count, "cuda:0") == count


@pytest.mark.parametrize("seed,count", fuzz.COMMITTED_RUNS_NEWER)
def test_the_committed_runs_of_the_newer_deck_pass(seed, count):
    """The selections, counts, reductions, scans and compactions between the first deck's ops, a deferred sort pending before every second
    window's newer ops: bits where the result is defined exactly, the stated bound of the term count where it is a float sum or product."""
    assert fuzz.run(seed, count, "cuda:0", deck="newer") == count


@pytest.mark.parametrize("seed,count", fuzz.COMMITTED_RUNS_THIRD)
def test_the_committed_runs_of_the_third_deck_pass(seed, count):
    """repeat_interleave, isin, mode and the dim= forms of unique / unique_consecutive between the other decks' ops, a deferred sort
    pending in front of every second window: every output bit for bit against torch on the CPU and numpy."""
    assert fuzz.run(seed, count, "cuda:0", deck="third") == count


def test_a_kept_layout_meets_other_values_between_other_ops(capsys):
    """Three 1-D sorts of one element count above the pool-form minimum through vrs.sort (key + position pairs: the minimum of that kind)
    on the shared context: uniform, then so skewed that the regions kept from the first cannot fit, then uniform again, with vrs.unique
    and vrs.topk of the same count in between.  Everything is checked as the fuzz checks it; the second sort must not have run in the
    first one's layout unchanged: either it sampled for itself or its kept layout was found stale.

    That alone also holds when no sort of the sequence ever starts in a kept layout -- and after the refusal of the seven-valued unique
    the adaptive back-off may well send the sorts that follow to the counted form.  So the scenario begins with one more uniform sort
    in front of the first: the first of the three has other keys of the same distribution and must start in its layout and fit.  The
    two back-offs are started afresh before that (both tunings set to the default they already have), so that what ran earlier on the
    shared context does not decide whether a kept layout is tried."""
    from vkradixsort_amd import capi

    t = fuzz.thresholds()
    n = fuzz._first(lambda v: t.sort_form(v, 4, 1) == "pool", 1, 1 << 27) + 12345
    assert t.sort_form(n, 4, 1) == "pool" and t.sort_form(n, 4, 0) == "pool"
    device = torch.device("cuda:0")
    ctx = vrs_torch.context_for(device)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL, 1)               # (the default: ends a pause of the form after a refusal)
    ctx.setTuning(capi.VRS_TUNE_MSD_POOL_REUSE_LAYOUT, 1)  # (the default: ends a pause after stale layouts, drops a kept layout)
    rng = np.random.Generator(np.random.PCG64(5))
    uniform0 = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32))
    uniform1 = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32))
    skewed = torch.from_numpy((rng.integers(0, 1 << 10, size=n, dtype=np.int64) + 2 ** 30).astype(np.int32))  # ten varying bits
    uniform2 = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32))
    seven = torch.from_numpy(rng.integers(0, 7, size=n, dtype=np.int64).astype(np.int32))
    floats = torch.from_numpy(rng.standard_normal(n, dtype=np.float32))

    def sort_case(x):
        case = {"op": "sort", "dim": 0, "descending": False}
        out = vrs.sort(x.to(device))
        torch.cuda.synchronize(device)
        assert fuzz.check(case, {"x": x}, out) == []
        return pool_layouts(ctx)

    start = pool_layouts(ctx)
    seen = [start, sort_case(uniform0), sort_case(uniform1)]
    case = {"op": "unique", "return_inverse": True, "return_counts": True}
    assert fuzz.check(case, {"x": seven}, vrs.unique(seven.to(device), return_inverse=True, return_counts=True)) == []
    before = pool_layouts(ctx)
    after = sort_case(skewed)
    case = {"op": "topk", "k": 100, "largest": True, "sorted": True}
    assert fuzz.check(case, {"x": floats}, vrs.topk(floats.to(device), 100)) == []
    seen += [before, after, sort_case(uniform2)]
    with capsys.disabled():
        print(f"\n(reused, stale) at the start, after uniform, uniform, [unique], skewed, [topk], uniform: n = {n}: {seen}")
    assert seen[1] == start, seen                          # nothing kept yet: sampled
    assert seen[2] == (start[0] + 1, start[1]), seen       # the kept-layout code is reached: started in the layout, and it fitted
    # (a sort that starts in a kept layout counts in `reused`; one the layout did not fit also in `stale`, and runs again sampled)
    assert after[1] - before[1] == after[0] - before[0], seen
