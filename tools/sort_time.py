"""Times the torch.sort drop-in (vkradixsort_amd.sort / sort_values over vrs_sort_rank_keys, the segmented or one-call sort and
vrs_sort_restore) against torch.sort on the same device and, for 32-bit dtypes sorted along the last dim, against sort_rows: HIP events
around whole calls, median of --reps after --warmup, the implementations alternating rep by rep in one process.  Every case's outputs are
checked against torch.sort(x, stable=True) on the device in the same run (values bit for bit, indices index for index).  Then the
64-bit segmented sort's one-call crossover: rows of L int64 keys (2^24 in all) sorted by the global tier (one-call threshold 0 = never)
and by the one-call tier (threshold L), keys only and with indices.  Writes JSON (default profiles/labs/sort_time.json).

    python tools/sort_time.py [--reps 5] [--warmup 2] [--no-yardsticks] [--no-sweep] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def event_ms(torch, work) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    work()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(torch, works: dict, reps: int, warmup: int) -> dict:
    times = {k: [] for k in works}
    for r in range(warmup + reps):
        for k, w in works.items():
            t = event_ms(torch, w)
            if r >= warmup:
                times[k].append(t)
    out = {}
    for k, t in times.items():
        t = sorted(t)
        out[k] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": len(t)}
    return out


BITS = {"float16": "int16", "bfloat16": "int16", "float32": "int32", "float64": "int64"}


def same(torch, a, b) -> bool:
    name = str(a.dtype).replace("torch.", "")
    if name in BITS:
        a, b = a.view(getattr(torch, BITS[name])), b.view(getattr(torch, BITS[name]))
    return bool(torch.equal(a, b))


def make(torch, dtype, shape, g):
    dev = torch.device("cuda", 0)
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g, device=dev, dtype=torch.float32).to(dtype)
    return torch.randint(-(1 << 62), 1 << 62, shape, generator=g, device=dev, dtype=torch.int64).to(dtype)


# (label, dtype, shape, dim, descending, with indices)
CASES = [
    ("1e8 float32", "float32", (10 ** 8,), -1, False, True),
    ("1e8 float32 descending", "float32", (10 ** 8,), -1, True, True),
    ("1e8 int64 values only", "int64", (10 ** 8,), -1, False, False),
    ("1e8 int64", "int64", (10 ** 8,), -1, False, True),
    ("1e8 float64", "float64", (10 ** 8,), -1, False, True),
    ("[24414, 4096] int64", "int64", (24414, 4096), -1, False, True),
    ("[1e5, 1000] float64", "float64", (10 ** 5, 1000), -1, False, True),
    ("[1e6, 100] int64", "int64", (10 ** 6, 100), -1, False, True),
    ("[64, 2^17] int64 (global tier)", "int64", (64, 1 << 17), -1, False, True),
    ("[4096, 4096] float32 dim=0", "float32", (4096, 4096), 0, False, True),
    ("[24414, 4096] bfloat16 (1e8)", "bfloat16", (24414, 4096), -1, False, True),
]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-yardsticks", action="store_true", help="time the library only (profiler runs)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "sort_time.json"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": [], "crossover_u64": []}
    for label, dname, shape, dim, desc, with_idx in CASES:
        dtype = getattr(torch, dname)
        x = make(torch, dtype, shape, g)
        ref = torch.sort(x, dim=dim, descending=desc, stable=True)
        out = None
        if with_idx:
            out = vrs.sort(x, dim=dim, descending=desc)
            exact = same(torch, out.values, ref.values) and bool(torch.equal(out.indices, ref.indices))
            works = {"vrs": lambda: vrs.sort(x, dim=dim, descending=desc)}
        else:
            exact = same(torch, vrs.sort_values(x, dim=dim, descending=desc), ref.values)
            works = {"vrs": lambda: vrs.sort_values(x, dim=dim, descending=desc)}
        del out
        if not args.no_yardsticks:
            works["torch"] = lambda: torch.sort(x, dim=dim, descending=desc)
            if dname in ("float32", "int32") and not desc and dim == -1:
                x2 = x.view(-1, shape[-1])
                works["sort_rows"] = lambda: vrs.sort_rows(x2, return_indices=with_idx)
        t = alternate(torch, works, args.reps, args.warmup)
        row = {"case": label, "dtype": dname, "shape": list(shape), "dim": dim, "descending": desc, "indices": with_idx,
               "exact_vs_torch": exact, **t}
        if "torch" in t:
            row["speedup_vs_torch"] = t["torch"]["median_ms"] / t["vrs"]["median_ms"]
        if "sort_rows" in t:
            row["speedup_vs_sort_rows"] = t["sort_rows"]["median_ms"] / t["vrs"]["median_ms"]
        results["cases"].append(row)
        print(json.dumps(row), flush=True)
        del x, ref
        torch.cuda.empty_cache()

    if not args.no_sweep:
        ctx = context_for(dev)
        total = 1 << 24
        try:
            for L in (1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22):
                x = make(torch, torch.int64, (total // L, L), g)
                for with_idx in (False, True):
                    fn = (lambda: vrs.sort(x)) if with_idx else (lambda: vrs.sort_values(x))
                    works = {}
                    for tier, thr in (("global", 0), ("one_call", L)):
                        def work(thr=thr, fn=fn):
                            ctx.setTuning(capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, thr)
                            fn()
                        works[tier] = work
                    t = alternate(torch, works, args.reps, args.warmup)
                    row = {"row_len": L, "rows": total // L, "indices": with_idx, **t,
                           "one_call_over_global": t["one_call"]["median_ms"] / t["global"]["median_ms"]}
                    results["crossover_u64"].append(row)
                    print(json.dumps(row), flush=True)
                del x
                torch.cuda.empty_cache()
        finally:
            ctx.setTuning(capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT)

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")
    print(f"wrote {args.out}")
    return 0 if all(c["exact_vs_torch"] for c in results["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
