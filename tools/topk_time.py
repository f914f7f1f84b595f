"""Times the top-k selection (vkradixsort_amd.topk over vrs_topk_segments) with HIP events around the whole call, median of --reps after
--warmup, beside its yardsticks: torch.topk, and the sort-then-slice that exists without it (sort_rows(x, return_indices=True), then
the first / last k columns).  Writes JSON (default profiles/labs/topk_time.json).

Cases (float32 unless named): (a) 1e8 keys as one segment, k = 1, 64, 1024, 65536, smallest and largest; (b) [64, 131072], k = 50 and
1024 (fewer rows than CUs: the case the grid threshold is about); (c) [4096, 4096], k = 32; (d) [100000, 1000], k = 10; (e) 1e8 keys of
only 8 distinct values, k = 1024 (every refinement level keeps an eighth of the keys).  Read share: the keys' bytes over the time,
against 8 TB/s.

--crossover: rows of L keys (L from 16384 to 4M, R * L about 8.4e6, at least 1 row), each timed with VRS_TUNE_TOPK_GRID_MIN_KEYS = 1
(every segment beyond the LDS tier takes the grid tier) and = 0 (the BLOCK tier): where the grid tier starts to win is the default.

--dtypes: the torch.topk drop-in (vkradixsort_amd.torch_topk, largest, sorted) beside torch.topk and beside sort-then-slice
(vkradixsort_amd.sort descending, then the first k): [1, 1e8] and [64, 131072] for bfloat16, float16, float32, int64 and float64,
[100000, 1000] and [65536, 256] for bfloat16 and float32, k = 1, 8, 64, 1024 (those that fit the row).  Every timed call allocates its
results and scratch inside.  The sort does not depend on k: timed once per shape and dtype.  No other table runs with --dtypes.

    python tools/topk_time.py [--cases abcde] [--reps 5] [--warmup 2] [--scale 1.0] [--crossover] [--dtypes] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_BYTES_PER_S = 8.0e12


def timed(torch, work, reps: int, warmup: int) -> dict:
    times = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        work()
        b.record()
        b.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
    t = sorted(times)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": len(t)}


def cases_for(name: str, scale: float):
    """(label, shape, k list, largest list, distinct values or None)"""
    big = max(int(1e8 * scale), 1)
    if name == "a":
        return [("a", (big,), [1, 64, 1024, 65536], [False, True], None)]
    if name == "b":
        return [("b", (64, max(int(131072 * scale), 1)), [50, 1024], [True], None)]
    if name == "c":
        return [("c", (4096, max(int(4096 * scale), 64)), [32], [True], None)]
    if name == "d":
        return [("d", (max(int(100000 * scale), 1), 1000), [10], [True], None)]
    if name == "e":
        return [("e", (big,), [1024], [False], 8)]
    raise ValueError(name)


def dtype_table(torch, vrs, dev, g, args) -> list:
    """the torch.topk drop-in per dtype and shape: medians beside torch.topk and sort-then-slice"""
    wide = [torch.bfloat16, torch.float16, torch.float32, torch.int64, torch.float64]
    short = [torch.bfloat16, torch.float32]
    big = max(int(1e8 * args.scale), 1)
    shapes = [((1, big), wide), ((64, max(int(131072 * args.scale), 1)), wide), ((max(int(100000 * args.scale), 1), 1000), short),
              ((max(int(65536 * args.scale), 1), 256), short)]
    rows = []
    for shape, dtypes in shapes:
        for dtype in dtypes:
            if dtype == torch.int64:
                x = torch.randint(-(1 << 62), 1 << 62, shape, device=dev, generator=g, dtype=torch.int64)
            else:
                x = torch.randn(shape, device=dev, generator=g, dtype=torch.float32).to(dtype)
            sort_ms = timed(torch, lambda: vrs.sort(x, dim=-1, descending=True), args.reps, args.warmup)["median_ms"]
            for k in (1, 8, 64, 1024):
                if k > shape[1]:
                    continue
                ours, theirs = vrs.torch_topk(x, k), torch.topk(x, k, dim=-1)
                row = {"table": "dtypes", "dtype": str(dtype).replace("torch.", ""), "shape": list(shape), "k": k,
                       "equals_torch_values": bool(torch.equal(ours.values, theirs.values)),
                       "torch_topk_dropin_ms": timed(torch, lambda: vrs.torch_topk(x, k), args.reps, args.warmup)["median_ms"],
                       "torch_topk_ms": timed(torch, lambda: torch.topk(x, k, dim=-1), args.reps, args.warmup)["median_ms"],
                       "sort_then_slice_ms": sort_ms}
                row["speedup_vs_torch_topk"] = row["torch_topk_ms"] / row["torch_topk_dropin_ms"]
                row["speedup_vs_sort_then_slice"] = sort_ms / row["torch_topk_dropin_ms"]
                row["read_share_of_8TBps"] = x.numel() * x.element_size() / (row["torch_topk_dropin_ms"] * 1e-3) / PEAK_BYTES_PER_S
                print(json.dumps(row), flush=True)
                rows.append(row)
            del x
            torch.cuda.empty_cache()
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--dtypes", action="store_true", help="the table of torch_topk per dtype and shape, and nothing else")
    ap.add_argument("--no-yardsticks", action="store_true", help="time the selection only (profiler runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "topk_time.json"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ctx = context_for(dev)
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "scale": args.scale,
               "grid_min_keys": capi.TOPK_GRID_MIN_KEYS_DEFAULT, "cases": []}
    if args.dtypes:
        results["dtypes"] = dtype_table(torch, vrs, dev, g, args)
    for name in "" if args.dtypes else args.cases:
        for label, shape, ks, dirs, distinct in cases_for(name, args.scale):
            if distinct:
                x = (torch.randint(0, distinct, shape, device=dev, generator=g).float() * 0.5 - 1.0).contiguous()
            else:
                x = torch.randn(shape, device=dev, generator=g)
            rows = 1 if x.dim() == 1 else x.shape[0]
            x2 = x.view(rows, -1)
            for k in ks:
                for largest in dirs:
                    row = {"case": label, "shape": list(shape), "k": k, "largest": largest, "distinct": distinct}
                    v, i = vrs.topk(x, k, largest=largest)
                    tv, ti = torch.topk(x, k, dim=-1, largest=largest)
                    row["equals_torch_values"] = bool(torch.equal(v, tv))
                    row["topk"] = timed(torch, lambda: vrs.topk(x, k, largest=largest), args.reps, args.warmup)
                    if not args.no_yardsticks:
                        row["torch_topk"] = timed(torch, lambda: torch.topk(x, k, dim=-1, largest=largest), args.reps, args.warmup)

                        def sort_slice():
                            sv, si = vrs.sort_rows(x2, return_indices=True)
                            return (sv[:, -k:], si[:, -k:]) if largest else (sv[:, :k], si[:, :k])

                        row["sort_then_slice"] = timed(torch, sort_slice, args.reps, args.warmup)
                        row["speedup_vs_sort_then_slice"] = row["sort_then_slice"]["median_ms"] / row["topk"]["median_ms"]
                        row["speedup_vs_torch_topk"] = row["torch_topk"]["median_ms"] / row["topk"]["median_ms"]
                    row["read_share_of_8TBps"] = x.numel() * 4 / (row["topk"]["median_ms"] * 1e-3) / PEAK_BYTES_PER_S
                    print(json.dumps(row), flush=True)
                    results["cases"].append(row)
            del x, x2
            torch.cuda.empty_cache()
    if args.crossover and not args.dtypes:
        sweep = []
        for L in [16384, 32768, 65536, 131072, 262144, 524288, 1 << 20, 1 << 22]:
            R = max(1, int((1 << 23) * args.scale) // L)
            x = torch.randn((R, L), device=dev, generator=g)
            for k in (50, 1024):
                entry = {"rows": R, "length": L, "k": k}
                for label, thr in (("grid", 1), ("block", 0)):
                    ctx.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, thr)
                    entry[label] = timed(torch, lambda: vrs.topk(x, k), args.reps, args.warmup)["median_ms"]
                entry["grid_faster"] = entry["grid"] < entry["block"]
                print(json.dumps(entry), flush=True)
                sweep.append(entry)
            del x
        ctx.setTuning(capi.VRS_TUNE_TOPK_GRID_MIN_KEYS, capi.TOPK_GRID_MIN_KEYS_DEFAULT)
        results["crossover"] = sweep
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1))
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
