"""Times unique and unique_consecutive (vkradixsort_amd.unique over vrs_unique / vrs_run_length_encode) against torch.unique and
torch.unique_consecutive on the same device, with HIP events around the whole call (the host read of R included, as in torch), median of
--reps after --warmup; the two implementations alternate rep by rep in one process.  Writes JSON (default profiles/labs/unique_time.json).

Cases: n = 1e6, 1e7, 1e8; distinct values: all distinct, about 2^16, 16; dtypes int32, int64, float32; each without flags and with
return_inverse + return_counts.  unique_consecutive runs on the same (unsorted) input.  Besides, the encode kernel alone
(vrs_run_length_encode of sorted uint32 / uint64 keys into run ids, and into every output) for the byte rate against the device-copy
rate (5.13 TB/s, README).

    python tools/unique_time.py [--sizes 1e6,1e7,1e8] [--reps 5] [--warmup 2] [--no-yardsticks] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_BYTES_PER_S = 5.13e12  # device-to-device copy on the MI355X (README)


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


def make_input(torch, n: int, distinct: str, dtype, g):
    dev = torch.device("cuda", 0)
    if distinct == "all":
        v = torch.randperm(n, device=dev, generator=g)
    else:
        v = torch.randint(0, 1 << 16 if distinct == "2^16" else 16, (n,), device=dev, generator=g)
    if dtype.is_floating_point:
        return (v.to(torch.float64) * 0.5 - 1000.0).to(dtype)
    return (v - (n // 2 if distinct == "all" else 7)).to(dtype) * 3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e6,1e7,1e8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-yardsticks", action="store_true", help="time the library only (profiler runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "unique_time.json"))
    args = ap.parse_args()

    import importlib

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import engine
    from vkradixsort_amd._torch import context_for

    uq = importlib.import_module("vkradixsort_amd.unique")

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    sizes = [int(float(s)) for s in args.sizes.split(",")]
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "cases": [], "encode_kernel": []}
    for n in sizes:
        for distinct in ("all", "2^16", "16"):
            for dtype in (torch.int32, torch.int64, torch.float32):
                x = make_input(torch, n, distinct, dtype, g)
                for flags in (False, True):
                    kw = {"return_inverse": flags, "return_counts": flags}
                    for op, mine, theirs in (("unique", vrs.unique, torch.unique),
                                             ("unique_consecutive", vrs.unique_consecutive, torch.unique_consecutive)):
                        works = {"vrs": lambda: mine(x, **kw)}
                        if not args.no_yardsticks:
                            works["torch"] = lambda: theirs(x, **kw)
                        t = alternate(torch, works, args.reps, args.warmup)
                        row = {"op": op, "n": n, "distinct": distinct, "dtype": str(dtype).replace("torch.", ""), "inverse_counts": flags,
                               "runs": int(mine(x).numel()), "vrs": t["vrs"]}
                        if "torch" in t:
                            row["torch"] = t["torch"]
                            row["speedup"] = t["torch"]["median_ms"] / t["vrs"]["median_ms"]
                        results["cases"].append(row)
                        print(json.dumps(row), flush=True)
                del x
                torch.cuda.empty_cache()

    # the encode kernel alone over sorted keys: bytes it must move over the time, against the copy rate
    ctx = context_for(dev)
    S = engine.Buffer.BufferSettings
    n = max(sizes)
    for dtype, kb in ((torch.int32, 4), (torch.int64, 8)):
        for distinct in ("all", "2^16", "16"):
            keys = torch.sort(make_input(torch, n, distinct, dtype, g))[0]
            R = int(torch.unique_consecutive(keys).numel())
            out_keys = torch.empty(n, dtype=dtype, device=dev)
            offs, cnts, ids = (torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                               torch.empty(n, dtype=torch.int32, device=dev))
            runs = torch.empty(1, dtype=torch.int32, device=dev)
            scratch = torch.empty(max(uq.rle_scratch_bytes(n, kb, True), 4), dtype=torch.uint8, device=dev)
            ts = [keys, out_keys, offs, cnts, ids, runs, scratch]
            bufs = [engine.Buffer(ctx, S(t.numel() * t.element_size()), device_ptr=t.data_ptr()) for t in ts]
            h = [b.handle for b in bufs]
            # bytes: keys read and run ids written per element; per run its key and start written, then the counts launch reads two
            # offsets and writes a count
            for label, outs, moved in (("run_ids", (None, None, None, h[4]), n * (kb + 4)),
                                       ("all", (h[1], h[2], h[3], h[4]), n * (kb + 4) + R * (kb + 16))):
                def work(outs=outs):
                    ctx.check(ctx.lib.vrs_run_length_encode(ctx.handle, h[0], n, kb, *outs, h[5], h[6]))
                t = alternate(torch, {"encode": work}, args.reps, args.warmup)["encode"]
                rate = moved / (t["median_ms"] * 1e-3)
                row = {"key_bytes": kb, "n": n, "distinct": distinct, "runs": R, "outputs": label, "bytes_moved": moved, "time": t,
                       "bytes_per_s": rate, "share_of_copy_rate": rate / COPY_BYTES_PER_S}
                results["encode_kernel"].append(row)
                print(json.dumps(row), flush=True)
            for b in bufs:
                b.release()
            del keys, out_keys, offs, cnts, ids, scratch
            torch.cuda.empty_cache()

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
