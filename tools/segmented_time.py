"""Times the segmented sorts (vrs_sort_segments_u32 / _pairs_u32) with HIP events over warmed repetitions, beside their yardsticks, and
measures the crossover between the global tier (one workgroup per segment) and the one-call tier that VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS
is set from.  Writes JSON (default profiles/labs/segmented_time.json).

Cases (keys and pairs each): (a) 1e8 keys in 4096-key segments, (b) 1e8 keys in 1000-key segments, (c) 1e6 segments of uniform length
1..200, (d) 64 segments of 1.5e6 keys, (e) log-uniform lengths 1..2^21 totalling 1e8.  Yardsticks: torch.sort(x.view(B, L), dim=-1,
stable=True) for (a) and (b); a loop of vrs_sort_keys_u32 / vrs_sort_pairs_u32 over the segments for (c) and (d) -- over the first
--loop-segments segments of (c), scaled to all of them.  Share of peak: the least traffic (one read and one write of every key and
payload: 8 B per key, 16 per pair) over the measured time, against 8 TB/s.

    python tools/segmented_time.py [--cases abcde] [--reps 10] [--warmup 3] [--scale 1.0] [--crossover] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_BYTES_PER_S = 8.0e12


def lengths_for(case: str, scale: float, rng) -> np.ndarray:
    total = int(1e8 * scale)
    if case == "a":
        return np.full(total // 4096, 4096, dtype=np.int64)
    if case == "b":
        return np.full(total // 1000, 1000, dtype=np.int64)
    if case == "c":
        return rng.integers(1, 201, max(int(1e6 * scale), 1)).astype(np.int64)
    if case == "d":
        return np.full(64, max(int(1.5e6 * scale), 1), dtype=np.int64)
    if case == "e":
        out, s = [], 0
        while s < total:
            L = int(np.exp(rng.uniform(0, np.log(1 << 21))))
            out.append(L)
            s += L
        out[-1] -= s - total
        return np.array(out, dtype=np.int64)
    raise ValueError(case)


class Timer:
    def __init__(self, torch, reps: int, warmup: int):
        self.torch, self.reps, self.warmup = torch, reps, warmup

    def __call__(self, rearm, work) -> list:
        """ms of each timed repetition: rearm() outside the window, work() between two events on torch's stream"""
        torch = self.torch
        times = []
        for r in range(self.warmup + self.reps):
            rearm()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            work()
            b.record()
            b.synchronize()
            if r >= self.warmup:
                times.append(a.elapsed_time(b))
        return times


def summary(times: list) -> dict:
    t = sorted(times)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": len(t)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--loop-segments", type=int, default=2000)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "segmented_time.json"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi, engine
    if not torch.cuda.is_available():
        print("segmented_time: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = engine.GPUContext(0, stream=stream.cuda_stream)
    ctx.init()
    lib = ctx.lib
    S_ = engine.Buffer.BufferSettings
    timer = Timer(torch, args.reps, args.warmup)
    rng = np.random.default_rng(2024)
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "scale": args.scale,
               "peak_bytes_per_s": PEAK_BYTES_PER_S, "cases": {}}

    def wrap(t):
        return engine.Buffer(ctx, S_(t.numel() * 4), device_ptr=t.data_ptr())

    def setup(lengths):
        n = int(lengths.sum())
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), device=dev).to(torch.int32)
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=dev)
        vsrc = torch.arange(n, dtype=torch.int32, device=dev)
        t = {"src": src, "vsrc": vsrc, "k": src.clone(), "kt": torch.empty_like(src), "v": vsrc.clone(), "vt": torch.empty_like(src),
             "off": offs}
        return n, t, {name: wrap(x) for name, x in t.items() if name not in ("src", "vsrc")}

    def time_segmented(lengths, pairs, label):
        n, t, b = setup(lengths)
        S = lengths.size

        def rearm():
            t["k"].copy_(t["src"])
            if pairs:
                t["v"].copy_(t["vsrc"])

        def work():
            if pairs:
                ctx.check(lib.vrs_sort_segments_pairs_u32(ctx.handle, b["k"].handle, b["kt"].handle, b["v"].handle, b["vt"].handle, n,
                                                          b["off"].handle, S))
            else:
                ctx.check(lib.vrs_sort_segments_u32(ctx.handle, b["k"].handle, b["kt"].handle, n, b["off"].handle, S))
        before = vrs.segmented_stats(ctx)
        times = timer(rearm, work)
        after = vrs.segmented_stats(ctx)
        runs = args.warmup + args.reps
        tiers = {k: (after[k] - before[k]) // runs for k in after}
        for x in b.values():
            x.release()
        s = summary(times)
        byts = n * (16 if pairs else 8)
        s.update({"elements": n, "segments": int(S), "tiers": tiers, "min_bytes": byts,
                  "gb_per_s": byts / (s["median_ms"] * 1e-3) / 1e9, "share_of_peak": byts / (s["median_ms"] * 1e-3) / PEAK_BYTES_PER_S})
        print(f"{label}: {s['median_ms']:.3f} ms  ({s['gb_per_s']:.0f} GB/s, {100 * s['share_of_peak']:.1f} % of peak)  tiers {tiers}", flush=True)
        return s, t

    def time_torch(t, lengths, pairs, label):
        L = int(lengths[0])
        x = t["src"].view(-1, L)
        times = timer(lambda: None, lambda: torch.sort(x, dim=-1, stable=True))
        s = summary(times)
        print(f"{label} torch.sort: {s['median_ms']:.3f} ms", flush=True)
        return s

    def time_loop(t, lengths, pairs, label, limit):
        offs = np.concatenate([[0], np.cumsum(lengths)])
        k = min(limit, lengths.size)
        views = []
        for i in range(k):
            lo, hi = int(offs[i]), int(offs[i + 1])
            vs = [wrap(t[name][lo:hi]) for name in (("k", "kt", "v", "vt") if pairs else ("k", "kt"))]
            views.append((hi - lo, vs))

        def rearm():
            t["k"].copy_(t["src"])
            if pairs:
                t["v"].copy_(t["vsrc"])

        def work():
            for L, vs in views:
                if pairs:
                    ctx.check(lib.vrs_sort_pairs_u32(ctx.handle, vs[0].handle, vs[1].handle, vs[2].handle, vs[3].handle, L))
                else:
                    ctx.check(lib.vrs_sort_keys_u32(ctx.handle, vs[0].handle, vs[1].handle, L))
        times = timer(rearm, work)
        for _, vs in views:
            for v in vs:
                v.release()
        s = summary(times)
        f = lengths.size / k
        s.update({"segments_timed": k, "scaled_median_ms": s["median_ms"] * f})
        print(f"{label} loop of one-call sorts: {s['median_ms']:.3f} ms over {k} segments -> {s['scaled_median_ms']:.3f} ms for all",
              flush=True)
        return s

    for case in args.cases:
        lengths = lengths_for(case, args.scale, rng)
        for pairs in (False, True):
            label = f"({case}) {'pairs' if pairs else 'keys'}"
            s, t = time_segmented(lengths, pairs, label)
            if case in "ab":
                s["yardstick"] = {"torch_sort_stable": time_torch(t, lengths, pairs, label)}
            elif case in "cd":
                s["yardstick"] = {"vrs_sort_loop": time_loop(t, lengths, pairs, label, args.loop_segments if case == "c" else 64)}
            results["cases"][f"{case}_{'pairs' if pairs else 'keys'}"] = s
            del t
            torch.cuda.empty_cache()

    if args.crossover:
        # equal segments of L keys, 2^25 keys in all (at least 8 segments): the global tier (threshold 0 = never the one-call tier)
        # against the one-call tier (threshold 1: every segment beyond the LDS tiers)
        xs = []
        for L in (1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21):
            L = int(L * max(args.scale, 1e-3)) if args.scale < 1 else L
            lengths = np.full(max((1 << 25) // L, 8), L, dtype=np.int64)
            row = {"length": L, "segments": int(lengths.size)}
            for setting, name in ((0, "global"), (1, "one_call")):
                ctx.check(lib.vrs_set_tuning(ctx.handle, capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, setting))
                s, t = time_segmented(lengths, False, f"crossover L={L} {name}")
                row[name] = s["median_ms"]
                del t
            xs.append(row)
        ctx.check(lib.vrs_set_tuning(ctx.handle, capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT))
        results["crossover"] = xs

    ctx.shutdown()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    results["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
    out.write_text(json.dumps(results, indent=1))
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
