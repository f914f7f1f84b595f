"""Times vkradixsort_amd.cumsum and cummax (the whole wrapper: scratch allocation, the kernels) against torch.cumsum / torch.cummax on
the same tensors in the same process: HIP events around each call, the contenders alternating, median of --reps after --warmup.  Per
case: our median, torch's and its ratio to ours, a device-to-device copy of the bytes the call has to move (the input read once, the
results written once) and that copy's time as a fraction of ours; the tier that ran.  Prints one line per case and writes the table
(default profiles/labs/k14_scan.txt).

Cases: (f) float32 along one row of 1e8; (r) 1e5 rows of 1e3 along dim 1; (c) [1e5, 1e3] along dim 0 -- cumsum and cummax each;
(k) the two knobs on the 1e8 row: VRS_TUNE_SCAN_TILE_ROWS 256 .. 8192 and VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS 0 (the three-launch form)
against the default.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table, which is rewritten after every
line.

    python tools/scan_time.py [--cases frck] [--reps 5] [--warmup 2] [--scale 1.0] [--budget SECONDS] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, works, reps: int, warmup: int):
    """median ms of every work, one call of each per round"""
    t = [[] for _ in works]
    for r in range(warmup + reps):
        for i, work in enumerate(works):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            work()
            b.record()
            b.synchronize()
            if r >= warmup:
                t[i].append(a.elapsed_time(b))
    return [sorted(v)[len(v) // 2] for v in t]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="frck")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k14_scan.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    ctx = context_for(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median), scratch allocation inside "
             "ours; x = torch's time / ours; copy ms = a device-to-device copy of the bytes the call has to move (input once, results once); of copy = that "
             "time / ours; tier = what ran",
             f"{'case':<64}{'ours ms':>10}{'torch ms':>10}{'x':>7}{'copy ms':>10}{'of copy':>9}  tier"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    def sz(x):
        return max(int(x * args.scale), 1)

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)  # (a copy of b bytes moves 2 b)
        dst = torch.empty_like(src)
        return timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]

    def run(label, x, dim, fn):
        if args.budget and time.perf_counter() - started > args.budget:
            record(f"{label:<64}{'not run: past --budget':>30}")
            return
        ours, theirs = getattr(vrs, fn), getattr(torch, fn)
        before = vrs.scan_stats(ctx)
        t_ours, t_torch = timed(torch, [lambda: ours(x, dim), lambda: theirs(x, dim)], args.reps, args.warmup)
        after = vrs.scan_stats(ctx)
        tier = "+".join(k for k in ("tile", "three_launch", "single_pass") if after[k] > before[k])
        moved = x.numel() * x.element_size() * 2 + (x.numel() * 8 if fn == "cummax" else 0)
        t_copy = copy_ms(moved)
        record(f"{label:<64}{t_ours:>10.3f}{t_torch:>10.3f}{t_torch / t_ours:>7.2f}{t_copy:>10.3f}{t_copy / t_ours:>9.2f}  {tier}")

    g = torch.Generator(device=dev).manual_seed(1)
    shapes = {"f": ((sz(1e8),), 0), "r": ((sz(1e5), 1000), 1), "c": ((sz(1e5), 1000), 0)}
    for case, (shape, dim) in shapes.items():
        if case not in args.cases:
            continue
        x = torch.randn(shape, generator=g, device=dev)
        for fn in ("cumsum", "cummax"):
            run(f"{case} {fn} float32 {list(shape)} dim={dim}", x, dim, fn)
        del x
    if "k" in args.cases:
        x = torch.randn(sz(1e8), generator=g, device=dev)
        for tile_rows in (256, 512, 1024, 2048, 4096, 8192):
            ctx.setTuning(capi.VRS_TUNE_SCAN_TILE_ROWS, tile_rows)
            for min_rows in (capi.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT, 0):
                ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, min_rows)
                run(f"k cumsum float32 [{x.numel()}] tile_rows={tile_rows} single_pass_min_rows={min_rows}", x, 0, "cumsum")
        ctx.setTuning(capi.VRS_TUNE_SCAN_TILE_ROWS, capi.SCAN_TILE_ROWS_DEFAULT)
        ctx.setTuning(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, capi.SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
