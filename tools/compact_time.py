"""Times vkradixsort_amd.nonzero, masked_select and masked_scatter (the whole wrapper: scratch and output allocation, the kernels, the
host read of the count) against torch's functions on the same tensors in the same process: HIP events around each call, the contenders
alternating, median of --reps after --warmup.  Per case: our median, torch's and its ratio to ours, a device-to-device copy of the bytes
the call has to move (the flags read once, the values it needs read once, the results written once) and that copy's time as a fraction
of ours.  Prints one line per case and writes the table (default profiles/labs/k15_compact.txt).

Cases, on 1e8 elements: flags of bool, float32 and int64; set flags at 0, 1 %, 50 %, 99 % and 100 % uniformly, and clustered in runs of
1e5 (half of the runs set); outputs (f) flat positions -- nonzero of a 1-D tensor --, (c) [R, 2] coordinates -- nonzero of [1e4, 1e4] --,
(s) masked_select of float32 and (m) masked_scatter of float32, the last two with the bool mask torch asks for; (k) key 40,
VRS_TUNE_COMPACT_TILE_ELEMS, over its range on the flat output of bool flags at 1 % and 50 %.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table, which is rewritten after every
line.

    python tools/compact_time.py [--cases fcsmk] [--reps 5] [--warmup 2] [--scale 1.0] [--budget SECONDS] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DENSITIES = ["0", "1%", "50%", "99%", "100%", "runs"]


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
    ap.add_argument("--cases", default="fcsmk")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k15_compact.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    ctx = context_for(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median), scratch and output "
             "allocation and the host read of the count inside both; x = torch's time / ours; copy ms = a device-to-device copy of the bytes the call "
             "has to move (flags and values read once, results written once); of copy = that time / ours",
             f"{'case':<72}{'ours ms':>10}{'torch ms':>10}{'x':>7}{'copy ms':>10}{'of copy':>9}"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    side = max(int(10 ** 4 * args.scale ** 0.5), 2)
    n = side * side
    g = torch.Generator(device=dev).manual_seed(15)

    def copy_ms(nbytes):
        if nbytes < 2:
            return 0.0
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)  # (a copy of b bytes moves 2 b)
        dst = torch.empty_like(src)
        return timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]

    def mask_of(density):
        if density == "0":
            return torch.zeros(n, dtype=torch.bool, device=dev)
        if density == "100%":
            return torch.ones(n, dtype=torch.bool, device=dev)
        if density == "runs":  # runs of 1e5 elements, half of them set
            run = max(n // 1000, 1)
            on = torch.rand(-(-n // run), generator=g, device=dev) < 0.5
            return on.repeat_interleave(run)[:n].contiguous()
        return torch.rand(n, generator=g, device=dev) < float(density[:-1]) / 100

    def run(label, ours, theirs, moved):
        if args.budget and time.perf_counter() - started > args.budget:
            record(f"{label:<72}{'not run: past --budget':>30}")
            return
        t_ours, t_torch = timed(torch, [ours, theirs], args.reps, args.warmup)
        t_copy = copy_ms(moved)
        record(f"{label:<72}{t_ours:>10.3f}{t_torch:>10.3f}{t_torch / t_ours:>7.2f}{t_copy:>10.3f}{t_copy / t_ours:>9.2f}")

    for density in DENSITIES:
        mask = mask_of(density)
        R = int(mask.sum())
        for dtype in (torch.bool, torch.float32, torch.int64):
            flags = mask if dtype == torch.bool else mask.to(dtype)
            name = str(dtype).replace("torch.", "")
            if "f" in args.cases:
                run(f"f nonzero {name} [{n}] set {density}", lambda: vrs.nonzero(flags), lambda: torch.nonzero(flags), n * flags.element_size() + 8 * R)
            if "c" in args.cases:
                grid = flags.view(side, side)
                run(f"c nonzero {name} [{side}, {side}] set {density}", lambda: vrs.nonzero(grid), lambda: torch.nonzero(grid),
                    n * flags.element_size() + 16 * R)
            del flags
        if "s" in args.cases or "m" in args.cases:
            x = torch.randn(n, generator=g, device=dev)
            if "s" in args.cases:
                run(f"s masked_select float32 [{n}] set {density}", lambda: vrs.masked_select(x, mask), lambda: torch.masked_select(x, mask), n + 8 * R)
            if "m" in args.cases:
                source = torch.randn(n, generator=g, device=dev)
                run(f"m masked_scatter float32 [{n}] set {density}", lambda: vrs.masked_scatter(x, mask, source),
                    lambda: torch.masked_scatter(x, mask, source), n + 8 * n + 4 * R)
                del source
            del x
        del mask
    if "k" in args.cases:
        for density in ("1%", "50%"):
            mask = mask_of(density)
            R = int(mask.sum())
            for tile in range(capi.COMPACT_TILE_ELEMS_MIN, capi.COMPACT_TILE_ELEMS_MAX + 1, capi.COMPACT_TILE_ELEMS_MIN):
                if tile & (tile - 1):
                    continue  # (the powers of two of the range)
                ctx.setTuning(capi.VRS_TUNE_COMPACT_TILE_ELEMS, tile)
                run(f"k nonzero bool [{n}] set {density} tile_elems={tile}", lambda: vrs.nonzero(mask), lambda: torch.nonzero(mask), n + 8 * R)
            ctx.setTuning(capi.VRS_TUNE_COMPACT_TILE_ELEMS, capi.COMPACT_TILE_ELEMS_DEFAULT)
            del mask
    return 0


if __name__ == "__main__":
    sys.exit(main())
