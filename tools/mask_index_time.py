"""Times vkradixsort_amd.mask_index and mask_index_put (the whole wrapper: scratch and output allocation, the kernels, the host read of
the count) against torch's x[mask] / torch.index_put on the same tensors in the same process, and against this library's own element
form, masked_select(x, mask[:, None]) / masked_scatter(x, mask[:, None], values): HIP events around each call, the contenders
alternating, median of --reps after --warmup.  Per case: our median, torch's and the element form's with their ratios to ours, a
device-to-device copy of the bytes the call has to move (the flags read once, the rows it needs read once, the results written once)
and that copy's time as a fraction of ours.  Prints one line per case and writes the table (default profiles/labs/k17_mask_index.txt).

Cases: float32 x of about 1 GB as [N, row bytes / 4] with rows of 8, 64, 1024 and 16384 bytes, 1 %, 50 % and 100 % of a 1-D mask set;
(g) mask_index, (p) mask_index_put with values of exactly [R, row]; (s) the bytes a full tile's slice is sized for (kCompactRowSliceBytes
in csrc/vrs_compact_order.hpp, a first setting) swept through the environment variable VRS_COMPACT_ROW_SLICE_BYTES on the 1024-byte row.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table, which is rewritten after every
line.

    python tools/mask_index_time.py [--cases gps] [--reps 5] [--warmup 2] [--scale 1.0] [--budget SECONDS] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROW_BYTES = [8, 64, 1024, 16384]
DENSITIES = [0.01, 0.5, 1.0]
SLICE_BYTES = [16 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20, 1 << 30]  # (the last: one slice per tile)
KNOB = "VRS_COMPACT_ROW_SLICE_BYTES"


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
    ap.add_argument("--cases", default="gps")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k17_mask_index.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs

    dev = torch.device("cuda", 0)
    total = int((1 << 30) * args.scale)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median), scratch and output "
             "allocation and the host read of the count inside every contender; torch x, elem x = torch's / the element form's time over ours "
             "(the element form: masked_select / masked_scatter with mask[:, None]); copy ms = a device-to-device copy of the bytes the call has "
             "to move (flags and rows read once, results written once); of copy = that time / ours",
             f"{'case':<64}{'ours ms':>10}{'torch ms':>10}{'torch x':>9}{'elem ms':>10}{'elem x':>8}{'copy ms':>10}{'of copy':>9}"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    g = torch.Generator(device=dev).manual_seed(17)

    def copy_ms(nbytes):
        if nbytes < 2:
            return 0.0
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)  # (a copy of b bytes moves 2 b)
        dst = torch.empty_like(src)
        return timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]

    def run(label, ours, theirs, element, moved):
        if args.budget and time.perf_counter() - started > args.budget:
            record(f"{label:<64}{'not run: past --budget':>30}")
            return
        works = [ours, theirs] + ([element] if element else [])
        t = timed(torch, works, args.reps, args.warmup)
        t_copy = copy_ms(moved)
        elem = f"{t[2]:>10.3f}{t[2] / t[0]:>8.2f}" if element else f"{'-':>10}{'-':>8}"
        record(f"{label:<64}{t[0]:>10.3f}{t[1]:>10.3f}{t[1] / t[0]:>9.2f}{elem}{t_copy:>10.3f}{t_copy / t[0]:>9.2f}")

    def case(row_bytes, density, kinds, note="", element=True):
        n, cols = max(total // row_bytes, 1), row_bytes // 4
        x = torch.randn(n, cols, generator=g, device=dev)
        mask = torch.ones(n, dtype=torch.bool, device=dev) if density >= 1.0 else torch.rand(n, generator=g, device=dev) < density
        R = int(mask.sum())
        shape = f"[{n}, {cols}] rows of {row_bytes} B set {density:.0%}{note}"
        wide = mask[:, None]
        if "g" in kinds:
            run(f"g mask_index {shape}", lambda: vrs.mask_index(x, mask), lambda: x[mask], (lambda: vrs.masked_select(x, wide)) if element else None,
                n + 2 * R * row_bytes)
        if "p" in kinds:
            values = torch.randn(R, cols, generator=g, device=dev)
            run(f"p mask_index_put {shape}", lambda: vrs.mask_index_put(x, mask, values), lambda: torch.index_put(x, (mask,), values),
                (lambda: vrs.masked_scatter(x, wide, values)) if element else None, n + 2 * n * row_bytes)

    for row_bytes in ROW_BYTES:
        for density in DENSITIES:
            case(row_bytes, density, args.cases)
    if "s" in args.cases:
        before = os.environ.get(KNOB)
        for slice_bytes in SLICE_BYTES:
            os.environ[KNOB] = str(slice_bytes)
            for density in (0.01, 0.5):
                case(1024, density, "gp", note=f" slice_bytes={slice_bytes}", element=False)
        if before is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = before
    return 0


if __name__ == "__main__":
    sys.exit(main())
