"""Times vkradixsort_amd.quantile (the whole wrapper: scratch and output allocation and the kernels of vrs_quantile_segments) against
torch.quantile on the same tensors in the same process, against this library's sort followed by a gather (the wrapper's own path for a q
of more than 16 targets), and against a device-to-device copy of the input (its bytes read once and written once): HIP events around
each call, the contenders alternating, median of --reps after --warmup.  Prints one line per case and writes the table (default
profiles/labs/k16_quantile.txt); a row where the call loses to sort-then-gather says so.

Cases: one row of 1e8 and [1e5, 1e3] along dim 1; Q = 1, 3 and 8; "linear" and "lower"; float32 and float64; uniform, normal and
constant inputs.  torch.quantile refuses more than 2^24 elements: such a case's torch column says so, and a second line times all three
on the case's first 2^24 elements (its first 16777 rows), the most torch takes.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table, which is rewritten after every
line.

    python tools/quantile_time.py [--reps 5] [--warmup 2] [--scale 1.0] [--budget SECONDS] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TORCH_LIMIT = 1 << 24  # torch.quantile refuses inputs of more elements ("input tensor is too large")


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k16_quantile.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd.quantile import _sort_rows

    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median), scratch and output "
             "allocation inside all three; x torch = torch.quantile's time / ours; sort+gather = this library's sort along the dim, a gather and the "
             "same interpolation (the wrapper's path beyond 16 targets); x sort = its time / ours (below 1: the call LOSES to it); copy ms = a "
             "device-to-device copy of the input; of copy = that time / ours",
             f"{'case':<64}{'ours ms':>10}{'torch ms':>10}{'x torch':>9}{'sort+g ms':>11}{'x sort':>8}{'copy ms':>9}{'of copy':>9}"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    g = torch.Generator(device=dev).manual_seed(16)
    shapes = [(1, max(int(10 ** 8 * args.scale), 2)), (max(int(10 ** 5 * args.scale), 2), 1000)]
    for shape in shapes:
        for dtype in (torch.float32, torch.float64):
            for kind in ("uniform", "normal", "constant"):
                if kind == "uniform":
                    x = torch.rand(shape, generator=g, device=dev, dtype=dtype)
                elif kind == "normal":
                    x = torch.randn(shape, generator=g, device=dev, dtype=dtype)
                else:
                    x = torch.full(shape, 1.25, device=dev, dtype=dtype)
                dst = torch.empty_like(x)
                t_copy = timed(torch, [lambda: dst.copy_(x)], args.reps, args.warmup)[0]
                del dst
                for Q in (1, 3, 8):
                    q = torch.linspace(0.01, 0.99, Q, dtype=dtype, device=dev) if Q > 1 else torch.tensor([0.5], dtype=dtype, device=dev)
                    qs = [float(v) for v in q.tolist()]
                    for interpolation in ("linear", "lower"):
                        label = f"{list(shape)} {str(dtype).replace('torch.', '')} {kind} Q={Q} {interpolation}"
                        if args.budget and time.perf_counter() - started > args.budget:
                            record(f"{label:<64}{'not run: past --budget':>30}")
                            continue
                        t_ours, t_sort = timed(torch, [lambda: vrs.quantile(x, q, 1, interpolation=interpolation),
                                                       lambda: _sort_rows(x, qs, interpolation, False)], args.reps, args.warmup)
                        if x.numel() <= TORCH_LIMIT:
                            t_torch = timed(torch, [lambda: torch.quantile(x, q, 1, interpolation=interpolation)], args.reps, args.warmup)[0]
                            theirs = f"{t_torch:>10.3f}{t_torch / t_ours:>9.2f}"
                        else:  # (torch.quantile: "input tensor is too large" beyond 2^24 elements; the row below is the largest it takes)
                            theirs = f"{'refused':>10}{'--':>9}"
                        note = "  LOSES to sort+gather" if t_sort < t_ours else ""
                        record(f"{label:<64}{t_ours:>10.3f}{theirs}{t_sort:>11.3f}{t_sort / t_ours:>8.2f}{t_copy:>9.3f}{t_copy / t_ours:>9.2f}{note}")
                        if x.numel() > TORCH_LIMIT:
                            xs = x[:, :TORCH_LIMIT] if shape[0] == 1 else x[:TORCH_LIMIT // shape[1]]
                            t_o, t_t, t_s = timed(torch, [lambda: vrs.quantile(xs, q, 1, interpolation=interpolation),
                                                          lambda: torch.quantile(xs, q, 1, interpolation=interpolation),
                                                          lambda: _sort_rows(xs, qs, interpolation, False)], args.reps, args.warmup)
                            note = "  LOSES to sort+gather" if t_s < t_o else ""
                            record(f"{'  its first ' + str(list(xs.shape)) + ' (the most torch.quantile takes)':<64}{t_o:>10.3f}{t_t:>10.3f}{t_t / t_o:>9.2f}"
                                   f"{t_s:>11.3f}{t_s / t_o:>8.2f}{'':>9}{'':>9}{note}")
                del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
