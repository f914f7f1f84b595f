"""Times vkradixsort_amd.kthvalue / median / nanmedian (vrs_select_segments: scratch allocation, row offsets, classification and every
phase inside the timed call) against two yardsticks on the same tensors in the same process: torch.kthvalue / median / nanmedian on the
device, and the library's way before the selection existed, sort(x, dim) then one column.  HIP events around each call, the three
alternating, median of --reps after --warmup, the values compared before anything is timed.  Per case: our median, torch's, the sort's,
both ratios, the bytes of the input over our time as a fraction of a device-to-device copy of as many bytes on this device, and the
tier taken.  Prints one line per case and writes the table (default profiles/labs/k12_select.txt).

Cases: (o) one row of 1e8 elements: float32, float64 (randn and uniform bits), int64 (uniform and below 2^20), bfloat16, int8; median,
kthvalue at a quarter, nanmedian.  (r) many rows: 2^26 float32 elements as rows of 2^10 .. 2^20.  (g) the sweep behind
VRS_TUNE_SELECT_GRID_MIN_KEYS: 2^26 float32 / float64 elements as rows of 2^14 .. 2^22, each with the grid tier off and on.  (d) the
sweep behind VRS_TUNE_SELECT_COMPACT_DIVISOR: one row of 1e8 float64 (uniform bits, randn) and int64 below 2^20 at divisors 0, 16,
64, 256 and 4096.

    python tools/select_time.py [--cases orgd] [--reps 7] [--warmup 2] [--scale 1.0] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, works, reps: int, warmup: int):
    """median ms of every callable of `works` (None: not run), one call of each per round"""
    t = [[] for _ in works]
    for r in range(warmup + reps):
        for i, work in enumerate(works):
            if work is None:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            work()
            b.record()
            b.synchronize()
            if r >= warmup:
                t[i].append(a.elapsed_time(b))
    return [sorted(v)[len(v) // 2] if v else None for v in t]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="orgd")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k12_select.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ctx = context_for(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median); scratch allocation and "
             "row offsets inside ours; /torch = torch / ours, /sort = (sort then one column) / ours; copy = input bytes / ours as a fraction of a "
             "device-to-device copy of as many bytes",
             f"{'case':<74}{'tier':>6}{'cmp':>4}{'ours ms':>10}{'torch ms':>10}{'sort ms':>10}{'/torch':>8}{'/sort':>7}{'copy':>6}"]
    print("\n".join(lines), flush=True)

    def sz(x):
        return max(int(x * args.scale), 1)

    copy_rate = {}

    def copy_ms(nbytes):
        if nbytes not in copy_rate:
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy_rate[nbytes] = timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]
            del src, dst
        return copy_rate[nbytes]

    def tune(grid_min=capi.SELECT_GRID_MIN_KEYS_DEFAULT, divisor=capi.SELECT_COMPACT_DIVISOR_DEFAULT):
        ctx.setTuning(capi.VRS_TUNE_SELECT_GRID_MIN_KEYS, grid_min)
        ctx.setTuning(capi.VRS_TUNE_SELECT_COMPACT_DIVISOR, divisor)

    def run(label, x, op, k=None, dim=-1, yardsticks=True):
        """op: "kthvalue", "median" or "nanmedian" of x along dim"""
        ours_fn, torch_fn = getattr(vrs, op), getattr(torch, op)
        pre = (k,) if op == "kthvalue" else ()
        ours = lambda: ours_fn(x, *pre, dim)  # noqa: E731
        theirs = (lambda: torch_fn(x, *pre, dim)) if yardsticks else None
        length = x.shape[dim]
        j = (k - 1) if op == "kthvalue" else (length - 1) // 2  # (the sort's column: inputs without NaNs)
        by_sort = (lambda: vrs.sort(x, dim).values.select(dim, j)) if yardsticks else None
        before = vrs.select_stats(ctx)
        got = ours().values
        after = vrs.select_stats(ctx)
        tier = "+".join(t for t in ("lds", "block", "grid") if after[t] != before[t]) + ("*" if after["compacted"] != before["compacted"] else "")
        if yardsticks:
            same = torch.equal(got, by_sort()) and torch.allclose(got.double(), theirs().values.double(), rtol=0, atol=0, equal_nan=True)
            if not same:
                raise RuntimeError(f"{label}: the values differ")
        o, t, s = timed(torch, [ours, theirs, by_sort], args.reps, args.warmup)
        nbytes = x.numel() * x.element_size()
        line = (f"{label:<74}{tier:>6}{'ok' if yardsticks else '-':>4}{o:>10.3f}" + (f"{t:>10.3f}{s:>10.3f}{t / o:>8.2f}{s / o:>7.2f}" if yardsticks
                                                                                      else f"{'-':>10}{'-':>10}{'-':>8}{'-':>7}") + f"{copy_ms(nbytes) / o:>6.2f}")
        print(line, flush=True)
        lines.append(line)

    def draw(kind, n):
        if kind == "float32 randn":
            return torch.randn(n, device=dev, generator=g)
        if kind == "float64 randn":
            return torch.randn(n, device=dev, generator=g, dtype=torch.float64)
        if kind == "float64 uniform bits":  # (finite: the exponent's top bit cleared -- no NaN, no inf)
            return (torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device=dev, generator=g, dtype=torch.int64) & ~(1 << 62)).view(torch.float64)
        if kind == "int64 uniform":
            return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device=dev, generator=g, dtype=torch.int64)
        if kind == "int64 below 2^20":
            return torch.randint(0, 1 << 20, (n,), device=dev, generator=g, dtype=torch.int64)
        if kind == "bfloat16 randn":
            return torch.randn(n, device=dev, generator=g).to(torch.bfloat16)
        if kind == "int8 uniform":
            return torch.randint(-128, 128, (n,), device=dev, generator=g, dtype=torch.int8)
        raise ValueError(kind)

    for case in args.cases:
        if case == "o":
            n = sz(1e8)
            for kind in ("float32 randn", "float64 randn", "float64 uniform bits", "int64 uniform", "int64 below 2^20", "bfloat16 randn", "int8 uniform"):
                x = draw(kind, n)
                run(f"o median {kind} n={n:.0e}", x, "median", dim=0)
                run(f"o kthvalue k=n/4 {kind} n={n:.0e}", x, "kthvalue", k=max(n // 4, 1), dim=0)
                if x.dtype.is_floating_point:
                    run(f"o nanmedian {kind} n={n:.0e}", x, "nanmedian", dim=0)
                del x
        elif case == "r":
            total = sz(1 << 26)
            for length in (1 << 10, 1 << 13, 1 << 14, 1 << 17, 1 << 20):
                length = min(length, total)
                x = draw("float32 randn", total // length * length).view(-1, length)
                run(f"r median float32 randn rows={x.shape[0]} L={length}", x, "median")
                del x
        elif case == "g":
            total = sz(1 << 26)
            for kind in ("float32 randn", "float64 randn"):
                for length in (1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 22):
                    length = min(length, total)
                    x = draw(kind, total // length * length).view(-1, length)
                    for grid_min, name in ((0, "grid off"), (8193, "grid on")):
                        tune(grid_min=grid_min)
                        run(f"g median {kind} rows={x.shape[0]} L={length} {name}", x, "median", yardsticks=False)
                    tune()
                    del x
        elif case == "d":
            n = sz(1e8)
            for kind in ("float64 uniform bits", "float64 randn", "int64 below 2^20", "float32 randn"):
                x = draw(kind, n)
                for divisor in (0, 16, 64, 256, 4096):
                    tune(divisor=divisor)
                    run(f"d median {kind} n={n:.0e} divisor={divisor}", x, "median", dim=0, yardsticks=False)
                tune()
                del x
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
