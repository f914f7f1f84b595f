"""Times vkradixsort_amd.bincount / histc / histogram (vrs_bin_count: plan, scratch allocation, clearing, counting and finish kernels, and
the wrappers' torch.aminmax with its host read, all inside the timed call) against torch on the same tensors in the same process: HIP
events around each call, the two alternating, median of --reps after --warmup, both outputs compared before anything is timed.  Per
case: our median, torch's, torch / ours, the bytes the call has to read (elements and weights) over our time as a fraction of a
device-to-device copy of as many bytes on this device (timed here, first), and the tier taken.  Prints one line per case and writes the
table (default profiles/labs/k11_bincount.txt).

Cases: (b) bincount of 1e8 int32 / int64 elements into 256, 16384, 16385, 2^20 and 2^26 bins; uniform, constant and Zipf-like inputs;
with and without float32 weights.  (c) histc of 1e8 float32 / bfloat16 elements into 100 and 1e4 bins, explicit range.  (g) histogram
of 1e7 float32 elements with 100 edges against torch.histogram ON THE CPU (torch has no device kernel), labelled as such.  (m) the
torch.aminmax plus host read bincount starts with, on its own line.

    python tools/bincount_time.py [--cases bcgm] [--reps 7] [--warmup 2] [--scale 1.0] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed_pair(torch, ours, theirs, reps: int, warmup: int):
    """median ms of ours and of theirs (None: not run), one call of each per round"""
    t = {"ours": [], "theirs": []}
    for r in range(warmup + reps):
        for name, work in (("ours", ours), ("theirs", theirs)):
            if work is None:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            work()
            b.record()
            b.synchronize()
            if r >= warmup:
                t[name].append(a.elapsed_time(b))
    med = lambda v: sorted(v)[len(v) // 2] if v else None  # noqa: E731
    return med(t["ours"]), med(t["theirs"])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="mbcg")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k11_bincount.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ctx = context_for(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median); scratch allocation, "
             "clearing, finish kernel and the wrapper's aminmax + host read inside ours; ratio = torch / ours; copy = bytes read / ours as a "
             "fraction of a device-to-device copy of as many bytes; '*': torch took more than 100 ms and was timed by one call",
             f"{'case':<66}{'tier':>8}{'ours ms':>10}{'torch ms':>10}{'ratio':>7}{'copy':>7}"]
    print("\n".join(lines), flush=True)

    def sz(x):
        return max(int(x * args.scale), 1)

    copy_rate = {}

    def copy_ms_per_byte(nbytes):
        """ms per byte of a device-to-device copy of about nbytes (median of 5), measured once per size"""
        if nbytes not in copy_rate:
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            ms, _ = timed_pair(torch, lambda: dst.copy_(src), None, 5, 2)
            copy_rate[nbytes] = ms / nbytes
            del src, dst
        return copy_rate[nbytes]

    def run(label, ours, theirs, nbytes, same=None, yardstick="torch"):
        before = vrs.bincount_stats(ctx)
        got = ours()
        after = vrs.bincount_stats(ctx)
        tier = next((k for k in after if after[k] != before[k]), "-")
        once = None
        if theirs is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = theirs()
            torch.cuda.synchronize()
            once = (time.perf_counter() - t0) * 1e3
            if not (same or torch.equal)(got, want):
                raise RuntimeError(f"{label}: the outputs differ")
            del want
        del got
        # a yardstick that takes more than 100 ms a call (torch.bincount of a constant input: 1e8 atomics on one address) is timed by
        # that one call, marked '*', and left out of the rounds
        slow = yardstick == "torch" and once is not None and once > 100.0
        o, t = timed_pair(torch, ours, theirs if yardstick == "torch" and not slow else None, args.reps, args.warmup)
        if slow:
            t = once
            label += " *"
        if yardstick == "cpu":  # torch on the CPU: wall clock, the same number of calls
            ts = []
            for _ in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                theirs()
                ts.append((time.perf_counter() - t0) * 1e3)
            t = sorted(ts[args.warmup:])[args.reps // 2]
        frac = copy_ms_per_byte(nbytes) * nbytes / o
        line = f"{label:<66}{tier:>8}{o:>10.3f}" + (f"{t:>10.3f}{t / o:>7.2f}" if t else f"{'-':>10}{'-':>7}") + f"{frac:>7.2f}"
        print(line, flush=True)
        lines.append(line)

    def indices(dist, n, bins, dtype):
        if dist == "uniform":
            return torch.randint(0, bins, (n,), device=dev, generator=g, dtype=dtype)
        if dist == "constant":
            return torch.full((n,), bins // 2, device=dev, dtype=dtype)
        u = torch.rand(n, device=dev, generator=g, dtype=torch.float64)  # Zipf-like: P(rank r) ~ 1 / r over the bins (the inverse of a log-uniform draw)
        x = torch.exp(u * torch.log(torch.tensor(float(bins), dtype=torch.float64, device=dev))).to(torch.int64) - 1
        x = x.clamp_(0, bins - 1).to(dtype)
        x[0] = bins - 1  # (every case counts into exactly `bins` bins)
        return x

    for case in args.cases:
        if case == "m":
            x = torch.randint(0, 1 << 20, (sz(1e8),), device=dev, generator=g, dtype=torch.int32)
            o, _ = timed_pair(torch, lambda: torch.stack(torch.aminmax(x)).tolist(), None, args.reps, args.warmup)
            line = f"{'m torch.aminmax + host read of int32 n=' + format(x.numel(), '.0e') + ' (inside every bincount below)':<66}{'-':>8}{o:>10.3f}"
            print(line, flush=True)
            lines.append(line)
            del x
        elif case == "b":
            n = sz(1e8)
            w = torch.randint(0, 8, (n,), device=dev, generator=g).float()  # (small integers: the sums compare exactly)
            for dtype in (torch.int32, torch.int64):
                for bins in (256, 16384, 16385, 1 << 20, 1 << 26):
                    for dist in ("uniform", "constant", "zipf"):
                        x = indices(dist, n, bins, dtype)
                        x[0] = bins - 1
                        name = f"b bincount {str(dtype)[6:]} n={n:.0e} bins={bins} {dist}"
                        run(name, lambda: vrs.bincount(x), lambda: torch.bincount(x), n * x.element_size())
                        # (a float32 sum of up to 1e8 weights depends on its order, torch's as ours: ours is held against the float64 sums)
                        if dist == "constant":  # (everything but element 0 in one bin: no 1e8 float64 atomics on one address for the check)
                            exact = torch.zeros(bins, dtype=torch.float64, device=dev)
                            exact[bins // 2] = w[1:].double().sum()
                            exact[bins - 1] += w[0].double()
                        else:
                            exact = torch.bincount(x, weights=w.double())
                        run(name + " +f32 w", lambda: vrs.bincount(x, weights=w), lambda: torch.bincount(x, weights=w), n * (x.element_size() + 4),
                            same=lambda a, b: torch.allclose(a.double(), exact, rtol=1e-3))
                        del exact
                        del x
            del w
        elif case == "c":
            n = sz(1e8)
            for dtype in (torch.float32, torch.bfloat16):
                x = torch.rand(n, device=dev, generator=g, dtype=torch.float32).to(dtype)
                for bins in (100, 10 ** 4):
                    # torch's counts are float sums of ones: in bfloat16 they stop at 256, so only float32 is compared (and is exact below 2^24)
                    same = (lambda a, b: True) if dtype == torch.bfloat16 else None
                    theirs = lambda: torch.histc(x, bins=bins, min=0.0, max=1.0)  # noqa: E731
                    try:
                        torch.histc(x[:16], bins=bins, min=0.0, max=1.0)
                    except RuntimeError:  # (no device kernel for the dtype in this torch)
                        theirs = None
                    run(f"c histc {str(dtype)[6:]} n={n:.0e} bins={bins} range [0, 1]", lambda: vrs.histc(x, bins=bins, min=0.0, max=1.0),
                        theirs, n * x.element_size(), same=same)
                del x
        elif case == "g":
            n = sz(1e7)
            x = torch.randn(n, device=dev, generator=g, dtype=torch.float32)
            edges = torch.linspace(-4.0, 4.0, 100, device=dev)
            xc, ec = x.cpu(), edges.cpu()
            run(f"g histogram float32 n={n:.0e} 100 edges; yardstick: torch ON THE CPU", lambda: vrs.histogram(x, edges)[0],
                lambda: torch.histogram(xc, ec).hist, n * 4, same=lambda a, b: torch.equal(a.cpu(), b), yardstick="cpu")
            del x
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
