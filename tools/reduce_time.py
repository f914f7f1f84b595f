"""Times vkradixsort_amd.index_add and segment_reduce (the whole wrapper: sort of (index, position), search for the offsets, scratch
allocation, classify and reduce kernels) against what a caller has today, on the same tensors in the same process: HIP events around
each call, the contenders alternating, median of --reps after --warmup.  Per case: our median, torch with
use_deterministic_algorithms(True), torch with (False), this library's weighted bincount (C = 1 only), each as a ratio to ours, and the
bytes the call has to read (index, source rows, input rows) over our time as a fraction of a device-to-device copy of as many bytes
(timed here).  Prints one line per case and writes the table (default profiles/labs/k13_segment_reduce.txt).

Cases: (i) index_add of 1e8 float32 elements as rows of C = 1, 64, 256 into 16385 and 2^20 destinations; uniform, constant and Zipf-like
indices (tools/bincount_time.py's).  (s) segment_reduce 'sum' of the same 1e8 elements over equal and Zipf-like lengths against
torch.segment_reduce.  (k) the two knobs: VRS_TUNE_REDUCE_CHUNK_ROWS 64 .. 4096 and VRS_TUNE_REDUCE_LANE_ROWS 0 .. 64 on the Zipf-like
index_add at C = 1 and 64.

--budget SECONDS: no case is started after that many seconds (the torch contenders of the skewed inputs take 0.1 to 2.5 s a call); the
cases left out are named in the table, which is rewritten after every line.

    python tools/reduce_time.py [--cases isk] [--reps 5] [--warmup 2] [--scale 1.0] [--budget SECONDS] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, works, reps: int, warmup: int):
    """median ms of every work (None: not run), one call of each per round"""
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
    ap.add_argument("--cases", default="isk")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k13_segment_reduce.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ctx = context_for(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median); sort, search, scratch "
             "allocation and the wrapper's aminmax + host read inside ours; det / atomic = torch with use_deterministic_algorithms(True) / (False); "
             "bincount = this library's weighted bincount (C = 1); x = that time / ours; copy = bytes read / ours as a fraction of a device-to-device "
             "copy of as many bytes; '*': took more than 50 ms and was timed by one call; '-': not run or not supported",
             f"{'case':<72}{'ours ms':>10}{'det ms':>10}{'x':>6}{'atomic ms':>10}{'x':>6}{'bincount':>10}{'x':>6}{'copy':>6}"]
    print("\n".join(lines), flush=True)

    def sz(x):
        return max(int(x * args.scale), 1)

    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    def out_of_time(label):
        if args.budget and time.perf_counter() - started > args.budget:
            record(f"{label:<72}{'not run: past --budget':>30}")
            return True
        return False

    copy_rate = {}

    def copy_ms(nbytes):
        if nbytes not in copy_rate:
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy_rate[nbytes] = timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]
            del src, dst
        return copy_rate[nbytes]

    def once_ms(work):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            out = work()
        except RuntimeError:  # (no deterministic / device implementation in this torch)
            return None, None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def run(label, ours, contenders, nbytes, exact):
        """contenders: up to three works (None: none); each is run once first and left out of the rounds when that one call took more than
        50 ms.  Ours is held against `exact`, the float64 sums: a float32 sum of up to 1e8 terms depends on its order, and the
        contenders' atomics, which add one term at a time to a sum that has outgrown it, are not what ours should equal."""
        if out_of_time(label):
            return
        got = ours()
        if not torch.allclose(got.double(), exact, rtol=1e-5, atol=1e-3):
            raise RuntimeError(f"{label}: ours differs from the float64 sums")
        del got, exact
        first, works = [], []
        for work in contenders:
            ms, out = once_ms(work) if work is not None else (None, None)
            del out
            first.append(ms)
            works.append(work if ms is not None and ms <= 50.0 else None)
        med = timed(torch, [ours] + works, args.reps, args.warmup)
        o = med[0]
        line = f"{label:<72}{o:>10.3f}"
        for ms, m in zip(first, med[1:]):
            t, mark = (m, "") if m is not None else (ms, "*" if ms is not None else "")
            line += f"{t:>9.3f}{mark or ' '}{t / o:>6.2f}" if t is not None else f"{'-':>10}{'-':>6}"
        line += f"{copy_ms(nbytes) / o:>6.2f}"
        record(line)

    def indices(dist, n, bins):
        if dist == "uniform":
            return torch.randint(0, bins, (n,), device=dev, generator=g, dtype=torch.int64)
        if dist == "constant":
            return torch.full((n,), bins // 2, device=dev, dtype=torch.int64)
        u = torch.rand(n, device=dev, generator=g, dtype=torch.float64)  # Zipf-like: P(rank r) ~ 1 / r (tools/bincount_time.py's)
        x = torch.exp(u * torch.log(torch.tensor(float(bins), dtype=torch.float64, device=dev))).to(torch.int64) - 1
        return x.clamp_(0, bins - 1)

    def with_determinism(flag, work):
        def call():
            torch.use_deterministic_algorithms(flag)
            try:
                return work()
            finally:
                torch.use_deterministic_algorithms(False)
        return call

    def index_add_case(C, M, dist, label_extra=""):
        n = sz(1e8) // C
        if out_of_time(f"i index_add float32 n={n:.0e} C={C} M={M} {dist}{label_extra}"):
            return
        idx = indices(dist, n, M)
        src = torch.randint(0, 8, (n, C), device=dev, generator=g).float()  # (small integers: the float64 sums are exact)
        base = torch.zeros(M, C, device=dev)
        exact = torch.zeros(M, C, dtype=torch.float64, device=dev)
        if dist == "constant":  # (no 1e8 float64 atomics on one row for the check)
            exact[M // 2] = src.double().sum(0)
        else:
            exact.index_add_(0, idx, src.double())
        theirs = lambda: base.index_add(0, idx, src)  # noqa: E731
        binc = (lambda: vrs.bincount(idx, weights=src.view(-1), minlength=M).view(M, 1)) if C == 1 else None
        run(f"i index_add float32 n={n:.0e} C={C} M={M} {dist}{label_extra}", lambda: vrs.index_add(base, 0, idx, src),
            [with_determinism(True, theirs), with_determinism(False, theirs), binc], n * (8 + 4 * C) + 4 * M * C, exact)

    for case in args.cases:
        if case == "i":
            for C in (64, 256, 1):
                for M in (16385, 1 << 20):
                    for dist in ("uniform", "constant", "zipf"):
                        index_add_case(C, M, dist)
                        torch.cuda.empty_cache()
        elif case == "s":
            for C in (1, 64):
                n = sz(1e8) // C
                data = torch.randint(0, 8, (n, C), device=dev, generator=g).float()
                for name, S in (("equal lengths", 16385), ("equal lengths", 1 << 20), ("zipf lengths", 16385)):
                    if name == "equal lengths":
                        lengths = torch.full((S,), n // S, device=dev, dtype=torch.int64)
                        lengths[-1] += n - int(lengths.sum())
                    else:
                        lengths = torch.bincount(indices("zipf", n, S), minlength=S)
                    theirs = lambda: torch.segment_reduce(data, "sum", lengths=lengths, unsafe=True)  # noqa: E731
                    ends = lengths.cumsum(0)
                    sums = torch.cat((torch.zeros(1, C, dtype=torch.float64, device=dev), data.double().cumsum(0)))  # (integers below 2^53: exact)
                    exact = sums[ends] - sums[ends - lengths]
                    del sums
                    run(f"s segment_reduce sum float32 n={n:.0e} C={C} S={S} {name}; det = torch.segment_reduce",
                        lambda: vrs.segment_reduce(data, "sum", lengths=lengths, unsafe=True), [theirs, None, None], n * 4 * C + 8 * S, exact)
                del data
                torch.cuda.empty_cache()
        elif case == "k":
            for C in (1, 64):
                for chunk in (64, 128, 256, 512, 1024, 4096):
                    ctx.setTuning(capi.VRS_TUNE_REDUCE_CHUNK_ROWS, chunk)
                    index_add_case(C, 16385, "zipf", f" CHUNK_ROWS={chunk}")
                ctx.setTuning(capi.VRS_TUNE_REDUCE_CHUNK_ROWS, capi.REDUCE_CHUNK_ROWS_DEFAULT)
            for lane_rows in (0, 4, 16, 64):
                ctx.setTuning(capi.VRS_TUNE_REDUCE_LANE_ROWS, lane_rows)
                index_add_case(1, 1 << 20, "uniform", f" LANE_ROWS={lane_rows}")
            ctx.setTuning(capi.VRS_TUNE_REDUCE_LANE_ROWS, capi.REDUCE_LANE_ROWS_DEFAULT)
            torch.cuda.empty_cache()
    out_path.write_text("\n".join(lines) + "\n")
    print(f"wrote {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
