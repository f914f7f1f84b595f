"""Times vkradixsort_amd.isin (the whole wrapper: the sort of the test set, the membership search, every allocation inside) against
torch.isin on the same tensors in the same process, and against the composition the membership form replaces, this library's own
sort + searchsorted + clamp + gather + == (+ logical_not with invert): HIP events around each call, the contenders alternating, median
of --reps after --warmup.  Per case also a device-to-device copy of the bytes the call has to move (the elements and the test set read
once, one byte per element written), and the two steps separately: the membership search alone over a test set sorted beforehand (its
output and scratch allocated inside) and the sort of the test set alone.

Cases: --elements elements (10^8) against test sets of 10^2, 10^4, 10^6 and 10^8; int64, int32, float32 and int16; each with and without
invert.  Both sides hold whole numbers drawn evenly from [0, 2 * test set) (int16: from the dtype's whole range), so about 4 in 10
elements are members.  Prints one line per case and writes the table (default profiles/labs/k19_isin.txt), rewritten after every line.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table.

    python tools/isin_time.py [--dtypes int64,int32,float32,int16] [--tests 100,10000,1000000,100000000] [--reps 5] [--warmup 2]
                              [--elements 100000000] [--budget S] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
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
    ap.add_argument("--dtypes", default="int64,int32,float32,int16")
    ap.add_argument("--tests", default="100,10000,1000000,100000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--elements", type=int, default=10 ** 8)
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k19_isin.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import buffers, context_for
    from vkradixsort_amd.search import TIER_NAMES
    from vkradixsort_amd.sort import _dtype_code

    dev = torch.device("cuda", 0)
    n = args.elements
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}; {n} elements; ms per call (median), every allocation "
             "inside every contender; torch x, comp x = torch.isin's / the composition's time over ours (the composition: this library's "
             "sort_values, searchsorted, then clamp_, a gather, == and with invert logical_not); copy ms = a device-to-device copy of the "
             "bytes the call has to move (elements and test set read, one byte per element written); of copy = that time / ours; search ms "
             "= the membership call alone over a sorted test set (output and scratch allocated inside), in `tier`; sort ms = the sort of "
             "the test set alone",
             f"{'case':<40}{'ours ms':>10}{'torch ms':>10}{'torch x':>9}{'comp ms':>10}{'comp x':>8}{'copy ms':>10}{'of copy':>9}{'search ms':>11}{'sort ms':>10}{'tier':>9}"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    g = torch.Generator(device=dev).manual_seed(19)
    ctx = context_for(dev)

    def copy_ms(nbytes):
        src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)  # (a copy of b bytes moves 2 b)
        dst = torch.empty_like(src)
        return timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]

    for name in args.dtypes.split(","):
        dt = getattr(torch, name)
        code = _dtype_code(torch, dt)
        for m in (int(v) for v in args.tests.split(",")):
            lo, hi = (-32768, 32768) if name == "int16" else (0, 2 * m)
            x = t = None
            for invert in (False, True):
                label = f"{name} {m} tests{', invert' if invert else ''}"
                if args.budget and time.perf_counter() - started > args.budget:
                    record(f"{label:<40}{'not run: past --budget':>30}")
                    continue
                if x is None:
                    x = torch.randint(lo, hi, (n,), generator=g, device=dev).to(dt)
                    t = torch.randint(lo, hi, (m,), generator=g, device=dev).to(dt)
                    s = vrs.sort_values(t)
                    tier, need = ctypes.c_int(), ctypes.c_uint64()
                    ctx.check(ctx.lib.vrs_search_plan(ctx.handle, m, m, n, n, code, 0, ctypes.byref(tier), ctypes.byref(need)))
                flags = capi.VRS_SEARCH_MEMBER | (capi.VRS_SEARCH_MEMBER_INVERT if invert else 0)

                def composed():
                    srt = vrs.sort_values(t)
                    idx = vrs.searchsorted(srt, x).clamp_(max=m - 1)
                    hit = srt[idx] == x
                    return hit.logical_not_() if invert else hit

                def search():
                    out = torch.empty(n, dtype=torch.bool, device=dev)
                    scratch = torch.empty(need.value, dtype=torch.uint8, device=dev) if need.value else None
                    with buffers(ctx, s, x, out, scratch) as (bnd, qry, res, scr):
                        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, bnd, m, m, qry, n, n, code, flags, None, res, scr))
                    return out

                works = [lambda: vrs.isin(x, t, invert=invert), lambda: torch.isin(x, t, invert=invert), composed, search,
                         lambda: vrs.sort_values(t)]
                want = works[1]()
                assert torch.equal(works[0](), want) and torch.equal(works[2](), want) and torch.equal(works[3](), want)
                del want
                ms = timed(torch, works, args.reps, args.warmup)
                t_copy = copy_ms((n + m) * x.element_size() + n)
                record(f"{label:<40}{ms[0]:>10.3f}{ms[1]:>10.3f}{ms[1] / ms[0]:>9.2f}{ms[2]:>10.3f}{ms[2] / ms[0]:>8.2f}{t_copy:>10.3f}"
                       f"{t_copy / ms[0]:>9.2f}{ms[3]:>11.3f}{ms[4]:>10.3f}{TIER_NAMES[tier.value]:>9}")
            del x, t
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
