"""Times vkradixsort_amd.repeat_interleave (the whole wrapper: cumsum, the host read of the total, the identity search, index_select, every
allocation inside) against torch.repeat_interleave on the same tensors in the same process, and against the composition the merge kernel
replaces, this library's own searchsorted(cumsum(repeats), arange(total), right=True) (followed by the same index_select in the 1-D
float32 form): HIP events around each call, the contenders alternating, median of --reps after --warmup.  Per case also a device-to-
device copy of the bytes the call has to move (the repeats read once, the indices written once; the values read and written once), and
the decode (the identity search alone, its output allocated inside) and the index_select separately.

Cases: --outputs outputs (10^8) from 10^6, 10^7 and 10^8 runs; (u) uniform repeats, (g) one giant run among runs of one, (z) 90 % of the
repeats zero; (1) the one-argument form, (f) the 1-D float32 form.  Prints one line per case and writes the table (default
profiles/labs/k18_repeat_interleave.txt), rewritten after every line.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table.

    python tools/repeat_interleave_time.py [--patterns ugz] [--forms 1f] [--reps 5] [--warmup 2] [--outputs 100000000] [--budget S] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RUNS = [10 ** 6, 10 ** 7, 10 ** 8]


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


def repeats_for(torch, pattern: str, runs: int, outputs: int, g, dev):
    """int64 repeats of `runs` runs that sum to `outputs` (runs <= outputs)"""
    if pattern == "u":  # uniform: outputs // runs each, the remainder over the first runs
        r = torch.full((runs,), outputs // runs, dtype=torch.int64, device=dev)
        r[:outputs % runs] += 1
    elif pattern == "g":  # runs of one and one giant run in the middle
        r = torch.ones(runs, dtype=torch.int64, device=dev)
        r[runs // 2] += outputs - runs
    else:  # 90 % zeros: the other tenth shares the outputs evenly
        r = torch.zeros(runs, dtype=torch.int64, device=dev)
        live = torch.nonzero(torch.rand(runs, generator=g, device=dev) < 0.1).flatten()
        r[live] = outputs // live.numel()
        r[live[:outputs % live.numel()]] += 1
    assert int(r.sum()) == outputs
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="ugz")
    ap.add_argument("--forms", default="1f")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--outputs", type=int, default=10 ** 8)
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k18_repeat_interleave.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import buffers, context_for

    dev = torch.device("cuda", 0)
    names = {"u": "uniform", "g": "one giant run", "z": "90 % zeros"}
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}; {args.outputs} outputs, int64 repeats; ms per call (median), "
             "every allocation and the host read of the total inside every contender; torch x, comp x = torch.repeat_interleave's / the "
             "composition's time over ours (the composition: this library's searchsorted(cumsum(repeats), arange(total), right=True), then "
             "the same index_select in the float32 form); copy ms = a device-to-device copy of the bytes the call has to move (repeats read, "
             "indices written; float32 form: values read and written too, the indices written and read); of copy = that time / ours; decode "
             "ms = the identity search alone over ready run ends (its output allocated inside); select ms = the index_select alone",
             f"{'case':<46}{'ours ms':>10}{'torch ms':>10}{'torch x':>9}{'comp ms':>10}{'comp x':>8}{'copy ms':>10}{'of copy':>9}{'decode ms':>11}{'select ms':>11}"]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    g = torch.Generator(device=dev).manual_seed(18)
    ctx = context_for(dev)

    def copy_ms(nbytes):
        src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)  # (a copy of b bytes moves 2 b)
        dst = torch.empty_like(src)
        return timed(torch, [lambda: dst.copy_(src)], 5, 2)[0]

    for runs in RUNS:
        if runs > args.outputs:
            continue
        for pattern in args.patterns:
            for form in args.forms:
                label = f"{'index' if form == '1' else 'float32'} {runs} runs, {names[pattern]}"
                if args.budget and time.perf_counter() - started > args.budget:
                    record(f"{label:<46}{'not run: past --budget':>30}")
                    continue
                r = repeats_for(torch, pattern, runs, args.outputs, g, dev)
                total = args.outputs
                x = torch.randn(runs, generator=g, device=dev) if form == "f" else None
                ends = vrs.cumsum(r, 0)

                def composed():
                    idx = vrs.searchsorted(vrs.cumsum(r, 0), torch.arange(int(r.sum()), device=dev), right=True)
                    return idx if x is None else x.index_select(0, idx)

                def decode():
                    idx = torch.empty(total, dtype=torch.int64, device=dev)
                    with buffers(ctx, ends, idx) as (bnd, res):
                        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, bnd, runs, runs, None, total, total, capi.VRS_SORT_INT64,
                                                            capi.VRS_SEARCH_RIGHT | capi.VRS_SEARCH_OUT_INT64, None, res, None))
                    return idx

                if form == "1":
                    works = [lambda: vrs.repeat_interleave(r), lambda: torch.repeat_interleave(r), composed, decode]
                    moved = 8 * runs + 8 * total
                else:
                    index = decode()
                    works = [lambda: vrs.repeat_interleave(x, r), lambda: torch.repeat_interleave(x, r), composed, decode,
                             lambda: x.index_select(0, index)]
                    moved = 8 * runs + 2 * 8 * total + 4 * runs + 4 * total
                want = works[1]()
                assert torch.equal(works[0](), want) and torch.equal(works[2](), want)
                del want
                t = timed(torch, works, args.reps, args.warmup)
                t_copy = copy_ms(moved)
                select = f"{t[4]:>11.3f}" if form == "f" else f"{'-':>11}"
                record(f"{label:<46}{t[0]:>10.3f}{t[1]:>10.3f}{t[1] / t[0]:>9.2f}{t[2]:>10.3f}{t[2] / t[0]:>8.2f}{t_copy:>10.3f}{t_copy / t[0]:>9.2f}"
                       f"{t[3]:>11.3f}{select}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
