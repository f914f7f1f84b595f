"""Times vkradixsort_amd.mode (the whole wrapper: the rank map, the bare-key sort, the mode form of vrs_sort_restore, every allocation
inside) against torch.mode on the same tensor in the same process, and against the composition a user of this library had before it:
vkradixsort_amd.sort (which carries a position payload through every pass) plus run detection in torch ops (a comparison of
neighbours, cummax, argmax, two gathers).  HIP events around each call, the contenders alternating, median and spread (min .. max) of
--reps after --warmup.

Per case also the three steps separately, through the C calls on buffers allocated beforehand -- the rank map, the sort, the mode form
(two memsets, three launches) -- and the mode form's achieved bytes per second, counting one read of the ranks and one of the input,
beside a clone of a tensor of the same byte count timed in the same run.

Cases: 1 x 10^8 int32 with 10^3 distinct values, 1 x 10^8 float32 uniform, 10^5 x 10^3 int32, 10^6 x 32 bfloat16, 1 x 5*10^7 int64.
Before a case is timed, ours is checked against the composition (values and indices equal) and against torch.mode on the device
(its value as frequent as ours and not smaller: torch's GPU mode answers any of the most frequent values).  Prints one line per case and writes the table (default profiles/labs/k20_mode.txt), rewritten after every line.

--budget SECONDS: no case is started after that many seconds; the cases left out are named in the table.  torch.mode is timed --torch-reps
times only (it is the slow one at some shapes), and once only when that one call takes more than --torch-slow seconds.

    python tools/mode_time.py [--cases 0,1,2,3,4] [--scale 1.0] [--reps 5] [--warmup 2] [--torch-reps 3] [--budget S] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, works, reps: int, warmup: int):
    """(median, min, max) ms of every work, one call of each per round"""
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
    return [(sorted(v)[len(v) // 2], min(v), max(v)) for v in t]


def cell(m) -> str:
    return f"{m[0]:.3f} ({m[1]:.3f}..{m[2]:.3f})"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2,3,4")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every case's rows (or its one row's length): a quick look")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-slow", type=float, default=3.0)
    ap.add_argument("--budget", type=float, default=0.0, help="start no case after this many seconds (0: no limit)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k20_mode.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import buffers, context_for, row_offsets
    from vkradixsort_amd.sort import _dtype_code

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20)
    s = args.scale

    def scaled(v):
        return max(1, int(v * s))

    cases = [
        ("1 x 1e8 int32, 1e3 distinct", lambda: torch.randint(0, 1000, (1, scaled(10 ** 8)), generator=g, device=dev, dtype=torch.int32)),
        ("1 x 1e8 float32 uniform", lambda: torch.rand((1, scaled(10 ** 8)), generator=g, device=dev)),
        ("1e5 x 1e3 int32, 64 distinct", lambda: torch.randint(0, 64, (scaled(10 ** 5), 1000), generator=g, device=dev, dtype=torch.int32)),
        ("1e6 x 32 bfloat16 normal", lambda: torch.randn((scaled(10 ** 6), 32), generator=g, device=dev).to(torch.bfloat16)),
        ("1 x 5e7 int64, 1e3 distinct", lambda: torch.randint(0, 1000, (1, scaled(5 * 10 ** 7)), generator=g, device=dev) << 24),
    ]
    head = (f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup} (torch.mode: {args.torch_reps}, 1); scale {s}; ms per call: "
            "median (min..max), every allocation inside ours, torch's and the composition's; torch x, comp x = torch.mode's / the composition's "
            "median over ours (the composition: this library's sort with its position payload, then != of neighbours, cummax, argmax and two "
            "gathers in torch); rank, sort, form = the three C calls of ours on buffers allocated beforehand (form: two memsets and three "
            "launches); form GB/s = one read of the ranks and one of the input over form's median; clone = a clone of a tensor of that "
            "many bytes (it reads and writes them), GB/s counted the same way")
    cols = f"{'case':<30}{'ours ms':>24}{'torch ms':>38}{'torch x':>10}{'comp ms':>32}{'comp x':>9}{'rank ms':>9}{'sort ms':>9}{'form ms':>9}{'form GB/s':>11}{'clone ms':>10}{'clone GB/s':>12}"
    lines = [head, cols]
    print("\n".join(lines), flush=True)
    started = time.perf_counter()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(line):
        print(line, flush=True)
        lines.append(line)
        out_path.write_text("\n".join(lines) + "\n")

    ctx = context_for(dev)
    lib = ctx.lib

    for k in (int(v) for v in args.cases.split(",")):
        label, make = cases[k]
        if args.budget and time.perf_counter() - started > args.budget:
            record(f"{label:<30}{'not run: past --budget':>30}")
            continue
        x = make()
        rows, L = x.shape
        n = rows * L

        def composed():
            st = vrs.sort(x, -1)
            v, order = st.values, st.indices
            at = torch.arange(L, device=dev)
            first = torch.ones((rows, L), dtype=torch.bool, device=dev)
            first[:, 1:] = v[:, 1:] != v[:, :-1]
            start = torch.cummax(torch.where(first, at, 0), 1).values
            score = (at - start + 1) * (L + 1) + (L - start)  # the longest run; of equally long ones the first
            j = score.argmax(1, keepdim=True)                  # (its last element: the stable sort put the last occurrence there)
            return v.gather(1, j).squeeze(1), order.gather(1, j).squeeze(1)

        ours = vrs.mode(x, 1)
        theirs = composed()
        assert torch.equal(ours.values, theirs[0]) and torch.equal(ours.indices, theirs[1]), label
        del theirs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            ref = torch.mode(x, 1)
            torch.cuda.synchronize()
        except RuntimeError as e:  # (torch's own limits: the table says so and goes on)
            ref = None
            print(f"torch.mode failed on {label}: {str(e).splitlines()[0]}", flush=True)
        once = time.perf_counter() - t0
        if ref is not None:  # torch's GPU mode picks any of the most frequent values: as frequent as ours, and not below it
            count = lambda v: (x == v.unsqueeze(1)).sum(1)  # noqa: E731
            assert torch.equal(count(ours.values), count(ref.values)) and bool((ours.values <= ref.values).all()), label
            assert bool((x.gather(1, ref.indices.unsqueeze(1)).squeeze(1) == ref.values).all()), label
        del ours
        ms = timed(torch, [lambda: vrs.mode(x, 1), composed], args.reps, args.warmup)
        if ref is None:
            t_torch = (float("nan"),) * 3
        elif once > args.torch_slow:
            t_torch = (once * 1e3,) * 3
        else:
            t_torch = timed(torch, [lambda: torch.mode(x, 1)], args.torch_reps, 1)[0]
        del ref

        # the three steps, on buffers of their own
        wide = x.dtype in (torch.int64, torch.float64)
        rdt, w = (torch.int64, "u64") if wide else (torch.int32, "u32")
        code = _dtype_code(torch, x.dtype)
        ranks, tmp = torch.empty(n, dtype=rdt, device=dev), torch.empty(n, dtype=rdt, device=dev)
        scratch, vals, idx = torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, dtype=x.dtype, device=dev), torch.empty(rows, dtype=torch.int64, device=dev)
        offsets = row_offsets(rows, L, dev) if rows > 1 else None
        with buffers(ctx, x, ranks, tmp, scratch, vals, idx, offsets) as (src, rk, rk_tmp, scr, bv, bi, offs):
            steps = [lambda: ctx.check(lib.vrs_sort_rank_keys(ctx.handle, src, n, L, code, 0, rk, None)),
                     (lambda: ctx.check(getattr(lib, f"vrs_sort_keys_{w}")(ctx.handle, rk, rk_tmp, n))) if rows == 1 else
                     (lambda: ctx.check(getattr(lib, f"vrs_sort_segments_{w}")(ctx.handle, rk, rk_tmp, n, offs, rows))),
                     lambda: ctx.check(lib.vrs_sort_restore(ctx.handle, src, rk, scr, n, L, code, capi.VRS_SORT_MODE, bv, bi))]
            t_steps = timed(torch, steps, args.reps, args.warmup)  # (in this order every round: the sort always sorts fresh ranks)
        nbytes = n * (x.element_size() + ranks.element_size())
        del ranks, tmp
        blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        t_clone = timed(torch, [lambda: blob.clone()], args.reps, args.warmup)[0]
        del blob
        record(f"{label:<30}{cell(ms[0]):>24}{cell(t_torch):>38}{t_torch[0] / ms[0][0]:>10.2f}{cell(ms[1]):>32}{ms[1][0] / ms[0][0]:>9.2f}"
               f"{t_steps[0][0]:>9.3f}{t_steps[1][0]:>9.3f}{t_steps[2][0]:>9.3f}{nbytes / t_steps[2][0] / 1e6:>11.1f}{t_clone[0]:>10.3f}{nbytes / t_clone[0] / 1e6:>12.1f}")
        del x
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
