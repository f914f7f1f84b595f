"""Times vkradixsort_amd.searchsorted / bucketize (vrs_search_sorted: plan, scratch allocation, table or index build and query kernel,
all inside the timed call) against torch.searchsorted / torch.bucketize on the same tensors in the same process: HIP events around each
call, the two alternating, median of --reps after --warmup, both outputs compared before anything is timed.  Prints one line per case
and writes the table (default profiles/labs/k10_searchsorted.txt).

Cases: (a) bucketize of 1e8 float32 / bfloat16 / int64 values into 1e2, 1e3, 1e4 boundaries; (b) 1-D M = Q in {1e6, 1e7, 1e8}, float32
and int64, uniform queries and queries drawn from the boundaries; (c) M = 1e8 float32 with Q = 1e3 .. 1e8, the direct and the indexed
tier each forced: their crossover; (d) [1e5, 1e3] rows against [1e5, 1e3] queries; (e) sorter on / off at M = Q = 1e7; (l) the LDS
tier's capacity: M = 4096 .. 40960 float32 boundaries, 1e8 queries, VRS_TUNE_SEARCH_LDS_BYTES at 64, 96, 128 and 160 KiB against the
tiers beyond it; (t) the table's threshold: bfloat16 / uint8 queries of 2^8 .. 2^24 with the table forced and switched off.

    python tools/searchsorted_time.py [--cases abcdelt] [--reps 7] [--warmup 2] [--scale 1.0] [--out FILE]
"""
from __future__ import annotations

import argparse
import sys
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
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    return med(t["ours"]), med(t["theirs"])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcdelt")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="sizes x scale (rehearsals)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k10_searchsorted.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs
    from vkradixsort_amd import capi
    from vkradixsort_amd._torch import context_for

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ctx = context_for(dev)
    keys = (capi.VRS_TUNE_SEARCH_LDS_BYTES, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES)
    defaults = (capi.SEARCH_LDS_BYTES_DEFAULT, capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT, capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT)
    lines = [f"# {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, scale {args.scale}; ms per call (median), index / table build"
             " and scratch allocation inside ours; ratio = torch / ours",
             f"{'case':<58}{'tier':>8}{'ours ms':>10}{'torch ms':>10}{'ratio':>7}"]
    print("\n".join(lines), flush=True)

    def sz(x):
        return max(int(x * args.scale), 1)

    def rand(shape, dtype):
        if dtype.is_floating_point:
            return torch.randn(shape, device=dev, generator=g, dtype=torch.float32).to(dtype)
        return torch.randint(-10 ** 9, 10 ** 9, shape if isinstance(shape, tuple) else (shape,), device=dev, generator=g, dtype=dtype)

    def run(label, seq, x, settings=None, sorter=None, yardstick=True, right=False):
        for key, value in zip(keys, settings or defaults):
            ctx.setTuning(key, defaults[keys.index(key)] if value is None else value)
        before = vrs.search_stats(ctx)
        got = vrs.searchsorted(seq, x, right=right, sorter=sorter)
        after = vrs.search_stats(ctx)
        tier = next(k for k in after if after[k] != before[k])
        want = torch.searchsorted(seq, x, right=right, sorter=sorter)
        if not torch.equal(got, want):
            raise RuntimeError(f"{label}: the outputs differ")
        del got, want
        ours, theirs = timed_pair(torch, lambda: vrs.searchsorted(seq, x, right=right, sorter=sorter),
                                  (lambda: torch.searchsorted(seq, x, right=right, sorter=sorter)) if yardstick else None, args.reps, args.warmup)
        line = f"{label:<58}{tier:>8}{ours:>10.3f}" + (f"{theirs:>10.3f}{theirs / ours:>7.2f}" if theirs else f"{'-':>10}{'-':>7}")
        print(line, flush=True)
        lines.append(line)

    for case in args.cases:
        if case == "a":
            for dtype in (torch.float32, torch.bfloat16, torch.int64):
                x = rand(sz(1e8), dtype)
                for m in (100, 1000, 10000):
                    run(f"a bucketize {str(dtype)[6:]} Q=1e8*{args.scale:g} M={m}", torch.sort(rand(m, dtype)).values, x)
                del x
        elif case == "b":
            for dtype in (torch.float32, torch.int64):
                for n in (1e6, 1e7, 1e8):
                    seq = torch.sort(rand(sz(n), dtype)).values
                    run(f"b 1-D {str(dtype)[6:]} M=Q={sz(n):.0e} uniform queries", seq, rand(sz(n), dtype))
                    run(f"b 1-D {str(dtype)[6:]} M=Q={sz(n):.0e} queries from the boundaries", seq,
                        seq[torch.randint(0, seq.numel(), (sz(n),), device=dev, generator=g)])
                    del seq
        elif case == "c":
            seq = torch.sort(rand(sz(1e8), torch.float32)).values
            for q in (1e3, 1e4, 1e5, 1e6, 1e7, 1e8):
                x = rand(max(int(q), 1), torch.float32)
                run(f"c M={seq.numel():.0e} float32 Q={int(q):.0e} direct", seq, x, (None, 0, 0))
                run(f"c M={seq.numel():.0e} float32 Q={int(q):.0e} indexed", seq, x, (None, 0, 1), yardstick=False)
                del x
            del seq
        elif case == "d":
            b = sz(1e5)
            for dtype in (torch.float32, torch.float64):
                seq = torch.sort(rand((b, 1000), dtype), dim=-1).values
                run(f"d rows [{b}, 1000] x [{b}, 1000] {str(dtype)[6:]}", seq, rand((b, 1000), dtype))
                del seq
        elif case == "e":
            raw = rand(sz(1e7), torch.float32)
            x = rand(sz(1e7), torch.float32)
            srt = torch.argsort(raw)
            run(f"e M=Q={raw.numel():.0e} float32 sorter", raw, x, sorter=srt)
            run(f"e M=Q={raw.numel():.0e} float32 no sorter", raw[srt], x)
            run(f"e M=1e4 Q={raw.numel():.0e} float32 sorter", raw[:10000].contiguous(), x, sorter=torch.argsort(raw[:10000]))
            del raw, x, srt
        elif case == "l":
            x = rand(sz(1e8), torch.float32)
            for m in (4096, 8192, 16384, 24576, 32768, 40960):
                seq = torch.sort(rand(m, torch.float32)).values
                for lds in (64, 96, 128, 160):
                    if m * 4 <= lds * 1024:
                        run(f"l M={m} float32 Q={x.numel():.0e} LDS tier, {lds} KiB claimed", seq, x, (lds * 1024, 0, None), yardstick=(lds == 160))
                run(f"l M={m} float32 Q={x.numel():.0e} indexed instead", seq, x, (0, 0, 1), yardstick=False)
                run(f"l M={m} float32 Q={x.numel():.0e} direct instead", seq, x, (0, 0, 0), yardstick=False)
            del x
        elif case == "t":
            for dtype, m in ((torch.bfloat16, 1000), (torch.bfloat16, 10 ** 6), (torch.uint8, 1000)):
                seq = torch.sort(rand(m, torch.float32).to(dtype) if dtype != torch.uint8 else torch.randint(0, 256, (m,), device=dev, dtype=dtype)).values
                for q in (2 ** 8, 2 ** 12, 2 ** 16, 2 ** 20, 2 ** 24):
                    x = rand(q, torch.float32).to(dtype) if dtype != torch.uint8 else torch.randint(0, 256, (q,), device=dev, dtype=dtype)
                    run(f"t {str(dtype)[6:]} M={m} Q=2^{q.bit_length() - 1} table", seq, x, (None, 1, None))
                    run(f"t {str(dtype)[6:]} M={m} Q=2^{q.bit_length() - 1} no table", seq, x, (None, 0, None), yardstick=False)
        torch.cuda.empty_cache()
    for key, value in zip(keys, defaults):
        ctx.setTuning(key, value)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
