"""Times unique(dim=0) and unique_consecutive(dim=0) (the row form of vrs_unique / vrs_run_length_encode) with return_inverse and
return_counts, HIP events around the whole call -- allocation and the host read of R inside every contender -- median of --reps, the
contenders alternating rep by rep, the whole run repeated --repeats times so a spread can be given (the range of the medians).

Contenders: ours; torch.unique(dim=0) / torch.unique_consecutive(dim=0) on the device; the composition a caller writes today with this
library (per group of columns a stable argsort and a gather, then adjacent compare, cumsum and scatter in torch); a device copy of
the bytes the call must move (the rows read, R rows, the int64 inverse and counts written).

For ours the kernels of one call are reported apart (the pack of each round, each sort, the encode, the counts, the row gather): a
child process runs the call alone under `rocprofv3 --kernel-trace` and the trace of its last call is summed per stage.  Besides,
unique of as many int64 keys as the first int32 x 2 shape has rows, in the same run: the same work apart from the pack and the gather.

    python tools/unique_rows_time.py [--shapes 0,1,...] [--reps 5] [--repeats 3] [--no-stages] [--out profiles/labs/k21_unique_rows.txt]
"""
from __future__ import annotations

import argparse
import csv
import glob
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# (name, rows, columns, dtype, what the words are, consecutive too)
SHAPES = [("edges int64", 50_000_000, 2, "int64", "edges", True), ("edges int32", 50_000_000, 2, "int32", "edges", True),
          ("few distinct", 30_000_000, 3, "int32", "few", False), ("float32 x 4", 10_000_000, 4, "float32", "random", False),
          ("float32 x 16", 1_000_000, 16, "float32", "random", False), ("int32 x 128", 100_000, 128, "int32", "random", False)]


def make(torch, shape, seed=1):
    _, n, C, dtype, kind, _ = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = getattr(torch, dtype)
    if kind == "edges":  # random edges, about 10 % of the rows a second occurrence
        x = torch.randint(0, 1 << 24, (n, C), device="cuda", generator=g)
        dup = n // 10
        x[n - dup:] = x[torch.randint(0, n - dup, (dup,), device="cuda", generator=g)]
        return x.to(dt)
    if kind == "few":
        return torch.randint(0, 4, (n, C), device="cuda", generator=g).to(dt)
    x = torch.randint(0, 1 << 20, (n, C), device="cuda", generator=g)
    x[:, : C - 1] = x[:, : C - 1] % 3  # rows tie in all but the last column: every round matters
    return (x.to(dt) - 7) * (0.5 if dt.is_floating_point else 3)


def composition(torch, vrs, x):
    """what a caller writes without the row form: LSD over groups of columns by vrs.argsort(stable) and gathers, then torch passes"""
    n, C = x.shape
    perm = None
    c = C
    while c > 0:
        if x.dtype == torch.int32 and c >= 2:  # two int32 columns as one int64 key
            cols = x[:, c - 2:c] if perm is None else x[perm, c - 2:c]
            key = (cols[:, 0].to(torch.int64) << 32) | (cols[:, 1].to(torch.int64) + (1 << 31))
            c -= 2
        else:
            key = x[:, c - 1] if perm is None else x[perm, c - 1]
            c -= 1
        idx = vrs.argsort(key.contiguous(), stable=True)
        perm = idx if perm is None else perm[idx]
    rows = x[perm]
    head = torch.ones(n, dtype=torch.bool, device=x.device)
    head[1:] = (rows[1:] != rows[:-1]).any(1)
    ids = torch.cumsum(head, 0) - 1
    inverse = torch.empty(n, dtype=torch.int64, device=x.device)
    inverse[perm] = ids
    starts = torch.nonzero(head).view(-1)  # (a host read of R, as in every contender)
    counts = torch.diff(starts, append=torch.tensor([n], device=x.device))
    return rows[starts], inverse, counts


def event_ms(torch, work) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    work()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def medians(torch, works: dict, reps: int, repeats: int) -> dict:
    """per contender: the median of `reps` per repeat; reported: the middle of these medians and their range"""
    for w in works.values():
        w()  # warm-up (and the one-call sort's plan)
    out = {k: [] for k in works}
    for _ in range(repeats):
        times = {k: [] for k in works}
        for _ in range(reps):
            for k, w in works.items():
                times[k].append(event_ms(torch, w))
        for k, t in times.items():
            out[k].append(sorted(t)[len(t) // 2])
    return {k: {"ms": sorted(m)[len(m) // 2], "lo": min(m), "hi": max(m)} for k, m in out.items()}


def stage_of(name: str):
    for tag, stage in (("rows_pack_kernel", "pack"), ("rle_rows_kernel", "encode"), ("rows_out_kernel", "gather"), ("rle_counts_kernel", "counts")):
        if tag in name:
            return stage
    return "sort"


def stages(index: int):
    """the kernels of one of our calls, per stage in milliseconds, by a child process under the profiler"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "ours", "--", sys.executable, str(Path(__file__).resolve()),
               "--ours-only", str(index)]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
        if proc.returncode != 0 or not files:
            return f"the profiled run failed (exit {proc.returncode}): {proc.stderr[-300:]}"
        rows = list(csv.DictReader(open(files[0])))
    try:
        ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows), key=lambda k: k[0])
    except KeyError as e:
        return f"unexpected trace columns ({e})"
    firsts = [i for i, k in enumerate(ks) if "rows_pack_kernel" in k[2] and "true>" in k[2].replace(" ", "")]
    if not firsts:
        return "no row-form call in the trace"
    out, rnd = [], 0
    for start, end, name in ks[firsts[-1]:]:
        stage = stage_of(name)
        if stage == "pack":
            rnd += 1
        label = f"{stage} {rnd}" if stage in ("pack", "sort") else stage
        if out and out[-1][0] == label:
            out[-1][1] += (end - start) * 1e-6
        else:
            out.append([label, (end - start) * 1e-6])
        if stage == "gather":
            break
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--ours-only", type=int, default=None, help="run our call on one shape three times and exit (for a profiler)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "labs" / "k21_unique_rows.txt"))
    args = ap.parse_args()

    import torch

    import vkradixsort_amd as vrs

    if args.ours_only is not None:
        x = make(torch, SHAPES[args.ours_only])
        for _ in range(3):
            vrs.unique(x, return_inverse=True, return_counts=True, dim=0)
        torch.cuda.synchronize()
        return 0

    lines = [f"unique(dim=0) with inverse and counts on {torch.cuda.get_device_name(0)}: medians of {args.reps}, the middle of {args.repeats} "
             "repeats [lowest .. highest median], ms; allocation and the host read of R inside every contender", ""]

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    kw = {"return_inverse": True, "return_counts": True, "dim": 0}
    chosen = [int(s) for s in args.shapes.split(",") if s != ""]
    for i in chosen:
        shape = SHAPES[i]
        name, n, C, dtype, _, consecutive = shape
        x = make(torch, shape)
        values, _, _ = vrs.unique(x, **kw)
        R = values.shape[0]
        moved = n * C * x.element_size() + R * C * x.element_size() + 8 * n + 8 * R
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        works = {"ours": lambda: vrs.unique(x, **kw), "torch": lambda: torch.unique(x, **kw), "composition": lambda: composition(torch, vrs, x),
                 "copy": lambda: src.clone()}
        if i == 1:  # the same work apart from the pack and the row gather: the word form on as many int64 keys
            flat = (x[:, 0].to(torch.int64) << 32) | x[:, 1].to(torch.int64)
            works["unique of n int64 keys"] = lambda: vrs.unique(flat, return_inverse=True, return_counts=True)
        t = medians(torch, works, args.reps, args.repeats)
        emit(f"[{n}, {C}] {dtype} ({name}), R = {R}, must move {moved / 1e6:.0f} MB")
        for k, v in t.items():
            emit(f"  {k:24s} {v['ms']:10.3f}  [{v['lo']:.3f} .. {v['hi']:.3f}]   x{v['ms'] / t['ours']['ms']:.2f} of ours")
        if not args.no_stages:
            st = stages(i)
            emit("  ours, one call's kernels: " + (st if isinstance(st, str) else ", ".join(f"{k} {ms:.3f}" for k, ms in st) +
                                                    f"; sum {sum(ms for _, ms in st):.3f}"))
        if consecutive:
            y = x[vrs.argsort(x[:, 0].contiguous(), stable=True)]  # runs: the rows grouped by their first column
            works = {"ours": lambda: vrs.unique_consecutive(y, **kw), "torch": lambda: torch.unique_consecutive(y, **kw), "copy": lambda: src.clone()}
            t = medians(torch, works, args.reps, args.repeats)
            emit(f"  unique_consecutive(dim=0) of the rows ordered by column 0, R = {vrs.unique_consecutive(y, dim=0).shape[0]}")
            for k, v in t.items():
                emit(f"    {k:22s} {v['ms']:10.3f}  [{v['lo']:.3f} .. {v['hi']:.3f}]   x{v['ms'] / t['ours']['ms']:.2f} of ours")
            del y
        emit()
        del x, src, values
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
