#!/usr/bin/env python3
"""What the compiler made of a kernel's LDS and store pipelining: compiles ONE unit of vkradixsort_amd/csrc to gfx950 assembly (device
code only, the flags of vkradixsort_amd/build.py) and prints, per function whose name matches a pattern:

  vgprs / scratch / lds / occ   the assembler's own resource summary of the function
  spills / hot                  instructions carrying the assembler's "Folded Spill" / "Folded Reload" comment; hot: those of them in a basic
                                block without a call (registers saved and restored in the block that calls an out-of-line copy are not hot)
  dep_reads                     ds_read_b32 whose NEXT instruction is s_waitcnt ... lgkmcnt(0): an LDS round trip nothing overlaps (a select
                                over an LDS read that became a branch with the read sunk into it looks like this -- DESIGN.md K5c).  Not
                                counted: such a read directly behind s_barrier -- a wave's first LDS access after a workgroup barrier, which
                                has emptied its queues: there is nothing of the wave's own to overlap it with (a scan's read of its own bin)
  store_waits                   s_waitcnt ... vmcnt(0) with a global store before it AND behind it in one chain of basic blocks (a chain
                                ends at an unconditional branch, a call, a return, the program's end or a workgroup barrier): stores
                                that wait for earlier stores to be acknowledged -- what the reload of a spilled register costs.  The
                                wait of a release fence the source asks for (it follows a buffer_wbl2) is not counted.
  saveexec / lgkm0              exec-mask branches, and all waits for an empty LDS queue

It looks for nothing else.  No GPU needed.

    python tools/isa_audit.py vkradixsort_amd/csrc/vrs_msd_pool_local.hip --pattern 'pool_local_sort_(wave_)?kernel'
    python tools/isa_audit.py --asm saved.s            # a listing made earlier
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("vgprs", "scratch", "lds", "occ", "spills", "hot", "dep_reads", "store_waits", "saveexec", "lgkm0")

_FUNC = re.compile(r"^(\w+):\s*; @\1\s*$")
_END = re.compile(r"^\.Lfunc_end\d+:")
_INFO = {"vgprs": re.compile(r"^; NumVgprs: (\d+)"), "scratch": re.compile(r"^; ScratchSize: (\d+)"),
         "lds": re.compile(r"^; LDSByteSize: (\d+)"), "occ": re.compile(r"^; Occupancy: (\d+)")}
_CHAIN_END = ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64", "s_barrier")


def _instruction(line: str):
    """(mnemonic, operands, comment) of an instruction line; ("label", ..) for a label; None for directives, comments and blank lines."""
    code, _, comment = line.partition(";")
    code = code.strip()
    if code.endswith(":"):
        return "label", code, comment
    if not code or code.startswith("."):
        return None
    mnemonic, _, operands = code.partition(" ")
    return mnemonic.strip(), operands.strip(), comment


def _count_body(body, first_line):
    """the counts of one function's lines, and under "where" the listing's line numbers of the spills, dependent reads and store waits"""
    ins, block, blocks, calling = [], 0, [], set()  # blocks[n]: the basic block of instruction n; calling: the blocks that hold a call
    for n, i in enumerate(map(_instruction, body)):
        if not i:
            continue
        if i[0] == "label":
            block += 1
            continue
        ins.append((first_line + n, *i))
        blocks.append(block)
        if i[0] == "s_swappc_b64":
            calling.add(block)
        if i[0].startswith("s_cbranch") or i[0] in ("s_branch", "s_setpc_b64", "s_endpgm"):
            block += 1
    c = dict(saveexec=0, lgkm0=0)
    where = dict(spills=[], hot=[], dep_reads=[], store_waits=[])
    # store_waits: per chain, the vmcnt(0) waits seen since the chain's first store count once the next store shows up
    stored, pending = False, []
    for n, (at, m, ops, comment) in enumerate(ins):
        if "Folded Spill" in comment or "Folded Reload" in comment:
            where["spills"].append(at)
            if blocks[n] not in calling:
                where["hot"].append(at)
        if "saveexec" in m:
            c["saveexec"] += 1
        if m == "s_waitcnt":
            if "lgkmcnt(0)" in ops:
                c["lgkm0"] += 1
                if n > 0 and ins[n - 1][1] == "ds_read_b32" and not (n > 1 and ins[n - 2][1] == "s_barrier"):
                    where["dep_reads"].append(at)
            if "vmcnt(0)" in ops and stored and ins[n - 1][1] != "buffer_wbl2":
                pending.append(at)
        elif m.startswith("global_store"):
            where["store_waits"] += pending
            stored, pending = True, []
        elif m in _CHAIN_END:
            stored, pending = False, []
    c.update({k: len(v) for k, v in where.items()})
    c["where"] = where
    return c


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or next((str(p) for p in (Path("/opt/rocm/lib/llvm/bin/llvm-cxxfilt"), Path("/opt/rocm/llvm/bin/llvm-cxxfilt"))
                                                 if p.exists()), None) or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    lines = out.stdout.splitlines()
    return dict(zip(names, lines)) if out.returncode == 0 and len(lines) == len(names) else {n: n for n in names}


def short(name: str) -> str:
    """a demangled name without its parameter list and namespaces: pool_local_sort_kernel<256, 7, 4, 7u>"""
    name = re.sub(r"^void ", "", name)
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            cut = i
            break
    return name[:cut].replace("vrs::", "").replace("(anonymous namespace)::", "")


def parse(text: str):
    """[{name (mangled), vgprs, scratch, lds, occ, spills, hot, dep_reads, store_waits, saveexec, lgkm0, where}] of every function of a listing, in
    its order; lds and occ are None for a function that is no kernel."""
    out, name, body, first, cur = [], None, [], 0, None
    for at, line in enumerate(text.splitlines(), 1):
        if name is None:
            m = _FUNC.match(line)
            if m:
                name, body, first = m.group(1), [], at + 1
                continue
            if cur is not None:  # the resource summary follows the function it belongs to
                for key, rx in _INFO.items():
                    m = rx.match(line)
                    if m and cur[key] is None:
                        cur[key] = int(m.group(1))
        elif _END.match(line):
            cur = dict(name=name, vgprs=None, scratch=None, lds=None, occ=None, **_count_body(body, first))
            out.append(cur)
            name = None
        else:
            body.append(line)
    return out


def compile_unit(source: Path, arch: str = "gfx950") -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / "unit.s"
        cmd = [hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'vkradixsort_amd' / 'csrc'}", "-S",
               "--cuda-device-only", str(source), "-o", str(asm)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("compile failed: %s\n%s" % (" ".join(cmd), proc.stderr))
        return asm.read_text()


def audit(text: str, pattern: str = "."):
    """parse() of the functions whose mangled or demangled name matches, each with its short demangled name under "short"."""
    rows = parse(text)
    names = demangle([r["name"] for r in rows])
    rx = re.compile(pattern)
    keep = []
    for r in rows:
        r["short"] = short(names[r["name"]])
        if rx.search(r["name"]) or rx.search(names[r["name"]]):
            keep.append(r)
    return keep


def table(rows) -> str:
    width = max([len(r["short"]) for r in rows] + [8])
    head = f"{'function':<{width}} " + " ".join(f"{f:>9}" for f in FIELDS)
    lines = [head]
    for r in rows:
        lines.append(f"{r['short']:<{width}} " + " ".join(f"{'-' if r[f] is None else r[f]:>9}" for f in FIELDS))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", nargs="?", help="a .hip unit to compile")
    ap.add_argument("--asm", help="audit this assembly listing instead of compiling")
    ap.add_argument("--where", action="store_true", help="also print the listing's line numbers of every spill, dependent read and store wait")
    ap.add_argument("--pattern", default="kernel", help="regular expression over mangled and demangled function names (default: kernel)")
    args = ap.parse_args()
    if not args.source and not args.asm:
        ap.error("a source file or --asm")
    text = Path(args.asm).read_text() if args.asm else compile_unit(Path(args.source))
    rows = audit(text, args.pattern)
    if not rows:
        print("no function matches", file=sys.stderr)
        return 1
    print(table(rows))
    if args.where:
        for r in rows:
            for kind, lines in r["where"].items():
                if lines:
                    print(f"{r['short']}: {kind} at lines {' '.join(map(str, lines))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
