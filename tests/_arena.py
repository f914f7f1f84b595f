"""One guarded, poisoned allocation that holds every buffer of one C call: the memory contract of an entry point, checked byte by byte.

A case places all of a call's buffers into one Arena, each with exactly the bytes the header documents (never rounded up), a role that
says which of its bytes the call may change, and the alignment the header demands.  Between the ranges lie guards the test owns.  The
whole allocation -- outputs, scratch and guards included -- is filled with seeded random bytes (no constant canary: a kernel that
stores zeros or one repeated byte must not be able to match it), the inputs are copied in, and after the call every byte outside the
writable intervals is compared with a snapshot taken before it.  No fixtures live here and nothing here needs a GPU: the checker's own
tests run on the CPU (test_arena_cpu.py).

Roles:  "in"       no byte may change
        "scratch"  any byte may change
        "out", "inout"   only the byte intervals given as `writable` (relative to the range's start) may change
Layouts: "round"   every range starts on a 256-byte boundary
         "tight"   every range starts on exactly its demanded alignment and off the next larger power of two (up to 16 bytes: a range
                   that demands 16 starts at 16 mod 32), which drives the misaligned head and tail paths
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

GUARD = 4096             # at least this many bytes before every range
TAIL_GUARD = 64 * 1024   # at least this many behind the last
ROUND = 256
LAYOUTS = ("round", "tight")
ROLES = ("in", "scratch", "out", "inout")


@dataclass
class Range:
    name: str
    start: int
    nbytes: int
    role: str
    align: int
    writable: list = field(default_factory=list)  # (begin, end) byte intervals relative to start

    @property
    def end(self) -> int:
        return self.start + self.nbytes


class ArenaViolation(AssertionError):
    """A byte changed that the contract forbids.  range_name: the range the first such byte lies in or directly behind (None when it
    lies in the guard before the first range); offset_from_end: its distance from that range's end (0 = the first byte behind it,
    negative = inside); next_name / before_next: the range that follows and the distance to its start (1 = the last guard byte
    before it); index: its offset in the arena; count: how many forbidden bytes changed."""

    def __init__(self, message, range_name, offset_from_end, next_name, before_next, index, count):
        super().__init__(message)
        self.range_name, self.offset_from_end = range_name, offset_from_end
        self.next_name, self.before_next = next_name, before_next
        self.index, self.count = index, count


def tight_start(cursor: int, align: int) -> int:
    """the first offset >= cursor that is a multiple of `align` and not of 2 * align (align capped at 16)"""
    a = min(align, 16)
    start = -(-cursor // a) * a
    return start if start % (2 * a) else start + a


class Arena:
    def __init__(self, device, seed: int, layout: str, case: str = ""):
        assert layout in LAYOUTS, layout
        self.device, self.seed, self.layout, self.case = torch.device(device), seed, layout, case
        self.ranges: dict[str, Range] = {}
        self._cursor = 0
        self.mem = None        # the arena's bytes, its first on a 256-byte boundary
        self._snapshot = None
        self._buffers = []

    # ---------------------------------------------------------------------------------------------- laying out
    def place(self, name: str, nbytes: int, role: str, align: int, writable=None) -> Range:
        """nbytes: exactly what the header documents.  writable (out / inout): byte intervals [(begin, end), ...] relative to the range."""
        assert self.mem is None, "place every range before fill()"
        assert role in ROLES and name not in self.ranges and nbytes >= 0 and align in (1, 2, 4, 8, 16), (name, role, nbytes, align)
        cursor = self._cursor + GUARD
        start = -(-cursor // ROUND) * ROUND if self.layout == "round" else tight_start(cursor, align)
        if role in ("out", "inout"):
            assert writable is not None, f"{name}: an {role} range lists what may change"
            spans = [(int(b), int(e)) for b, e in writable if e > b]
            assert all(0 <= b and e <= nbytes for b, e in spans), (name, spans, nbytes)
        else:
            assert writable is None, f"{name}: only out and inout ranges take writable intervals"
            spans = [(0, nbytes)] if role == "scratch" else []
        r = Range(name, start, int(nbytes), role, align, spans)
        self.ranges[name] = r
        self._cursor = r.end
        return r

    def fill(self) -> None:
        """allocates the arena and fills all of it with the seed's random bytes"""
        assert self.mem is None
        size = self._cursor + TAIL_GUARD
        raw = torch.empty(size + ROUND, dtype=torch.uint8, device=self.device)
        skip = -raw.data_ptr() % ROUND
        self._raw = raw
        self.mem = raw[skip:skip + size]
        words = np.random.default_rng(self.seed).integers(0, 1 << 63, (size + 7) // 8, dtype=np.int64)
        self.mem.copy_(torch.from_numpy(words.view(np.uint8)[:size]))

    def write(self, name: str, data) -> None:
        """copies a numpy array or CPU tensor into the front of a range, as bytes"""
        r = self.ranges[name]
        if isinstance(data, torch.Tensor):
            data = data.contiguous().view(-1).view(torch.uint8)
        else:
            data = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8))
        assert data.numel() <= r.nbytes, (name, data.numel(), r.nbytes)
        self.mem[r.start:r.start + data.numel()].copy_(data)

    def snapshot(self) -> None:
        self._snapshot = self.mem.clone()

    # ---------------------------------------------------------------------------------------------- handing to the library
    def ptr(self, name: str) -> int:
        return self.mem.data_ptr() + self.ranges[name].start

    def buffer(self, ctx, name: str, nbytes: int | None = None):
        """an engine.Buffer over the range, of exactly its bytes (or of `nbytes`, for the size refusals); None for a range not placed"""
        from vkradixsort_amd import engine

        if name not in self.ranges:
            return None
        size = self.ranges[name].nbytes if nbytes is None else nbytes
        b = engine.Buffer(ctx, engine.Buffer.BufferSettings(size, name), device_ptr=self.ptr(name))
        self._buffers.append(b)
        return b.handle

    def release(self) -> None:
        for b in self._buffers:
            b.release()
        self._buffers = []

    # ---------------------------------------------------------------------------------------------- checking
    def writable_mask(self):
        mask = torch.zeros(self.mem.numel(), dtype=torch.bool, device=self.device)
        for r in self.ranges.values():
            for b, e in r.writable:
                mask[r.start + b:r.start + e] = True
        return mask

    def check(self, nothing_writable: bool = False) -> None:
        """every byte of the arena outside the writable intervals equals the snapshot (nothing_writable: every byte of the arena)"""
        assert self._snapshot is not None, "snapshot() before the call"
        bad = self.mem != self._snapshot
        if not nothing_writable:
            bad &= ~self.writable_mask()
        count = int(bad.sum())
        if count == 0:
            return
        index = int(torch.argmax(bad.to(torch.uint8)))
        ordered = sorted(self.ranges.values(), key=lambda r: r.start)
        behind = [r for r in ordered if r.start <= index]
        ahead = [r for r in ordered if r.start > index]
        at, nxt = (behind[-1] if behind else None), (ahead[0] if ahead else None)
        lo = max(0, min(index - 4, self.mem.numel() - 16))
        before = bytes(self._snapshot[lo:lo + 16].cpu().tolist()).hex(" ")
        after = bytes(self.mem[lo:lo + 16].cpu().tolist()).hex(" ")
        if at is None:
            where = f"in the guard before the first range, {nxt.start - index} bytes before '{nxt.name}'"
        elif index < at.end:
            where = f"inside '{at.name}' ({at.role}, {at.nbytes} bytes) at byte {index - at.start}: {index - at.end} from its end"
        else:
            where = f"behind '{at.name}' ({at.role}, {at.nbytes} bytes): {index - at.end} bytes past its end"
            where += f", {nxt.start - index} before '{nxt.name}'" if nxt is not None else ", in the arena's tail guard"
        message = (f"case '{self.case}', layout {self.layout}, seed {self.seed}: {count} forbidden byte(s) changed; the first {where} "
                   f"(arena offset {index})\n  before [{lo}..{lo + 16}): {before}\n  after  [{lo}..{lo + 16}): {after}")
        raise ArenaViolation(message, at.name if at else None, index - at.end if at else None, nxt.name if nxt else None,
                             nxt.start - index if nxt else None, index, count)

    # ---------------------------------------------------------------------------------------------- reading
    def read(self, name: str, dtype, count: int | None = None) -> np.ndarray:
        """a range's contents on the CPU as `dtype` (whole elements only; the first `count` of them)"""
        r = self.ranges[name]
        item = np.dtype(dtype).itemsize
        n = r.nbytes // item if count is None else count
        assert n * item <= r.nbytes
        return self.mem[r.start:r.start + n * item].cpu().numpy().view(dtype).copy()

    def outputs(self) -> dict:
        """the bytes of every out / inout range's writable intervals, per range: what two runs under different poison must agree on"""
        got = {}
        for r in self.ranges.values():
            if r.role in ("out", "inout"):
                parts = [self.mem[r.start + b:r.start + e] for b, e in r.writable]
                got[r.name] = torch.cat(parts).cpu().numpy().tobytes() if parts else b""
        return got
