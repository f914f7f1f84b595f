"""The arena's checker must not be vacuous: one planted byte at every kind of forbidden place fails check() and is named rightly, writes
the contract allows pass, and the tight layout really sits off the next alignment.  Runs on the CPU; the arena itself needs no GPU."""
import numpy as np
import pytest

from ._arena import GUARD, LAYOUTS, ROUND, TAIL_GUARD, Arena, ArenaViolation, tight_start

torch = pytest.importorskip("torch")

IN_BYTES, OUT_BYTES, SCRATCH_BYTES = 4 * 37, 8 * 21 + 3, 1037  # none a multiple of 16
OUT_WRITABLE = [(0, 8 * 5), (8 * 9, 8 * 13)]                  # two intervals with a forbidden stretch between and behind


def make(layout, seed=1):
    a = Arena("cpu", seed, layout, case="cpu-selftest")
    a.place("src", IN_BYTES, "in", 4)
    a.place("out", OUT_BYTES, "out", 8, writable=OUT_WRITABLE)
    a.place("scratch", SCRATCH_BYTES, "scratch", 16)
    a.fill()
    a.write("src", np.arange(37, dtype=np.uint32))
    a.snapshot()
    return a


def flip(a, index):
    a.mem[index] = a.mem[index] ^ 0x40


def failure(a):
    with pytest.raises(ArenaViolation) as info:
        a.check()
    return info.value


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_untouched_arena_and_allowed_writes_pass(layout):
    a = make(layout)
    a.check()
    a.check(nothing_writable=True)
    out, scratch = a.ranges["out"], a.ranges["scratch"]
    for b, e in OUT_WRITABLE:
        a.mem[out.start + b:out.start + e] ^= 0xFF  # every writable byte, the first and the last of each interval included
    a.mem[scratch.start:scratch.end] ^= 0xFF
    a.check()
    with pytest.raises(ArenaViolation):  # a refusal must leave those alone too
        a.check(nothing_writable=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["src", "out", "scratch"])
def test_the_last_guard_byte_before_a_range(layout, name):
    a = make(layout)
    r = a.ranges[name]
    flip(a, r.start - 1)
    e = failure(a)
    assert e.count == 1 and e.index == r.start - 1 and e.next_name == name and e.before_next == 1
    previous = {"src": None, "out": "src", "scratch": "out"}[name]
    assert e.range_name == previous
    if previous is not None:
        assert e.offset_from_end == r.start - 1 - a.ranges[previous].end >= GUARD - 1
        assert f"behind '{previous}'" in str(e) and f"1 before '{name}'" in str(e)
    else:
        assert "before the first range" in str(e) and "1 bytes before 'src'" in str(e)
    assert "cpu-selftest" in str(e) and layout in str(e)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["src", "out", "scratch"])
def test_the_first_guard_byte_after_a_range(layout, name):
    a = make(layout)
    flip(a, a.ranges[name].end)
    e = failure(a)
    assert e.count == 1 and e.range_name == name and e.offset_from_end == 0
    assert f"behind '{name}'" in str(e) and "0 bytes past its end" in str(e)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("at", [0, IN_BYTES // 2, IN_BYTES - 1])
def test_an_input_byte(layout, at):
    a = make(layout)
    flip(a, a.ranges["src"].start + at)
    e = failure(a)
    assert e.count == 1 and e.range_name == "src" and e.offset_from_end == at - IN_BYTES
    assert f"inside 'src' (in, {IN_BYTES} bytes) at byte {at}" in str(e)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("at", [OUT_WRITABLE[0][1], OUT_WRITABLE[1][0] - 1, OUT_WRITABLE[1][1], OUT_BYTES - 1])
def test_an_output_byte_just_outside_its_writable_intervals(layout, at):
    a = make(layout)
    flip(a, a.ranges["out"].start + at)
    e = failure(a)
    assert e.count == 1 and e.range_name == "out" and e.offset_from_end == at - OUT_BYTES
    assert f"inside 'out' (out, {OUT_BYTES} bytes) at byte {at}" in str(e)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_arenas_last_byte(layout):
    a = make(layout)
    last = a.mem.numel() - 1
    flip(a, last)
    e = failure(a)
    assert e.count == 1 and e.index == last and e.range_name == "scratch" and e.next_name is None
    assert e.offset_from_end == last - a.ranges["scratch"].end >= TAIL_GUARD - 1
    assert "tail guard" in str(e)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_message_counts_every_byte_and_shows_before_and_after(layout):
    a = make(layout)
    r = a.ranges["out"]
    a.mem[r.end:r.end + 5] = 0  # a kernel that stores zeros cannot match random poison for long
    want = int((a._snapshot[r.end:r.end + 5] != 0).sum())
    e = failure(a)
    assert e.count == want and "before [" in str(e) and "after  [" in str(e)
    lines = str(e).splitlines()
    assert len(lines[1].split(": ")[1].split()) == 16 and len(lines[2].split(": ")[1].split()) == 16 and lines[1] != lines[2]


def test_two_seeds_poison_differently_and_one_seed_repeats():
    a, b, c = make("round", 1), make("round", 2), make("round", 1)
    assert torch.equal(a.mem, c.mem) and not torch.equal(a.mem, b.mem)
    for name in ("out", "scratch"):
        assert not np.array_equal(a.read(name, np.uint8), b.read(name, np.uint8))
    assert np.array_equal(a.read("src", np.uint32), np.arange(37, dtype=np.uint32))  # the inputs are the same under both
    assert np.array_equal(b.read("src", np.uint32), np.arange(37, dtype=np.uint32))
    # no constant canary: the poison holds many byte values
    assert len(np.unique(a.read("scratch", np.uint8))) > 200


def test_layouts_guards_and_alignment():
    for align in (1, 2, 4, 8, 16):
        for cursor in range(0, 200):
            s = tight_start(cursor, align)
            assert cursor <= s < cursor + 2 * align and s % align == 0 and s % (2 * align) != 0
    for layout in LAYOUTS:
        a = Arena("cpu", 3, layout)
        for i, align in enumerate((4, 8, 16, 4, 1, 2, 16, 8)):
            a.place(f"r{i}", 1 + 13 * i, "scratch", align)
        a.fill()
        assert a.mem.data_ptr() % ROUND == 0
        end = 0
        for r in a.ranges.values():
            assert r.start - end >= GUARD
            address = a.ptr(r.name)
            if layout == "round":
                assert address % ROUND == 0
            else:  # on the demanded alignment and off the next one
                assert address % r.align == 0 and address % (2 * r.align) == r.align, (r.name, r.align, address)
            end = r.end
        assert a.mem.numel() - end >= TAIL_GUARD


def test_read_and_outputs():
    a = make("tight")
    r = a.ranges["out"]
    a.mem[r.start:r.start + 16] = torch.arange(16, dtype=torch.uint8)
    assert a.read("out", np.uint64, 2).tolist() == [0x0706050403020100, 0x0F0E0D0C0B0A0908]
    assert a.read("out", np.uint64).size == OUT_BYTES // 8
    got = a.outputs()
    assert set(got) == {"out"} and len(got["out"]) == sum(e - b for b, e in OUT_WRITABLE) and got["out"][:16] == bytes(range(16))


def test_place_refuses_what_makes_no_sense():
    a = Arena("cpu", 1, "round")
    with pytest.raises(AssertionError):
        a.place("o", 16, "out", 4)  # an output says what may change
    with pytest.raises(AssertionError):
        a.place("o", 16, "out", 4, writable=[(0, 17)])
    with pytest.raises(AssertionError):
        a.place("i", 16, "in", 4, writable=[(0, 4)])
    a.place("i", 16, "in", 4)
    with pytest.raises(AssertionError):
        a.place("i", 16, "in", 4)
