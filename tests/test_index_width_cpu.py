"""Index width near 2^32 elements, without a device.

Every entry point takes uint32_t num_elements (fewer than 2^32 elements).  Two patterns break there: a uint32 loop `i += step` against a
bound that can exceed 2^32 - step (i + step wraps to a small value still below the bound: the loop never ends), and a uint32
`(x + C - 1) / C` where x can exceed 2^32 - C (it wraps to a tiny count).  A source lint keeps both out of the kernels, and the pure
host functions (tier classification, scratch sizes, the sort-form decision) are checked at the edges 2^31 - 1, 2^31, 2^32 - 2^21 + 1
and 2^32 - 1.
"""
import ctypes
import re
from pathlib import Path

import pytest

from vkradixsort_amd import capi

CSRC = Path(__file__).resolve().parent.parent / "vkradixsort_amd" / "csrc"
SOURCES = sorted(p for pat in ("*.hip", "*.hpp", "*.h") for p in CSRC.glob(pat))
EDGES = [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2 ** 21 + 1, 2 ** 32 - 1]
WIDE_TYPES = ("size_t", "uint64_t", "int64_t", "unsigned long long", "long long")


# ---------------------------------------------------------------------------------------------- the lint

def _strip_comments(text):
    """The source with // and /* */ comments blanked (newlines kept, so offsets still give line numbers)."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)


def _for_headers(text):
    """(offset, init, condition, step) of every `for (init; condition; step)` (the header may span lines and nest parentheses)."""
    for m in re.finditer(r"\bfor\s*\(", text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        parts = text[m.end():i - 1].split(";")
        if len(parts) == 3:  # (a range-based for has none)
            yield m.start(), *(p.strip() for p in parts)


def _from_grid(text, name, at):
    """Whether the nearest declaration of `name` before offset `at` (a variable or a parameter) initialises it from gridDim."""
    decls = list(re.finditer(rf"\b[\w:>]+\s+{name}\s*([=,)])", text[:at]))
    if not decls or decls[-1].group(1) != "=":
        return False
    return re.search(r"\bgridDim\b", re.match(r"[^;,]*", text[decls[-1].end():]).group(0)) is not None


def _wide(init):
    return any(re.match(rf"(const\s+)?{re.escape(t)}\s+\w+\s*=", init) for t in WIDE_TYPES)


def grid_stride_loops(text):
    """(line, header, wide) of every for loop whose step involves gridDim; wide: its induction variable is declared 64-bit."""
    text = _strip_comments(text)
    out = []
    for at, init, cond, step in _for_headers(text):
        if re.search(r"\bgridDim\b", step) or any(_from_grid(text, n, at) for n in re.findall(r"\b[A-Za-z_]\w*\b", step)):
            out.append((text.count("\n", 0, at) + 1, f"for ({init}; {cond}; {step})", _wide(init)))
    return out


def test_lint_recognises_both_forms():
    src = """
    __global__ void k(uint32_t *p, uint32_t n) {
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) p[i] = 0;  // wraps
        for (size_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) p[i] = 0;
        const size_t stride = static_cast<size_t>(gridDim.x) * 256u;
        for (unsigned i = threadIdx.x; i < n;
             i += stride) p[i] = 0;
        for (uint64_t i = threadIdx.x; i < n; i += stride) p[i] = 0;
        for (uint32_t c = threadIdx.x; c < 256u; c += blockDim.x) p[c] = 0;  // (not a grid stride)
        for (const auto &x : v) (void)x;
    }
    __device__ uint32_t sum(const uint32_t *p, uint32_t r1, uint32_t stride) {  // (another function's `stride`: a parameter)
        for (uint32_t r = 0; r < r1; r += 4 * stride) p[r];
    }"""
    loops = grid_stride_loops(src)
    assert [(line, wide) for line, _, wide in loops] == [(3, False), (4, True), (6, False), (8, True)]


def test_every_grid_stride_loop_counts_in_64_bits():
    """A grid-stride loop's i + gridDim.x * blockDim.x passes 2^32 - 1 for a bound within one stride of 2^32 (grids of 8192 blocks of
    256 threads: 2^32 - 2^21) and wraps to a small value that is still below the bound: the kernel never ends.  Every such loop in the
    kernels counts in 64 bits (verify_keys_kernel's form), whatever its bound."""
    seen, narrow = 0, []
    for path in SOURCES:
        for line, header, wide in grid_stride_loops(path.read_text()):
            seen += 1
            if not wide:
                narrow.append(f"{path.name}:{line}: {header}")
    assert not narrow, "32-bit grid-stride loops:\n" + "\n".join(narrow)
    assert seen >= 14, f"the lint found only {seen} grid-stride loops: has it stopped matching them?"


def _body(text, name):
    """The body of the function named `name` (its definition: `void name(` ... the matching brace)."""
    m = re.search(rf"\bvoid\s+{name}\s*\(", text)
    assert m, name
    i = text.index("{", m.end())
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[i:j]


# loops over one segment's keys (up to 2^32 - 1 of them) by a fixed step, and the grid tier's tile count
@pytest.mark.parametrize("source,function,step", [
    ("vrs_segmented.hip", "segmented_global_sort_kernel", "THREADS"),
    ("vrs_segmented.hip", "segmented_global_sort_kernel", "TILE"),
    ("vrs_topk.hip", "topk_workgroup_kernel", "TILE"),
    ("vrs_topk.hip", "fill_tail", "threads"),
])
def test_segment_length_loops_count_in_64_bits(source, function, step):
    body = _strip_comments(_body((CSRC / source).read_text(), function))
    loops = [(init, cond) for _, init, cond, st in _for_headers(body) if re.fullmatch(rf"\w+\s*\+=\s*{step}", st)]
    assert loops, f"no `+= {step}` loop in {function}"
    for init, cond in loops:
        assert _wide(init), f"{function}: for ({init}; {cond}; ... += {step}) counts in 32 bits"


def test_topk_tile_count_is_64_bit():
    """A grid-tier segment of len > 2^32 - 16384 keys: (len + 16383) / 16384 in uint32 is 0 tiles (the selection walks nothing)."""
    body = _strip_comments(_body((CSRC / "vrs_topk.hip").read_text(), "topk_classify_kernel"))
    m = re.search(r"\btiles\s*=\s*([^;]*kTopkTile[^;]*);", body)
    assert m and re.search(r"static_cast<(uint64_t|size_t)>\(len\)", m.group(1)), m and m.group(1)


# ---------------------------------------------------------------------------------------------- host functions at the edges

@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _tier(fn, *args):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert fn(*args, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
    return t.value, cb.value, ce.value


def _ranges(n):
    """(begin, end) pairs around and past 2^31 and up to 2^32 - 1, for num_elements n."""
    out = []
    for b in (0, 2 ** 31 - 5, 2 ** 31, 2 ** 31 + 7, 2 ** 32 - 2 ** 21 + 1, 2 ** 32 - 9000, 2 ** 32 - 2):
        for e in (b + 1, b + 1789, b + 1790, b + 13313, b + 14334, b + 2 ** 20, b + 2 ** 30 + 17, 2 ** 32 - 1, b - 1):
            if 0 <= e < 2 ** 32:
                out.append((b, e))
    return out


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("n", EDGES)
def test_segment_tier_for_past_2_31(lib, n, wide):
    fn = lib.vrs_segment_tier_for_u64 if wide else lib.vrs_segment_tier_for
    for pairs in (0, 1):
        wave = capi.SEGMENT_WAVE_MAX_U64 if wide else capi.SEGMENT_WAVE_MAX
        block = ((capi.SEGMENT_BLOCK_MAX_PAIRS_U64 if pairs else capi.SEGMENT_BLOCK_MAX_KEYS_U64) if wide
                 else (capi.SEGMENT_BLOCK_MAX_PAIRS if pairs else capi.SEGMENT_BLOCK_MAX_KEYS))
        for min_keys in (0, 1 << 20, 2 ** 31):
            for b, e in _ranges(n):
                cb, ce = min(b, n), min(max(b, e), n)
                length = ce - cb
                want = (capi.VRS_SEGMENT_WAVE if length <= wave else capi.VRS_SEGMENT_BLOCK if length <= block
                        else capi.VRS_SEGMENT_ONE_CALL if min_keys and length >= min_keys else capi.VRS_SEGMENT_GLOBAL)
                assert _tier(fn, b, e, n, pairs, min_keys) == (want, cb, ce), (b, e, n, pairs, min_keys)


@pytest.mark.parametrize("n", EDGES)
def test_topk_tier_for_past_2_31(lib, n):
    for grid_min in (0, capi.TOPK_GRID_MIN_KEYS_DEFAULT, 2 ** 31):
        for b, e in _ranges(n) + [(0, n), (0, 2 ** 32 - 1)]:
            cb, ce = min(b, n), min(max(b, e), n)
            length = ce - cb
            want = (capi.VRS_TOPK_LDS if length <= capi.TOPK_LDS_MAX else capi.VRS_TOPK_GRID if grid_min and length >= grid_min
                    else capi.VRS_TOPK_BLOCK)
            assert _tier(lib.vrs_topk_tier_for, b, e, n, grid_min) == (want, cb, ce), (b, e, n, grid_min)


def _bytes(fn, *args):
    out = ctypes.c_uint64()
    rc = fn(*args, ctypes.byref(out))
    return rc, out.value


def _status_bytes(n):  # the encode's tile ticket and one 8-byte look-back word per 4096-key tile
    return 16 + 8 * -(-n // capi.RLE_TILE)


@pytest.mark.parametrize("n", EDGES)
def test_rle_scratch_bytes_at_the_edges(lib, n):
    for key_bytes in (4, 8):
        for flags in (0, capi.VRS_RLE_COUNTS):
            rc, got = _bytes(lib.vrs_run_length_encode_scratch_bytes, n, key_bytes, flags)
            assert rc == capi.VRS_OK
            need = _status_bytes(n) + (4 * (n + 1) if flags else 0)  # (counts without offsets: the n + 1 offsets in scratch)
            assert need <= got < need + 4096, (n, key_bytes, flags, got)


@pytest.mark.parametrize("n", EDGES)
def test_unique_scratch_bytes_at_the_edges(lib, n):
    for key_type, kb in ((capi.VRS_UNIQUE_U32, 4), (capi.VRS_UNIQUE_F32, 4), (capi.VRS_UNIQUE_U64, 8), (capi.VRS_UNIQUE_I64, 8)):
        for inverse in (0, capi.VRS_UNIQUE_INVERSE):
            for counts in (0, capi.VRS_UNIQUE_COUNTS):
                rc, got = _bytes(lib.vrs_unique_scratch_bytes, n, key_type, inverse | counts)
                assert rc == capi.VRS_OK
                # the status block, the mapped keys and their sort partner, (inverse) the iota payloads and partner, (counts) offsets
                need = _status_bytes(n) + 2 * kb * n + (2 * 4 * n if inverse else 0) + (4 * (n + 1) if counts else 0)
                assert need <= got < need + 4096, (n, key_type, inverse, counts, got)


@pytest.mark.parametrize("n,S,k", [
    (2 ** 32 - 1, 1, 1000),                        # one segment of 2^32 - 1 keys: its tiles' counts
    (2 ** 32 - 1, 1048000, 4097),                  # S * k = 4.2937e9, just below 2^32: the sort area
    (2 ** 32 - 1, 1, 2 ** 32 - 1),                 # k = 2^32 - 1
    (2 ** 31, 2 ** 16, 2 ** 16 - 1),               # S * k = 2^32 - 2^16
    (2 ** 32 - 2 ** 21 + 1, 4096 + 7, 5000),       # more segments than grid slots
    (2 ** 31 - 1, 2 ** 31 - 1, 2),                 # S * k = 2^32 - 2
])
def test_topk_scratch_bytes_at_the_edges(lib, n, S, k):
    assert S * k < 2 ** 32
    for flags in (0, capi.VRS_TOPK_SORTED, capi.VRS_TOPK_SORTED | capi.VRS_TOPK_LARGEST):
        rc, got = _bytes(lib.vrs_topk_scratch_bytes, n, S, k, flags)
        assert rc == capi.VRS_OK
        slots = min(S, n // (capi.TOPK_LDS_MAX + 1), 4096)  # grid-tier segments (64-byte slot, 2048-bin histogram each)
        tiles = n // 16384 + slots if slots else 0        # their 16384-key tiles (8 bytes of counts each)
        need = 16 + 64 * slots + 2048 * 4 * slots + 8 * tiles
        if flags & capi.VRS_TOPK_SORTED and k > capi.TOPK_SORT_IN_LDS_MAX_K:
            need += 16 * S * k  # keys, keys_tmp, values, values_tmp of S * k entries for the segmented sort
        else:
            need += 4 * S  # the tiers' segment list
        assert need <= got < need + 5 * 256, (n, S, k, flags, got)  # (each area rounded up to 256 bytes)


@pytest.mark.parametrize("S,k", [(2 ** 16, 2 ** 16), (2, 2 ** 31), (2 ** 32 - 1, 2), (1048576, 4096)])
def test_topk_scratch_bytes_refuses_2_32_slots(lib, S, k):
    """S * k >= 2^32: refused (the result would not fit the uint32 slot indices), never sized modulo 2^32."""
    assert S * k >= 2 ** 32
    rc, _ = _bytes(lib.vrs_topk_scratch_bytes, 2 ** 32 - 1, S, k, capi.VRS_TOPK_SORTED)
    assert rc == capi.VRS_ERROR_INVALID_ARGUMENT


def _form(lib, n, key_bytes, pairs):
    form = ctypes.c_int(-1)
    assert lib.vrs_sort_form_for(n, key_bytes, pairs, None, 0, ctypes.byref(form), None) == capi.VRS_OK
    return capi.FORM_NAMES[form.value]


@pytest.mark.parametrize("key_bytes,pairs", [(4, 0), (4, 1), (8, 0), (8, 1)], ids=["u32", "u32_pairs", "u64", "u64_pairs"])
def test_sort_form_from_2_30_on_is_contract(lib, key_bytes, pairs):
    """From 2^30 keys on (the look-back words carry 28-bit stream counts) every one-call sort takes the contract stages: the form
    tests/test_gpu_max_sizes.py runs with payloads and 64-bit keys."""
    for n in (2 ** 30, 2 ** 31 + 12345, 2 ** 32 - 2 ** 21 + 1, 2 ** 32 - 1):
        assert _form(lib, n, key_bytes, pairs) == "contract", n
    assert _form(lib, 2 ** 30 - 1, key_bytes, pairs) != "contract"
