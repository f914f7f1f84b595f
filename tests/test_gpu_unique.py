"""Run-length encoding and unique on the device (vrs_run_length_encode, vrs_unique, vkradixsort_amd.unique), every result compared with
numpy: the runs of the bit patterns for the encode, np.unique of the rank-mapped bit patterns for unique, and torch.unique /
torch.unique_consecutive at the torch level."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

uq = importlib.import_module("vkradixsort_amd.unique")

pytestmark = pytest.mark.gpu

TILE = capi.RLE_TILE
SENTINEL = 0xA5
PAD = 64  # entries past n (n + 1) of every output buffer that must stay untouched


@pytest.fixture(scope="module")
def ctx():
    c = vrs.GPUContext(0)
    c.init()
    yield c
    c.shutdown()


def upload(c, arr):
    arr = np.ascontiguousarray(arr)
    return vrs.Buffer.fillDeviceWithStagingBuffer(c, vrs.Buffer.BufferSettings(max(arr.nbytes, 4)), arr if arr.nbytes else np.zeros(1, np.uint32))


def download(buf, dtype, count):
    out = np.empty(max(buf.getSizeBytes() // np.dtype(dtype).itemsize, 1), dtype)
    buf.downloadWithStagingBuffer(out)
    return out[:count]


def sentinel_buffer(c, dtype, entries):
    return upload(c, np.full((entries + PAD) * np.dtype(dtype).itemsize, SENTINEL, np.uint8))


def garbage_scratch(c, nbytes, seed):
    return upload(c, np.random.default_rng(seed).integers(0, 256, max(nbytes, 4), dtype=np.uint8))


def ref_runs(a):
    """(keys, offsets incl. n, counts, run ids) of the runs of bit-identical consecutive entries"""
    n = a.size
    if n == 0:
        return a[:0], np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)  # n == 0: not even offsets[0]
    heads = np.empty(n, bool)
    heads[0] = True
    heads[1:] = a[1:] != a[:-1]
    starts = np.flatnonzero(heads)
    offsets = np.append(starts, n).astype(np.uint32)
    return a[starts], offsets, np.diff(offsets).astype(np.uint32), (np.cumsum(heads) - 1).astype(np.uint32)


# ---- encode ----------------------------------------------------------------------------------------------------------------------------

def rle_input(kind, n, width, seed):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        v = np.full(n, 0x9E3779B9, np.uint64)
    elif kind == "distinct":
        v = np.arange(n, dtype=np.uint64) * np.uint64(2654435761)
    elif kind == "few":
        v = rng.integers(0, 3, n).astype(np.uint64)
    elif kind == "loguniform":  # run lengths log-uniform in [1, 10^6]: runs that span many tiles
        lengths = np.exp(rng.uniform(0, np.log(1e6), n // 1000 + 8)).astype(np.int64) + 1
        lengths = lengths[:np.searchsorted(np.cumsum(lengths), n) + 1]  # just enough runs to cover n
        v = np.repeat(np.arange(lengths.size, dtype=np.uint64) % np.uint64(5), lengths)[:n]
        if v.size < n:
            v = np.concatenate([v, np.full(n - v.size, 7, np.uint64)])
    elif kind == "tile_edges":  # runs ending at multiples of the tile, one before and one after
        cuts = sorted({t * TILE + d for t in range(1, n // TILE + 2) for d in (-1, 0, 1) if 0 < t * TILE + d < n})
        heads = np.zeros(n, np.uint64)
        heads[cuts] = 1
        v = np.cumsum(heads) % np.uint64(2)
    else:
        raise ValueError(kind)
    if width == 8:  # runs that differ only in the high word, and a low word that is the same everywhere
        return (v << np.uint64(32)) | np.uint64(0x01234567)
    return (v * np.uint64(0x10001) + np.uint64(0x80000000)).astype(np.uint32)


def run_rle(c, a, outputs, seed=0):
    """vrs_run_length_encode of `a` with the outputs named in `outputs` (a subset of keys/offsets/counts/run_ids); checks the
    sentinels past R (R + 1) and n (n + 1), the input, and returns (R, {name: array})"""
    n, width = a.size, a.dtype.itemsize
    kb = upload(c, a)
    bufs = {"keys": sentinel_buffer(c, a.dtype, n) if "keys" in outputs else None,
            "offsets": sentinel_buffer(c, np.uint32, n + 1) if "offsets" in outputs else None,
            "counts": sentinel_buffer(c, np.uint32, n) if "counts" in outputs else None,
            "run_ids": sentinel_buffer(c, np.uint32, n) if "run_ids" in outputs else None}
    runs = upload(c, np.full(1, 0xDEADBEEF, np.uint32))
    need = uq.rle_scratch_bytes(n, width, counts="counts" in outputs and "offsets" not in outputs)
    scr = garbage_scratch(c, need, seed)
    uq.run_length_encode(c, kb, n, runs, scr, width, out_keys=bufs["keys"], out_offsets=bufs["offsets"], out_counts=bufs["counts"],
                         out_run_ids=bufs["run_ids"])
    R = int(download(runs, np.uint32, 1)[0])
    got = {}
    for name, b in bufs.items():
        if b is None:
            continue
        dt = a.dtype if name == "keys" else np.dtype(np.uint32)
        whole = download(b, dt, b.getSizeBytes() // dt.itemsize)
        live = {"keys": R, "offsets": R + 1 if n else 0, "counts": R, "run_ids": n}[name]
        tail = whole[live:].view(np.uint8)
        assert np.all(tail == SENTINEL), f"{name} written past {live} entries"
        got[name] = whole[:live]
        b.release()
    if n:
        assert np.array_equal(download(kb, a.dtype, n), a), "the input was written"
    for b in (kb, runs, scr):
        b.release()
    return R, got


def check_rle(c, a, outputs, seed=0):
    R, got = run_rle(c, a, outputs, seed)
    keys, offsets, counts, ids = ref_runs(a)
    assert R == keys.size
    ref = {"keys": keys, "offsets": offsets, "counts": counts, "run_ids": ids}
    for name, v in got.items():
        assert np.array_equal(v, ref[name]), f"{name} differs at {np.flatnonzero(v != ref[name])[:8]}"


ALL = ("keys", "offsets", "counts", "run_ids")
COMBOS = [set(s) for r in range(len(ALL) + 1) for s in itertools.combinations(ALL, r)]
KINDS = ["equal", "distinct", "few", "loguniform", "tile_edges"]


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("n", [0, 1, 2, TILE - 1, TILE, TILE + 1, 10 ** 6 + 3])
@pytest.mark.parametrize("kind", KINDS)
def test_encode_every_output_combination(ctx, width, n, kind):
    a = rle_input(kind, n, width, n)
    for i, outputs in enumerate(COMBOS):
        check_rle(ctx, a, outputs, seed=i)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_encode_large(ctx, width, kind):
    n = (1 << 24) + 5
    a = rle_input(kind, n, width, 7)
    check_rle(ctx, a, set(ALL), seed=1)
    check_rle(ctx, a, {"counts"}, seed=2)  # the offsets in the scratch


def test_encode_with_no_elements_writes_only_the_count(ctx):
    runs = upload(ctx, np.full(1, 0xDEADBEEF, np.uint32))
    out = sentinel_buffer(ctx, np.uint32, 1)
    scr = garbage_scratch(ctx, 4, 0)
    keys = upload(ctx, np.zeros(1, np.uint32))
    uq.run_length_encode(ctx, keys, 0, runs, scr, 4, out_keys=out, out_offsets=out, out_counts=out, out_run_ids=out)
    assert download(runs, np.uint32, 1)[0] == 0
    assert np.all(download(out, np.uint8, out.getSizeBytes()) == SENTINEL)
    for b in (runs, out, scr, keys):
        b.release()


def test_encode_refuses_undersized_buffers(ctx):
    n = 1000
    keys = upload(ctx, np.zeros(n, np.uint32))
    runs = upload(ctx, np.zeros(1, np.uint32))
    small = upload(ctx, np.zeros(n - 1, np.uint32))
    scr = upload(ctx, np.zeros(uq.rle_scratch_bytes(n, 4), np.uint8))
    lib = ctx.lib
    for args in ((small, None, None, None), (None, small, None, None), (None, None, small, None), (None, None, None, small)):
        h = [b.handle if b is not None else None for b in args]
        assert lib.vrs_run_length_encode(ctx.handle, keys.handle, n, 4, *h, runs.handle, scr.handle) == capi.VRS_ERROR_INVALID_ARGUMENT
    full = upload(ctx, np.zeros(n, np.uint32))  # counts without offsets: the scratch must hold the offsets too
    assert lib.vrs_run_length_encode(ctx.handle, keys.handle, n, 4, None, None, full.handle, None, runs.handle, scr.handle) == \
        capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_run_length_encode(ctx.handle, keys.handle, n, 8, None, None, None, None, runs.handle, scr.handle) == \
        capi.VRS_ERROR_INVALID_ARGUMENT  # 8-byte keys: `keys` is too small
    assert lib.vrs_run_length_encode(ctx.handle, keys.handle, n, 4, None, None, None, None, None, scr.handle) == \
        capi.VRS_ERROR_INVALID_ARGUMENT
    for b in (keys, runs, small, scr, full):
        b.release()


# ---- unique ----------------------------------------------------------------------------------------------------------------------------

KT = {"u32": capi.VRS_UNIQUE_U32, "i32": capi.VRS_UNIQUE_I32, "f32": capi.VRS_UNIQUE_F32,
      "u64": capi.VRS_UNIQUE_U64, "i64": capi.VRS_UNIQUE_I64, "f64": capi.VRS_UNIQUE_F64}


def rank(bits, kt):
    if bits.dtype == np.uint32:
        top = np.uint32(1 << 31)
        if kt == "i32":
            return bits ^ top
        if kt == "f32":
            return bits ^ np.where(bits & top, np.uint32(0xFFFFFFFF), top).astype(np.uint32)
        return bits
    top = np.uint64(1 << 63)
    if kt == "i64":
        return bits ^ top
    if kt == "f64":
        return bits ^ np.where(bits & top, np.uint64(0xFFFFFFFFFFFFFFFF), top).astype(np.uint64)
    return bits


def unique_input(kt, n, distinct, seed):
    rng = np.random.default_rng(seed)
    wide = kt.endswith("64")
    dt = np.uint64 if wide else np.uint32
    pool = rng.integers(0, 1 << 63, max(distinct, 1), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, max(distinct, 1), dtype=np.uint64)
    if kt == "f32":
        specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x3F800000],
                            np.uint64)
        pool = np.concatenate([rng.standard_normal(max(distinct, 1)).astype(np.float32).view(np.uint32).astype(np.uint64), specials])
    elif kt == "f64":
        specials = np.array([0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF8000000000001,
                             0xFFF8000000000000, 0x7FF0000000000001], np.uint64)
        pool = np.concatenate([rng.standard_normal(max(distinct, 1)).view(np.uint64), specials])
    return pool[rng.integers(0, pool.size, n)].astype(dt)


def run_unique(c, bits, kt, inverse=True, counts=True, seed=0):
    n = bits.size
    kb = upload(c, bits)
    ok = sentinel_buffer(c, bits.dtype, n)
    oc = sentinel_buffer(c, np.uint32, n) if counts else None
    oi = sentinel_buffer(c, np.uint32, n) if inverse else None
    runs = upload(c, np.full(1, 0xDEADBEEF, np.uint32))
    scr = garbage_scratch(c, uq.unique_scratch_bytes(n, kt, inverse, counts), seed)
    uq.unique_keys(c, kb, n, ok, runs, scr, key_type=kt, out_counts=oc, out_inverse=oi)
    R = int(download(runs, np.uint32, 1)[0])
    out = {}
    for name, b, live in (("keys", ok, R), ("counts", oc, R), ("inverse", oi, n)):
        if b is None:
            continue
        dt = bits.dtype if name == "keys" else np.dtype(np.uint32)
        whole = download(b, dt, b.getSizeBytes() // dt.itemsize)
        assert np.all(whole[live:].view(np.uint8) == SENTINEL), f"{name} written past {live} entries"
        out[name] = whole[:live]
        b.release()
    if n:
        assert np.array_equal(download(kb, bits.dtype, n), bits), "the input was written"
    for b in (kb, runs, scr):
        b.release()
    return R, out


def check_unique(c, bits, kt, inverse=True, counts=True, seed=0):
    R, got = run_unique(c, bits, kt, inverse, counts, seed)
    r = rank(bits, kt)
    u, first, inv, cnt = np.unique(r, return_index=True, return_inverse=True, return_counts=True)
    assert R == u.size
    assert np.array_equal(got["keys"], bits[first]), "keys differ"
    if counts:
        assert np.array_equal(got["counts"], cnt.astype(np.uint32)), "counts differ"
    if inverse:
        assert np.array_equal(got["inverse"], inv.reshape(-1).astype(np.uint32)), "inverse differs"


@pytest.mark.parametrize("kt", list(KT))
@pytest.mark.parametrize("n,distinct", [(1, 1), (2, 2), (777, 5), (TILE + 1, 100), (100000, 100000), (300001, 1 << 16)])
def test_unique_every_key_type(ctx, kt, n, distinct):
    bits = unique_input(kt, n, distinct, n + distinct)
    for inverse, counts in itertools.product((True, False), repeat=2):
        check_unique(ctx, bits, kt, inverse, counts, seed=int(inverse) + 2 * int(counts))


def test_unique_with_no_elements(ctx):
    R, got = run_unique(ctx, np.zeros(0, np.uint32), "u32")
    assert R == 0 and all(v.size == 0 for v in got.values())


def sort_form(ctx, n, key_bytes, pairs):
    form = ctypes.c_int()
    assert ctx.lib.vrs_sort_form_for(n, key_bytes, int(pairs), None, 0, ctypes.byref(form), None) == 0
    return capi.FORM_NAMES[form.value]


# (n, key type, with the inverse = the pairs sort) -> the inner sort's form on a fresh context
FORMS = [(3000, "u32", False, "single"), (5000, "i32", False, "contract"), (100000, "f32", False, "lsd"), (9000, "u32", True, "lsd"),
         (300000, "i64", True, "lsd"), ((1 << 22) + 11, "u32", False, "pool"), (26000000, "i32", True, "pool"),
         (21000000, "u64", False, "counted")]


@pytest.mark.parametrize("n,kt,inverse,form", FORMS)
def test_unique_through_every_inner_sort_form(n, kt, inverse, form):
    with vrs.GPUContext(0) as c:  # a fresh context: the defaults vrs_sort_form_for assumes
        assert sort_form(c, n, 8 if kt.endswith("64") else 4, inverse) == form
        bits = unique_input(kt, n, n // 3 + 1, n)
        check_unique(c, bits, kt, inverse=inverse, counts=True)


def test_unique_1e8_all_distinct(ctx):
    n = 10 ** 8
    keys = np.random.default_rng(1).permutation(n).astype(np.uint32)
    R, got = run_unique(ctx, keys, "u32")
    assert R == n
    assert np.array_equal(got["keys"], np.arange(n, dtype=np.uint32))
    assert np.all(got["counts"] == 1)
    assert np.array_equal(got["inverse"], keys)  # a permutation of 0 .. n-1 is its own rank


def test_unique_1e8_about_1e6_distinct(ctx):
    n = 10 ** 8
    v = np.random.default_rng(2).integers(0, 1 << 20, n).astype(np.uint32)
    keys = v * np.uint32(4095) + np.uint32(12345)  # spread over the key range, still ascending in v
    R, got = run_unique(ctx, keys, "u32")
    hist = np.bincount(v, minlength=1 << 20)
    present = np.flatnonzero(hist)
    assert R == present.size
    assert np.array_equal(got["keys"], present.astype(np.uint32) * np.uint32(4095) + np.uint32(12345))
    assert np.array_equal(got["counts"], hist[present].astype(np.uint32))
    lut = (np.cumsum(hist > 0) - 1).astype(np.uint32)
    assert np.array_equal(got["inverse"], lut[v])


# ---- torch -----------------------------------------------------------------------------------------------------------------------------

torch = pytest.importorskip("torch")
DTYPES = [torch.int32, torch.int64, torch.float32, torch.float64]
SHAPES = [(1000,), (33, 257), (4, 5, 6001), (0,), (3, 0, 2)]


def torch_input(dtype, shape, distinct, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randint(0, distinct, shape, device="cuda", generator=g)
    if dtype.is_floating_point:
        return (v.to(dtype) - distinct / 2) * 0.25 + 0.125  # no NaN, no -0.0
    return (v - distinct // 2).to(dtype) * 977


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("distinct", [7, 5000])
def test_torch_unique_equals_torch(dtype, shape, distinct):
    x = torch_input(dtype, shape, distinct, len(shape) * 100 + distinct)
    for inv, cnt in itertools.product((False, True), repeat=2):
        for srt in (True, False):
            got = vrs.unique(x, sorted=srt, return_inverse=inv, return_counts=cnt)
            ref = torch.unique(x, sorted=True, return_inverse=inv, return_counts=cnt)
            got, ref = (got, ref) if isinstance(ref, tuple) else ((got,), (ref,))
            assert isinstance(got, tuple) and len(got) == len(ref)
            for a, b in zip(got, ref):
                same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("distinct", [3, 5000])
def test_torch_unique_consecutive_equals_torch(dtype, shape, distinct):
    x = torch_input(dtype, shape, distinct, len(shape) * 10 + distinct)
    if distinct == 3:  # long runs too
        x = torch.sort(x.reshape(-1))[0].reshape(shape) if x.numel() else x
    for inv, cnt in itertools.product((False, True), repeat=2):
        got = vrs.unique_consecutive(x, return_inverse=inv, return_counts=cnt)
        ref = torch.unique_consecutive(x, return_inverse=inv, return_counts=cnt)
        got, ref = (got, ref) if isinstance(ref, tuple) else ((got,), (ref,))
        assert isinstance(got, tuple) and len(got) == len(ref)
        for a, b in zip(got, ref):
            same(a, b)


def test_torch_input_just_queued_on_the_current_stream():
    for _ in range(3):
        base = torch.randint(0, 1 << 30, (3_000_000,), device="cuda", dtype=torch.int64)
        x = (base * 7919) % 65536 - 30000  # queued behind the generator, no synchronise in between
        got = vrs.unique(x, return_inverse=True, return_counts=True)
        ref = torch.unique(x, return_inverse=True, return_counts=True)
        for a, b in zip(got, ref):
            same(a, b)
        y = torch.repeat_interleave(torch.arange(5000, device="cuda", dtype=torch.int32), 300)
        for a, b in zip(vrs.unique_consecutive(y, return_counts=True), torch.unique_consecutive(y, return_counts=True)):
            same(a, b)
