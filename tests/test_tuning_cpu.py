"""The tuning settings' one table (csrc/vrs_tuning.hpp) without a device: host/test/tuning_host.cpp walks it key by key under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program and prints every key's default and range; the Python copies
(capi's *_DEFAULT, *_MIN, *_MAX names and capi.TUNING_DEFAULTS) are held against what it printed, the keys against the public header;
and the context and vrs_set_tuning keep no copy of a default or a range of their own."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi, engine

ROOT = Path(__file__).resolve().parent.parent
HAS_HIPCC = shutil.which("hipcc") is not None or Path("/opt/rocm/bin/hipcc").exists()
MOVED = ("xcd_remap fused_prefix one_call_min_keys single_max_keys os_fused_plan os_groups os_spin_budget os_hold_tile os_misplace os_hybrid os_fast_count "
         "os_hybrid_min_keys os_async os_plan_wait_ms os_reserve os_pool os_pool_top_bits os_pool_pairs os_pool_pairs_packed os_pool_min_keys "
         "os_pool_sub_bits os_pool_reuse os_pool_reuse_rooms seg_one_call_min_keys topk_grid_min_keys select_grid_min_keys select_compact_divisor "
         "search_lds_bytes search_table_min_queries search_index_min_queries bincount_lds_bytes reduce_chunk_rows reduce_lane_rows scan_tile_rows "
         "scan_single_pass_min_rows scan_spin_budget compact_tile_elems").split()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{key: (default, min, max, multiple)} as tuning_host printed it (None = no default / no bound), after all its checks held."""
    if not HAS_HIPCC:
        pytest.skip("needs the ROCm toolchain")
    exe = tmp_path_factory.mktemp("tuning") / "tuning_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(build.HOST / "test" / "tuning_host.cpp"), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "tuning_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
    rows = {}
    for line in run.stdout.splitlines():
        if re.fullmatch(r"\d+( (-|-?\d+)){4}", line):
            key, *rest = line.split()
            rows[int(key)] = tuple(None if f == "-" else int(f) for f in rest)
    return rows


def test_the_table_under_sanitizers_has_a_row_for_every_key_of_the_header(table):
    text = (ROOT / "include" / "vkradixsort_amd_tune.h").read_text()
    enum = text[text.index("typedef enum vrs_tuning_key"):text.index("} vrs_tuning_key;")]
    header = {name: int(value) for name, value in re.findall(r"\b(VRS_TUNE_\w+)\s*=\s*(\d+)", enum)}
    assert sorted(header.values()) == list(range(41)) == sorted(table)
    ours = {name: value for name, value in vars(capi).items() if name.startswith("VRS_TUNE_")}
    assert ours == header


def test_the_python_copies_equal_the_table(table):
    """every capi NAME_DEFAULT / NAME_MIN / NAME_MAX whose VRS_TUNE_NAME exists, and every entry of capi.TUNING_DEFAULTS"""
    column = {"DEFAULT": 0, "MIN": 1, "MAX": 2}
    seen = []
    for name, value in sorted(vars(capi).items()):
        m = re.fullmatch(r"(\w+)_(DEFAULT|MIN|MAX)", name)
        key = getattr(capi, "VRS_TUNE_" + m.group(1), None) if m else None
        if key is None:
            continue
        assert table[key][column[m.group(2)]] == value, (name, value, table[key])
        seen.append(name)
    assert len(seen) == 22 and sum(name.endswith("_DEFAULT") for name in seen) == 16, seen  # (the names as they stand: none was skipped)
    assert len(capi.TUNING_DEFAULTS) == 16
    for key, value in capi.TUNING_DEFAULTS.items():
        assert table[key][0] == value, (key, value, table[key])
    for key in (capi.VRS_TUNE_SCAN_TILE_ROWS, capi.VRS_TUNE_COMPACT_TILE_ELEMS):  # the two "multiple of" keys: a multiple of their minimum
        assert table[key][3] == table[key][1] > 1
    assert all(row[3] == 1 for key, row in table.items() if key not in (capi.VRS_TUNE_SCAN_TILE_ROWS, capi.VRS_TUNE_COMPACT_TILE_ELEMS))


def test_tuned_is_what_was_set_else_the_default():
    ctx = engine.GPUContext()  # (never initialised: tuned() asks the dictionary, not the device)
    assert ctx.tuning == {} and ctx.tuned(capi.VRS_TUNE_SCAN_TILE_ROWS) == capi.SCAN_TILE_ROWS_DEFAULT
    ctx.tuning[capi.VRS_TUNE_SCAN_TILE_ROWS] = 512
    assert ctx.tuned(capi.VRS_TUNE_SCAN_TILE_ROWS) == 512 and ctx.tuned(capi.VRS_TUNE_REDUCE_CHUNK_ROWS) == capi.REDUCE_CHUNK_ROWS_DEFAULT
    assert ctx.tuning == {capi.VRS_TUNE_SCAN_TILE_ROWS: 512}  # only what was set
    with pytest.raises(KeyError):
        ctx.tuned(capi.VRS_TUNE_XCD_REMAP)  # no Python copy of that default: nothing to answer with
    for wrapper in ("scan.py", "compact.py", "reduce.py"):
        assert "tuning.get(" not in (build.PKG_DIR / wrapper).read_text()


def test_the_context_and_the_setter_hold_no_copy():
    host = (build.CSRC / "vrs_host.hpp").read_text()
    context = host[host.index("struct vrs_context_t {"):host.index("struct vrs_buffer_t {")]
    assert "vrs::Tuning tune;" in context
    for name in MOVED:  # none is a member of the context any more (os_pool_fail_alloc, os_pool_skip ... are state and stay)
        assert not re.search(rf"\b{name}\b\s*(=|;|\[)", context), name
    capi_src = (build.CSRC / "vrs_capi.hip").read_text()
    setter = capi_src[capi_src.index("int vrs_set_tuning("):]
    assert "vrs::tuning_refusal(key, value)" in setter and "vrs::tuning_store(ctx->tune, key, value)" in setter
    assert not re.search(r"value\s*(<|>|%)", setter) and "fail(ctx, VRS_ERROR_INVALID_ARGUMENT, \"" not in setter  # no range, no message of its own
    assert setter.index("settle_pending") < setter.index("tuning_refusal") < setter.index("tuning_store") < setter.index("switch (key)")
    for source in build.CSRC.glob("vrs_capi*.hip"):  # every reader goes through ctx->tune
        text = source.read_text()
        for name in MOVED:
            assert not re.search(rf"ctx->{name}\b", text), (source.name, name)
