"""tools/isa_audit.py: the parser on a small canned listing (no compiler), then the keys' local sorts of both forms as the compiler makes them today."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("isa_audit", ROOT / "tools" / "isa_audit.py")
isa_audit = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_audit)

CANNED = """
\t.text
\t.type\t_Z5firstPj,@function
_Z5firstPj:                             ; @_Z5firstPj
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_accvgpr_write_b32 a0, v9            ; 4-byte Folded Spill
\tds_read_b32 v1, v0
\ts_waitcnt lgkmcnt(0)
\tds_read_b32 v2, v0 offset:4
\tds_read_b32 v3, v0 offset:8
\ts_waitcnt lgkmcnt(1)
\tv_add_u32_e32 v1, v1, v2
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB0_2
; %bb.1:
\tds_read_b32 v4, v0 offset:12
\ts_waitcnt vmcnt(1) lgkmcnt(0)
.LBB0_2:
\ts_or_b64 exec, exec, s[2:3]
\tds_read_b128 v[4:7], v0
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v8, v1, s[0:1]
\tv_accvgpr_read_b32 v9, a0             ; 4-byte Folded Reload
\ts_waitcnt vmcnt(0)
\tglobal_store_dword v8, v9, s[0:1] offset:4
\ts_waitcnt vmcnt(0)
\ts_barrier
\ts_waitcnt vmcnt(0)
\tglobal_store_dword v8, v2, s[0:1] offset:8
\tbuffer_wbl2 sc0 sc1
\ts_waitcnt vmcnt(0)
\tglobal_store_dword v8, v3, s[0:1] offset:12
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z5firstPj, .Lfunc_end0-_Z5firstPj
; Kernel info:
; NumVgprs: 10
; ScratchSize: 8
; LDSByteSize: 4096 bytes/workgroup (compile time only)
; Occupancy: 8
\t.type\t_Z6secondv,@function
_Z6secondv:                             ; @_Z6secondv
; %bb.0:
\tscratch_load_dword v40, off, s32        ; 4-byte Folded Reload
\ts_swappc_b64 s[30:31], s[4:5]
\ts_waitcnt lgkmcnt(0)
\ts_setpc_b64 s[30:31]
.Lfunc_end1:
; Function info:
; NumVgprs: 41
; ScratchSize: 4
"""


def test_the_parser_counts_what_it_says_it_counts():
    first, second = isa_audit.parse(CANNED)
    assert first["name"] == "_Z5firstPj" and second["name"] == "_Z6secondv"
    assert (first["vgprs"], first["scratch"], first["lds"], first["occ"]) == (10, 8, 4096, 8)
    assert (first["spills"], first["hot"]) == (2, 2)
    # two reads are waited for on their own (the second under an exec-mask branch, its wait shared with vmcnt); the pipelined pair and the
    # 16-byte read are not
    assert first["dep_reads"] == 2 and first["lgkm0"] == 3 and first["saveexec"] == 1
    # one wait stands between two stores of a chain; the one in front of the barrier has no store behind it in its chain, the one behind the
    # barrier none before it, and the last is a release fence the source asked for
    assert first["store_waits"] == 1 and first["where"]["store_waits"] == [25]
    # a function that is no kernel: no LDS or occupancy line, and its spill sits next to a call
    assert (second["vgprs"], second["scratch"], second["lds"], second["occ"]) == (41, 4, None, None)
    assert (second["spills"], second["hot"], second["dep_reads"], second["lgkm0"]) == (1, 0, 0, 1)


def test_names_and_the_table():
    assert isa_audit.short("void vrs::(anonymous namespace)::pool_local_sort_kernel<256, 7, 4, 7u>(unsigned int const*, unsigned int*)") == \
        "pool_local_sort_kernel<256, 7, 4, 7u>"
    rows = isa_audit.audit(CANNED, "first")
    assert len(rows) == 1
    lines = isa_audit.table(rows).splitlines()
    assert lines[0].split() == ["function", *isa_audit.FIELDS] and lines[1].split()[1:] == ["10", "8", "4096", "8", "2", "2", "2", "1", "1", "3"]


@pytest.fixture(scope="module")
def listings():
    """the two units that hold the keys' local sorts, compiled side by side (device code only, about a minute; tests/test_sanitizers_cpu.py
    builds the whole library twice).  No toolchain is a failure, not a skip: the library cannot be built without it either."""
    from concurrent.futures import ThreadPoolExecutor
    units = ("vrs_msd_pool_local.hip", "vrs_msd_hybrid.hip")
    with ThreadPoolExecutor(max_workers=2) as pool:
        texts = list(pool.map(lambda u: isa_audit.compile_unit(ROOT / "vkradixsort_amd" / "csrc" / u), units))
    return dict(zip(units, texts))


def test_the_pool_local_sort_has_no_spill_and_no_serialised_read_on_its_hot_path(listings):
    """The pool form's keys kernels of every shape: no spill instruction at all in the workgroup kernels (the save and restore around the
    guarded copy's call included: today there is none), no wait between output stores, no counter read that is waited for on its own,
    registers and LDS within today's occupancy (4 / 5 / 2 workgroups per CU)."""
    rows = isa_audit.audit(listings["vrs_msd_pool_local.hip"], r"pool_local_sort_kernel(<|I)")
    assert len(rows) == 9  # three shapes x three widths of the second pass
    for r in rows:
        threads, vec = map(int, re.search(r"pool_local_sort_kernelILi(\d+)ELi(\d+)E", r["name"]).groups())  # (the mangled name: no demangler needed)
        assert (r["spills"], r["hot"], r["store_waits"], r["dep_reads"]) == (0, 0, 0, 0), (r["short"], r["where"])
        assert r["vgprs"] <= (102 if vec == 4 else 128) and r["lds"] <= {(256, 4): 28048, (256, 7): 40336, (512, 7): 78224}[(threads, vec)], r["short"]


def test_the_one_wave_kernels_and_the_counted_form(listings):
    """The one-wave kernels of both forms and the counted form's workgroup kernels (the same bodies, sorting in place).  No spill on a hot
    path and no wait between output stores anywhere.  The workgroup kernels have no read waited for on its own.  The one-wave kernels keep a
    few, all in their seven-row case: 28 keys, 28 ranks and the reads in flight do not fit 128 registers, and the scheduler itself issues
    the last reads of a pass one by one (8 in the pool form's kernel, 4 in the counted form's; 164 each before the reads were pinned) -- the
    numbers are today's, so that a read sunk into a branch again shows.  That vrs_msd_hybrid.hip compiles at all is a check too: the
    unconditional reads of wave_sort_body's out-of-line copy once failed in the backend (wave_sort_bucket has the note)."""
    pool = isa_audit.audit(listings["vrs_msd_pool_local.hip"], r"pool_local_sort_wave_kernel")
    assert len(pool) == 3
    for r in pool:
        assert (r["hot"], r["store_waits"]) == (0, 0) and r["dep_reads"] <= 8 and r["vgprs"] <= 128 and r["lds"] <= 9488, (r["short"], r["where"])
    counted = {r["name"]: r for r in isa_audit.audit(listings["vrs_msd_hybrid.hip"], r"msd_local_sort_(keys|wave)_kernel")}
    assert len(counted) == 3
    for name, r in counted.items():
        wave = "wave" in name
        assert (r["hot"], r["store_waits"]) == (0, 0) and r["dep_reads"] <= (4 if wave else 0) and r["vgprs"] <= 128, (r["short"], r["where"])
        if not wave:
            assert r["spills"] == 0, r["short"]
