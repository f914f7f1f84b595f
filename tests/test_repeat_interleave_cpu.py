"""Run-length decode without a device: the refusals of vrs.repeat_interleave on CPU tensors, the header's statement of the NULL-queries
form of vrs_search_sorted, and the chunk function of the merge kernel (csrc/vrs_search.hpp: search_identity_chunk) run on the host
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import shutil
import subprocess
from pathlib import Path

import pytest

from vkradixsort_amd import build, capi

ROOT = Path(__file__).resolve().parent.parent


def test_exported_from_the_package():
    import vkradixsort_amd as vrs
    from vkradixsort_amd import repeat

    assert vrs.repeat_interleave is repeat.repeat_interleave


def test_refusals_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    x = torch.arange(6.0).reshape(2, 3)
    for thunk in (lambda: vrs.repeat_interleave(torch.tensor([1, 2, 3])),                    # CPU tensors: no fallback
                  lambda: vrs.repeat_interleave(torch.tensor([1, 2, 3]), output_size=6),
                  lambda: vrs.repeat_interleave(x, torch.tensor([1, 2]), 0),
                  lambda: vrs.repeat_interleave(x, torch.tensor(2)),
                  lambda: vrs.repeat_interleave(x, 2),
                  lambda: vrs.repeat_interleave(x, 0, 1)):
        with pytest.raises(vrs.VrsError, match="GPU") as e:
            thunk()
        assert e.value.code == capi.VRS_ERROR_INVALID_ARGUMENT
    # what torch refuses with a RuntimeError is refused alike, before the device is looked at
    for thunk, text in ((lambda: vrs.repeat_interleave(x, torch.tensor([1.0, 2.0]), 0), "Long or Int"),
                        (lambda: vrs.repeat_interleave(torch.tensor([1.0, 2.0])), "Long or Int"),
                        (lambda: vrs.repeat_interleave(x, torch.tensor([1, 2], dtype=torch.int16), 0), "Long or Int"),
                        (lambda: vrs.repeat_interleave(x, torch.tensor([[1, 2]]), 0), "0-dim or 1-dim"),
                        (lambda: vrs.repeat_interleave(torch.tensor(3)), "1D"),
                        (lambda: vrs.repeat_interleave(x, -1), "non-negative")):
        with pytest.raises(RuntimeError, match=text) as e:
            thunk()
        assert not isinstance(e.value, vrs.VrsError)
    with pytest.raises(IndexError):
        vrs.repeat_interleave(x, 2, 2)
    for thunk in (lambda: vrs.repeat_interleave([1, 2]), lambda: vrs.repeat_interleave(x, 2.0), lambda: vrs.repeat_interleave(x, True),
                  lambda: vrs.repeat_interleave(x, 2, 0, output_size=-1), lambda: vrs.repeat_interleave(torch.tensor([1]), dim=0)):
        with pytest.raises(TypeError):
            thunk()


def test_the_header_states_the_null_queries_form():
    text = (ROOT / "include" / "vkradixsort_amd_ops.h").read_text()
    start = text.index("Sorted-sequence search (build extension")
    block = " ".join(t for t in text[start:text.index("enum { VRS_SEARCH_RIGHT", start)].split() if t != "*")
    for phrase in ("queries == NULL", "0, 1, ..., query_row_len - 1", "VRS_SORT_INT32 or VRS_SORT_INT64", "2^31", "sorter",
                   "vrs_search_stats", "vrs_search_plan"):
        assert phrase in block, phrase


def test_null_queries_keep_their_refusals_without_a_context():
    lib = capi.load_library()
    bad = capi.VRS_ERROR_INVALID_ARGUMENT
    # a NULL context is refused before the queries are looked at, whatever else holds
    for code in (capi.VRS_SORT_INT32, capi.VRS_SORT_INT64, capi.VRS_SORT_FLOAT32):
        assert lib.vrs_search_sorted(None, None, 10, 10, None, 10, 10, code, capi.VRS_SEARCH_RIGHT, None, None, None) == bad
        assert b"NULL" in lib.vrs_last_error(None)


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="needs the ROCm toolchain")
def test_chunk_function_on_the_host_under_sanitizers(tmp_path):
    """The same search_identity_chunk the kernel runs, as a team of one over heap arrays of exact size, against a naive loop: runs of
    one, all boundaries equal, a run across three chunks, 10000 equal boundaries inside a chunk, boundaries at a chunk's edges, negative
    leading boundaries, Q below and above the last boundary, and boundaries in no order (answers inside the row, stores inside out)."""
    src = build.HOST / "test" / "search_identity_host.cpp"
    exe = tmp_path / "search_identity_host"
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
           str(src), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image  # the program is instrumented
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=build.sanitizer_env("asan"))
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert "search_identity_host: ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
