"""Phase times of one tile (tools/lab/pool_phase_marks.hip): K sorts of N keys back to back, as bench.py runs them, then the stamps of
the launches that ran last.
usage: VRS_LIB=tools/lab/libs/libvrs_marks_pool.so pool_phase_marks.py pool [N] [K]
       VRS_LIB=tools/lab/libs/libvrs_marks_contract.so pool_phase_marks.py contract [N] [K]   (the contract stages: the pass with shift 24 ran last)"""
import ctypes
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from vkradixsort_amd import capi  # noqa: E402
import vkradixsort_amd as vrs  # noqa: E402

which = sys.argv[1]
n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10 ** 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 6
KERNELS, BLOCKS = 3, 16384
PHASES = [("entry -> key loads issued", 6, 0), ("loads issued -> keys landed, counters zeroed", 0, 1), ("rank", 1, 2), ("scan (+ reservation asked)", 2, 3),
          ("re-bucket (+ reservation answered)", 3, 4), ("write-out issued", 4, 5), ("entry -> last store issued", 6, 5)]

keys = np.random.RandomState(1).randint(0, 2 ** 32, size=n, dtype=np.uint32)
with vrs.GPUContext(0) as gpu:
    S = vrs.Buffer.BufferSettings
    src = vrs.Buffer.fillDeviceWithStagingBuffer(gpu, S(4 * n), keys)
    batches = [vrs.Buffer(gpu, S(4 * n)) for _ in range(K)]
    tmp = vrs.Buffer(gpu, S(4 * n))
    if which == "contract":
        gpu.setTuning(capi.VRS_TUNE_ONE_CALL_MIN_KEYS, 0)
    for rep in range(2):  # (the first round warms up: scratch, the probe, the kept layout)
        for b in batches:
            b.copyFrom(src)
        gpu.waitIdle()
        for b in batches:
            gpu.check(gpu.lib.vrs_sort_keys_u32(gpu.handle, b.handle, tmp.handle, n))
        gpu.waitIdle()
    marks = np.zeros((KERNELS, BLOCKS, 8), dtype=np.uint64)
    lab = ctypes.CDLL(str(capi.LIB_PATH))
    lab.vrs_lab_read_marks.argtypes = [ctypes.c_void_p]
    if lab.vrs_lab_read_marks(marks.ctypes.data) != 0:
        raise SystemExit("reading the marks failed")
    out = np.empty(n, np.uint32)
    batches[-1].downloadWithStagingBuffer(out)
    print(f"{which}: N={n}, K={K} sorts back to back, sorted={bool(np.all(out[1:] >= out[:-1]))}; ticks of 10 ns")
    names = {0: "scatter_kernel (contract, shift 24)", 1: "pool_pass_a_kernel<false>", 2: "pool_pass_b_kernel<7,false>"}
    for k in ((0,) if which == "contract" else (1, 2)):
        m = marks[k].astype(np.int64)
        live = np.nonzero((m[:, 5] > 0) & (m[:, 6] > 0) & (m[:, 0] >= m[:, 6]) & (m[:, 5] >= m[:, 4]))[0]
        if live.size == 0:
            print(f"{names[k]}: no marks")
            continue
        mid = live[live.size // 2]
        span = (m[live, 7].max() - m[live, 6].min()) / 100.0
        print(f"{names[k]}: {live.size} workgroups with marks, first entry -> last exit {span:.1f} us")
        for label, a, b in PHASES:
            d = (m[live, b] - m[live, a]) / 100.0
            print(f"    {label:46s} mean {d.mean():6.2f} us  median {np.median(d):6.2f}  p90 {np.percentile(d, 90):6.2f}   workgroup {mid}: {(m[mid, b] - m[mid, a]) / 100.0:6.2f}")
