// Lab: where does a tile of the pool form's scatter passes spend its time, set against the contract scatter's?  Forced in front of ONE
// unit of the library (vrs_msd_pool or vrs_contract), it turns the VRS_MARK hooks of scatter_chunk and of the kernels into time stamps:
//   tools/lab/build_local_variant.sh marks_pool vrs_msd_pool -include tools/lab/pool_phase_marks.hip
//   tools/lab/build_local_variant.sh marks_contract vrs_contract -include tools/lab/pool_phase_marks.hip
// and tools/lab/pool_phase_marks.py reads them back.  Thread 0 stamps the constant 100 MHz clock into LDS (no global round trip inside a
// phase); the kernel's last instruction writes the eight stamps of its workgroup out.
#pragma once
#include <hip/hip_runtime.h>

namespace vrs_lab {
constexpr unsigned kMarkKernels = 3, kMarkBlocks = 16384;
__device__ unsigned long long g_marks[kMarkKernels][kMarkBlocks][8];
}  // namespace vrs_lab
__shared__ unsigned long long vrs_lab_s_marks[8];

#define VRS_MARK(i)                                                            \
    do {                                                                       \
        if (threadIdx.x == 0) vrs_lab_s_marks[(i)] = wall_clock64();           \
    } while (0)
#define VRS_MARK_FLUSH(...)                                                                                                   \
    do {                                                                                                                      \
        if (threadIdx.x == 0) {                                                                                               \
            vrs_lab_s_marks[7] = wall_clock64();                                                                              \
            for (int i_ = 0; i_ < 8; ++i_) vrs_lab::g_marks[__VA_ARGS__ + 0][blockIdx.x % vrs_lab::kMarkBlocks][i_] = vrs_lab_s_marks[i_]; \
        }                                                                                                                     \
    } while (0)

// every stamp of the launches that ran last, [kernel][workgroup][mark]; out: kMarkKernels * kMarkBlocks * 8 words of 64 bits
extern "C" __attribute__((visibility("default"))) int vrs_lab_read_marks(unsigned long long *out) {
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vrs_lab::g_marks), sizeof(vrs_lab::g_marks)) == hipSuccess ? 0 : 1;
}
