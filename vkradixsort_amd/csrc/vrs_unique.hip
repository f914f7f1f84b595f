// vrs_unique.hip -- run-length encoding (vrs_run_length_encode) and the encode half of unique (vrs_unique), plus unique's rank map.
//   rle_kernel: one pass over the keys.  Tiles of 4096 keys are taken in order from a ticket; wave w of a tile walks 16 chunks of 64
//     consecutive keys.  Head of i: i == 0 || k[i] != k[i-1] (the key in front of a lane comes by shuffle, in front of a wave from
//     memory); a chunk's heads are one __ballot, a lane's rank among them mbcnt.  The heads in front of the tile come by decoupled
//     look-back over one 64-bit status word per tile ({flag, count}: the word is its own flag, agent-scope atomics, no fence).
//     Every element writes its run id, every head its run's key and start.  The tile and the look-back live in vrs_rle_tile.hpp with
//     the key source a template parameter; here it is the keys themselves (vrs_unique_rows.hip: rows).
//   rle_counts_kernel: counts[j] = offsets[j + 1] - offsets[j] for j < R, R read on the device; the grid is sized from n.
//   unique_map_kernel: keys -> ranks (and the iota payloads the sort carries for the inverse).
//   The grid-stride loops count in 64 bits: a 32-bit i + stride wraps to a small value still below a bound near 2^32 (a hang).
#include "vrs_rle_tile.hpp"

#include <algorithm>

namespace vrs {
namespace {

template <typename K>
__global__ __launch_bounds__(kRleThreads) void rle_kernel(RleArgs a) {
    rle_block(a, RlePlainSource<K>{static_cast<const K *>(a.keys)});
}

__global__ __launch_bounds__(256) void rle_counts_kernel(const uint32_t *offsets, const uint32_t *num_runs, uint32_t *counts) {
    const uint32_t R = *num_runs;
    for (size_t j = blockIdx.x * 256u + threadIdx.x; j < R; j += gridDim.x * 256u) counts[j] = offsets[j + 1u] - offsets[j];
}

template <typename K>
__global__ __launch_bounds__(256) void unique_map_kernel(const K *keys, uint32_t n, int key_type, K *mapped, uint32_t *vals) {
    for (size_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        mapped[i] = unique_rank(keys[i], key_type);
        if (vals) vals[i] = static_cast<uint32_t>(i);
    }
}

uint32_t stride_grid(uint32_t n, uint32_t per_block) { return static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(n) + per_block - 1u) / per_block, 8192u)); }

}  // namespace

hipError_t launch_rle(hipStream_t stream, const RleArgs &a) {
    hipError_t e = hipMemsetAsync(a.status, 0, rle_status_bytes(a.n), stream);
    if (e != hipSuccess) return e;
    if (a.key_bytes == 8)
        hipLaunchKernelGGL(rle_kernel<uint64_t>, dim3(rle_tiles(a.n)), dim3(kRleThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(rle_kernel<uint32_t>, dim3(rle_tiles(a.n)), dim3(kRleThreads), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.out_counts) e = launch_rle_counts(stream, a);
    return e;
}

hipError_t launch_rle_counts(hipStream_t stream, const RleArgs &a) {
    hipLaunchKernelGGL(rle_counts_kernel, dim3(stride_grid(a.n, 1024u)), dim3(256), 0, stream, a.out_offsets, a.out_num_runs, a.out_counts);
    return hipGetLastError();
}

hipError_t launch_unique_map(hipStream_t stream, const void *keys, uint32_t n, int key_type, void *mapped, uint32_t *vals) {
    const dim3 grid(stride_grid(n, 1024u));
    if (unique_key_bytes(key_type) == 8)
        hipLaunchKernelGGL(unique_map_kernel<uint64_t>, grid, dim3(256), 0, stream, static_cast<const uint64_t *>(keys), n, key_type,
                           static_cast<uint64_t *>(mapped), vals);
    else
        hipLaunchKernelGGL(unique_map_kernel<uint32_t>, grid, dim3(256), 0, stream, static_cast<const uint32_t *>(keys), n, key_type,
                           static_cast<uint32_t *>(mapped), vals);
    return hipGetLastError();
}

}  // namespace vrs
