// vrs_unique_rows.hip -- the row form of vrs_unique and vrs_run_length_encode (VRS_UNIQUE_COLUMNS(C), C >= 2): distinct rows of an
// n x C matrix of 4- or 8-byte words.  The rules are vrs_unique_rows_order.hpp's.
//   rows_pack_kernel: one round's sort keys.  Lane i packs the ranks of a group's columns (8 or 4 contiguous bytes) of row p: p = i in
//     round 0, where the columns are read where they lie and pos[i] = i is written; p = pos[i] afterwards, a gather of one segment per
//     lane.  The stable pair sort of (key, pos) between the rounds is the host's (vrs_capi_unique.hip).
//   rle_rows_kernel: vrs_rle_tile.hpp's tile with a row source.  A lane keeps a top key per element (SORTED: the last round's sorted
//     keys; else the row's own first 8 bytes) and the shuffles carry it as in the word form; the columns behind it are fetched, through
//     pos when SORTED, only by a lane whose top key equals the one in front.  Run ids go through pos to the inverse; run starts always go
//     to the offsets.
//   rows_out_kernel: out[j, :] = x[pos[offsets[j]], :] (the encode: x[offsets[j], :]) for j < R, R read on the device, the grid sized
//     from n x C; consecutive lanes write consecutive words; the input's own bits, no unrank.
//   Word indices are 64 bits wide: n x C < 2^32 words, up to 2^35 bytes.
#include "vrs_unique_rows_order.hpp"

#include "vrs_rle_tile.hpp"

#include <algorithm>

namespace vrs {
namespace {

template <typename W, typename K, bool SORTED>
struct RleRowSource {
    using Key = K;
    static constexpr bool kPlain = false;
    const K *top;
    const W *x;
    const uint32_t *pos;
    uint32_t cols, c0;
    __device__ __forceinline__ K load(uint32_t i) const {
        if constexpr (SORTED)
            return top[i];
        else
            return rows_front(x, cols, i);
    }
    __device__ __forceinline__ bool head(K key, K prev, uint32_t i) const {
        return rows_head<W, K>(key, prev, x, cols, SORTED ? pos : nullptr, i, c0, cols);
    }
};

template <typename W, typename K, bool SORTED>
__global__ __launch_bounds__(kRleThreads) void rle_rows_kernel(RleRowArgs r) {
    rle_block(r.a, RleRowSource<W, K, SORTED>{static_cast<const K *>(r.a.keys), static_cast<const W *>(r.rows), r.pos, r.cols, r.c0});
}

template <typename W, typename K, uint32_t COUNT, bool FIRST>
__global__ __launch_bounds__(256) void rows_pack_kernel(const W *x, uint32_t n, uint32_t cols, uint32_t c, int key_type, K *keys, uint32_t *pos) {
    for (size_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t p = FIRST ? static_cast<uint32_t>(i) : pos[i];
        const W *row = x + static_cast<uint64_t>(p) * cols;
        if constexpr (COUNT == 2u)
            keys[i] = rows_pack2(row, c, key_type);
        else
            keys[i] = rows_pack1(row, c, key_type);
        if (FIRST) pos[i] = p;
    }
}

template <typename W>
__global__ __launch_bounds__(256) void rows_out_kernel(const W *x, uint32_t cols, const uint32_t *offsets, const uint32_t *pos, const uint32_t *num_runs,
                                                       W *out) {
    const uint64_t words = static_cast<uint64_t>(*num_runs) * cols;
    for (uint64_t w = blockIdx.x * 256u + threadIdx.x; w < words; w += gridDim.x * 256u) {
        const uint32_t j = static_cast<uint32_t>(w / cols), c = static_cast<uint32_t>(w - static_cast<uint64_t>(j) * cols);
        uint32_t row = offsets[j];
        if (pos) row = pos[row];
        out[w] = x[static_cast<uint64_t>(row) * cols + c];
    }
}

uint32_t stride_grid(uint64_t n, uint32_t per_block) { return static_cast<uint32_t>(std::min<uint64_t>((n + per_block - 1u) / per_block, 8192u)); }

template <typename W, typename K, uint32_t COUNT>
void pack(hipStream_t stream, const void *rows, uint32_t n, uint32_t cols, uint32_t c, int key_type, void *keys, uint32_t *pos, bool first) {
    const dim3 grid(stride_grid(n, 1024u));
    if (first)
        hipLaunchKernelGGL((rows_pack_kernel<W, K, COUNT, true>), grid, dim3(256), 0, stream, static_cast<const W *>(rows), n, cols, c, key_type,
                           static_cast<K *>(keys), pos);
    else
        hipLaunchKernelGGL((rows_pack_kernel<W, K, COUNT, false>), grid, dim3(256), 0, stream, static_cast<const W *>(rows), n, cols, c, key_type,
                           static_cast<K *>(keys), pos);
}

}  // namespace

hipError_t launch_rows_pack(hipStream_t stream, const void *rows, uint32_t n, uint32_t cols, uint32_t word, int key_type, uint32_t g, void *keys,
                            uint32_t *pos) {
    const RowsGroup group = rows_group(cols, word, g);
    if (word == 8u)
        pack<uint64_t, uint64_t, 1u>(stream, rows, n, cols, group.first, key_type, keys, pos, g == 0u);
    else if (group.count == 2u)
        pack<uint32_t, uint64_t, 2u>(stream, rows, n, cols, group.first, key_type, keys, pos, g == 0u);
    else
        pack<uint32_t, uint32_t, 1u>(stream, rows, n, cols, group.first, key_type, keys, pos, g == 0u);
    return hipGetLastError();
}

hipError_t launch_rle_rows(hipStream_t stream, const RleRowArgs &r) {
    const RleArgs &a = r.a;
    hipError_t e = hipMemsetAsync(a.status, 0, rle_status_bytes(a.n), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(rle_tiles(a.n)), block(kRleThreads);
    if (!r.pos) {
        if (r.word == 8u)
            hipLaunchKernelGGL((rle_rows_kernel<uint64_t, uint64_t, false>), grid, block, 0, stream, r);
        else
            hipLaunchKernelGGL((rle_rows_kernel<uint32_t, uint64_t, false>), grid, block, 0, stream, r);
    } else if (r.word == 8u) {
        hipLaunchKernelGGL((rle_rows_kernel<uint64_t, uint64_t, true>), grid, block, 0, stream, r);
    } else if (a.key_bytes == 8) {
        hipLaunchKernelGGL((rle_rows_kernel<uint32_t, uint64_t, true>), grid, block, 0, stream, r);
    } else {
        hipLaunchKernelGGL((rle_rows_kernel<uint32_t, uint32_t, true>), grid, block, 0, stream, r);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.out_counts && (e = launch_rle_counts(stream, a)) != hipSuccess) return e;
    if (a.out_keys) {
        const dim3 out_grid(stride_grid(static_cast<uint64_t>(a.n) * r.cols, 1024u));
        if (r.word == 8u)
            hipLaunchKernelGGL(rows_out_kernel<uint64_t>, out_grid, dim3(256), 0, stream, static_cast<const uint64_t *>(r.rows), r.cols, a.out_offsets, r.pos,
                               a.out_num_runs, static_cast<uint64_t *>(a.out_keys));
        else
            hipLaunchKernelGGL(rows_out_kernel<uint32_t>, out_grid, dim3(256), 0, stream, static_cast<const uint32_t *>(r.rows), r.cols, a.out_offsets, r.pos,
                               a.out_num_runs, static_cast<uint32_t *>(a.out_keys));
        e = hipGetLastError();
    }
    return e;
}

}  // namespace vrs
