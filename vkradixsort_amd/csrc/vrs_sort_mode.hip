// vrs_sort_mode.hip -- the mode form of vrs_sort_restore (VRS_SORT_MODE): the most frequent value of every sorted row and the last place
// it sits in the input, without a position payload through the sort.  Three launches behind two memsets (the rules: vrs_sort_mode_order.hpp):
//   mode_runs_kernel: one read of the sorted ranks.  A workgroup takes one tile of kModeTile ranks, finds the run heads (a ballot per 64
//     ranks, kept in LDS; a wave's first lane gets its predecessor from the wave before it through LDS, the tile's first from memory),
//     gives every run it owns its length -- the distance to the next head, or for the tile's last run one search in the rest of the
//     sorted row by one lane -- and reduces the runs' words per row of the tile: in registers and by a wave maximum while 64 ranks
//     share a row, by LDS atomicMax where rows are shorter or heads are few.  Then at most one atomicMax per (tile, row) goes to
//     scratch[row].
//   mode_index_kernel: one read of the input in the same tiles, the highest first.  Every element compares its rank with the modal rank
//     of its row (ranks[row * row_len + the word's start], fetched once per row of the tile into LDS) and the hits' places are reduced the same way: at most one atomicMax per
//     (tile, row) to out_indices[row], so the highest place wins -- the last occurrence.
//   mode_values_kernel: out_values[row] = src[row * row_len + out_indices[row]], the element's own bits.
// No launch waits for, polls or depends on what another workgroup of the same launch writes: the workgroups meet in an order-independent
// atomicMax alone (a tile first reads the word and skips an atomic that could not raise it -- a filter whose outcome changes no result),
// so the result is the same bits on every run and every grid.
#include "vrs_sort_mode_order.hpp"
#include "vrs_sort_rank.hpp"

namespace vrs {
namespace {

constexpr uint32_t kModeWaves = kModeThreads / 64u, kModeMasks = kModeTile / 64u;
static_assert(kModeTile % kModeThreads == 0u && kModeThreads % 64u == 0u && kModeItems <= 32u, "a tile is whole waves; the head bits fit a word");

__device__ inline unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

// One wave's 64 consecutive elements into the tile's table (0: nothing to say).  A wave with nothing to say does nothing.  Rows do not
// decrease along the lanes, so a wave whose first and last lane share a row is in one row: when more than kModeDirect of its lanes
// speak, one wave maximum and one LDS atomic; a few lanes (a few heads, a few hits) make their own.  Called by whole waves only.
// kModeDirect is A FIRST SETTING, NOT A CROSSOVER: nobody has measured it against its neighbours.
constexpr int kModeDirect = 8;
template <typename W>
__device__ inline void table_max(W *table, uint32_t local_row, W word) {
    const unsigned long long speaking = __ballot(word != 0u);
    if (speaking == 0ull) return;
    const uint32_t first = __builtin_amdgcn_readfirstlane(local_row);
    if (__popcll(speaking) > kModeDirect && first == static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(local_row), 63))) {
        word = wave_max(word);
        if ((threadIdx.x & 63u) == 0u) atomicMax(&table[first], word);
    } else if (word != 0u) {
        atomicMax(&table[local_row], word);
    }
}

// The tile's word of one row to the row's global word: one atomicMax at most.  The word only grows, so a tile that reads a word no
// smaller than its own has nothing to add -- the read is a filter, never waited for and free to be stale (a stale word is a smaller
// one: the atomic is then made for nothing) -- which keeps the tiles of one long row from queueing at one address.
__device__ inline void global_max(unsigned long long *word, unsigned long long mine) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(word, mine);
}

extern __shared__ unsigned long long mode_table[];  // the tile's tables: mode_tile_rows_max(row_len) entries each, sized at the launch

template <typename R>
__global__ __launch_bounds__(kModeThreads) void mode_runs_kernel(const R *__restrict__ ranks, uint32_t n, uint32_t row_len, CompactDiv div,
                                                                 unsigned long long *__restrict__ scratch) {
    unsigned long long *table = mode_table;           // the best word of every row of the tile
    __shared__ unsigned long long masks[kModeMasks];  // the heads among ranks [64 m, 64 m + 64) of the tile
    __shared__ R last[kModeMasks];                    // rank 64 m + 63 of the tile: the predecessor of the next 64 ranks' first
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = mode_tile_base(blockIdx.x), end = mode_tile_end(blockIdx.x, n);
    const uint32_t row0 = compact_div(static_cast<uint32_t>(base), div), row1 = compact_div(static_cast<uint32_t>(end - 1u), div);
    const uint32_t tile_rows = row1 - row0 + 1u;
    const bool one_row = row0 == row1;
    for (uint32_t lr = tid; lr < tile_rows; lr += kModeThreads) table[lr] = 0ull;

    R r[kModeItems];  // (all of the lane's loads first: sixteen in flight)
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j) {
        const uint64_t i = base + j * kModeThreads + tid;
        r[j] = i < end ? ranks[i] : static_cast<R>(0);
    }
    const R before = tid == 0u && base > 0u ? ranks[base - 1u] : static_cast<R>(0);  // the tile's first rank reads its predecessor from memory
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j)
        if (lane == 63u) last[j * kModeWaves + wave] = r[j];
    __syncthreads();

    uint32_t heads = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j) {
        const uint64_t i = base + j * kModeThreads + tid;
        const bool valid = i < end;
        const uint32_t m = j * kModeWaves + wave;
        R previous = __shfl_up(r[j], 1);
        if (lane == 0u) previous = m != 0u ? last[m - 1u] : before;
        const uint32_t row = one_row ? row0 : compact_div(static_cast<uint32_t>(valid ? i : end - 1u), div);
        const bool head = valid && mode_is_head<R>(static_cast<uint32_t>(i - mode_row_begin(row, row_len)), r[j], previous);
        const unsigned long long mask = __ballot(head);
        if (lane == 0u) masks[m] = mask;
        heads |= (head ? 1u : 0u) << j;
    }
    __syncthreads();

    unsigned long long best = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j) {
        const uint64_t i = base + j * kModeThreads + tid;
        const uint32_t row = one_row ? row0 : compact_div(static_cast<uint32_t>(i < end ? i : end - 1u), div);
        unsigned long long word = 0ull;
        if (heads >> j & 1u) {
            uint32_t m = j * kModeWaves + wave;
            unsigned long long rest = lane == 63u ? 0ull : masks[m] >> (lane + 1u);
            uint64_t stop;
            if (rest != 0ull) {
                stop = i + 1u + static_cast<uint32_t>(__builtin_ctzll(rest));
            } else {
                for (++m; m < kModeMasks; ++m)
                    if ((rest = masks[m]) != 0ull) break;
                if (m < kModeMasks) {
                    stop = base + m * 64u + static_cast<uint32_t>(__builtin_ctzll(rest));
                } else {  // the tile's last run: one lane of the workgroup comes here
                    stop = mode_last_run_end<R>([ranks](uint64_t at) { return ranks[at]; }, end, mode_row_end(row, row_len), r[j]);
                }
            }
            word = mode_pack(static_cast<uint32_t>(stop - i), static_cast<uint32_t>(i - mode_row_begin(row, row_len)));
        }
        if (one_row) best = mode_better(best, word);
        else table_max(table, row - row0, word);
    }
    if (one_row) table_max(table, 0u, best);
    __syncthreads();
    for (uint32_t lr = tid; lr < tile_rows; lr += kModeThreads) {
        const unsigned long long word = table[lr];
        if (word != 0ull) global_max(&scratch[row0 + lr], word);
    }
}

template <typename S, typename R, bool FLOAT, bool SIGNED>
__global__ __launch_bounds__(kModeThreads) void mode_index_kernel(const S *__restrict__ src, const R *__restrict__ ranks,
                                                                  const unsigned long long *__restrict__ scratch, uint32_t n, uint32_t row_len,
                                                                  CompactDiv div, R inf_bits, unsigned long long *__restrict__ out_indices) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    // per row of the tile: its modal rank, fetched once (two chained reads), and the highest place of a hit + 1, 0: no hit
    R *modal = reinterpret_cast<R *>(mode_table);
    uint32_t *table = reinterpret_cast<uint32_t *>(modal + mode_tile_rows_max(row_len));
    const uint32_t tid = threadIdx.x;
    // the highest tiles first: the highest place wins, so the tiles that follow mostly find a word they cannot raise (global_max)
    const uint32_t tile = gridDim.x - 1u - blockIdx.x;
    const uint64_t base = mode_tile_base(tile), end = mode_tile_end(tile, n);
    const uint32_t row0 = compact_div(static_cast<uint32_t>(base), div), row1 = compact_div(static_cast<uint32_t>(end - 1u), div);
    const uint32_t tile_rows = row1 - row0 + 1u;
    const bool one_row = row0 == row1;
    S mine[kModeItems];  // (all of the lane's loads first: sixteen in flight)
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j) {
        const uint64_t i = base + j * kModeThreads + tid;
        mine[j] = i < end ? src[i] : static_cast<S>(0);
    }
    for (uint32_t lr = tid; lr < tile_rows; lr += kModeThreads) {
        // where the row's longest run starts (a start past the row cannot come from mode_runs_kernel; it is held inside)
        const uint32_t start = mode_word_start(scratch[row0 + lr]);
        modal[lr] = ranks[mode_row_begin(row0 + lr, row_len) + (start < row_len ? start : row_len - 1u)];
        table[lr] = 0u;
    }
    __syncthreads();
    uint32_t best = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kModeItems; ++j) {
        const uint64_t i = base + j * kModeThreads + tid;
        const bool valid = i < end;
        const uint32_t row = one_row ? row0 : compact_div(static_cast<uint32_t>(valid ? i : end - 1u), div);
        uint32_t hit = 0u;
        if (valid && sort_rank<R, B, FLOAT, SIGNED>(static_cast<R>(mine[j]), inf_bits, false) == modal[row - row0])
            hit = static_cast<uint32_t>(i - mode_row_begin(row, row_len)) + 1u;
        if (one_row) best = hit > best ? hit : best;
        else table_max(table, row - row0, hit);
    }
    if (one_row) table_max(table, 0u, best);
    __syncthreads();
    for (uint32_t lr = tid; lr < tile_rows; lr += kModeThreads) {
        const uint32_t hit = table[lr];
        if (hit != 0u) global_max(&out_indices[row0 + lr], static_cast<unsigned long long>(hit - 1u));
    }
}

template <typename S>
__global__ __launch_bounds__(kModeThreads) void mode_values_kernel(const S *__restrict__ src, const unsigned long long *__restrict__ indices,
                                                                   uint32_t rows, uint32_t row_len, S *__restrict__ values) {
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kModeThreads + threadIdx.x;
    if (row >= rows) return;
    const unsigned long long at = indices[row];
    values[row] = src[row * row_len + (at < row_len ? at : row_len - 1u)];
}

template <typename S, typename R, bool FLOAT, bool SIGNED>
hipError_t mode_as(hipStream_t stream, const void *src, const void *ranks, uint64_t *scratch, uint32_t n, uint32_t row_len, R inf_bits,
                   void *out_values, int64_t *out_indices) {
    const uint32_t rows = n / row_len, tiles = mode_tiles(n);
    const CompactDiv div = compact_div_make(row_len);
    auto *words = reinterpret_cast<unsigned long long *>(scratch);
    auto *places = reinterpret_cast<unsigned long long *>(out_indices);  // (never negative: an unsigned maximum is the signed one)
    hipError_t e;
    if ((e = hipMemsetAsync(scratch, 0, static_cast<size_t>(rows) * sizeof(uint64_t), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(out_indices, 0, static_cast<size_t>(rows) * sizeof(int64_t), stream)) != hipSuccess) return e;
    const uint32_t table_rows = mode_tile_rows_max(row_len);
    hipLaunchKernelGGL((mode_runs_kernel<R>), dim3(tiles), dim3(kModeThreads), table_rows * sizeof(uint64_t), stream, static_cast<const R *>(ranks), n, row_len, div, words);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((mode_index_kernel<S, R, FLOAT, SIGNED>), dim3(tiles), dim3(kModeThreads), table_rows * (sizeof(R) + sizeof(uint32_t)), stream, static_cast<const S *>(src),
                       static_cast<const R *>(ranks), words, n, row_len, div, inf_bits, places);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(rows) + kModeThreads - 1u) / kModeThreads);
    hipLaunchKernelGGL((mode_values_kernel<S>), dim3(blocks), dim3(kModeThreads), 0, stream, static_cast<const S *>(src), places, rows, row_len,
                       static_cast<S *>(out_values));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sort_mode(hipStream_t stream, const void *src, const void *ranks, uint64_t *scratch, uint32_t n, uint32_t row_len, int dtype,
                            void *out_values, int64_t *out_indices) {
    if (n == 0u) return hipSuccess;
    switch (dtype) {
        case kSortI8: return mode_as<uint8_t, uint32_t, false, true>(stream, src, ranks, scratch, n, row_len, 0u, out_values, out_indices);
        case kSortU8: return mode_as<uint8_t, uint32_t, false, false>(stream, src, ranks, scratch, n, row_len, 0u, out_values, out_indices);
        case kSortI16: return mode_as<uint16_t, uint32_t, false, true>(stream, src, ranks, scratch, n, row_len, 0u, out_values, out_indices);
        case kSortI32: return mode_as<uint32_t, uint32_t, false, true>(stream, src, ranks, scratch, n, row_len, 0u, out_values, out_indices);
        case kSortI64: return mode_as<uint64_t, uint64_t, false, true>(stream, src, ranks, scratch, n, row_len, 0ull, out_values, out_indices);
        case kSortF16: return mode_as<uint16_t, uint32_t, true, false>(stream, src, ranks, scratch, n, row_len, 0x7C00u, out_values, out_indices);
        case kSortBF16: return mode_as<uint16_t, uint32_t, true, false>(stream, src, ranks, scratch, n, row_len, 0x7F80u, out_values, out_indices);
        case kSortF32:
            return mode_as<uint32_t, uint32_t, true, false>(stream, src, ranks, scratch, n, row_len, 0x7F800000u, out_values, out_indices);
        case kSortF64:
            return mode_as<uint64_t, uint64_t, true, false>(stream, src, ranks, scratch, n, row_len, 0x7FF0000000000000ull, out_values,
                                                            out_indices);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vrs
