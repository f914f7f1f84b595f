// vrs_sort_mode_order.hpp -- the rules of the mode form of vrs_sort_restore (VRS_SORT_MODE), written down once for the kernels
// (vrs_sort_mode.hip) and for their restatement on the host (mode_tile_host below, which host/test/sort_mode_host.cpp runs against a
// brute-force count): what a run head is, which tile owns a run, where a run that leaves its tile ends, the word a run is reduced by
// and the tile and row arithmetic up to 2^32 - 1 elements.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vrs_compact_order.hpp"

namespace vrs {

constexpr int kSortMode = 2;  // VRS_SORT_MODE
// THE TILE: the flat array of n = rows x row_len sorted ranks (and, in the index pass, of input elements) is cut into tiles of kModeTile
// consecutive elements, whatever the rows; one workgroup of kModeThreads lanes takes one tile, lane t the elements t + j * kModeThreads.
constexpr uint32_t kModeTile = 4096u, kModeThreads = 256u, kModeItems = kModeTile / kModeThreads;

// tiles that cover n (n < 2^32: at most 2^20), and a tile's bounds -- in 64 bits: the last tile's end passes 2^32 - 1
__host__ __device__ inline uint32_t mode_tiles(uint64_t n) { return static_cast<uint32_t>((n + kModeTile - 1u) / kModeTile); }
__host__ __device__ inline uint64_t mode_tile_base(uint32_t tile) { return static_cast<uint64_t>(tile) * kModeTile; }
__host__ __device__ inline uint64_t mode_tile_end(uint32_t tile, uint64_t n) {
    const uint64_t end = mode_tile_base(tile) + kModeTile;
    return end < n ? end : n;
}
// rows: their bounds in 64 bits (row * row_len is below 2^32, (row + 1) * row_len may be 2^32 - 1 + row_len)
__host__ __device__ inline uint64_t mode_row_begin(uint32_t row, uint32_t row_len) { return static_cast<uint64_t>(row) * row_len; }
__host__ __device__ inline uint64_t mode_row_end(uint32_t row, uint32_t row_len) { return mode_row_begin(row, row_len) + row_len; }
// the rows one tile can touch, at most: kModeTile of them at row_len == 1, the whole rows inside it and a partial one at either end else
__host__ __device__ inline uint32_t mode_tile_rows_max(uint32_t row_len) {
    const uint32_t rows = (kModeTile - 1u) / row_len + 2u;
    return rows < kModeTile ? rows : kModeTile;
}

// THE HEAD RULE.  Element i (at `in_row` = i mod row_len of its row) begins a run when it begins its row or differs from its
// predecessor: a run never continues across a row boundary, whatever the neighbouring row begins with.
template <typename R>
__host__ __device__ inline bool mode_is_head(uint32_t in_row, R rank, R previous) {
    return in_row == 0u || rank != previous;
}

// THE WORD a run is reduced by: its length above where it starts in its row, complemented -- so the larger word is the longer run and,
// among equally long ones, the one that starts first (the smaller value: the row is sorted).  count >= 1: a cleared word never wins.
__host__ __device__ inline uint64_t mode_pack(uint32_t count, uint32_t start_in_row) {
    return static_cast<uint64_t>(count) << 32 | (0xFFFFFFFFu - start_in_row);
}
__host__ __device__ inline uint32_t mode_word_count(uint64_t word) { return static_cast<uint32_t>(word >> 32); }
__host__ __device__ inline uint32_t mode_word_start(uint64_t word) { return 0xFFFFFFFFu - static_cast<uint32_t>(word); }
__host__ __device__ inline uint64_t mode_better(uint64_t a, uint64_t b) { return a > b ? a : b; }  // what atomicMax does, in any order

// THE OWNER of a run is the tile its head lies in.  A run whose next head lies in the same tile ends there.  The tile's last run has no
// next head in the tile: it ends at the tile's end when the row ends there or before, else at the upper bound of its rank in the rest
// of its row, ranks[tile_end, row_end) -- sorted, so a search by one lane: probes at tile_end + 0, 1, 3, 7, ... until one differs (a run
// that ends just behind the tile, the usual one, costs a read or two of the next cache line), then a binary search between the last two
// probes.  At most 2 x 32 reads, and 2 log2 of the run's length behind the tile.  Nothing is handed from tile to tile.
template <typename R, typename RanksAt>
__host__ __device__ inline uint64_t mode_last_run_end(RanksAt ranks_at, uint64_t tile_end, uint64_t row_end, R rank) {
    if (row_end <= tile_end) return row_end;
    uint64_t lo = tile_end, hi = row_end, step = 1u;  // ranks[tile_end, lo) are `rank`; hi is row_end or an index whose rank is not
    while (lo < hi) {
        const uint64_t at = step - 1u < hi - 1u - lo ? lo + (step - 1u) : hi - 1u;
        if (ranks_at(at) != rank) {
            hi = at;
            break;
        }
        lo = at + 1u;
        step *= 2u;
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (ranks_at(mid) == rank) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// One tile's runs on the host, by the rules above and in the kernel's terms (rows by the multiply-by-constant division): calls
// emit(row, word) once for every run the tile owns.  The kernel reduces the same words per row with mode_better before it hands
// scratch[row] one atomicMax.  ranks_at(i): the sorted rank at flat index i (an array, or a rule: arithmetic near 2^32 without the data).
template <typename R, typename RanksAt, typename Emit>
inline void mode_tile_host(RanksAt ranks_at, uint64_t n, uint32_t row_len, uint32_t tile, Emit emit) {
    const CompactDiv div = compact_div_make(row_len);
    const uint64_t base = mode_tile_base(tile), end = mode_tile_end(tile, n);
    uint64_t head = end;  // the open run's head; `end`: none yet (the elements in front of the tile's first head are an earlier tile's)
    uint32_t head_row = 0u;
    for (uint64_t i = base; i < end; ++i) {
        const uint32_t row = compact_div(static_cast<uint32_t>(i), div);
        const uint32_t in_row = static_cast<uint32_t>(i - mode_row_begin(row, row_len));
        const R r = ranks_at(i);
        if (!mode_is_head<R>(in_row, r, i > 0u ? ranks_at(i - 1u) : r)) continue;
        if (head != end)
            emit(head_row, mode_pack(static_cast<uint32_t>(i - head), static_cast<uint32_t>(head - mode_row_begin(head_row, row_len))));
        head = i;
        head_row = row;
    }
    if (head == end) return;
    const uint64_t stop = mode_last_run_end<R>(ranks_at, end, mode_row_end(head_row, row_len), ranks_at(head));
    emit(head_row, mode_pack(static_cast<uint32_t>(stop - head), static_cast<uint32_t>(head - mode_row_begin(head_row, row_len))));
}

// the three launches behind two memsets (scratch and out_indices to 0): scratch: `rows` uint64 words; ranks: n uint32 / uint64, every row
// sorted ascending; out_values: `rows` elements of dtype; out_indices: `rows` int64
hipError_t launch_sort_mode(hipStream_t stream, const void *src, const void *ranks, uint64_t *scratch, uint32_t n, uint32_t row_len, int dtype,
                            void *out_values, int64_t *out_indices);

}  // namespace vrs
