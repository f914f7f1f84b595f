// vrs_compact_order.hpp -- the ordered stream compaction's rules, written down once for the kernels (vrs_compact.hip) and for their
// restatement on the host (vrs_compact_host in vrs_capi_compact.hip): which element counts as nonzero, how the n elements are cut into
// tiles, and how a flat position becomes coordinates (division by constants made on the host).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vrs_sort_rank.hpp"

namespace vrs {

// dtypes: the nine of vrs_sort_dtype and bool (one byte, read as it lies)
constexpr int kCompactBool = 9;
// T, the elements of one tile (VRS_TUNE_COMPACT_TILE_ELEMS): a multiple of kCompactChunk, the elements a 256-lane workgroup covers with one
// 16-byte load per lane of a 1-byte dtype -- and, for every dtype, with 16 elements per lane
constexpr uint32_t kCompactChunk = 4096u, kCompactTileMin = 4096u, kCompactTileMax = 65536u, kCompactTileDefault = 16384u;
constexpr uint32_t kCompactThreads = 256u;
// the carries: one workgroup of kCompactCarryThreads lanes takes kCompactCarryBlock tile counts per step (four per lane)
constexpr uint32_t kCompactCarryThreads = 1024u, kCompactCarryBlock = 4096u;
constexpr uint32_t kCompactMaxDims = 8u;
constexpr int kCompactRows = 0, kCompactColumns = 1;  // coordinates as [R, ndim] or as [ndim, R]
constexpr size_t kCompactHeaderBytes = 256u;          // the total R (uint64) in front of the tiles' words

__host__ __device__ inline bool compact_dtype_known(int dtype) { return sort_dtype_known(dtype) || dtype == kCompactBool; }
__host__ __device__ inline int compact_dtype_bytes(int dtype) { return dtype == kCompactBool ? 1 : sort_dtype_bytes(dtype); }
__host__ __device__ inline bool compact_tile_known(uint32_t T) { return T >= kCompactTileMin && T <= kCompactTileMax && T % kCompactChunk == 0u; }
__host__ __device__ inline bool compact_value_bytes_known(uint32_t b) { return b == 1u || b == 2u || b == 4u || b == 8u; }

// THE PREDICATE.  An element is nonzero when (bits & keep) != 0: keep is every bit for integers and bool, every bit but the sign for
// floats -- so -0.0 is zero, and NaNs, infinities and subnormals are nonzero.
__host__ __device__ inline uint64_t compact_keep_mask(int dtype) {
    switch (dtype) {
        case kSortF16:
        case kSortBF16: return 0x7fffull;
        case kSortF32: return 0x7fffffffull;
        case kSortF64: return 0x7fffffffffffffffull;
        default: return ~0ull;
    }
}
__host__ __device__ inline bool compact_nonzero(uint64_t bits, uint64_t keep) { return (bits & keep) != 0ull; }

// tiles of T elements that cover n (n < 2^32: at most 2^20)
__host__ __device__ inline uint32_t compact_tiles(uint64_t n, uint32_t T) { return static_cast<uint32_t>((n + T - 1u) / T); }

// Division of a 32-bit numerator by a constant d >= 1 that is known on the host: q = the high 64 bits of m x a with m = floor((2^64 - 1) / d)
// + 1, exact for every 32-bit a and d >= 2 (the error of m x a against 2^64 a / d is below a d / d < 2^32 <= 2^64 / d); d == 1 is m == 0.
struct CompactDiv {
    uint64_t m;
    uint32_t d, pad;
};
__host__ __device__ inline CompactDiv compact_div_make(uint32_t d) {
    CompactDiv c{};
    c.d = d;
    c.m = d <= 1u ? 0ull : ~0ull / d + 1ull;
    return c;
}
__host__ __device__ inline uint32_t compact_div(uint32_t a, const CompactDiv &c) {
    if (c.m == 0ull) return a;
    // (m x a) >> 64 with a below 2^32: two 32 x 32 -> 64 products
    const uint64_t lo = (c.m & 0xffffffffull) * a, hi = (c.m >> 32) * a;
    return static_cast<uint32_t>((hi + (lo >> 32)) >> 32);
}
__host__ __device__ inline uint32_t compact_mod(uint32_t a, const CompactDiv &c) { return a - compact_div(a, c) * c.d; }

// THE ROW FORM (row_elems = W >= 2): every flag stands for a dense row of row_bytes = W x value_bytes bytes, and a chunk's output is one
// contiguous span of bytes that consecutive lanes copy word by word.  THE WORD: 16 bytes when row_bytes and every base involved (the
// values and the output of a gather; the input, the source and the output of a scatter, or-ed into `bases`) are multiples of 16, else the
// largest of 8, 4, 2 and 1 bytes that divides them all -- so every row of every buffer starts on a word.
__host__ __device__ inline uint32_t compact_row_word_bytes(uint64_t row_bytes, uint64_t bases) {
    const uint64_t all = row_bytes | bases;
    uint32_t word = 16u;
    while (all & (word - 1u)) word >>= 1;
    return word;
}
// A chunk's span is indexed in 32 bits and cut into rows by compact_div while a row holds at most kCompactRowNarrowWords words
// (kCompactChunk rows of them are at most 2^32 words); wider rows are walked one by one with a 64-bit word index.
constexpr uint64_t kCompactRowNarrowWords = 1ull << 20;
// The row kernels run over (tiles, slices): every slice ranks its chunks' flags again (one flag per row) and copies every slices-th run
// of kCompactThreads words of the span.  slices = the bytes a full tile moves over kCompactRowSliceBytes, at most kCompactRowSlicesMax.
// kCompactRowSliceBytes is a FIRST SETTING, NOT A CROSSOVER: nobody has measured it (tools/mask_index_time.py sweeps it through
// VRS_COMPACT_ROW_SLICE_BYTES when it is given a device).
constexpr uint64_t kCompactRowSliceBytes = 256u * 1024u;
constexpr uint32_t kCompactRowSlicesMax = 2048u;
__host__ __device__ inline uint32_t compact_row_slices_for(uint64_t rows, uint64_t row_bytes, uint64_t slice_bytes) {
    const uint64_t want = (rows * row_bytes + slice_bytes - 1u) / slice_bytes;  // (rows <= 65536, row_bytes < 2^35: no wrap)
    return want < 1u ? 1u : want > kCompactRowSlicesMax ? kCompactRowSlicesMax : static_cast<uint32_t>(want);
}
__host__ __device__ inline uint32_t compact_row_slices(uint64_t n, uint32_t T, uint64_t row_bytes) {
    return compact_row_slices_for(n < T ? n : T, row_bytes, kCompactRowSliceBytes);
}

// A flat position in a contiguous array of `ndim` sizes: coordinate k = (p / stride[k]) mod size[k], stride[k] the product of the sizes
// behind k.  Every stride and size is at most n < 2^32.
struct CompactShape {
    uint32_t ndim, pad;
    CompactDiv stride[kCompactMaxDims], size[kCompactMaxDims];
};
inline CompactShape compact_shape_make(uint32_t ndim, const uint32_t *sizes) {
    CompactShape s{};
    s.ndim = ndim;
    uint64_t stride = 1u;
    for (uint32_t k = ndim; k-- > 0u;) {
        s.stride[k] = compact_div_make(static_cast<uint32_t>(stride));
        s.size[k] = compact_div_make(sizes[k]);
        stride *= sizes[k];
    }
    return s;
}
__host__ __device__ inline uint32_t compact_coordinate(uint32_t p, const CompactShape &s, uint32_t k) {
    return compact_mod(compact_div(p, s.stride[k]), s.size[k]);
}

}  // namespace vrs
