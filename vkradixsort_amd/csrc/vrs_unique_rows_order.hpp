// vrs_unique_rows_order.hpp -- the rules of the row form of vrs_unique / vrs_run_length_encode (key_type / key_bytes with
// VRS_UNIQUE_COLUMNS(C), C >= 2), as host and device functions the kernels of vrs_unique_rows.hip compile and host/test/unique_rows_host.cpp
// runs on the CPU.  Internal.
//   The plan: the C columns of a row, `word` (4 or 8) bytes each, are grouped from the last column backwards into groups of at most 8
//     bytes of ranks: two 4-byte columns (the more significant, lower-numbered column in the key's high half) or one 8-byte column.  A
//     lone 4-byte column left over is column 0 and gets a 32-bit key.  Group 0 is the least significant; rounds = ceil(C * word / 8).
//   The pack: key = the ranks (unique_rank) of a group's columns, so ascending keys are ascending (sub-)rows.
//   The head rule: rows are equal when bit-identical (r is a bijection: equal ranks are equal bits); the top group is compared first, the
//     columns behind it only for a pair whose top groups are equal.
#pragma once
#include "vrs_unique.hpp"

namespace vrs {

constexpr uint32_t kRowsColumnsShift = 8u;  // VRS_UNIQUE_COLUMNS(c) = c << 8; the low byte is the key type / the width

__host__ __device__ inline uint32_t rows_columns(int encoded) { return static_cast<uint32_t>(encoded) >> kRowsColumnsShift; }
__host__ __device__ inline int rows_low_byte(int encoded) { return encoded & 0xFF; }

__host__ __device__ inline uint32_t rows_rounds(uint32_t cols, uint32_t word) { return (cols * word + 7u) / 8u; }

struct RowsGroup {
    uint32_t first, count;  // columns [first, first + count); the key has count * word bytes
};
// group g of the plan, 0 = the least significant (the last columns) ... rows_rounds - 1 = the top group (it begins at column 0)
__host__ __device__ inline RowsGroup rows_group(uint32_t cols, uint32_t word, uint32_t g) {
    const uint32_t per = 8u / word, end = cols - g * per;
    const uint32_t first = end >= per ? end - per : 0u;
    return RowsGroup{first, end - first};
}

// the key of columns [c, c + COUNT) of the row at `row` (W: uint32_t or uint64_t words)
__host__ __device__ inline uint64_t rows_pack2(const uint32_t *row, uint32_t c, int key_type) {
    return (static_cast<uint64_t>(unique_rank(row[c], key_type)) << 32) | unique_rank(row[c + 1u], key_type);
}
__host__ __device__ inline uint32_t rows_pack1(const uint32_t *row, uint32_t c, int key_type) { return unique_rank(row[c], key_type); }
__host__ __device__ inline uint64_t rows_pack1(const uint64_t *row, uint32_t c, int key_type) { return unique_rank(row[c], key_type); }

// columns [c0, c1) of rows ra and rb of the n x cols matrix x hold the same bits (64-bit word index: n * cols may be near 2^32)
template <typename W>
__host__ __device__ inline bool rows_equal(const W *x, uint32_t cols, uint32_t ra, uint32_t rb, uint32_t c0, uint32_t c1) {
    const W *a = x + static_cast<uint64_t>(ra) * cols, *b = x + static_cast<uint64_t>(rb) * cols;
    for (uint32_t c = c0; c < c1; ++c)
        if (a[c] != b[c]) return false;
    return true;
}

// the head rule: element i (> 0) starts a run when its top key differs from the one in front, or -- only when they are equal -- the
// columns [c0, c1) behind the top group differ between its row and the row in front.  pos: the sorted positions (unique), or null (the
// encode: rows i and i - 1 themselves).
template <typename W, typename K>
__host__ __device__ inline bool rows_head(K key, K prev, const W *x, uint32_t cols, const uint32_t *pos, uint32_t i, uint32_t c0, uint32_t c1) {
    if (key != prev) return true;
    if (c0 >= c1) return false;
    return !rows_equal(x, cols, pos ? pos[i] : i, pos ? pos[i - 1u] : i - 1u, c0, c1);
}

// the encode's own top key of row i: its first 8 bytes (the first two 4-byte columns, or the first 8-byte column), read where they lie
__host__ __device__ inline uint64_t rows_front(const uint32_t *x, uint32_t cols, uint32_t i) {
    const uint32_t *row = x + static_cast<uint64_t>(i) * cols;
    return (static_cast<uint64_t>(row[0]) << 32) | row[1];
}
__host__ __device__ inline uint64_t rows_front(const uint64_t *x, uint32_t cols, uint32_t i) { return x[static_cast<uint64_t>(i) * cols]; }

// the row form's scratch, whatever C is and whichever outputs are given: the status block, two key buffers of 8 bytes per row (a lone
// column 0's 32-bit keys use their front halves), the positions and their partner, the run offsets (the rows go out through them):
// at most 28 n + n / 256 + 4096 bytes
struct UniqueRowsLayout {
    size_t status, keys, keys_tmp, pos, pos_tmp, offsets, bytes;
};
inline UniqueRowsLayout unique_rows_layout(uint32_t n) {
    UniqueRowsLayout L{};
    if (n == 0u) return L;
    const size_t kb = rle_up(static_cast<size_t>(n) * 8u), vb = rle_up(static_cast<size_t>(n) * 4u);
    L.keys = rle_status_bytes(n);
    L.keys_tmp = L.keys + kb;
    L.pos = L.keys_tmp + kb;
    L.pos_tmp = L.pos + vb;
    L.offsets = L.pos_tmp + vb;
    L.bytes = L.offsets + rle_up((static_cast<size_t>(n) + 1u) * 4u);
    return L;
}
// the encode's row form: the status block and always the offsets area (used when the caller passes no out_offsets):
// at most 4 n + n / 256 + 2048 bytes
inline RleLayout rle_rows_layout(uint32_t n) { return rle_layout(n, kRleCounts); }

struct RleRowArgs {
    RleArgs a;            // a.keys: the top group's sorted keys (unique) or null (the encode); a.key_bytes: their width (the encode: 8);
                          // a.idx: the sorted positions when an inverse is wanted; a.out_keys: n x cols words for the R rows, or null;
                          // a.out_offsets: never null (the caller's or the scratch's)
    const void *rows;     // the n x cols input words, row-major
    const uint32_t *pos;  // unique: the sorted positions (the stable lexicographic argsort); the encode: null
    uint32_t cols, word;  // word: 4 or 8
    uint32_t c0;          // the columns [c0, cols) lie behind the top key
};

// one round's keys: keys[i] = pack(rank(x[p, c]) for c in group g), p = i in round 0 (pos[i] = i is written) and pos[i] afterwards
hipError_t launch_rows_pack(hipStream_t stream, const void *rows, uint32_t n, uint32_t cols, uint32_t word, int key_type, uint32_t g, void *keys,
                            uint32_t *pos);
// the encode over rows, the counts from the offsets (a.out_counts) and the R rows gathered into a.out_keys; n > 0
hipError_t launch_rle_rows(hipStream_t stream, const RleRowArgs &r);

}  // namespace vrs
