// vrs_compact.hip -- ordered stream compaction for gfx950 (wave64): keep the elements whose flag is nonzero, in input order.
// Three phases, none of which waits for memory another workgroup writes:
//   count    one workgroup per tile of T elements: 16-byte loads, the predicate's bits per lane, popcounts, one uint32 per tile
//   carries  one workgroup: the exclusive scan of the tiles' counts in place, kCompactCarryBlock of them per step; the total R
//   emit     one workgroup per tile again: the flags read a second time, every survivor's rank inside a chunk of 4096 elements (inside a
//            lane's vector, across the lanes of a wave, across waves and rounds through LDS), the survivors' positions staged in LDS in
//            output order, then dense stores -- consecutive lanes write consecutive output words.  The scatter form stages every
//            element's source index instead and writes all n outputs.
//   rows     the row form's emit (a flag stands for a row of W >= 2 elements): kernels of their own over (tiles, slices) that rank and
//            stage the same way and then copy a chunk's rows as one contiguous span of words.
// The rules (predicate, tiles, coordinates): vrs_compact_order.hpp.
#include "vrs_compact.hpp"

namespace vrs {
namespace {

constexpr uint32_t kNone = 0xffffffffu;  // scatter form: "this element keeps its input" (a source index is at most 2^32 - 2)

template <int BYTES>
struct CompactWord;
template <>
struct CompactWord<1> { using type = uint8_t; };
template <>
struct CompactWord<2> { using type = uint16_t; };
template <>
struct CompactWord<4> { using type = uint32_t; };
template <>
struct CompactWord<8> { using type = uint64_t; };

// The predicate's bits of the 16 / BYTES elements from e0 on (a multiple of 16 / BYTES): bit k = element e0 + k is nonzero.  One 16-byte
// load where the array starts on a 16-byte boundary and the vector lies inside it; single elements at an array's end or off the boundary.
template <int BYTES>
__device__ inline uint32_t vector_mask(const char *flags, bool aligned16, uint64_t e0, uint64_t n, uint64_t keep) {
    constexpr uint32_t EPV = 16u / BYTES;
    using W = typename CompactWord<BYTES>::type;
    uint32_t mask = 0u;
    if (e0 >= n) return mask;
    if (aligned16 && e0 + EPV <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(flags + e0 * BYTES);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t k = 0; k < EPV; ++k) {
            uint64_t bits;
            if constexpr (BYTES == 8) bits = w[2u * k] | (static_cast<uint64_t>(w[2u * k + 1u]) << 32);
            else if constexpr (BYTES == 4) bits = w[k];
            else if constexpr (BYTES == 2) bits = (w[k / 2u] >> (16u * (k & 1u))) & 0xffffu;
            else bits = (w[k / 4u] >> (8u * (k & 3u))) & 0xffu;
            mask |= static_cast<uint32_t>(compact_nonzero(bits, keep)) << k;
        }
    } else {
        const W *p = reinterpret_cast<const W *>(flags);
#pragma unroll
        for (uint32_t k = 0; k < EPV; ++k)
            if (e0 + k < n) mask |= static_cast<uint32_t>(compact_nonzero(p[e0 + k], keep)) << k;
    }
    return mask;
}

__device__ inline uint32_t wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint32_t o = __shfl_up(v, s);
        if (lane >= s) v += o;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------- count

template <int BYTES>
__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const char *flags, uint64_t n, uint32_t T, uint64_t keep, uint32_t *counts) {
    constexpr uint32_t EPV = 16u / BYTES;
    __shared__ uint32_t partial[kCompactThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * T;
    const bool aligned16 = (reinterpret_cast<uintptr_t>(flags) & 15u) == 0u;
    uint32_t c = 0u;
#pragma unroll 4
    for (uint32_t v = tid; v < T / EPV; v += kCompactThreads) c += __popc(vector_mask<BYTES>(flags, aligned16, base + static_cast<uint64_t>(v) * EPV, n, keep));
    c = wave_inclusive(c, tid & 63u);
    if ((tid & 63u) == 63u) partial[tid >> 6] = c;
    __syncthreads();
    if (tid == 0u) counts[blockIdx.x] = partial[0] + partial[1] + partial[2] + partial[3];
}

// ---------------------------------------------------------------------------------------------- carries

__global__ __launch_bounds__(kCompactCarryThreads) void compact_carries_kernel(uint32_t *words, uint32_t tiles, unsigned long long *total, long long *out_count) {
    __shared__ uint32_t wave_total[kCompactCarryThreads / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0u;  // (R <= n < 2^32)
    for (uint32_t b = 0u; b < tiles; b += kCompactCarryBlock) {  // (tiles <= 2^20: b never wraps)
        const uint32_t i = b + 4u * tid;
        uint32_t a[4] = {0u, 0u, 0u, 0u};
        if (i + 4u <= tiles) {
            const uint4 q = *reinterpret_cast<const uint4 *>(words + i);
            a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
        } else {
            for (uint32_t k = 0u; k < 4u; ++k)
                if (i + k < tiles) a[k] = words[i + k];
        }
        const uint32_t mine = a[0] + a[1] + a[2] + a[3];
        const uint32_t incl = wave_inclusive(mine, lane);
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t w = 0u; w < kCompactCarryThreads / 64u; ++w) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        uint32_t at = carry + before + incl - mine;
        if (i + 4u <= tiles) {
            uint4 q;
            q.x = at, q.y = at + a[0], q.z = at + a[0] + a[1], q.w = at + a[0] + a[1] + a[2];
            *reinterpret_cast<uint4 *>(words + i) = q;
        } else {
            for (uint32_t k = 0u; k < 4u; ++k) {
                if (i + k < tiles) words[i + k] = at;
                at += a[k];
            }
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0u) {
        *total = carry;
        if (out_count) *out_count = static_cast<long long>(carry);
    }
}

// ---------------------------------------------------------------------------------------------- emit

// One chunk of kCompactChunk elements from cbase on: lane `tid` takes, in round r, the vector of 16 / BYTES elements at
// cbase + r * 256 * (16 / BYTES) + tid * (16 / BYTES).  mask[r] = its predicate bits; slot[r] = the survivors of the chunk in front of that
// vector, in input order (rounds, then waves, then lanes).  Answers the chunk's survivors.  Ends behind a barrier; the caller puts
// another barrier in front of the next call (wave_total is read until then).
template <int BYTES>
__device__ inline uint32_t rank_chunk(const char *flags, bool aligned16, uint64_t cbase, uint64_t n, uint64_t keep, uint32_t (*wave_total)[kCompactThreads / 64u],
                                      uint32_t (&mask)[BYTES], uint32_t (&slot)[BYTES]) {
    constexpr uint32_t EPV = 16u / BYTES;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < BYTES; ++r)
        mask[r] = vector_mask<BYTES>(flags, aligned16, cbase + static_cast<uint64_t>(r) * (kCompactThreads * EPV) + tid * EPV, n, keep);
#pragma unroll
    for (int r = 0; r < BYTES; ++r) {
        const uint32_t c = __popc(mask[r]), incl = wave_inclusive(c, lane);
        slot[r] = incl - c;
        if (lane == 63u) wave_total[r][wave] = incl;
    }
    __syncthreads();
    uint32_t acc = 0u;
#pragma unroll
    for (int r = 0; r < BYTES; ++r) {
#pragma unroll
        for (uint32_t w = 0u; w < kCompactThreads / 64u; ++w) {
            if (w == wave) slot[r] += acc;
            acc += wave_total[r][w];
        }
    }
    return acc;
}

__device__ inline void copy_element(void *dst, uint64_t to, const void *src, uint64_t from, uint32_t value_bytes) {
    switch (value_bytes) {
        case 1u: static_cast<uint8_t *>(dst)[to] = static_cast<const uint8_t *>(src)[from]; break;
        case 2u: static_cast<uint16_t *>(dst)[to] = static_cast<const uint16_t *>(src)[from]; break;
        case 4u: static_cast<uint32_t *>(dst)[to] = static_cast<const uint32_t *>(src)[from]; break;
        default: static_cast<uint64_t *>(dst)[to] = static_cast<const uint64_t *>(src)[from]; break;
    }
}

struct TileSpan {
    uint32_t first, count;  // the tile's first output row and its survivors
};
__device__ inline TileSpan tile_span(const char *scratch, uint32_t tile, uint32_t tiles) {
    const uint32_t *offsets = reinterpret_cast<const uint32_t *>(scratch + kCompactHeaderBytes);
    const uint32_t first = offsets[tile];
    const uint32_t next = tile + 1u < tiles ? offsets[tile + 1u] : static_cast<uint32_t>(*reinterpret_cast<const unsigned long long *>(scratch));
    return {first, next - first};
}

// flat positions, coordinates and gathered values of the survivors
template <int BYTES>
__global__ __launch_bounds__(kCompactThreads) void compact_emit_kernel(CompactEmitArgs a, uint64_t keep, uint32_t tiles, CompactDiv by_ndim) {
    constexpr uint32_t EPV = 16u / BYTES;
    __shared__ uint32_t stage[kCompactChunk];
    __shared__ uint32_t wave_total[BYTES][kCompactThreads / 64u];
    __shared__ CompactShape shape;
    const uint32_t tid = threadIdx.x;
    const TileSpan span = tile_span(a.scratch, blockIdx.x, tiles);
    if (span.count == 0u) return;  // (the same in every lane: nothing of this tile survives, its flags are not read again)
    if (tid == 0u) shape = a.shape;
    const char *flags = static_cast<const char *>(a.flags);
    const bool aligned16 = (reinterpret_cast<uintptr_t>(flags) & 15u) == 0u;
    const uint64_t tbase = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint32_t ndim = a.shape.ndim;
    uint32_t done = 0u;  // survivors of this tile's earlier chunks
    for (uint32_t c = 0u; c < a.T && done < span.count; c += kCompactChunk) {
        const uint64_t cbase = tbase + c;
        uint32_t mask[BYTES], slot[BYTES];
        const uint32_t total = rank_chunk<BYTES>(flags, aligned16, cbase, a.n, keep, wave_total, mask, slot);
#pragma unroll
        for (int r = 0; r < BYTES; ++r) {
            const uint32_t p0 = static_cast<uint32_t>(cbase + static_cast<uint64_t>(r) * (kCompactThreads * EPV) + tid * EPV);  // (a position is < 2^32)
            uint32_t m = mask[r], at = slot[r];
            while (m) {
                stage[at++] = p0 + static_cast<uint32_t>(__ffs(m) - 1);
                m &= m - 1u;
            }
        }
        __syncthreads();
        const uint64_t row0 = static_cast<uint64_t>(span.first) + done;
        for (uint32_t j = tid; j < total; j += kCompactThreads) {
            const uint64_t row = row0 + j;
            if (row >= a.limit) break;
            const uint32_t p = stage[j];
            if (a.flat) a.flat[row] = static_cast<int64_t>(p);
            if (a.coords && a.coords_layout == kCompactColumns)
                for (uint32_t k = 0u; k < ndim; ++k) a.coords[static_cast<uint64_t>(k) * a.limit + row] = static_cast<int64_t>(compact_coordinate(p, shape, k));
            if (a.gather_out) copy_element(a.gather_out, row, a.gather_values, p, a.value_bytes);
        }
        if (a.coords && a.coords_layout == kCompactRows) {
            // [R, ndim]: one lane per output word, so that a wave's store is 512 consecutive bytes whatever ndim is
            for (uint32_t e = tid; e < total * ndim; e += kCompactThreads) {
                const uint32_t j = compact_div(e, by_ndim), k = e - j * ndim;
                const uint64_t row = row0 + j;
                if (row >= a.limit) break;
                a.coords[row * ndim + k] = static_cast<int64_t>(compact_coordinate(stage[j], shape, k));
            }
        }
        done += total;
        __syncthreads();
    }
}

// out[i] = flag[i] ? source[rank(i)] : input[i], rank(i) the set flags in front of i
template <int BYTES>
__global__ __launch_bounds__(kCompactThreads) void compact_scatter_kernel(CompactEmitArgs a, uint64_t keep, uint32_t tiles) {
    constexpr uint32_t EPV = 16u / BYTES;
    __shared__ uint32_t stage[kCompactChunk];
    __shared__ uint32_t wave_total[BYTES][kCompactThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const TileSpan span = tile_span(a.scratch, blockIdx.x, tiles);
    const char *flags = static_cast<const char *>(a.flags);
    const bool aligned16 = (reinterpret_cast<uintptr_t>(flags) & 15u) == 0u;
    const uint64_t tbase = static_cast<uint64_t>(blockIdx.x) * a.T;
    uint32_t done = 0u;
    for (uint32_t c = 0u; c < a.T; c += kCompactChunk) {
        const uint64_t cbase = tbase + c;
        if (cbase >= a.n) break;
        uint32_t mask[BYTES], slot[BYTES];
        const uint32_t total = rank_chunk<BYTES>(flags, aligned16, cbase, a.n, keep, wave_total, mask, slot);
#pragma unroll
        for (int r = 0; r < BYTES; ++r) {
            const uint32_t at = static_cast<uint32_t>(r) * (kCompactThreads * EPV) + tid * EPV;
            uint32_t rank = span.first + done + slot[r];
#pragma unroll
            for (uint32_t k = 0u; k < EPV; ++k) {
                const bool set = (mask[r] >> k) & 1u;
                stage[at + k] = set ? rank : kNone;
                rank += set ? 1u : 0u;
            }
        }
        __syncthreads();
        const uint64_t left = a.n - cbase;
        const uint32_t len = left < kCompactChunk ? static_cast<uint32_t>(left) : kCompactChunk;
        for (uint32_t j = tid; j < len; j += kCompactThreads) {
            const uint32_t s = stage[j];
            if (s != kNone && s < a.limit) copy_element(a.scatter_out, cbase + j, a.scatter_source, s, a.value_bytes);
            else copy_element(a.scatter_out, cbase + j, a.scatter_input, cbase + j, a.value_bytes);
        }
        done += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- rows

// The row form (row_elems = W >= 2): a flag stands for a row of row_bytes bytes, and what a chunk writes is one contiguous span of bytes
// -- its survivors' rows (gather), or all of its rows (scatter).  Consecutive lanes take consecutive words of the span, so stores are
// dense whatever the mask is, and loads are dense inside every row.  The word: compact_row_word_bytes.
struct CompactRowArgs {
    uint64_t row_bytes, words_per_row, slice_bytes;
    CompactDiv by_words;  // words_per_row as a divisor, for rows of at most kCompactRowNarrowWords words
    uint32_t word_bytes, pad;
};

CompactRowArgs compact_row_args(const CompactEmitArgs &a, const CompactRowForm &form, uint64_t bases) {
    CompactRowArgs r{};
    r.row_bytes = static_cast<uint64_t>(form.row_elems) * a.value_bytes;
    r.word_bytes = compact_row_word_bytes(r.row_bytes, bases);
    r.words_per_row = r.row_bytes / r.word_bytes;
    r.by_words = compact_div_make(r.words_per_row <= kCompactRowNarrowWords ? static_cast<uint32_t>(r.words_per_row) : 1u);
    r.slice_bytes = form.slice_bytes ? form.slice_bytes : kCompactRowSliceBytes;
    return r;
}

// dst[e] = *src_of(e) for the words e = first, first + stride, ... below `words`; four loads of a lane are in flight before its stores
template <class W, class Src>
__device__ inline void copy_words(W *dst, uint64_t words, uint64_t first, uint64_t stride, Src src_of) {
    uint64_t e = first;
    for (; e + 3u * stride < words; e += 4u * stride) {
        const uint64_t e1 = e + stride, e2 = e1 + stride, e3 = e2 + stride;
        const W v0 = *src_of(e), v1 = *src_of(e1), v2 = *src_of(e2), v3 = *src_of(e3);
        dst[e] = v0, dst[e1] = v1, dst[e2] = v2, dst[e3] = v3;
    }
    for (; e < words; e += stride) dst[e] = *src_of(e);
}

// `rows` rows from dst on, row j copied from row_of(j): as one span of rows x words_per_row words cut by the constant division while that
// index fits 32 bits, row by row with a 64-bit word index for wider rows.  This workgroup's lanes take the words first + k x stride.
template <class W, class Row>
__device__ inline void copy_rows(char *dst, uint32_t rows, const CompactRowArgs &r, uint64_t first, uint64_t stride, Row row_of) {
    if (r.words_per_row <= kCompactRowNarrowWords) {
        const uint32_t wpr = static_cast<uint32_t>(r.words_per_row);
        copy_words(reinterpret_cast<W *>(dst), static_cast<uint64_t>(rows) * wpr, first, stride, [&](uint64_t e) {  // (at most 2^32 words: e < 2^32)
            const uint32_t j = compact_div(static_cast<uint32_t>(e), r.by_words), w = static_cast<uint32_t>(e) - j * wpr;
            return reinterpret_cast<const W *>(row_of(j)) + w;
        });
    } else {
        for (uint32_t j = 0u; j < rows; ++j) {
            const W *src = reinterpret_cast<const W *>(row_of(j));
            copy_words(reinterpret_cast<W *>(dst + j * r.row_bytes), r.words_per_row, first, stride, [&](uint64_t w) { return src + w; });
        }
    }
}

template <class Row>
__device__ inline void copy_rows_as(char *dst, uint32_t rows, const CompactRowArgs &r, uint64_t first, uint64_t stride, Row row_of) {
    switch (r.word_bytes) {
        case 16u: copy_rows<uint4>(dst, rows, r, first, stride, row_of); break;
        case 8u: copy_rows<uint64_t>(dst, rows, r, first, stride, row_of); break;
        case 4u: copy_rows<uint32_t>(dst, rows, r, first, stride, row_of); break;
        case 2u: copy_rows<uint16_t>(dst, rows, r, first, stride, row_of); break;
        default: copy_rows<uint8_t>(dst, rows, r, first, stride, row_of); break;
    }
}

// gather_out row r = gather_values row position(r).  Grid (tiles, slices); a tile without survivors is skipped, and so are the slices
// its survivors do not need (a sparse tile moves few bytes, and every slice reads the tile's flags).
template <int BYTES>
__global__ __launch_bounds__(kCompactThreads) void compact_gather_rows_kernel(CompactEmitArgs a, CompactRowArgs r, uint64_t keep, uint32_t tiles) {
    constexpr uint32_t EPV = 16u / BYTES;
    __shared__ uint32_t stage[kCompactChunk];
    __shared__ uint32_t wave_total[BYTES][kCompactThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const TileSpan span = tile_span(a.scratch, blockIdx.x, tiles);
    if (span.count == 0u) return;
    const uint32_t want = compact_row_slices_for(span.count, r.row_bytes, r.slice_bytes), slices = want < gridDim.y ? want : gridDim.y;
    if (blockIdx.y >= slices) return;  // (the same in every lane)
    const uint64_t first = static_cast<uint64_t>(blockIdx.y) * kCompactThreads + tid, stride = static_cast<uint64_t>(slices) * kCompactThreads;
    const char *flags = static_cast<const char *>(a.flags), *values = static_cast<const char *>(a.gather_values);
    const bool aligned16 = (reinterpret_cast<uintptr_t>(flags) & 15u) == 0u;
    const uint64_t tbase = static_cast<uint64_t>(blockIdx.x) * a.T;
    uint32_t done = 0u;
    for (uint32_t c = 0u; c < a.T && done < span.count; c += kCompactChunk) {
        const uint64_t cbase = tbase + c;
        uint32_t mask[BYTES], slot[BYTES];
        const uint32_t total = rank_chunk<BYTES>(flags, aligned16, cbase, a.n, keep, wave_total, mask, slot);
#pragma unroll
        for (int k = 0; k < BYTES; ++k) {
            const uint32_t p0 = static_cast<uint32_t>(cbase + static_cast<uint64_t>(k) * (kCompactThreads * EPV) + tid * EPV);
            uint32_t m = mask[k], at = slot[k];
            while (m) {
                stage[at++] = p0 + static_cast<uint32_t>(__ffs(m) - 1);
                m &= m - 1u;
            }
        }
        __syncthreads();
        const uint64_t row0 = static_cast<uint64_t>(span.first) + done;
        if (row0 < a.limit) {  // (no output row from limit on is written)
            const uint64_t room = a.limit - row0;
            const uint32_t rows = room < total ? static_cast<uint32_t>(room) : total;
            copy_rows_as(static_cast<char *>(a.gather_out) + row0 * r.row_bytes, rows, r, first, stride,
                         [&](uint32_t j) { return values + stage[j] * r.row_bytes; });
        }
        done += total;
        __syncthreads();
    }
}

// scatter_out row i = flag[i] ? scatter_source row rank(i) : scatter_input row i.  Grid (tiles, slices); every slice has work.
template <int BYTES>
__global__ __launch_bounds__(kCompactThreads) void compact_scatter_rows_kernel(CompactEmitArgs a, CompactRowArgs r, uint64_t keep, uint32_t tiles) {
    constexpr uint32_t EPV = 16u / BYTES;
    __shared__ uint32_t stage[kCompactChunk];
    __shared__ uint32_t wave_total[BYTES][kCompactThreads / 64u];
    const uint32_t tid = threadIdx.x;
    const TileSpan span = tile_span(a.scratch, blockIdx.x, tiles);
    const uint64_t first = static_cast<uint64_t>(blockIdx.y) * kCompactThreads + tid, stride = static_cast<uint64_t>(gridDim.y) * kCompactThreads;
    const char *flags = static_cast<const char *>(a.flags), *source = static_cast<const char *>(a.scatter_source);
    const bool aligned16 = (reinterpret_cast<uintptr_t>(flags) & 15u) == 0u;
    const uint64_t tbase = static_cast<uint64_t>(blockIdx.x) * a.T;
    uint32_t done = 0u;
    for (uint32_t c = 0u; c < a.T; c += kCompactChunk) {
        const uint64_t cbase = tbase + c;
        if (cbase >= a.n) break;
        uint32_t mask[BYTES], slot[BYTES];
        const uint32_t total = rank_chunk<BYTES>(flags, aligned16, cbase, a.n, keep, wave_total, mask, slot);
#pragma unroll
        for (int k = 0; k < BYTES; ++k) {
            const uint32_t at = static_cast<uint32_t>(k) * (kCompactThreads * EPV) + tid * EPV;
            uint32_t rank = span.first + done + slot[k];
#pragma unroll
            for (uint32_t b = 0u; b < EPV; ++b) {
                const bool set = (mask[k] >> b) & 1u;
                stage[at + b] = set ? rank : kNone;
                rank += set ? 1u : 0u;
            }
        }
        __syncthreads();
        const uint64_t left = a.n - cbase;
        const uint32_t len = left < kCompactChunk ? static_cast<uint32_t>(left) : kCompactChunk;
        const char *input = static_cast<const char *>(a.scatter_input) + cbase * r.row_bytes;
        copy_rows_as(static_cast<char *>(a.scatter_out) + cbase * r.row_bytes, len, r, first, stride, [&](uint32_t j) {
            const uint32_t s = stage[j];
            return s != kNone && s < a.limit ? source + s * r.row_bytes : input + j * r.row_bytes;  // (no source row from limit on is read)
        });
        done += total;
        __syncthreads();
    }
}

uint64_t address(const void *p) { return reinterpret_cast<uintptr_t>(p); }

template <int BYTES>
hipError_t count_as(hipStream_t stream, const CompactCountArgs &a, uint32_t tiles) {
    uint32_t *words = reinterpret_cast<uint32_t *>(a.scratch + kCompactHeaderBytes);
    hipLaunchKernelGGL(compact_count_kernel<BYTES>, dim3(tiles), dim3(kCompactThreads), 0, stream, static_cast<const char *>(a.flags), a.n, a.T,
                       compact_keep_mask(a.dtype), words);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(compact_carries_kernel, dim3(1), dim3(kCompactCarryThreads), 0, stream, words, tiles, reinterpret_cast<unsigned long long *>(a.scratch),
                       a.out_count);
    return hipGetLastError();
}

template <int BYTES>
hipError_t emit_as(hipStream_t stream, const CompactEmitArgs &a, const CompactRowForm &form, uint32_t tiles) {
    const uint64_t keep = compact_keep_mask(a.dtype);
    const bool rows = form.row_elems >= 2u;
    if (a.flat || a.coords || (a.gather_out && !rows)) {
        CompactEmitArgs e = a;
        if (rows) e.gather_values = nullptr, e.gather_out = nullptr;  // (positions stay per flag; the rows have a kernel of their own)
        hipLaunchKernelGGL(compact_emit_kernel<BYTES>, dim3(tiles), dim3(kCompactThreads), 0, stream, e, keep, tiles, compact_div_make(a.shape.ndim));
        if (const hipError_t e = hipGetLastError()) return e;
    }
    if (a.gather_out && rows) {
        const CompactRowArgs r = compact_row_args(a, form, address(a.gather_values) | address(a.gather_out));
        const uint32_t slices = compact_row_slices_for(a.n < a.T ? a.n : a.T, r.row_bytes, r.slice_bytes);
        hipLaunchKernelGGL(compact_gather_rows_kernel<BYTES>, dim3(tiles, slices), dim3(kCompactThreads), 0, stream, a, r, keep, tiles);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    if (a.scatter_out && rows) {
        const CompactRowArgs r = compact_row_args(a, form, address(a.scatter_input) | address(a.scatter_source) | address(a.scatter_out));
        const uint32_t slices = compact_row_slices_for(a.n < a.T ? a.n : a.T, r.row_bytes, r.slice_bytes);
        hipLaunchKernelGGL(compact_scatter_rows_kernel<BYTES>, dim3(tiles, slices), dim3(kCompactThreads), 0, stream, a, r, keep, tiles);
        if (const hipError_t e = hipGetLastError()) return e;
    } else if (a.scatter_out) {
        hipLaunchKernelGGL(compact_scatter_kernel<BYTES>, dim3(tiles), dim3(kCompactThreads), 0, stream, a, keep, tiles);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_compact_count(hipStream_t stream, const CompactCountArgs &a) {
    const uint32_t tiles = compact_tiles(a.n, a.T);
    switch (compact_dtype_bytes(a.dtype)) {
        case 1: return count_as<1>(stream, a, tiles);
        case 2: return count_as<2>(stream, a, tiles);
        case 4: return count_as<4>(stream, a, tiles);
        default: return count_as<8>(stream, a, tiles);
    }
}

hipError_t launch_compact_emit(hipStream_t stream, const CompactEmitArgs &a, const CompactRowForm &rows) {
    const uint32_t tiles = compact_tiles(a.n, a.T);
    switch (compact_dtype_bytes(a.dtype)) {
        case 1: return emit_as<1>(stream, a, rows, tiles);
        case 2: return emit_as<2>(stream, a, rows, tiles);
        case 4: return emit_as<4>(stream, a, rows, tiles);
        default: return emit_as<8>(stream, a, rows, tiles);
    }
}

}  // namespace vrs
