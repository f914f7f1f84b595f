// vrs_reduce_order.hpp -- THE order of the segmented reduction (vrs_segment_reduce): which rows are combined with which, in what sequence,
// for one segment of L rows and one column.  The kernels (vrs_segreduce.hip) and the host restatement (vrs_segment_reduce_host) compile the
// same functions from here, so that the two agree bit for bit.  Everything below depends on (L, C, dtype, op, CH, LANE_ROWS) alone: never on
// timing, on the grid, on where the segment sits in the buffer or on its neighbours.  Internal.
//
//   reduce(rows[0, L))  = chunk(rows)                                                                   when L <= CH
//                       = reduce([chunk(rows[i * CH, min(L, (i + 1) * CH))) for i = 0 ..])              otherwise
//   chunk(rows) starts every accumulator at the op's identity (sum +0, prod 1, min +inf / the type's maximum, max -inf / the type's minimum)
//   and combines acc = op(acc, row) -- so a sum that is zero is +0.0 whatever the signs of the zeros that went in.
//     lane / columns map: one accumulator, the rows in order.
//     rows map (C < 64, more than LANE_ROWS rows): G = 64 / C' accumulators, C' the power of two at or above C; row t goes to
//       accumulator t mod G, in order; an accumulator without a row keeps the identity, which changes nothing it is combined with; then
//       for s = G / 2, G / 4 .. 1: acc[g] = op(acc[g], acc[g + s]) for g < s, and acc[0] is the answer.
//   The partials are kept in the accumulator type (float32 for float16 / bfloat16 values, the value type otherwise); with an init row the
//   answer is op(init, reduce(rows)), rounded to the value type once; an empty segment answers init's own bits (the identity without init).
#pragma once
#include <cstdint>
#include <limits>
#include <type_traits>

#include "vrs_bincount.hpp"

namespace vrs {

constexpr int kReduceSum = 0, kReduceProd = 1, kReduceMin = 2, kReduceMax = 3;     // vrs_reduce_op
constexpr int kReduceMapLane = 0, kReduceMapRows = 1, kReduceMapColumns = 2;       // vrs_reduce_map
constexpr uint32_t kReduceWave = 64u;                                              // columns from which lanes run across columns
constexpr uint32_t kReduceChunkMin = 64u, kReduceChunkMax = 4096u, kReduceChunkDefault = 512u;  // VRS_TUNE_REDUCE_CHUNK_ROWS
constexpr uint32_t kReduceLaneRowsMax = 64u, kReduceLaneRowsDefault = 16u;                      // VRS_TUNE_REDUCE_LANE_ROWS
constexpr uint32_t kReduceMaxLevels = 8u;  // (64^6 > 2^32: six levels at the most)

__host__ __device__ inline bool reduce_op_known(int op) { return op >= kReduceSum && op <= kReduceMax; }
__host__ __device__ inline bool reduce_dtype_known(int dtype) { return dtype == kSortI32 || dtype == kSortI64 || (dtype >= kSortF16 && dtype <= kSortF64); }

// the lane map of a chunk of `len` rows of C columns
__host__ __device__ inline int reduce_map(uint32_t len, uint32_t C, uint32_t lane_rows) {
    return C >= kReduceWave ? kReduceMapColumns : len <= lane_rows ? kReduceMapLane : kReduceMapRows;
}
// C' and G of the rows map (C < 64)
__host__ __device__ inline uint32_t reduce_padded_width(uint32_t C) {
    uint32_t p = 1u;
    while (p < C) p <<= 1;
    return p;
}
__host__ __device__ inline uint32_t reduce_groups(uint32_t C) { return kReduceWave / reduce_padded_width(C); }
// chunks of a list of `len` rows (an empty list is one chunk without rows) / levels until one chunk is left
__host__ __device__ inline uint32_t reduce_chunks(uint32_t len, uint32_t CH) { return len <= CH ? 1u : static_cast<uint32_t>((static_cast<uint64_t>(len) + CH - 1u) / CH); }
__host__ __device__ inline uint32_t reduce_levels(uint32_t len, uint32_t CH) {
    uint32_t levels = 1u;
    while (len > CH) {
        len = reduce_chunks(len, CH);
        ++levels;
    }
    return levels;
}

template <typename A>
__host__ __device__ inline A reduce_identity(int op) {
    if constexpr (std::is_floating_point<A>::value) {
        const A inf = static_cast<A>(__builtin_huge_val());
        return op == kReduceSum ? static_cast<A>(0) : op == kReduceProd ? static_cast<A>(1) : op == kReduceMin ? inf : -inf;
    } else {
        return op == kReduceSum ? static_cast<A>(0) : op == kReduceProd ? static_cast<A>(1)
               : op == kReduceMin ? std::numeric_limits<A>::max() : std::numeric_limits<A>::min();
    }
}

// op(a, b): min and max answer NaN when either side is one (a's first); integer sums and products wrap
template <typename A>
__host__ __device__ inline A reduce_combine(int op, A a, A b) {
    if constexpr (std::is_floating_point<A>::value) {
        switch (op) {
            case kReduceSum: return a + b;
            case kReduceProd: return a * b;
            case kReduceMin: return a != a ? a : b != b ? b : b < a ? b : a;
            default: return a != a ? a : b != b ? b : b > a ? b : a;
        }
    } else {
        using U = typename std::make_unsigned<A>::type;
        switch (op) {
            case kReduceSum: return static_cast<A>(static_cast<U>(a) + static_cast<U>(b));
            case kReduceProd: return static_cast<A>(static_cast<U>(a) * static_cast<U>(b));
            case kReduceMin: return b < a ? b : a;
            default: return b > a ? b : a;
        }
    }
}

// float32 to the 16 bits of a float16 / bfloat16, round to nearest even (integer arithmetic: the same bits on the host and the device)
__host__ __device__ inline uint16_t reduce_narrow_f16(float f) {
    uint32_t x = __builtin_bit_cast(uint32_t, f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return static_cast<uint16_t>(sign | 0x7E00u);   // NaN
    if (x >= 0x477FF000u) return static_cast<uint16_t>(sign | 0x7C00u);  // 65520 and beyond round to inf
    if (x < 0x38800000u) {                                               // below 2^-14: a float16 subnormal, in units of 2^-24
        if (x < 0x33000000u) return static_cast<uint16_t>(sign);         // below 2^-25
        const uint32_t shift = 126u - (x >> 23), m = (x & 0x7FFFFFu) | 0x800000u;
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (q & 1u))) ++q;
        return static_cast<uint16_t>(sign | q);
    }
    x += 0xFFFu + ((x >> 13) & 1u);
    return static_cast<uint16_t>(sign | ((x - 0x38000000u) >> 13));
}
__host__ __device__ inline uint16_t reduce_narrow_bf16(float f) {
    uint32_t x = __builtin_bit_cast(uint32_t, f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<uint16_t>((x >> 16) | 0x0040u);  // NaN stays one
    x += 0x7FFFu + ((x >> 16) & 1u);
    return static_cast<uint16_t>(x >> 16);
}

// How a dtype is stored (S) and accumulated (A).
struct ReduceI32 { using S = int32_t; using A = int32_t; };
struct ReduceI64 { using S = int64_t; using A = int64_t; };
struct ReduceF16 { using S = uint16_t; using A = float; };
struct ReduceBF16 { using S = uint16_t; using A = float; };
struct ReduceF32 { using S = float; using A = float; };
struct ReduceF64 { using S = double; using A = double; };

template <typename T>
__host__ __device__ inline typename T::A reduce_widen(typename T::S s) {
    if constexpr (std::is_same<T, ReduceF16>::value) return bin_widen_f16(s);
    else if constexpr (std::is_same<T, ReduceBF16>::value) return bin_widen_bf16(s);
    else return s;
}
template <typename T>
__host__ __device__ inline typename T::S reduce_narrow(typename T::A a) {
    if constexpr (std::is_same<T, ReduceF16>::value) return reduce_narrow_f16(a);
    else if constexpr (std::is_same<T, ReduceBF16>::value) return reduce_narrow_bf16(a);
    else return a;
}

// chunk(rows) of one column: row(t) is row t of the chunk in the accumulator type
template <typename A, typename Row>
__host__ __device__ inline A reduce_chunk(int op, uint32_t len, uint32_t C, uint32_t lane_rows, Row row) {
    const A identity = reduce_identity<A>(op);
    if (reduce_map(len, C, lane_rows) != kReduceMapRows) {
        A acc = identity;
        for (uint32_t t = 0; t < len; ++t) acc = reduce_combine(op, acc, row(t));
        return acc;
    }
    const uint32_t G = reduce_groups(C);
    A acc[kReduceWave];
    for (uint32_t g = 0; g < G; ++g) {
        acc[g] = identity;
        for (uint32_t t = g; t < len; t += G) acc[g] = reduce_combine(op, acc[g], row(t));
    }
    for (uint32_t s = G / 2u; s >= 1u; s >>= 1)
        for (uint32_t g = 0; g < s; ++g) acc[g] = reduce_combine(op, acc[g], acc[g + s]);
    return acc[0];
}

}  // namespace vrs
