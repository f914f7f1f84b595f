// vrs_scan_order.hpp -- THE order of the prefix scan over rows (vrs_scan_rows): which rows are combined with which, in what sequence, for
// one segment of L rows and one column.  The kernels (vrs_scan.hip) and the host restatement (vrs_scan_rows_host) compile the functions
// below, so that the two agree bit for bit.  Everything here depends on (L, C, dtype, op, T) alone: never on timing, on the grid, on S or
// on where the segment lies.  Internal.
//
//   A segment is cut into tiles of T rows (VRS_TUNE_SCAN_TILE_ROWS, a multiple of 256); F = 64; (+) is the op's combine; every fold below
//   is LEFT TO RIGHT and starts at the op's identity:  fold(x_0 .. x_n) = (((identity (+) x_0) (+) x_1) ..) (+) x_n.
//     A(0)_j  = the aggregate of tile j by the in-tile order
//     A(k)_m  = fold(A(k-1)_{mF} .. A(k-1)_{mF+F-1})                        (complete groups only: nothing reads another)
//     P_j     = fold of, for k from the top level down to 0, A(k)_m for m in [F * floor(j / F^(k+1)), floor(j / F^k))
//     out[i]  = P_j (+) incl_j(i)        for L > T;     out[i] = incl_0(i)   for L <= T (P_0 is the identity, which changes no bit)
//   The in-tile order has two maps.  A row beyond the tile's end counts as the identity, which changes no accumulator's bits.
//     flat map (C == 1): chunks of 256 rows; lane l of 64 holds rows 256 q + 4 l + k, k = 0 .. 3, of chunk q
//         a_l = fold(x_0 .. x_3);  I = a;  for d = 1, 2, 4 .. 32: I_l = I_{l-d} (+) I_l for l >= d, all lanes at once
//         E_l = I_{l-1} (the identity for l = 0);  G_q = I_63;  Q_0 = identity, Q_{q+1} = Q_q (+) G_q
//         incl(256 q + 4 l + k) = ((Q_q (+) E_l) (+) x_0) .. (+) x_k;   A(0) = Q after the last chunk
//     columns map (C > 1): runs of 16 rows; local_r = fold of the run's rows up to r; g_q = local at the run's end;
//         Q_0 = identity, Q_{q+1} = Q_q (+) g_q;  incl(r) = Q_q (+) local_r;  A(0) = Q after the last run
//   Accumulators: float32 for float16 and bfloat16 sums and products, rounded to the value type once per output; the output type
//   otherwise; integers wrap.  A float sum starts at +0.0, so no accumulator is ever -0.0 and cumsum([-0.0]) is +0.0.
//   MAX and MIN combine (value, row) pairs by torch's CPU rule -- a NaN on the right always replaces; a non-NaN on the right replaces a
//   non-NaN on the left when it is >= (MIN: <=) -- which is associative and exact: any tiling gives torch's bits.  Their identity is
//   the pair without a row (row -1).
#pragma once
#include <cstdint>
#include <type_traits>
#include <vector>

#include "vrs_reduce_order.hpp"

namespace vrs {

constexpr int kScanSum = 0, kScanProd = 1, kScanMax = 2, kScanMin = 3;                  // vrs_scan_op
constexpr int kScanTierTile = 0, kScanTierThreeLaunch = 1, kScanTierSinglePass = 2;     // vrs_scan_tier
constexpr uint32_t kScanFan = 64u, kScanFanBits = 6u;                                   // F
constexpr uint32_t kScanLaneRows = 4u, kScanChunk = 64u * kScanLaneRows;                // flat map: rows per lane and per chunk
constexpr uint32_t kScanRun = 16u;                                                      // columns map: rows per run
constexpr uint32_t kScanMaxLevels = 4u;                                                 // (64^4 tiles of 256 rows = 2^32 rows)
constexpr uint32_t kScanTileMin = 256u, kScanTileMax = 8192u, kScanTileDefault = 2048u; // VRS_TUNE_SCAN_TILE_ROWS
constexpr uint32_t kScanSinglePassMinRowsDefault = 1u << 20;                            // VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS
constexpr uint32_t kScanSpinBudgetDefault = 4096u, kScanSpinBudgetMax = 1u << 20;       // VRS_TUNE_SCAN_SPIN_BUDGET

__host__ __device__ inline bool scan_op_known(int op) { return op >= kScanSum && op <= kScanMin; }
__host__ __device__ inline bool scan_tile_rows_known(uint32_t T) { return T >= kScanTileMin && T <= kScanTileMax && T % kScanChunk == 0u; }
// the (dtype, out_dtype, op) triples the call takes
__host__ __device__ inline bool scan_kind_known(int dtype, int out_dtype, int op) {
    if (!scan_op_known(op) || dtype < kSortI8 || dtype > kSortF64) return false;
    if (op >= kScanMax) return out_dtype == dtype;
    if (!reduce_dtype_known(out_dtype)) return false;
    return dtype == out_dtype || (out_dtype == kSortI64 && (dtype == kSortI8 || dtype == kSortU8 || dtype == kSortI16 || dtype == kSortI32));
}
// bytes of one accumulator in scratch: a (value, row) pair takes 16
__host__ __device__ inline uint32_t scan_acc_bytes(int out_dtype, int op) { return op >= kScanMax ? 16u : sort_dtype_bytes(out_dtype) == 8 ? 8u : 4u; }

__host__ __device__ inline uint32_t scan_tiles(uint32_t L, uint32_t T) { return static_cast<uint32_t>((static_cast<uint64_t>(L) + T - 1u) / T); }
// levels of aggregates above the rows: 0 for one tile, 1 up to F tiles, one more per factor of F
__host__ __device__ inline uint32_t scan_levels(uint32_t L, uint32_t T) {
    const uint64_t tiles = scan_tiles(L, T);
    if (tiles <= 1u) return 0u;
    uint32_t K = 1u;
    for (uint64_t cap = kScanFan; cap < tiles; cap *= kScanFan) ++K;
    return K;
}
// words of level k that exist for `tiles` tiles (the last group may be short: its A(k) is never read, but has a place)
__host__ __device__ inline uint32_t scan_level_words(uint32_t tiles, uint32_t k) {
    return static_cast<uint32_t>((static_cast<uint64_t>(tiles) + (1ull << (kScanFanBits * k)) - 1u) >> (kScanFanBits * k));
}
// the longest chain of combines behind any output of a segment of L rows (combines with the identity counted)
__host__ __device__ inline uint32_t scan_depth(uint32_t L, uint32_t C, uint32_t T) {
    if (L == 0u) return 0u;
    const uint32_t n = L < T ? L : T, K = scan_levels(L, T);
    uint32_t aggregate, incl;
    if (C == 1u) {
        const uint32_t chunks = (n + kScanChunk - 1u) / kScanChunk;
        aggregate = kScanLaneRows + kScanFanBits + chunks;  // a_l, the six steps, Q
        incl = aggregate + 1u + kScanLaneRows;              // Q (+) E, then the lane's rows
    } else {
        const uint32_t runs = (n + kScanRun - 1u) / kScanRun;
        aggregate = kScanRun + runs;
        incl = aggregate + 1u;
    }
    if (K == 0u) return incl;
    const uint32_t prefix = aggregate + kScanFan * (K - 1u) + (kScanFan - 1u) * K;  // the first word of the top level, through every fold
    return (prefix > incl ? prefix : incl) + 1u;
}
// which tier runs (S, L, C, dtype -> out_dtype, op): a pure function of these and the two knobs
__host__ __device__ inline int scan_tier(uint32_t S, uint32_t L, uint32_t C, int out_dtype, int op, uint32_t T, uint32_t single_pass_min_rows) {
    if (L <= T) return kScanTierTile;
    const bool word = op <= kScanProd && (out_dtype == kSortI32 || out_dtype == kSortF16 || out_dtype == kSortBF16 || out_dtype == kSortF32);
    if (C == 1u && word && single_pass_min_rows != 0u && static_cast<uint64_t>(S) * L >= single_pass_min_rows) return kScanTierSinglePass;
    return kScanTierThreeLaunch;
}

// ---------------------------------------------------------------------------------------------- the algebras
// X::In, X::Out: how a row is stored on the way in and out; X::Acc: what is combined.

template <typename T, typename In_>
struct ScanArith {  // SUM and PROD; T: a Reduce* of vrs_reduce_order.hpp for the output dtype
    using In = In_;
    using Out = typename T::S;
    using Acc = typename T::A;
    static constexpr bool kPairs = false;
    __host__ __device__ static Acc identity(int op) { return reduce_identity<Acc>(op); }
    __host__ __device__ static Acc load(In v, int64_t) {
        if constexpr (std::is_same<In, Out>::value) return reduce_widen<T>(v);
        else return static_cast<Acc>(v);  // the widening load: int8, uint8, int16, int32 rows into int64
    }
    __host__ __device__ static Acc combine(int op, Acc a, Acc b) {  // (reduce_combine's sum and product, without its other two ops)
        if constexpr (std::is_floating_point<Acc>::value) {
            return op == kScanSum ? a + b : a * b;
        } else {
            using U = typename std::make_unsigned<Acc>::type;
            return static_cast<Acc>(op == kScanSum ? static_cast<U>(a) + static_cast<U>(b) : static_cast<U>(a) * static_cast<U>(b));
        }
    }
    __host__ __device__ static void store(Out *out, int64_t *, size_t at, Acc a) { out[at] = reduce_narrow<T>(a); }
};

template <typename S_>
struct ScanPair {
    int64_t i;
    S_ v;
};
template <typename S_, int FLOAT16>  // FLOAT16: 0 the type compares as it is, 1 float16 bits, 2 bfloat16 bits
struct ScanPairs {                   // MAX and MIN
    using In = S_;
    using Out = S_;
    using Acc = ScanPair<S_>;
    static constexpr bool kPairs = true;
    __host__ __device__ static Acc identity(int) { return Acc{-1, S_{}}; }
    __host__ __device__ static Acc load(In v, int64_t row) { return Acc{row, v}; }
    __host__ __device__ static auto key(S_ v) {
        if constexpr (FLOAT16 == 1) return bin_widen_f16(v);
        else if constexpr (FLOAT16 == 2) return bin_widen_bf16(v);
        else return v;
    }
    __host__ __device__ static Acc combine(int op, Acc a, Acc b) {
        if (b.i < 0) return a;
        if (a.i < 0) return b;
        const auto ka = key(a.v), kb = key(b.v);
        const bool take = kb != kb || (!(ka != ka) && (op == kScanMax ? kb >= ka : kb <= ka));
        return take ? b : a;
    }
    __host__ __device__ static void store(Out *out, int64_t *idx, size_t at, Acc a) {
        out[at] = a.v;
        idx[at] = a.i;
    }
};

// ---------------------------------------------------------------------------------------------- the levels (host and device)

// fold(child(0) .. child(count - 1)): A(k)_m from its F children, and every other fold of the order
template <class X, class Child>
__host__ __device__ inline typename X::Acc scan_fold(int op, uint32_t count, Child child) {
    typename X::Acc acc = X::identity(op);
    for (uint32_t i = 0; i < count; ++i) acc = X::combine(op, acc, child(i));
    return acc;
}
// first and one past the last word of level k that P_j folds
__host__ __device__ inline uint32_t scan_prefix_lo(uint32_t j, uint32_t k) { return (j >> (kScanFanBits * (k + 1u))) << kScanFanBits; }
__host__ __device__ inline uint32_t scan_prefix_hi(uint32_t j, uint32_t k) { return j >> (kScanFanBits * k); }
// P_j of a segment of K levels: word(k, m) is A(k)_m
template <class X, class Word>
__host__ __device__ inline typename X::Acc scan_tile_prefix(int op, uint32_t j, uint32_t K, Word word) {
    typename X::Acc p = X::identity(op);
    for (uint32_t k = K; k-- > 0u;)
        for (uint32_t m = scan_prefix_lo(j, k), hi = scan_prefix_hi(j, k); m < hi; ++m) p = X::combine(op, p, word(k, m));
    return p;
}

// ---------------------------------------------------------------------------------------------- the columns map (host and device)

// One tile of n rows of one column: row(r) is row r as an accumulator; emit(r, value) takes out[] of row r (MODE 1: incl; MODE 2:
// P (+) incl; MODE 0: nothing).  Answers A(0).
template <class X, int MODE, class Row, class Emit>
__host__ __device__ inline typename X::Acc scan_tile_columns(int op, uint32_t n, typename X::Acc P, Row row, Emit emit) {
    using Acc = typename X::Acc;
    Acc Q = X::identity(op);
    for (uint32_t r0 = 0; r0 < n; r0 += kScanRun) {
        Acc local = X::identity(op);
        const uint32_t r1 = n - r0 < kScanRun ? n : r0 + kScanRun;
        for (uint32_t r = r0; r < r1; ++r) {
            local = X::combine(op, local, row(r));
            if constexpr (MODE != 0) {
                const Acc incl = X::combine(op, Q, local);
                emit(r, MODE == 2 ? X::combine(op, P, incl) : incl);
            }
        }
        Q = X::combine(op, Q, local);
    }
    return Q;
}

// ---------------------------------------------------------------------------------------------- the flat map on the host

// One chunk: x[256] in, E[64] out; answers G.
template <class X>
inline typename X::Acc scan_chunk_host(int op, const typename X::Acc *x, typename X::Acc *E) {
    using Acc = typename X::Acc;
    Acc I[64], before[64];
    for (uint32_t l = 0; l < 64u; ++l) I[l] = scan_fold<X>(op, kScanLaneRows, [&](uint32_t k) { return x[kScanLaneRows * l + k]; });
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        for (uint32_t l = 0; l < 64u; ++l) before[l] = I[l];
        for (uint32_t l = d; l < 64u; ++l) I[l] = X::combine(op, before[l - d], before[l]);
    }
    E[0] = X::identity(op);
    for (uint32_t l = 1; l < 64u; ++l) E[l] = I[l - 1u];
    return I[63];
}
// One tile of n rows (the arguments of scan_tile_columns).
template <class X, int MODE, class Row, class Emit>
inline typename X::Acc scan_tile_flat_host(int op, uint32_t n, typename X::Acc P, Row row, Emit emit) {
    using Acc = typename X::Acc;
    Acc Q = X::identity(op), x[kScanChunk], E[64];
    for (uint32_t r0 = 0; r0 < n; r0 += kScanChunk) {
        for (uint32_t t = 0; t < kScanChunk; ++t) x[t] = r0 + t < n ? row(r0 + t) : X::identity(op);
        const Acc G = scan_chunk_host<X>(op, x, E);
        if constexpr (MODE != 0) {
            for (uint32_t l = 0; l < 64u; ++l) {
                Acc v = X::combine(op, Q, E[l]);
                for (uint32_t k = 0; k < kScanLaneRows; ++k) {
                    v = X::combine(op, v, x[kScanLaneRows * l + k]);
                    const uint32_t r = r0 + kScanLaneRows * l + k;
                    if (r < n) emit(r, MODE == 2 ? X::combine(op, P, v) : v);
                }
            }
        }
        Q = X::combine(op, Q, G);
    }
    return Q;
}

// The whole call on the host: S segments of L rows of C columns.
template <class X>
void scan_rows_on_host(const void *values, uint32_t S, uint32_t L, uint32_t C, int op, uint32_t T, void *out, int64_t *idx) {
    using Acc = typename X::Acc;
    const auto *in = static_cast<const typename X::In *>(values);
    auto *res = static_cast<typename X::Out *>(out);
    const uint32_t tiles = scan_tiles(L, T), K = scan_levels(L, T);
    std::vector<Acc> A[kScanMaxLevels], P(tiles, X::identity(op));
    for (uint32_t s = 0; s < S; ++s) {
        for (uint32_t c = 0; c < C; ++c) {
            auto at = [&](uint32_t j, uint32_t r) { return (static_cast<size_t>(s) * L + static_cast<size_t>(j) * T + r) * C + c; };
            auto tile = [&](uint32_t j, int mode) {
                const uint32_t n = L - j * T < T ? L - j * T : T;
                auto row = [&](uint32_t r) { return X::load(in[at(j, r)], static_cast<int64_t>(j) * T + r); };
                auto emit = [&](uint32_t r, Acc v) { X::store(res, idx, at(j, r), v); };
                if (C == 1u) return mode == 0 ? scan_tile_flat_host<X, 0>(op, n, P[j], row, emit) : mode == 1 ? scan_tile_flat_host<X, 1>(op, n, P[j], row, emit)
                                                                                                  : scan_tile_flat_host<X, 2>(op, n, P[j], row, emit);
                return mode == 0 ? scan_tile_columns<X, 0>(op, n, P[j], row, emit) : mode == 1 ? scan_tile_columns<X, 1>(op, n, P[j], row, emit)
                                                                                   : scan_tile_columns<X, 2>(op, n, P[j], row, emit);
            };
            if (K == 0u) {
                if (tiles) tile(0u, 1);
                continue;
            }
            A[0].resize(tiles);
            for (uint32_t j = 0; j < tiles; ++j) A[0][j] = tile(j, 0);
            for (uint32_t k = 1; k < K; ++k) {
                const uint32_t full = tiles >> (kScanFanBits * k);  // complete groups
                A[k].resize(full);
                for (uint32_t m = 0; m < full; ++m) A[k][m] = scan_fold<X>(op, kScanFan, [&](uint32_t i) { return A[k - 1u][m * kScanFan + i]; });
            }
            for (uint32_t j = 0; j < tiles; ++j) {
                P[j] = scan_tile_prefix<X>(op, j, K, [&](uint32_t k, uint32_t m) { return A[k][m]; });
                tile(j, 2);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the flat map on a wave
#if defined(__HIPCC__)

template <typename V>
__device__ __forceinline__ V scan_shfl_up(V v, uint32_t d) {
    static_assert(sizeof(V) % 4u == 0u, "whole words");
    uint32_t w[sizeof(V) / 4u];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(V) / 4u; ++i) w[i] = static_cast<uint32_t>(__shfl_up(static_cast<int>(w[i]), d));
    __builtin_memcpy(&v, w, sizeof(V));
    return v;
}
template <typename V>
__device__ __forceinline__ V scan_shfl(V v, uint32_t lane) {
    static_assert(sizeof(V) % 4u == 0u, "whole words");
    uint32_t w[sizeof(V) / 4u];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(V) / 4u; ++i) w[i] = static_cast<uint32_t>(__shfl(static_cast<int>(w[i]), static_cast<int>(lane)));
    __builtin_memcpy(&v, w, sizeof(V));
    return v;
}

// One chunk on one wave: the lane's x[0 .. 3] in, its E out; answers G (in every lane).
template <class X>
__device__ __forceinline__ typename X::Acc scan_chunk_wave(int op, const typename X::Acc (&x)[kScanLaneRows], uint32_t lane, typename X::Acc &E) {
    using Acc = typename X::Acc;
    Acc I = X::identity(op);
#pragma unroll
    for (uint32_t k = 0; k < kScanLaneRows; ++k) I = X::combine(op, I, x[k]);
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const Acc before = scan_shfl_up(I, d);
        if (lane >= d) I = X::combine(op, before, I);
    }
    E = scan_shfl_up(I, 1u);
    if (lane == 0u) E = X::identity(op);
    return scan_shfl(I, 63u);
}

// One tile of n rows on one wave, chunk after chunk: load(q, x) fills the lane's four rows of chunk q (the identity beyond the tile's
// end); emit(q, v) takes the lane's four outputs (MODE as scan_tile_columns).  Answers A(0).
template <class X, int MODE, class Load, class Emit>
__device__ __forceinline__ typename X::Acc scan_tile_flat_wave(int op, uint32_t n, uint32_t lane, typename X::Acc P, Load load, Emit emit) {
    using Acc = typename X::Acc;
    Acc Q = X::identity(op);
    for (uint32_t q = 0; q * kScanChunk < n; ++q) {
        Acc x[kScanLaneRows], E;
        load(q, x);
        const Acc G = scan_chunk_wave<X>(op, x, lane, E);
        if constexpr (MODE != 0) {
            Acc v = X::combine(op, Q, E), o[kScanLaneRows];
#pragma unroll
            for (uint32_t k = 0; k < kScanLaneRows; ++k) {
                v = X::combine(op, v, x[k]);
                o[k] = MODE == 2 ? X::combine(op, P, v) : v;
            }
            emit(q, o);
        }
        Q = X::combine(op, Q, G);
    }
    return Q;
}

// The single pass keeps a tile of up to NC chunks in registers between its aggregate and its outputs: the same combines in two halves.
template <class X, uint32_t NC>
struct ScanHeld {
    typename X::Acc x[NC][kScanLaneRows], base[NC];  // base[q] = Q_q (+) E_l
};
template <class X, uint32_t NC>
__device__ __forceinline__ typename X::Acc scan_tile_flat_hold(int op, uint32_t chunks, uint32_t lane, ScanHeld<X, NC> &h) {
    using Acc = typename X::Acc;
    Acc Q = X::identity(op);
#pragma unroll
    for (uint32_t q = 0; q < NC; ++q) {
        if (q < chunks) {
            Acc E;
            const Acc G = scan_chunk_wave<X>(op, h.x[q], lane, E);
            h.base[q] = X::combine(op, Q, E);
            Q = X::combine(op, Q, G);
        }
    }
    return Q;
}
template <class X, uint32_t NC>
__device__ __forceinline__ void scan_tile_flat_release(int op, uint32_t q, typename X::Acc P, const ScanHeld<X, NC> &h, typename X::Acc (&o)[kScanLaneRows]) {
    typename X::Acc v = h.base[q];
#pragma unroll
    for (uint32_t k = 0; k < kScanLaneRows; ++k) {
        v = X::combine(op, v, h.x[q][k]);
        o[k] = X::combine(op, P, v);
    }
}

// ---------------------------------------------------------------------------------------------- the single pass's words
// One 64-bit status word per A(k)_m: the 4-byte accumulator's bits below, 1 above -- the word is its own flag (zero: not published).

struct ScanWords {
    unsigned long long *level[kScanMaxLevels];  // level k: S x words[k] words
    uint32_t words[kScanMaxLevels];
    uint32_t K, budget;
    unsigned long long *takeovers;              // the context's counter
};
template <typename Acc>
__device__ __forceinline__ unsigned long long scan_word_of(Acc a) {
    static_assert(sizeof(Acc) == 4u, "a self-flagging word carries four bytes");
    return (1ull << 32) | __builtin_bit_cast(uint32_t, a);
}
template <typename Acc>
__device__ __forceinline__ Acc scan_word_value(unsigned long long w) { return __builtin_bit_cast(Acc, static_cast<uint32_t>(w)); }
__device__ __forceinline__ unsigned long long scan_word_load(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void scan_word_publish(unsigned long long *p, unsigned long long w) { __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A(LV)_m of segment s by the whole calling wave, without waiting: the published word, or else the same value computed -- level 0 from
// the tile's rows by the in-tile order (tile0(m)), a higher level from the level below by the same fold.
template <class X, int LV, class Tile0>
__device__ typename X::Acc scan_word_take(int op, const ScanWords &sw, uint32_t s, uint32_t m, Tile0 tile0) {
    using Acc = typename X::Acc;
    // every lane loads the same address; lane 0's answer is taken for all, so that the wave stays whole for the shuffles below whatever
    // the lanes saw
    const unsigned long long w = scan_shfl(scan_word_load(sw.level[LV] + static_cast<size_t>(s) * sw.words[LV] + m), 0u);
    if (w >> 32) return scan_word_value<Acc>(w);
    if constexpr (LV == 0) {
        return tile0(m);
    } else {
        Acc acc = X::identity(op);
        for (uint32_t i = 0; i < kScanFan; ++i) acc = X::combine(op, acc, scan_word_take<X, LV - 1>(op, sw, s, m * kScanFan + i, tile0));
        return acc;
    }
}

// Level LV's words of P_j -- A(LV)_m for m in [lo, lo + count) -- gathered by one wave: lane l polls word lo + l, at most sw.budget times
// over; then the wave computes what is missing itself.  Answers the lane's word; count comes back 0 for a level the segment does not have.
template <class X, int LV, class Tile0>
__device__ __forceinline__ typename X::Acc scan_lookback_level(int op, const ScanWords &sw, uint32_t s, uint32_t j, uint32_t lane, Tile0 tile0, uint32_t &count) {
    using Acc = typename X::Acc;
    count = 0u;
    if (static_cast<uint32_t>(LV) >= sw.K) return X::identity(op);
    const uint32_t lo = scan_prefix_lo(j, LV);
    count = scan_prefix_hi(j, LV) - lo;
    if (count == 0u) return X::identity(op);
    const unsigned long long *words = sw.level[LV] + static_cast<size_t>(s) * sw.words[LV] + lo;
    unsigned long long w;
    for (uint32_t polls = 0;; ++polls) {
        w = lane < count ? scan_word_load(words + lane) : 1ull << 32;
        uint64_t missing = __ballot((w >> 32) == 0u);
        if (!missing) break;
        if (polls < sw.budget) {
            __builtin_amdgcn_s_sleep(1);
            continue;
        }
        if (lane == 0u) atomicAdd(sw.takeovers, static_cast<unsigned long long>(__popcll(missing)));
        while (missing) {
            const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(missing));
            const Acc v = scan_word_take<X, LV>(op, sw, s, lo + l, tile0);
            if (lane == l) w = scan_word_of(v);
            missing &= missing - 1u;
        }
        break;
    }
    return scan_word_value<Acc>(w);
}
// acc (+) the first `count` lanes' words, left to right
template <class X>
__device__ __forceinline__ typename X::Acc scan_fold_lanes(int op, typename X::Acc acc, typename X::Acc mine, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i) acc = X::combine(op, acc, scan_shfl(mine, i));
    return acc;
}

// P_j of tile j of segment s, whose own aggregate `mine` is published here first.  The levels are gathered from the bottom up, and the
// last tile of a group publishes the group's word -- the fold of the level's words before its own, then its own -- as soon as that level
// is read: A(k+1)_m waits for words of level k only, never for a word of its own level.  P_j is then folded from the top level down.
template <class X, class Tile0>
__device__ __forceinline__ typename X::Acc scan_lookback_wave(int op, const ScanWords &sw, uint32_t s, uint32_t j, uint32_t lane, typename X::Acc mine, Tile0 tile0) {
    using Acc = typename X::Acc;
    if (lane == 0u) scan_word_publish(sw.level[0] + static_cast<size_t>(s) * sw.words[0] + j, scan_word_of(mine));
    Acc w[kScanMaxLevels], up = mine;
    uint32_t count[kScanMaxLevels];
    bool last = true;
    auto publish = [&](uint32_t k) {  // after level k is read
        last = last && k + 1u < sw.K && ((j + 1u) & ((1u << (kScanFanBits * (k + 1u))) - 1u)) == 0u;
        if (!last) return;
        up = X::combine(op, scan_fold_lanes<X>(op, X::identity(op), w[k], count[k]), up);  // fold(A(k)_{mF} .. A(k)_{mF+F-1})
        if (lane == 0u) scan_word_publish(sw.level[k + 1u] + static_cast<size_t>(s) * sw.words[k + 1u] + (j >> (kScanFanBits * (k + 1u))), scan_word_of(up));
    };
    w[0] = scan_lookback_level<X, 0>(op, sw, s, j, lane, tile0, count[0]);
    publish(0u);
    w[1] = scan_lookback_level<X, 1>(op, sw, s, j, lane, tile0, count[1]);
    publish(1u);
    w[2] = scan_lookback_level<X, 2>(op, sw, s, j, lane, tile0, count[2]);
    publish(2u);
    w[3] = scan_lookback_level<X, 3>(op, sw, s, j, lane, tile0, count[3]);
    Acc P = X::identity(op);
    P = scan_fold_lanes<X>(op, P, w[3], count[3]);
    P = scan_fold_lanes<X>(op, P, w[2], count[2]);
    P = scan_fold_lanes<X>(op, P, w[1], count[1]);
    return scan_fold_lanes<X>(op, P, w[0], count[0]);
}

#endif  // __HIPCC__

}  // namespace vrs
