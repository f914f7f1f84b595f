// vrs_quantile_order.hpp -- the quantile's arithmetic, written once and compiled into the kernels (vrs_quantile.hip) and the host
// (vrs_capi_quantile.hip: vrs_quantile_target_for, vrs_quantile_host): which order statistics a q asks for, the weight between them and
// the interpolation.  T is the input's dtype (float or double): every step is one rounded operation of T, in torch's order, so that the
// host and the device give the same bits.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace vrs {

constexpr int kQuantLinear = 0, kQuantLower = 1, kQuantHigher = 2, kQuantMidpoint = 3, kQuantNearest = 4;  // vrs_quantile_interpolation
constexpr int kQuantIgnoreNan = 1;                                                                          // VRS_QUANTILE_IGNORE_NAN
constexpr uint32_t kQuantMaxTargets = 16u;                                                                  // VRS_QUANTILE_MAX_TARGETS

__host__ __device__ inline bool quantile_interpolation_known(int interpolation) { return interpolation >= kQuantLinear && interpolation <= kQuantNearest; }
// order statistics one q asks for: the two neighbours for LINEAR and MIDPOINT, one entry for the rest
__host__ __device__ inline uint32_t quantile_sides(int interpolation) { return interpolation == kQuantLinear || interpolation == kQuantMidpoint ? 2u : 1u; }

// The entries lower <= upper (0-based, of the segment's ascending order) and the weight between them that q asks of a segment of len
// keys, nans of them NaN.  false: the segment has no answer (len == 0; any NaN without ignore_nan; NaNs alone with it).
//   q -> T;  r = q * T(L' - 1), one rounded multiply, L' = len, or len - nans with ignore_nan;  LOWER / HIGHER / NEAREST: r = floor /
//   ceil / round-half-even of r;  lower = floor(r), upper = ceil(r), both clamped to L' - 1 (T(L' - 1) rounds up past the last index
//   for float rows longer than 2^24);  weight = r - floor(r), 0.5 for MIDPOINT, 0 for the single-entry modes.
template <typename T>
__host__ __device__ inline bool quantile_target(int interpolation, double q, uint32_t len, uint32_t nans, bool ignore_nan, uint32_t *lower,
                                                uint32_t *upper, T *weight) {
    *lower = *upper = 0u;
    *weight = static_cast<T>(0);
    if (nans > len) return false;
    if (!ignore_nan && nans != 0u) return false;
    const uint32_t live = ignore_nan ? len - nans : len;
    if (live == 0u) return false;
    const uint32_t last = live - 1u;
    T r = static_cast<T>(q) * static_cast<T>(last);
    if (interpolation == kQuantLower) r = floor(r);
    else if (interpolation == kQuantHigher) r = ceil(r);
    else if (interpolation == kQuantNearest) r = rint(r);  // (round half to even: the default rounding mode)
    const T below = floor(r), above = ceil(r);
    const T cap = static_cast<T>(last);  // (exact comparison: a T at or above cap is clamped before it is converted)
    const uint32_t lo = below >= cap ? last : static_cast<uint32_t>(below);
    const uint32_t hi = above >= cap ? last : static_cast<uint32_t>(above);
    if (quantile_sides(interpolation) == 1u) {
        *lower = *upper = lo;
        return true;
    }
    *lower = lo;
    *upper = hi;
    *weight = interpolation == kQuantMidpoint ? static_cast<T>(0.5) : r - below;
    return true;
}

template <typename T>
__host__ __device__ inline T quantile_nan() {
    return static_cast<T>(__builtin_nan(""));  // the quiet NaN, sign clear: 0x7FC00000 / 0x7FF8000000000000
}

// torch's two-branch lerp of the two entries' values, every operation rounded on its own (no fused multiply-add); a NaN result (inf - inf)
// is the quiet NaN on the host and on the device alike.  The single-entry modes answer a itself.
template <typename T>
__host__ __device__ inline T quantile_lerp(int interpolation, T a, T b, T w) {
#pragma clang fp contract(off)
    if (quantile_sides(interpolation) == 1u) return a;
    const T d = b - a;
    T v;
    if (w < static_cast<T>(0.5)) {
        const T p = w * d;
        v = a + p;
    } else {
        const T u = static_cast<T>(1) - w;
        const T p = d * u;
        v = b - p;
    }
    return v != v ? quantile_nan<T>() : v;
}

}  // namespace vrs
