// vrs_key_order.hpp -- the order-preserving maps of 32- / 64-bit key patterns R onto unsigned keys, and their inverses (host and device;
// internal): unsigned keys as they are (no function); signed: the sign bit flipped; float: negative: every bit flipped, else the sign bit
// flipped (the IEEE-754 total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN).
#pragma once
#include <hip/hip_runtime.h>

namespace vrs {

template <typename R> constexpr R kKeySign = static_cast<R>(1) << (8 * sizeof(R) - 1);

template <typename R> __host__ __device__ inline R key_from_signed(R x) { return x ^ kKeySign<R>; }
template <typename R> __host__ __device__ inline R signed_from_key(R r) { return r ^ kKeySign<R>; }
template <typename R> __host__ __device__ inline R key_from_float(R x) { return x ^ ((x & kKeySign<R>) ? ~R{0} : kKeySign<R>); }
template <typename R> __host__ __device__ inline R float_from_key(R r) { return r ^ ((r & kKeySign<R>) ? kKeySign<R> : ~R{0}); }

}  // namespace vrs
