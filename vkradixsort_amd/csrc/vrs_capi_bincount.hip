// vrs_capi_bincount.hip -- the C ABI of the counting kernels (vrs_bin_count*): argument checks, the tier decision, the scratch layout,
// the clearing of what the call accumulates into and the launches of vrs_bincount.hip.
#include "vrs_bincount.hpp"
#include "vrs_host.hpp"

using namespace vrsh;

namespace {

// the checks every entry point shares about what is counted into what: 1 <= num_bins, counts as int64 or a float dtype, weighted sums
// in the weights' dtype
int check_counters(vrs_context ctx, uint32_t num_bins, int weight_dtype, int out_dtype) {
    if (num_bins == 0u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: num_bins must be 1 or more");
    if (weight_dtype != vrs::kBinNoWeights && !vrs::bin_weight_dtype(weight_dtype))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the weight dtype must be float32 or float64 (or VRS_BIN_NO_WEIGHTS)");
    if (weight_dtype == vrs::kBinNoWeights && !vrs::bin_count_out_dtype(out_dtype))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the out dtype of a count must be int64, float16, bfloat16, float32 or float64");
    if (weight_dtype != vrs::kBinNoWeights && out_dtype != weight_dtype)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the out dtype of a weighted sum must be the weight dtype");
    return VRS_OK;
}

// ... and about how an element becomes a bin
int check_mode(vrs_context ctx, int dtype, int mode, double lo, double hi) {
    if (mode != vrs::kBinIndex && mode != vrs::kBinLinear) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: unknown mode");
    if (mode == vrs::kBinIndex) {
        if (!vrs::bin_index_dtype(dtype))
            return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the dtype of index mode must be uint8, int8, int16, int32 or int64");
        return VRS_OK;
    }
    if (!vrs::bin_linear_dtype(dtype))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the dtype of linear mode must be float16, bfloat16, float32 or float64");
    // the range as the kernels see it: in float32 for every dtype but float64
    const bool wide = dtype == vrs::kSortF64;
    const double l = wide ? lo : static_cast<double>(static_cast<float>(lo)), h = wide ? hi : static_cast<double>(static_cast<float>(hi));
    if (!std::isfinite(l) || !std::isfinite(h)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the range [lo, hi] must be finite");
    if (!(l < h)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the range needs lo < hi");
    // ... and its width as the rule divides by it (lo = -3e38, hi = 3e38 in float32: inf, and every quotient 0 or NaN)
    const double width = wide ? h - l : static_cast<double>(static_cast<float>(h) - static_cast<float>(l));
    if (!std::isfinite(width)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "bin_count: the width hi - lo of the range overflows the type the rule is evaluated in");
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_bin_count_tier_for(uint32_t num_bins, uint32_t counter_bytes, uint32_t lds_bytes, int *tier) {
    if (!tier) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "tier is NULL");
    if (num_bins == 0u) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bin_count: num_bins must be 1 or more");
    if (counter_bytes != 4u && counter_bytes != 8u) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bin_count: counter_bytes must be 4 or 8");
    *tier = vrs::bin_count_tier(num_bins, counter_bytes, lds_bytes);
    return VRS_OK;
}

int vrs_bin_count_scratch_bytes(uint32_t num_bins, int weight_dtype, int out_dtype, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (const int rc = check_counters(nullptr, num_bins, weight_dtype, out_dtype)) return rc;
    *bytes = vrs::bin_count_layout(num_bins, weight_dtype, out_dtype).bytes;
    return VRS_OK;
}

int vrs_bin_count_plan(vrs_context ctx, uint32_t num_bins, int weight_dtype, int out_dtype, int *tier, uint64_t *scratch_bytes) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!tier || !scratch_bytes) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (const int rc = check_counters(ctx, num_bins, weight_dtype, out_dtype)) return rc;
    *tier = vrs::bin_count_tier(num_bins, vrs::bin_counter_bytes(weight_dtype), ctx->tune.bincount_lds_bytes);
    *scratch_bytes = vrs::bin_count_layout(num_bins, weight_dtype, out_dtype).bytes;
    return VRS_OK;
}

int vrs_bin_count_stats(vrs_context ctx, uint64_t *lds_calls, uint64_t *global_calls) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (lds_calls) *lds_calls = ctx->bincount_calls[vrs::kBinCountTierLds];
    if (global_calls) *global_calls = ctx->bincount_calls[vrs::kBinCountTierGlobal];
    return VRS_OK;
}

int vrs_bin_linear_host(const void *values, uint64_t num_values, int dtype, double lo, double hi, uint32_t num_bins, int64_t *bins) {
    if (num_bins == 0u) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bin_count: num_bins must be 1 or more");
    if (const int rc = check_mode(nullptr, dtype, vrs::kBinLinear, lo, hi)) return rc;
    if (num_values != 0u && (!values || !bins)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "values or bins is NULL");
    const float lo32 = static_cast<float>(lo), hi32 = static_cast<float>(hi);
    for (uint64_t i = 0; i < num_values; ++i) {
        int side = 0;
        uint32_t b;
        switch (dtype) {
            case vrs::kSortF16: b = vrs::bin_linear<float>(vrs::bin_widen_f16(static_cast<const uint16_t *>(values)[i]), lo32, hi32, num_bins, &side); break;
            case vrs::kSortBF16: b = vrs::bin_linear<float>(vrs::bin_widen_bf16(static_cast<const uint16_t *>(values)[i]), lo32, hi32, num_bins, &side); break;
            case vrs::kSortF32: b = vrs::bin_linear<float>(static_cast<const float *>(values)[i], lo32, hi32, num_bins, &side); break;
            default: b = vrs::bin_linear<double>(static_cast<const double *>(values)[i], lo, hi, num_bins, &side); break;
        }
        bins[i] = b == vrs::kBinNone ? -1 : static_cast<int64_t>(b);
    }
    return VRS_OK;
}

int vrs_bin_count(vrs_context ctx, vrs_buffer values, uint32_t num_values, int dtype, int mode, double lo, double hi, uint32_t num_bins,
                  vrs_buffer weights, int weight_dtype, int out_dtype, vrs_buffer out, vrs_buffer skipped, vrs_buffer scratch) {
    int rc;
    if ((rc = check_mode(ctx, dtype, mode, lo, hi)) || (rc = check_counters(ctx, num_bins, weight_dtype, out_dtype))) return rc;
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    const bool weighted = weight_dtype != vrs::kBinNoWeights;
    if (!out || !scratch || (num_values != 0u && (!values || (weighted && !weights))))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL (scratch: vrs_bin_count_plan)");
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype)), ob = static_cast<size_t>(vrs::sort_dtype_bytes(out_dtype));
    const size_t cb = vrs::bin_counter_bytes(weight_dtype);
    const vrs::BinCountLayout L = vrs::bin_count_layout(num_bins, weight_dtype, out_dtype);
    if ((rc = check_buffer(ctx, out, num_bins * ob, "out")) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")) ||
        (num_values != 0u && (rc = check_buffer(ctx, values, num_values * eb, "values"))) ||
        (num_values != 0u && weighted && (rc = check_buffer(ctx, weights, num_values * cb, "weights"))) ||
        (skipped && (rc = check_buffer(ctx, skipped, 2u * sizeof(uint64_t), "skipped"))))
        return rc;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    char *scr = static_cast<char *>(scratch->ptr);
    const bool in_out = L.bytes == L.counters;  // an int64 count or a weighted sum: accumulated in `out` itself
    VRS_HIP(ctx, hipMemsetAsync(scr, 0, L.bytes, ctx->stream));
    if (in_out) VRS_HIP(ctx, hipMemsetAsync(out->ptr, 0, num_bins * ob, ctx->stream));
    vrs::BinFinishArgs f{};
    f.counters = in_out ? nullptr : reinterpret_cast<const uint32_t *>(scr + L.counters);
    f.out = out->ptr;
    f.out_dtype = out_dtype;
    f.num_bins = num_bins;
    f.skip = reinterpret_cast<const uint32_t *>(scr + L.skip);
    f.skipped = skipped ? static_cast<unsigned long long *>(skipped->ptr) : nullptr;
    if (num_values != 0u) {
        vrs::BinCountArgs a{};
        a.values = values->ptr;
        a.weights = weighted ? weights->ptr : nullptr;
        a.acc = in_out ? out->ptr : scr + L.counters;
        a.skip = reinterpret_cast<uint32_t *>(scr + L.skip);
        a.n = num_values;
        a.num_bins = num_bins;
        a.acc_stride = !weighted && out_dtype == vrs::kSortI64 ? 2u : 1u;  // the low word of each little-endian int64 (a call counts fewer than 2^32)
        // values that start off a 16-byte boundary: the tiles start `shift` elements earlier, on the boundary before them; whole vectors
        // are loaded when that puts the weights' vectors on boundaries too (w[1:] with an int32 x[1:])
        const uintptr_t off = reinterpret_cast<uintptr_t>(a.values) % 16u;
        a.vec_ok = off % eb == 0u && (!weighted || (reinterpret_cast<uintptr_t>(a.weights) - (off / eb) * cb) % 16u == 0u);
        a.shift = a.vec_ok ? static_cast<uint32_t>(off / eb) : 0u;
        a.lo = lo;
        a.hi = hi;
        a.compute_units = ctx->scatter.compute_units;
        const int tier = vrs::bin_count_tier(num_bins, static_cast<uint32_t>(cb), ctx->tune.bincount_lds_bytes);
        VRS_HIP(ctx, vrs::launch_bin_count(ctx->stream, a, dtype, mode, weight_dtype, tier));
        ctx->bincount_calls[tier] += 1u;
    }
    if (f.counters || f.skipped) VRS_HIP(ctx, vrs::launch_bin_finish(ctx->stream, f));
    return VRS_OK;
}

}  // extern "C"
