// vrs_capi_quantile.hip -- the C ABI of the multi-rank selection (vrs_quantile_*): argument checks, the pure companions (target rule,
// level table, scratch size), the evaluation on the host (vrs_quantile_host), the statistics and the launches of vrs_quantile.hip.
#include "vrs_host.hpp"
#include "vrs_quantile.hpp"

using namespace vrsh;

namespace vrsh {

void quantile_release(vrs_context ctx) {
    if (ctx->quantile_stats) (void)hipFree(ctx->quantile_stats);
    ctx->quantile_stats = nullptr;
}

}  // namespace vrsh

namespace {

bool dtype_known(int dtype) { return dtype == vrs::kSortF32 || dtype == vrs::kSortF64; }

// what every entry point refuses about (dtype, q, interpolation, flags); nullptr: nothing
const char *refusal(int dtype, const double *q, uint32_t num_q, int interpolation, int flags) {
    if (!dtype_known(dtype)) return "quantile: the dtype must be float32 or float64";
    if (!vrs::quantile_interpolation_known(interpolation)) return "quantile: unknown interpolation";
    if (flags & ~vrs::kQuantIgnoreNan) return "quantile: unknown flag bits";
    if (num_q != 0u && !q) return "quantile: q is NULL";
    if (static_cast<uint64_t>(num_q) * vrs::quantile_sides(interpolation) > vrs::kQuantMaxTargets) return "quantile: more targets than VRS_QUANTILE_MAX_TARGETS";
    for (uint32_t i = 0; i < num_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return "quantile: q must be in [0, 1]";
    return nullptr;
}

template <typename S, typename T>
void host_segments(const S *src, uint32_t n, const uint32_t *offsets, uint32_t num_segments, const double *q, uint32_t num_q, int interpolation, bool ignore_nan,
                   T *out_values, T *out_lower, T *out_upper, T *out_weight) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    constexpr S ones = static_cast<S>(~static_cast<S>(0)), inf_bits = sizeof(S) == 4 ? static_cast<S>(0x7F800000u) : static_cast<S>(0x7FF0000000000000ull);
    auto value = [](S r) {
        bool exact;
        const S bits = vrs::sort_unrank<S, B, true, false>(r, false, &exact);
        if (!exact) return r == ones ? vrs::quantile_nan<T>() : static_cast<T>(0);
        T v;
        std::memcpy(&v, &bits, sizeof v);
        return v;
    };
    std::vector<S> ranks;
    for (uint32_t seg = 0; seg < num_segments; ++seg) {
        uint32_t b, e;
        (void)vrs::topk_tier(offsets[seg], offsets[seg + 1u], n, 0u, &b, &e);
        const uint32_t len = e - b;
        ranks.resize(len);
        uint32_t nans = 0;
        for (uint32_t p = 0; p < len; ++p) {
            ranks[p] = vrs::select_rank<S, B>(src[b + p], vrs::kSelFloat, inf_bits, false);
            if (ranks[p] == ones) ++nans;
        }
        std::sort(ranks.begin(), ranks.end());
        for (uint32_t i = 0; i < num_q; ++i) {
            T lo_v = vrs::quantile_nan<T>(), hi_v = lo_v, w = lo_v, v = lo_v;
            uint32_t lo, hi;
            if (vrs::quantile_target<T>(interpolation, q[i], len, nans, ignore_nan, &lo, &hi, &w)) {
                lo_v = value(ranks[lo]);
                hi_v = value(ranks[hi]);
                v = vrs::quantile_lerp<T>(interpolation, lo_v, hi_v, w);
            } else {
                w = vrs::quantile_nan<T>();
            }
            const size_t at = static_cast<size_t>(seg) * num_q + i;
            out_values[at] = v;
            if (out_lower) out_lower[at] = lo_v;
            if (out_upper) out_upper[at] = hi_v;
            if (out_weight) out_weight[at] = w;
        }
    }
}

}  // namespace

extern "C" {

int vrs_quantile_scratch_bytes(uint32_t num_elements, uint32_t num_segments, int dtype, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (!dtype_known(dtype)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "quantile: the dtype must be float32 or float64");
    *bytes = num_segments == 0u ? 0u : vrs::quantile_layout(num_elements, num_segments, dtype).bytes;
    return VRS_OK;
}

int vrs_quantile_level_for(int bits, int level, uint32_t *shift, uint32_t *mask, int *levels) {
    if (!shift || !mask || !levels) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (bits != 32 && bits != 64) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "quantile: ranks have 32 or 64 bits");
    *levels = vrs::quantile_levels(bits);
    if (level < 0 || level >= *levels) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "quantile: no such level");
    vrs::quantile_level(bits, level, shift, mask);
    return VRS_OK;
}

int vrs_quantile_target_for(int dtype, int interpolation, double q, uint32_t len, uint32_t nans, int ignore_nan, uint32_t *lower, uint32_t *upper,
                            double *weight, int *valid) {
    if (!lower || !upper || !weight || !valid) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (const char *why = refusal(dtype, &q, 1u, interpolation, 0)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, why);
    if (nans > len) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "quantile: more NaNs than keys");
    bool ok;
    if (dtype == vrs::kSortF32) {
        float w;
        ok = vrs::quantile_target<float>(interpolation, q, len, nans, ignore_nan != 0, lower, upper, &w);
        *weight = static_cast<double>(w);
    } else {
        ok = vrs::quantile_target<double>(interpolation, q, len, nans, ignore_nan != 0, lower, upper, weight);
    }
    *valid = ok ? 1 : 0;
    return VRS_OK;
}

int vrs_quantile_host(const void *src, uint32_t num_elements, const uint32_t *offsets, uint32_t num_segments, int dtype, const double *q,
                      uint32_t num_q, int interpolation, int flags, void *out_values, void *out_lower, void *out_upper, void *out_weight) {
    if (const char *why = refusal(dtype, q, num_q, interpolation, flags)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, why);
    if (num_segments == 0u || num_q == 0u) return VRS_OK;
    if ((!src && num_elements != 0u) || !offsets || !out_values) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "a pointer is NULL");
    const bool ignore_nan = (flags & vrs::kQuantIgnoreNan) != 0;
    if (dtype == vrs::kSortF32)
        host_segments<uint32_t, float>(static_cast<const uint32_t *>(src), num_elements, offsets, num_segments, q, num_q, interpolation, ignore_nan,
                                       static_cast<float *>(out_values), static_cast<float *>(out_lower), static_cast<float *>(out_upper),
                                       static_cast<float *>(out_weight));
    else
        host_segments<uint64_t, double>(static_cast<const uint64_t *>(src), num_elements, offsets, num_segments, q, num_q, interpolation, ignore_nan,
                                        static_cast<double *>(out_values), static_cast<double *>(out_lower), static_cast<double *>(out_upper),
                                        static_cast<double *>(out_weight));
    return VRS_OK;
}

int vrs_quantile_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments, uint64_t *sieved_segments) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long st[4];
    if (const int rc = read_counters(ctx, ctx->quantile_stats, st, 4)) return rc;
    if (lds_segments) *lds_segments = st[vrs::kTopkTierLds];
    if (block_segments) *block_segments = st[vrs::kTopkTierBlock];
    if (grid_segments) *grid_segments = st[vrs::kTopkTierGrid];
    if (sieved_segments) *sieved_segments = st[3];
    return VRS_OK;
}

int vrs_quantile_segments(vrs_context ctx, vrs_buffer src, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments, int dtype, const double *q,
                          uint32_t num_q, int interpolation, int flags, vrs_buffer out_values, vrs_buffer out_lower, vrs_buffer out_upper,
                          vrs_buffer out_weight, vrs_buffer scratch) {
    if (const char *why = refusal(dtype, q, num_q, interpolation, flags)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, why);
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (num_segments == 0u || num_q == 0u) return VRS_OK;
    if (!src || !offsets || !out_values || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype)), out_bytes = static_cast<size_t>(num_segments) * num_q * eb;
    const vrs::QuantLayout L = vrs::quantile_layout(num_elements, num_segments, dtype);
    int rc;
    if ((rc = check_buffer(ctx, src, static_cast<size_t>(num_elements) * eb, "src")) ||
        (rc = check_buffer(ctx, offsets, (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t), "offsets")) ||
        (rc = check_buffer(ctx, out_values, out_bytes, "out_values")) || (out_lower && (rc = check_buffer(ctx, out_lower, out_bytes, "out_lower"))) ||
        (out_upper && (rc = check_buffer(ctx, out_upper, out_bytes, "out_upper"))) ||
        (out_weight && (rc = check_buffer(ctx, out_weight, out_bytes, "out_weight"))) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    uintptr_t bits = reinterpret_cast<uintptr_t>(src->ptr) | reinterpret_cast<uintptr_t>(out_values->ptr) | reinterpret_cast<uintptr_t>(scratch->ptr);
    for (vrs_buffer b : {out_lower, out_upper, out_weight})
        if (b) bits |= reinterpret_cast<uintptr_t>(b->ptr);
    if (eb == 8u && (bits & 7u)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "quantile: float64 needs src, the outputs and scratch on 8-byte boundaries");
    if (reinterpret_cast<uintptr_t>(scratch->ptr) & 7u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "quantile: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if ((rc = make_counters(ctx, &ctx->quantile_stats, 4))) return rc;
    vrs::QuantileArgs a{};
    a.src = src->ptr;
    a.offsets = static_cast<const uint32_t *>(offsets->ptr);
    a.n = num_elements;
    a.num_segments = num_segments;
    a.num_q = num_q;
    a.grid_min_keys = ctx->tune.select_grid_min_keys;
    a.compact_divisor = ctx->tune.select_compact_divisor;
    a.dtype = dtype;
    a.interpolation = interpolation;
    a.flags = flags;
    for (uint32_t i = 0; i < num_q; ++i) a.q[i] = q[i];
    a.out_values = out_values->ptr;
    a.out_lower = out_lower ? out_lower->ptr : nullptr;
    a.out_upper = out_upper ? out_upper->ptr : nullptr;
    a.out_weight = out_weight ? out_weight->ptr : nullptr;
    a.scratch = static_cast<char *>(scratch->ptr);
    a.stats = ctx->quantile_stats;
    VRS_HIP(ctx, vrs::launch_quantile(ctx->stream, a, L));
    return VRS_OK;
}

}  // extern "C"
