// vrs_capi_segmented.hip -- the C ABI of the segmented sorts (vrs_sort_segments_*, 32- and 64-bit keys): argument checks, the context's work
// lists, the launches of vrs_segmented.hip, and the one-call tier (segments too long for one workgroup, sorted by the one-call sort on views
// of the buffers).
#include "vrs_host.hpp"
#include "vrs_segmented.hpp"

using namespace vrsh;

// device and pinned memory of a context's segmented sorts, grown on demand
struct vrs_segmented_state {
    vrs::SegControl *control = nullptr;  // list counts (zeroed by every sort) and the cumulative per-tier statistics
    uint2 *lists = nullptr;              // the work lists, back to back
    size_t list_entries = 0;
    uint32_t *host = nullptr, *host_dev = nullptr;  // pinned: [0] stamp, [1] count, then (begin, end) of each one-call segment
    size_t host_entries = 0;
    uint32_t stamp = 0;
};

namespace vrsh {

void segmented_release(vrs_context ctx) {
    vrs_segmented_state *s = ctx->seg;
    if (!s) return;
    if (s->control) (void)hipFree(s->control);
    if (s->lists) (void)hipFree(s->lists);
    if (s->host) (void)hipHostFree(s->host);
    delete s;
    ctx->seg = nullptr;
}

}  // namespace vrsh

namespace {

// entries each list can need: a list holds segments of at least `shortest` keys, and segments that do not overlap number at most n / shortest
uint32_t list_cap(uint32_t n, uint32_t num_segments, uint32_t shortest) { return std::min(num_segments, n / shortest); }

int segmented(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values, vrs_buffer values_tmp, uint32_t n, vrs_buffer offsets,
              uint32_t num_segments, bool pairs, int key_bytes) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!keys || !keys_tmp || !offsets || (pairs && (!values || !values_tmp)))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    if (n == 0u || num_segments == 0u) return VRS_OK;
    const size_t bytes = static_cast<size_t>(n) * sizeof(uint32_t), kbytes = static_cast<size_t>(n) * key_bytes;
    int rc;
    if ((rc = check_buffer(ctx, keys, kbytes, "keys")) || (rc = check_buffer(ctx, keys_tmp, kbytes, "keys_tmp"))) return rc;
    if (pairs && ((rc = check_buffer(ctx, values, bytes, "values")) || (rc = check_buffer(ctx, values_tmp, bytes, "values_tmp")))) return rc;
    if ((rc = check_buffer(ctx, offsets, (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t), "offsets"))) return rc;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;

    const bool wide = key_bytes == 8;
    const uint32_t block_cap = vrs::seg_block_cap(wide, pairs);
    const uint32_t min_keys = ctx->tune.seg_one_call_min_keys;
    vrs::SegLists lists{};
    lists.cap[vrs::kSegListWaveSmall] = list_cap(n, num_segments, 2u);
    lists.cap[vrs::kSegListWave] = list_cap(n, num_segments, vrs::kSegWaveSmallCap + 1u);
    lists.cap[vrs::kSegListBlockSmall] = list_cap(n, num_segments, vrs::seg_wave_cap(wide) + 1u);
    lists.cap[vrs::kSegListBlock] = list_cap(n, num_segments, vrs::kSegBlockSmallCap + 1u);
    const bool one_call = min_keys != 0u && n >= min_keys && n > block_cap;  // else no segment can reach the one-call tier
    const uint32_t global_max = one_call ? std::max(min_keys, block_cap + 1u) - 1u : n;  // longest segment of the global tier
    lists.cap[vrs::kSegListGlobal] = global_max > block_cap ? list_cap(n, num_segments, block_cap + 1u) : 0u;
    lists.cap[vrs::kSegListOneCall] = one_call ? list_cap(n, num_segments, std::max(min_keys, block_cap + 1u)) : 0u;
    size_t entries = 0;
    for (int l = 0; l < vrs::kSegLists; ++l) entries += lists.cap[l];

    if (!ctx->seg) ctx->seg = new (std::nothrow) vrs_segmented_state;
    vrs_segmented_state *s = ctx->seg;
    if (!s) return fail(ctx, VRS_ERROR_OUT_OF_MEMORY, "segmented sort state");
    if ((rc = make_counters(ctx, &s->control, 1))) return rc;
    if (entries > s->list_entries) {
        if (s->lists) {
            VRS_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier segmented sort may still read them)
            (void)hipFree(s->lists);
            s->lists = nullptr;
            s->list_entries = 0;
        }
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->lists), entries * sizeof(uint2));
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            s->lists = nullptr;
            return fail(ctx, VRS_ERROR_OUT_OF_MEMORY, "segmented sort: no room for the work lists");
        }
        VRS_HIP(ctx, e);
        s->list_entries = entries;
    }
    uint2 *at = s->lists;
    for (int l = 0; l < vrs::kSegLists; ++l) {
        lists.list[l] = at;
        at += lists.cap[l];
    }
    if (lists.cap[vrs::kSegListOneCall] > s->host_entries) {
        if (s->host) {
            VRS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipHostFree(s->host);
            s->host = s->host_dev = nullptr;
            s->host_entries = 0;
        }
        const size_t words = 2u + 2u * static_cast<size_t>(lists.cap[vrs::kSegListOneCall]);
        VRS_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&s->host), words * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
        s->host[0] = 0u;
        VRS_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&s->host_dev), s->host, 0));
        s->host_entries = lists.cap[vrs::kSegListOneCall];
    }
    uint32_t grid[vrs::kSegLists];
    for (int l = 0; l < vrs::kSegLists; ++l) grid[l] = lists.cap[l];
    if (++s->stamp == 0u) s->stamp = 1u;
    const uint32_t stamp = s->stamp;
    auto *kp = static_cast<char *>(keys->ptr), *tp = static_cast<char *>(keys_tmp->ptr);
    auto *vp = pairs ? static_cast<uint32_t *>(values->ptr) : nullptr, *vtp = pairs ? static_cast<uint32_t *>(values_tmp->ptr) : nullptr;
    VRS_HIP(ctx, vrs::launch_segmented(ctx->stream, kp, tp, vp, vtp, n, static_cast<const uint32_t *>(offsets->ptr), num_segments,
                                       one_call ? min_keys : 0u, s->control, lists, grid, one_call ? s->host_dev : nullptr, stamp, key_bytes));
    if (!one_call) return VRS_OK;

    // the one-call tier: wait for the classification's list (never for the sorts), then one sort per segment on views of the buffers
    volatile uint32_t *ready = &s->host[0];
    if ((rc = wait_for_host_word(ctx, [&] { return __atomic_load_n(ready, __ATOMIC_ACQUIRE) == stamp; }))) return rc;
    const uint32_t count = std::min(s->host[1], lists.cap[vrs::kSegListOneCall]);
    std::vector<uint32_t> ranges(s->host + 2, s->host + 2 + 2u * static_cast<size_t>(count));
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t b = ranges[2u * i], len = ranges[2u * i + 1u] - b;
        const size_t off = static_cast<size_t>(b), vb = static_cast<size_t>(len) * sizeof(uint32_t), kb = static_cast<size_t>(len) * key_bytes;
        vrs_buffer_t k = stack_view(ctx, kp + off * key_bytes, kb), kt = stack_view(ctx, tp + off * key_bytes, kb);
        vrs_buffer_t v = stack_view(ctx, pairs ? vp + off : nullptr, vb), vt = stack_view(ctx, pairs ? vtp + off : nullptr, vb);
        if ((rc = sort_all_passes(ctx, &k, &kt, pairs ? &v : nullptr, pairs ? &vt : nullptr, len, key_bytes))) return rc;
    }
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_sort_segments_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements, vrs_buffer offsets,
                          uint32_t num_segments) {
    return segmented(ctx, keys, keys_tmp, nullptr, nullptr, num_elements, offsets, num_segments, false, 4);
}

int vrs_sort_segments_pairs_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values, vrs_buffer values_tmp,
                                uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments) {
    return segmented(ctx, keys, keys_tmp, values, values_tmp, num_elements, offsets, num_segments, true, 4);
}

int vrs_sort_segments_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements, vrs_buffer offsets,
                          uint32_t num_segments) {
    return segmented(ctx, keys, keys_tmp, nullptr, nullptr, num_elements, offsets, num_segments, false, 8);
}

int vrs_sort_segments_pairs_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values, vrs_buffer values_tmp,
                                uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments) {
    return segmented(ctx, keys, keys_tmp, values, values_tmp, num_elements, offsets, num_segments, true, 8);
}

int vrs_segmented_stats(vrs_context ctx, uint64_t *wave_segments, uint64_t *block_segments, uint64_t *global_segments,
                        uint64_t *one_call_segments) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long st[4];
    if (const int rc = read_counters(ctx, ctx->seg && ctx->seg->control ? ctx->seg->control->stats : nullptr, st, 4)) return rc;
    if (wave_segments) *wave_segments = st[vrs::kSegTierWave];
    if (block_segments) *block_segments = st[vrs::kSegTierBlock];
    if (global_segments) *global_segments = st[vrs::kSegTierGlobal];
    if (one_call_segments) *one_call_segments = st[vrs::kSegTierOneCall];
    return VRS_OK;
}

int vrs_segment_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, int pairs, uint32_t one_call_min_keys, int *tier,
                         uint32_t *clamped_begin, uint32_t *clamped_end) {
    if (!tier || !clamped_begin || !clamped_end) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    *tier = vrs::segment_tier(begin, end, num_elements, pairs != 0, one_call_min_keys, clamped_begin, clamped_end);
    return VRS_OK;
}

int vrs_segment_tier_for_u64(uint32_t begin, uint32_t end, uint32_t num_elements, int pairs, uint32_t one_call_min_keys, int *tier,
                             uint32_t *clamped_begin, uint32_t *clamped_end) {
    if (!tier || !clamped_begin || !clamped_end) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    *tier = vrs::segment_tier(begin, end, num_elements, pairs != 0, one_call_min_keys, clamped_begin, clamped_end, true);
    return VRS_OK;
}

}  // extern "C"
