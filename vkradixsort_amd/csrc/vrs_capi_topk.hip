// vrs_capi_topk.hip -- the C ABI of the top-k selection (vrs_topk_*): argument checks, the scratch layout, the launches of vrs_topk.hip,
// and for VRS_TOPK_SORTED with k > kTopkSortCap the sort of the survivors by the segmented pairs sort (of 64-bit ranks for int64 / float64).
#include "vrs_host.hpp"
#include "vrs_topk.hpp"

using namespace vrsh;

// device memory of a context's top-k selections
struct vrs_topk_state {
    unsigned long long *stats = nullptr;  // [3] cumulative segments per tier, zeroed when it is made
};

namespace vrsh {

void topk_release(vrs_context ctx) {
    vrs_topk_state *s = ctx->topk;
    if (!s) return;
    if (s->stats) (void)hipFree(s->stats);
    delete s;
    ctx->topk = nullptr;
}

}  // namespace vrsh

namespace {

constexpr int kKnownFlags = vrs::kTopkLargest | vrs::kTopkSorted | vrs::kTopkRank64;

int check_shape(vrs_context ctx, uint32_t num_segments, uint32_t k, int flags) {
    if (flags & ~kKnownFlags) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: unknown flag bits");
    if (static_cast<uint64_t>(num_segments) * k >= (1ull << 32)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: num_segments * k must be below 2^32");
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_topk_scratch_bytes(uint32_t num_elements, uint32_t num_segments, uint32_t k, int flags, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (const int rc = check_shape(nullptr, num_segments, k, flags)) return rc;
    *bytes = (k == 0u || num_segments == 0u) ? 0u : vrs::topk_layout(num_elements, num_segments, k, flags).bytes;
    return VRS_OK;
}

int vrs_topk_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, uint32_t grid_min_keys, int *tier, uint32_t *clamped_begin,
                      uint32_t *clamped_end) {
    if (!tier || !clamped_begin || !clamped_end) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    *tier = vrs::topk_tier(begin, end, num_elements, grid_min_keys, clamped_begin, clamped_end);
    return VRS_OK;
}

int vrs_topk_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long st[3];
    if (const int rc = read_counters(ctx, ctx->topk ? ctx->topk->stats : nullptr, st, 3)) return rc;
    if (lds_segments) *lds_segments = st[vrs::kTopkTierLds];
    if (block_segments) *block_segments = st[vrs::kTopkTierBlock];
    if (grid_segments) *grid_segments = st[vrs::kTopkTierGrid];
    return VRS_OK;
}

int vrs_topk_segments(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments, uint32_t k,
                      int key_type, int flags, vrs_buffer out_keys, vrs_buffer out_indices, vrs_buffer scratch) {
    if (!vrs::topk_key_type_known(key_type)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: unknown key_type");
    int rc;
    if ((rc = check_shape(ctx, num_segments, k, flags))) return rc;
    const size_t eb = vrs::topk_elem_bytes(key_type), rb = vrs::topk_rank_bytes(key_type);
    if (((flags & vrs::kTopkRank64) != 0) != (rb == 8u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: VRS_TOPK_RANK64 goes with VRS_TOPK_DTYPE of int64 / float64, and with no other key_type");
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!keys || !offsets || !out_keys || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    if (k == 0u || num_segments == 0u) return VRS_OK;
    const size_t slots = static_cast<size_t>(num_segments) * k * sizeof(uint32_t), key_slots = static_cast<size_t>(num_segments) * k * eb;
    const vrs::TopkLayout L = vrs::topk_layout(num_elements, num_segments, k, flags);
    if ((rc = check_buffer(ctx, keys, static_cast<size_t>(num_elements) * eb, "keys")) ||
        (rc = check_buffer(ctx, offsets, (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t), "offsets")) ||
        (rc = check_buffer(ctx, out_keys, key_slots, "out_keys")) || (out_indices && (rc = check_buffer(ctx, out_indices, slots, "out_indices"))) ||
        (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    // the control block at its head holds a 64-bit word the classification adds to atomically
    if (reinterpret_cast<uintptr_t>(scratch->ptr) & 7u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: scratch must be on an 8-byte boundary");
    if (eb == 8u && ((reinterpret_cast<uintptr_t>(keys->ptr) | reinterpret_cast<uintptr_t>(out_keys->ptr)) & 7u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "top-k: 8-byte elements need keys and out_keys on 8-byte boundaries");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (!ctx->topk) ctx->topk = new (std::nothrow) vrs_topk_state;
    vrs_topk_state *s = ctx->topk;
    if (!s) return fail(ctx, VRS_ERROR_OUT_OF_MEMORY, "top-k state");
    if ((rc = make_counters(ctx, &s->stats, 3))) return rc;
    vrs::TopkArgs a{};
    a.keys = keys->ptr;
    a.offsets = static_cast<const uint32_t *>(offsets->ptr);
    a.n = num_elements;
    a.num_segments = num_segments;
    a.k = k;
    a.grid_min_keys = ctx->tune.topk_grid_min_keys;
    a.lds_cap = vrs::topk_lds_cap(key_type);
    a.key_type = key_type;
    a.flags = flags;
    a.out_keys = out_keys->ptr;
    a.out_indices = out_indices ? static_cast<uint32_t *>(out_indices->ptr) : nullptr;
    a.scratch = static_cast<char *>(scratch->ptr);
    // VRS_TOPK_DTYPE sorts (rank, position) and fetches the own bits by position: without out_indices the positions live in the sort area
    const bool torch_order = vrs::topk_key_type_torch(key_type);
    a.positions = (a.out_indices || !(torch_order && L.big_sort)) ? a.out_indices : vrs::topk_sort_positions(a, L);
    a.stats = s->stats;
    VRS_HIP(ctx, vrs::launch_topk(ctx->stream, a, L));
    if (!L.big_sort) return VRS_OK;

    // the survivors (ranks, and positions when asked for) of S segments of k slots each, sorted by the segmented sort: its offsets i * k
    // live in out_keys meanwhile (S + 1 <= S * k words), and it never hands a segment to the one-call sort (which would wait for the device)
    VRS_HIP(ctx, vrs::launch_topk_sort_prep(ctx->stream, a, L));
    const uint32_t sk = num_segments * k;
    const size_t vb = slots;
    char *area = a.scratch + L.sort;  // ranks, their tmp (sk * rb bytes each), positions, their tmp (vb each)
    const size_t kb = static_cast<size_t>(sk) * rb;
    vrs_buffer_t kv = stack_view(ctx, area, kb), kt = stack_view(ctx, area + kb, kb);
    vrs_buffer_t vv = stack_view(ctx, area + 2u * kb, vb), vt = stack_view(ctx, area + 2u * kb + vb, vb);
    vrs_buffer_t ov = stack_view(ctx, a.out_keys, (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t));
    const uint32_t saved = ctx->tune.seg_one_call_min_keys;
    ctx->tune.seg_one_call_min_keys = 0u;
    if (rb == 8u) rc = vrs_sort_segments_pairs_u64(ctx, &kv, &kt, &vv, &vt, sk, &ov, num_segments);
    else if (out_indices || torch_order) rc = vrs_sort_segments_pairs_u32(ctx, &kv, &kt, &vv, &vt, sk, &ov, num_segments);
    else rc = vrs_sort_segments_u32(ctx, &kv, &kt, sk, &ov, num_segments);
    ctx->tune.seg_one_call_min_keys = saved;
    if (rc) return rc;
    VRS_HIP(ctx, vrs::launch_topk_sort_back(ctx->stream, a, L));
    return VRS_OK;
}

}  // extern "C"
