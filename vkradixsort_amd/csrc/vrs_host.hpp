// vrs_host.hpp -- what the parts of the C ABI's implementation (vrs_capi*.hip) share: the context and buffer objects, error helpers,
// and the prototypes of the host functions that cross a file boundary.  Internal: never installed, never included by a caller.
#pragma once
#include "vkradixsort_amd.h"
#include "vkradixsort_amd_dist.h"
#include "vkradixsort_amd_ops.h"
#include "vkradixsort_amd_tune.h"

#include <hip/hip_runtime.h>

#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "vrs_kernels.h"
#include "vrs_tuning.hpp"

struct vrs_segmented_state;  // vrs_capi_segmented.hip
struct vrs_topk_state;       // vrs_capi_topk.hip
struct vrs_select_state;     // vrs_capi_select.hip
struct vrs_reduce_state;     // vrs_capi_segreduce.hip

struct vrs_context_t {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string last_error;
    vrs::PrefixScratch scratch;
    uint32_t scratch_workgroups = 0;  // capacity of scratch.offsets in workgroups
    uint32_t scratch_chunks = 0;      // capacity of scratch.chunk_sums in chunks
    uint32_t last_offsets_workgroups = 0;  // contract workgroups of the most recent RADIX_SORT stage
    void *offsets_hook_out = nullptr;      // one-shot (vrs_multi_radixsort_offsets_hook): the next RADIX_SORT stage copies its digit
    void *offsets_hook_event = nullptr;    //   offsets here and records this event BEFORE its scatter kernel
    uint32_t last_offsets_stride = 1;      // rows of scratch.offsets per contract workgroup (sub-tiled launches)
    // NUM_BLOCKS_PER_WORKGROUP > 32: the histogram stage also keeps the 8192-key sub-tile table it folded the
    // caller's table from; the sort stage uses it iff it is called for exactly the same (keys, N, shift, B)
    uint32_t *sub_hist = nullptr;
    uint32_t sub_hist_rows = 0;
    struct {
        const void *keys = nullptr;
        const void *hist = nullptr;  // the caller's table the sub-tile table was folded into
        uint32_t n = 0, shift = 0, blocks = 0;
        int key_bytes = 4;
        bool valid = false;
    } sub_cache;
    vrs::Tuning tune;  // what vrs_set_tuning stores (vrs_tuning.hpp): every setting a caller can make, but scatter.variant / .atomic_rank
    vrs::ScatterLaunch scatter;
    bool atomic_rank_verified = false;  // device self-test result (context creation)
    vrs_buffer sort_hist = nullptr;     // histogram table owned by the one-call entry points
    // profiling
    uint32_t profile_mask = 0;  // bit k: attach timing events to launches of vrs_kernel_id k
    struct EventPair {
        hipEvent_t start, stop;
    };
    std::vector<EventPair> events[VRS_KERNEL_COUNT];
    size_t events_used[VRS_KERNEL_COUNT] = {};
    // one-call sort for large N (K5 in vrs_one_call.hip)
    uint32_t *os_tables = nullptr;       // [4][kStreams][256] digit tables, zero between sorts
    vrs::OnesweepPlan *os_plan = nullptr;
    uint32_t *os_status = nullptr;       // look-back status rows
    size_t os_status_rows = 0;
    bool os_status_clean = false;        // every status word is zero: the last kernel on the stream that touched them was a local sort that cleared them
    vrs::OnesweepPlanHead *os_host_head = nullptr;      // pinned host copy of the plan's head (the plan kernel writes it)
    vrs::OnesweepPlanHead *os_host_head_dev = nullptr;  // the same memory as the device sees it
    uint32_t os_stamp = 0;               // stamp of the most recent plan (never 0)
    uint32_t *os_ticket = nullptr;       // fused plan: ticket word of the counting read's workgroups (zero between launches)
    uint32_t drift_seen = 0;             // OnesweepPlanHead::drift (host copy) as of the last probe
    uint64_t reprobes = 0;               // probes run because sorts reported workgroups off the probed placement
    bool xcc_map_valid = false;          // the probe found block b on an XCC that depends on b % 8 only
    unsigned long long xcc_map = 0;      // byte x = that XCC for b % 8 == x
    uint64_t os_lookback_passes = 0;
    uint64_t os_relaunched_passes = 0;
    // hybrid form (K5b)
    bool os_fast_count_armed[2] = {false, false};  // adaptive: the context's last hybrid-capable sort of keys [0] / pairs [1] took the hybrid form
    bool os_wide_refused = false;        // 64-bit keys: the last attempt at the hybrid form was refused
    uint32_t os_wide_skipped = 0;        //   ... sorts since (every 16th tries again)
    uint64_t os_hybrid_recounts = 0;     // sorts that started over as LSD sorts after a fast count and a refusal
    uint32_t *os_msd_counts = nullptr;   // [16384] top-14-bit histogram + [8][256] top-byte counts per pass-0 group, zero between sorts
    vrs::MsdPlan *os_msd_plan = nullptr;
    vrs::OnesweepPlan *os_plan_a = nullptr;  // seeds and streams of the first MSD pass
    uint64_t os_hybrid_sorts = 0;        // one-call sorts that took the hybrid form
    uint64_t os_fallback_passes = 0;
    uint64_t os_skipped_passes = 0;      // identity passes (one digit value holds every key) the one-call sort left out     // passes the one-call sort ran through the contract path (unbalanced streams)
    // pool form (vrs_msd_pool.hip): the hybrid form of bare uint32 keys without the counting read
    uint32_t os_pool_skip = 0;           // adaptive (tune.pool == 1): hybrid-capable sorts of bare keys left before the pool form is tried again
    uint32_t os_pool_skip_n = 0;         //   keys of the sort whose refusal started the count: a sort of another size class (beyond a factor of two) is another workload and starts afresh
    vrs::PoolPlan *os_pool_plan = nullptr;
    uint32_t *os_pool_overflow = nullptr;  // overflow regions of the first pass
    uint32_t os_pool_overflow_cap = 0;     //   keys they hold
    uint32_t *os_pool_slack = nullptr;     // the buckets' regions the second pass scatters into (about 1.5 n slots)
    uint32_t os_pool_slack_cap = 0;        //   slots
    uint32_t *os_pool_overflow_vals = nullptr, *os_pool_slack_vals = nullptr;  // key + payload pairs: the payloads' twins of the two (made with the first pool sort of pairs)
    uint32_t os_pool_vals_overflow_cap = 0, os_pool_vals_slack_cap = 0;
    uint64_t os_pool_pair_sorts = 0;
    uint64_t os_pool_sorts = 0, os_pool_refusals = 0, os_pool_retries = 0;  // (retries: sorts whose local sort was enqueued again in a larger shape)
    uint32_t os_pool_epoch = 0;             // pool sorts / finishes enqueued: its parity picks the PoolPlan::fail word of each
    bool os_pool_layout_valid = false;      // the regions of the first pass, kept from one sort to the next (tune.pool_reuse)
    uint32_t os_pool_layout_n = 0, os_pool_layout_base = 0, os_pool_layout_sub_bits = 0;
    uint32_t os_pool_stale_run = 0, os_pool_reuse_pause = 0;  // kept layouts found stale in a row / sorts left that sample for themselves although a layout is kept
    uint32_t os_pool_fail_alloc = 0;       // VRS_TUNE_DEBUG_POOL_NO_MEMORY: allocations of the pool form's scratch left to fail (test hook)
    uint64_t os_pool_no_memory = 0;        // pool sorts / finishes that found no room for the form's scratch and took another form
    uint64_t os_pool_layout_reuses = 0, os_pool_stale_layouts = 0;  // sorts that started in a kept layout / of those, sorts it did not fit (run again, sampled)
    bool os_cursors_open = false;        // a reserving pass may have run without the local sort that re-arms its counters behind it
                                         // (a refused plan, a partition with no finish, an error in between): cleared before the next use
    // a one-call sort between its two halves (see one_read_enqueue / one_read_complete)
    struct OneRead {
        bool active = false;    // enqueued, its plan not yet looked at
        bool deferred = false;  // async mode: the caller did not wait
        void *kptr[2] = {nullptr, nullptr}, *vptr[2] = {nullptr, nullptr};  // [0] the caller's buffers, [1] the ping-pong partners
        uint32_t n = 0;
        int key_bytes = 4;
        uint32_t group = 0;     // group of four passes that is on the stream
        uint32_t stamp = 0;     // of that group's plan
        uint32_t cur = 0, cur_at_start = 0;  // which of the two buffers holds the data (now / when the group started)
        uint32_t blind_passes = 0;
        bool msd_capable = false, fast_count = false, blind_tail = false, no_hybrid = false;
        bool pool = false, no_pool = false;  // the pool form is on the stream / was refused for this sort
        uint32_t pool_sub_bits = 0, pool_local = 0;  // its shape; pool_retried: a larger local sort has been enqueued behind a first one that left
        bool pool_retried = false;
        uint32_t pool_top_bits = 8;  // bits of its first pass
        uint32_t pool_par = 0;     // parity of its pool epoch
        bool pool_reused = false;  // its first pass ran in a kept layout
        size_t ev_lb_before = 0, ev_ls_before = 0;
        uint32_t key_base = 0;      // vrs_sort_keys_u32_ranged: every key is promised to be >= this (a multiple of 2^24)
        uint32_t bucket_hint = 0;   // blind tail: expected largest bucket (0 = from n); picks the local sort's workgroup shape
        uint32_t sub_bits = 6;      // bucket bits the second MSD pass sorts by (what its plan is made with)
        uint32_t pass_b_groups = 0; // second MSD pass over fewer than 256 groups (vrs_msd_finish_grouped_u32): XCD x walks groups x, x + 8, ...
    } one_read;
    bool one_read_settling = false;
    uint32_t os_msd_half_stamp = 0;      // stamp of the most recent vrs_msd_finish_u32's plan
    // segmented sorts (vrs_capi_segmented.hip)
    vrs_segmented_state *seg = nullptr;
    // top-k selection (vrs_capi_topk.hip)
    vrs_topk_state *topk = nullptr;
    // one-rank selection (vrs_capi_select.hip)
    vrs_select_state *select = nullptr;
    // multi-rank selection (vrs_capi_quantile.hip): its own device counters
    unsigned long long *quantile_stats = nullptr;  // [4] cumulative segments per tier and grid slots that sieved
    // sorted-sequence search (vrs_capi_search.hip)
    uint64_t search_calls[4] = {};                // calls per tier (vrs_search_stats)
    // counting (vrs_capi_bincount.hip)
    uint64_t bincount_calls[2] = {};              // calls per tier (vrs_bin_count_stats)
    // segmented reduction (vrs_capi_segreduce.hip)
    vrs_reduce_state *reduce = nullptr;
    // prefix scan (vrs_capi_scan.hip)
    uint64_t scan_calls[3] = {};                  // calls per tier (vrs_scan_stats)
    unsigned long long *scan_takeovers = nullptr; // device counter: words a waiting wave of the single pass computed itself
    // ordered compaction (vrs_capi_compact.hip)
    uint64_t compact_calls[2] = {};               // count calls, emit calls (vrs_compact_stats)
    uint64_t compact_elements = 0;                // elements the count calls were given
};

struct vrs_buffer_t {
    vrs_context ctx = nullptr;  // owner, compared for identity only after creation (may be destroyed before the buffer)
    int device = 0;
    void *ptr = nullptr;
    size_t size = 0;
    bool owned = false;
};


namespace vrsh {


// the kernels' own launch tile: 8192 uint32 keys or 4096 uint64 keys (32 KiB either way)
constexpr uint32_t launch_tile_blocks(int key_bytes) { return key_bytes == 8 ? 16u : 32u; }
extern thread_local std::string g_global_error;
// Contexts that are alive (vrs_context_create* ... vrs_context_destroy): a buffer may outlive its context (host-language finalisers
// run in any order), so vrs_buffer_release asks here before it touches buf->ctx.
extern std::mutex g_live_mutex;
extern std::set<vrs_context> g_live_contexts;


#define VRS_HIP(ctx, call)                                       \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return fail_hip((ctx), #call, e__); \
    } while (0)


struct OneReadGeometry {
    uint32_t G, T, tiles_total, group_len, tiles0, tile_cap, blind_cap, tiles_b_cap, local_cap;
    size_t rows;
    vrs::StreamCuts cuts0;
};

// the digit tables with the fused plan's ticket word behind them / the hybrid form's counts: one allocation each, zero between sorts
constexpr size_t kDigitTableBytes = (vrs::kDigitTableWords + 64) * sizeof(uint32_t);
constexpr size_t kMsdCountBytes = vrs::kMsdCountWords * sizeof(uint32_t);

constexpr int kPoolNoMemory = -4242;  // (internal: pool_scratch found no room on the device; never leaves the library)

int fail(vrs_context ctx, int code, const std::string &msg);
int fail_hip(vrs_context ctx, const char *what, hipError_t e);
int ensure_scratch(vrs_context ctx, uint32_t W);
int profile_events(vrs_context ctx, int id, vrs::LaunchEvents *ev);
int check_push_constants(vrs_context ctx, const vrs_push_constants *pc, int key_bytes = 4);
int check_buffer(vrs_context ctx, vrs_buffer b, size_t need, const char *name);
int atomic_rank_selftest(vrs_context ctx, uint32_t rounds, uint32_t seed, uint64_t *mismatches);
int probe_xcc_map(vrs_context ctx, int stray_block = -1);
uint32_t *drift_word(vrs_context ctx);
int reprobe_if_drifted(vrs_context ctx);
int create_context(int device_ordinal, hipStream_t borrowed, bool borrow, vrs_context *out_ctx);
int run_sort_stage(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out, vrs_buffer values_in,
                   vrs_buffer values_out, vrs_buffer histograms, const vrs_push_constants *pc, bool pairs,
                   int key_bytes = 4);
int run_histogram_stage(vrs_context ctx, vrs_buffer keys_in, vrs_buffer histograms,
                               const vrs_push_constants *pc, int key_bytes);
int ensure_sort_hist(vrs_context ctx, uint32_t workgroups);
int contract_pass(vrs_context ctx, vrs_buffer kin, vrs_buffer kout, vrs_buffer vin, vrs_buffer vout,
                         vrs_push_constants *pc, uint32_t shift, int key_bytes);
int wait_for_host_word(vrs_context ctx, const std::function<bool()> &arrived, bool *never = nullptr);
int wait_for_plan(vrs_context ctx, uint32_t stamp);
vrs_buffer_t stack_view(vrs_context ctx, void *ptr, size_t bytes);
OneReadGeometry one_read_geometry(vrs_context ctx, const vrs_context_t::OneRead &st);
// the stamp of the next plan (never 0)
inline uint32_t next_stamp(vrs_context ctx) {
    if (++ctx->os_stamp == 0) ctx->os_stamp = 1;
    return ctx->os_stamp;
}
// the look-back status words the context owns / those a counting read has to zero (none while every word is known to be zero)
inline size_t status_words(vrs_context ctx) { return ctx->os_status_rows * VRS_RADIX_SORT_BINS; }
inline size_t status_words_to_zero(vrs_context ctx) { return ctx->os_status_clean ? 0 : status_words(ctx); }
// the digit tables and the hybrid form's counts must be all zero when a counting read starts: after a failure between a counting
// read and its plan, re-arm them for the next sort (best effort: the caller is already on an error path)
inline void rearm_counting_tables(vrs_context ctx) {
    if (ctx->os_tables) (void)hipMemsetAsync(ctx->os_tables, 0, kDigitTableBytes, ctx->stream);
    if (ctx->os_msd_counts) (void)hipMemsetAsync(ctx->os_msd_counts, 0, kMsdCountBytes, ctx->stream);
}
// what every launch of this context is given (the test hooks tune.hold_tile / tune.misplace are NOT part of it: each call site says
// whether they apply)
inline vrs::LaunchSetup launch_setup(vrs_context ctx) {
    vrs::LaunchSetup s{};
    s.atomic_rank = ctx->scatter.atomic_rank;
    s.xcc_map = ctx->xcc_map;
    s.spin_budget = ctx->tune.spin_budget;
    s.drift = drift_word(ctx);
    s.compute_units = ctx->scatter.compute_units;
    return s;
}
// what the plan of a counting read over n keys is made from: the one place the sort's geometry becomes launcher arguments
inline vrs::PlanGeometry plan_geometry(vrs_context ctx, const OneReadGeometry &g, uint32_t n, uint32_t stamp) {
    vrs::PlanGeometry p{};
    p.n = n;
    p.group_len = g.group_len;
    p.tile = g.T;
    p.tile_cap = g.tile_cap;
    p.blind_cap = g.blind_cap;
    p.cuts0 = g.cuts0;
    p.stamp = stamp;
    p.host_head = ctx->os_host_head_dev;
    return p;
}
// launch_msd_plan's arguments as every caller gives them; the caller sets what differs: msd_only, max_shift (and, where they are
// not the defaults, msd_counts, host_log, sub_bits)
inline vrs::MsdPlanArgs msd_plan_args(vrs_context ctx, const OneReadGeometry &g, uint32_t n, uint32_t stamp) {
    vrs::MsdPlanArgs a{};
    a.msd_counts = ctx->os_msd_counts;
    a.msd = ctx->os_msd_plan;
    a.plan_a = ctx->os_plan_a;
    a.plan_lsd = ctx->os_plan;
    a.geo = plan_geometry(ctx, g, n, stamp);
    a.tiles_b_cap = g.tiles_b_cap;
    a.local_cap = g.local_cap;
    a.tables = ctx->os_tables;
    return a;
}
// the log of the vrs_msd_finish_* plans' decisions (kMsdLogWords words behind the pinned host head), as the device sees it
inline uint32_t *finish_log(vrs_context ctx) { return reinterpret_cast<uint32_t *>(ctx->os_host_head_dev + 1); }
int one_read_scratch(vrs_context ctx, const vrs_context_t::OneRead &st, const OneReadGeometry &g);
int one_read_lookback_pass(vrs_context ctx, vrs_context_t::OneRead &st, uint32_t i, uint32_t shift, uint32_t grid_tiles, int forced);
bool reserves(vrs_context ctx, uint32_t n, bool pairs);
int reservation_begin(vrs_context ctx);
int one_read_hybrid_tail(vrs_context ctx, vrs_context_t::OneRead &st, const OneReadGeometry &g, uint32_t tiles_b, uint32_t max_bucket,
                                bool status_was_clean = false);
int one_read_enqueue(vrs_context ctx);
void pool_scratch_release(vrs_context ctx, bool payloads_only = false);
int pool_scratch(vrs_context ctx, uint32_t room, uint32_t slack, bool pairs = false);
int one_read_enqueue_pool(vrs_context ctx, const OneReadGeometry &g);
int one_read_complete(vrs_context ctx, bool *done);
int one_read_settle(vrs_context ctx);
int settle_pending(vrs_context ctx);
void segmented_release(vrs_context ctx);
void topk_release(vrs_context ctx);
void select_release(vrs_context ctx);
void quantile_release(vrs_context ctx);
void reduce_release(vrs_context ctx);
void scan_release(vrs_context ctx);

// A context's cumulative device counters (count entries of T): made and zeroed on its stream at first use; read back once the calls
// before have finished (all zeros when they were never made: counters == NULL).
template <typename T>
int make_counters(vrs_context ctx, T **counters, size_t count) {
    if (*counters) return VRS_OK;
    VRS_HIP(ctx, hipMalloc(reinterpret_cast<void **>(counters), count * sizeof(T)));
    VRS_HIP(ctx, hipMemsetAsync(*counters, 0, count * sizeof(T), ctx->stream));
    return VRS_OK;
}
template <typename T>
int read_counters(vrs_context ctx, const T *counters, T *out, size_t count) {
    std::fill(out, out + count, T{});
    if (!counters) return VRS_OK;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if (const int rc = settle_pending(ctx)) return rc;
    VRS_HIP(ctx, hipMemcpyAsync(out, counters, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    VRS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VRS_OK;
}
int sort_one_read(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values, vrs_buffer values_tmp,
                         uint32_t n, int key_bytes, uint32_t key_base);
int sort_all_passes(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values,
                           vrs_buffer values_tmp, uint32_t n, int key_bytes = 4, uint32_t key_base = 0);
int msd_half_setup(vrs_context ctx, uint32_t n, vrs_context_t::OneRead *st, OneReadGeometry *g, uint32_t bucket_hint = 0,
                          uint32_t pass_b_groups = 0);
int fill_own_holes(vrs_context ctx, vrs_buffer grouped, vrs_buffer own, uint64_t own_offset, uint32_t top_bytes, const uint32_t *counts,
                          const uint32_t *own_counts);

}  // namespace vrsh
