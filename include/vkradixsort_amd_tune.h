/*
 * vkradixsort_amd_tune.h -- measurement, diagnostics, tuning and test hooks (no reference counterpart).
 *
 * For benchmarks, labs and the test suite: per-kernel timing, the counters that say which form a sort took, the form-decision
 * table, the tuning settings (performance only, never results) and, last, the vrs_debug_* test hooks.  Nothing an integrator
 * of the sort needs.
 */
#ifndef VKRADIXSORT_AMD_TUNE_H
#define VKRADIXSORT_AMD_TUNE_H

#include <stddef.h>
#include <stdint.h>

#include "vkradixsort_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- measurement (no reference counterpart) ------------------------- */

typedef enum vrs_kernel_id {
    VRS_KERNEL_HISTOGRAM = 0, /* stage RADIX_SORT_HISTOGRAMS */
    VRS_KERNEL_PREFIX = 1,    /* global digit prefix + per-workgroup offsets (both launches) */
    VRS_KERNEL_SCATTER = 2,   /* stable scatter (the dominant kernel) */
    VRS_KERNEL_SINGLE = 3,    /* single_radixsort */
    VRS_KERNEL_DIGIT_TABLES = 4,     /* one-call sort, large N: the single counting read of all four digits */
    VRS_KERNEL_LOOKBACK_SCATTER = 5, /* one-call sort, large N: scatter pass with decoupled look-back (stable), or -- MSD passes over bare keys --
                                        with reserved places */
    VRS_KERNEL_LOCAL_SORT = 6,       /* one-call sort, hybrid form: every top-14-bit bucket sorted inside LDS */
    VRS_KERNEL_POOL_SAMPLE = 7,      /* one-call sort, pool form: the sample (1/32 of the keys) that sizes the first MSD pass's regions */
    VRS_KERNEL_POOL_PASS_A = 8,      /* one-call sort, pool form: the first MSD pass (pool_pass_a_kernel: reserves in sampled regions) */
    VRS_KERNEL_POOL_PASS_B = 9,      /* one-call sort, pool form: the second MSD pass (pool_pass_b_kernel: scatters into the buckets' slack regions) */
    VRS_KERNEL_COUNT = 10
} vrs_kernel_id;

/* When enabled, every kernel launch carries a (start, stop) hipEvent pair on its own dispatch packet
 * (hipExtLaunchKernel) on the context's stream -- no separate event-record packets. */
int vrs_profile_enable(vrs_context ctx, int enabled);
/* Same, for a subset: bit k of `kernel_mask` selects vrs_kernel_id k (timing only the dominant kernel
 * keeps the instrumentation out of the other launches of a timed region). */
int vrs_profile_enable_mask(vrs_context ctx, uint32_t kernel_mask);
int vrs_profile_reset(vrs_context ctx);
/* Synchronises the stream, then returns launches and summed event time for one kernel id. */
int vrs_profile_query(vrs_context ctx, int kernel_id, uint64_t *launches, double *total_ms);
/* Same for ONE launch: `index` counts the instrumented launches of `kernel_id` since vrs_profile_reset. */
int vrs_profile_query_launch(vrs_context ctx, int kernel_id, uint64_t index, double *ms);

/* What the large-N form of the one-call sorts did on this context so far (cumulative): passes run as look-back
 * scatters, passes that fell back to a contract pass (streams too unequal), identity passes left out. */
int vrs_one_call_stats(vrs_context ctx, uint64_t *lookback_passes, uint64_t *fallback_passes, uint64_t *skipped_passes);
/* Look-back passes the one-call sort enqueued a second time: the speculative enqueue (made before the plan was known)
 * left at once because an earlier pass needed another form or because the pass's longest stream did not fit the
 * speculative grid.  Cumulative; diagnostics only. */
int vrs_one_call_relaunched_passes(vrs_context ctx, uint64_t *relaunched_passes);
/* One-call sorts that took the hybrid form (VRS_TUNE_HYBRID).  Cumulative; diagnostics only. */
int vrs_one_call_hybrid_sorts(vrs_context ctx, uint64_t *hybrid_sorts);
/* One-call sorts that, after a fast count (VRS_TUNE_HYBRID_FAST_COUNT) and a plan that refused the hybrid form, started over
 * as LSD sorts with a second counting read.  Cumulative; diagnostics only. */
int vrs_one_call_hybrid_recounts(vrs_context ctx, uint64_t *recounts);

/* WHICH FORM a one-call sort takes (host only, no device needed): the dispatcher's own decision function, so that its table --
 * form x size x kind x settings x what an earlier refusal left behind -- can be walked by a test.  key_bytes 4 or 8, pairs != 0 = with
 * uint32 payloads; knobs[VRS_FORM_KNOB_*] for knob_count entries, a negative entry (or one beyond knob_count) = what a fresh context on
 * a device whose probes passed holds; *form = VRS_FORM_*; memory_out (may be NULL): [0] = the adaptive pool skip, [1] = the 64-bit
 * keys' skip counter as the decision leaves them. */
typedef enum vrs_sort_form {
    VRS_FORM_NONE = 0,     /* nothing to sort */
    VRS_FORM_SINGLE = 1,   /* one single_radixsort launch */
    VRS_FORM_CONTRACT = 2, /* the reference's two stages, pass by pass */
    VRS_FORM_LSD = 3,      /* one counting read + a look-back scatter pass per key byte */
    VRS_FORM_COUNTED = 4,  /* the counted hybrid form */
    VRS_FORM_POOL = 5      /* the pool form (pairs: its stable variant) */
} vrs_sort_form;
typedef enum vrs_form_knob {
    VRS_FORM_KNOB_SINGLE_MAX_KEYS = 0, VRS_FORM_KNOB_ONE_CALL_MIN_KEYS = 1, VRS_FORM_KNOB_HYBRID_MIN_KEYS = 2, VRS_FORM_KNOB_POOL_MIN_KEYS = 3,
    VRS_FORM_KNOB_HYBRID = 4, VRS_FORM_KNOB_POOL = 5, VRS_FORM_KNOB_POOL_PAIRS = 6, VRS_FORM_KNOB_RESERVE = 7, VRS_FORM_KNOB_GROUPS = 8,
    VRS_FORM_KNOB_XCC_MAP_VALID = 9, VRS_FORM_KNOB_ATOMIC_RANK = 10,           /* what the context found out about the device */
    VRS_FORM_KNOB_POOL_SKIP = 11, VRS_FORM_KNOB_POOL_SKIP_N = 12, VRS_FORM_KNOB_WIDE_REFUSED = 13, VRS_FORM_KNOB_WIDE_SKIPPED = 14, /* memory */
    VRS_FORM_KNOB_NO_POOL = 15, VRS_FORM_KNOB_NO_HYBRID = 16,                   /* this sort is a retry after a refusal of that form */
    VRS_FORM_KNOB_COUNT = 17
} vrs_form_knob;
int vrs_sort_form_for(uint32_t num_elements, int key_bytes, int pairs, const int64_t *knobs, int knob_count, int *form, int64_t *memory_out);

/* One-call sorts of bare uint32 keys that took the pool form (the hybrid form without a counting read, VRS_TUNE_MSD_POOL), and
 * sorts whose pool form the plan refused (they ran in the counted form afterwards).  Cumulative; diagnostics only. */
int vrs_one_call_pool_sorts(vrs_context ctx, uint64_t *pool_sorts, uint64_t *pool_refusals);
/* What the pool form would do with num_elements bare uint32 keys (host only, no device needed): *sub_bits = S where the sort has
   256 << S buckets (6 or 7; 0 = the form does not take this size) -- the COUNT of buckets, not the cut: with the default cut a sort of
   16384 buckets runs a first pass by 7 bits and a second by 7, vrs_pool_form_shape_ex reports that --, *bucket_capacity = keys per bucket the local sort it enqueues takes (1789: one wave
   per bucket; 4093 / 7165: 256 threads; 14333: 512), *scratch_bytes = context scratch a sort of this size needs beside the caller's two
   buffers (slack buffer + first-pass overflow room + plan).  Any pointer may be NULL. */
int vrs_pool_form_shape(uint32_t num_elements, uint32_t *sub_bits, uint32_t *bucket_capacity, uint64_t *scratch_bytes);
/* The same with the cut as it runs: pairs != 0 = uint32 key + uint32 payload pairs (the stable pool form: other shapes, and the
   payloads' twins of the slack buffer and the overflow room in *scratch_bytes); top_bits_setting = VRS_TUNE_MSD_POOL_TOP_BITS as set on
   the context (0 = the library's default, 7).  *first_pass_bits / *second_pass_bits = the digits of the two MSD passes (7 + 7 by
   default, 8 + 7 where 32768 buckets are needed; 0 / 0 = the form does not take this size).  Any pointer may be NULL. */
int vrs_pool_form_shape_ex(uint32_t num_elements, int pairs, int top_bits_setting, uint32_t *first_pass_bits, uint32_t *second_pass_bits,
                           uint32_t *bucket_capacity, uint64_t *scratch_bytes);
/* sorts of the pool form whose local sort was enqueued a second time in a larger workgroup shape: the shape is chosen from
   num_elements alone (the form is enqueued blind), and a bucket of skewed keys may hold more than it takes -- no refusal, the bucket
   lies whole in its slack region; the settle asks for the larger shape (one more kernel, one more host round trip) */
int vrs_one_call_pool_retries(vrs_context ctx, uint64_t *retries);
/* sorts that found no room for the pool form's scratch (vrs_context_trim_scratch in vkradixsort_amd.h tells the rest) */
int vrs_one_call_pool_no_memory(vrs_context ctx, uint64_t *sorts);
/* VRS_TUNE_MSD_POOL_REUSE_LAYOUT: *reused = pool sorts that started in the regions of an earlier sort, *stale = those of them whose keys
   did not fit (run again with their own sample).  Either pointer may be NULL. */
int vrs_one_call_pool_layouts(vrs_context ctx, uint64_t *reused, uint64_t *stale);

/* Ranking method in effect: 1 = __ballot match-any, 2 = returning LDS atomics. */
int vrs_rank_mode(vrs_context ctx);

/* Tuning knobs (performance only, never results). */
typedef enum vrs_tuning_key {
    VRS_TUNE_XCD_REMAP = 0,      /* 1 (default): consecutive tiles share an XCD's L2 in the scatter */
    VRS_TUNE_SCATTER_VARIANT = 1, /* 0 (default): chosen from B; else ITEMS*1000 + WAVES*10 + RANK */
    VRS_TUNE_FUSED_PREFIX = 2,    /* 1 (default): single-launch prefix (chunk sums exchanged through tagged granules) */
    VRS_TUNE_RANK_MODE = 3,       /* 0 (default) auto: LDS-atomic ranking if the device self-test passed at
                                     context creation, else __ballot ranking; 1 force ballot; 2 force atomic */
    VRS_TUNE_ONE_CALL_MIN_KEYS = 4, /* vrs_sort_keys_u32 / _u64 / vrs_sort_pairs_u32 count all four digits in ONE read
                                     and scatter with decoupled look-back (36 instead of 48 bytes per key) from this many
                                     keys on; 0 = never (always the contract passes).  Default 2^13: it is the faster form at every
                                     size above the single-launch threshold (profiles/r02_one_call_crossover.csv). */
    VRS_TUNE_DEBUG_MISPLACE_STREAMS = 5, /* test hook (default 0): run every other tile of a look-back stream behind a
                                     different XCD's L2, i.e. without the placement the fast hand-off relies on */
    VRS_TUNE_LOOKBACK_SPIN_BUDGET = 6, /* polls of a predecessor's unpublished look-back row before a tile stops waiting
                                     and counts its stream's earlier keys itself (default 4096, about 2-4 ms) */
    VRS_TUNE_DEBUG_HOLD_TILE = 7,  /* test hook (default -1 = off): this tile of every look-back stream never publishes
                                     its counts, so its successors must run out of spin budget and recount */
    VRS_TUNE_DIGIT_TABLE_GROUPS = 8, /* groups per pass of the one-call sort's counting read: 8, 16, 32, or 0 (default):
                                     8 below 2^26 keys, 32 from there on */
    VRS_TUNE_HYBRID = 11,          /* vrs_sort_keys_u32 / vrs_sort_pairs_u32 / vrs_sort_keys_u64 of large inputs: 1 (default) = the 28-byte-per-key hybrid form (MSD
                                     partition by the top 14 bits in two look-back passes + an LDS-local sort of every
                                     bucket) whenever every bucket fits a workgroup's LDS, else the four LSD passes (decided
                                     on the device from the same counting read); 0 = always the LSD passes */
    VRS_TUNE_HYBRID_MIN_KEYS = 12, /* the hybrid form is considered from this many keys on, from 5/8 as many pairs and from
                                     half as many 64-bit keys; 0 (default): the measured crossovers -- 1.3 * 10^7 keys, 2.5 * 10^7
                                     pairs, 2 * 10^7 64-bit keys.  Never below 2^22 elements */
    VRS_TUNE_HYBRID_FAST_COUNT = 13, /* the counting read of a sort the hybrid form may take: 0 = always counts the LSD
                                     tables beside the bucket histogram (a refusal costs nothing extra); 2 = counts only
                                     the bucket histogram when the probed key range allows the hybrid form (1 LDS add per
                                     key instead of 5: about 20 us at 10^8 keys) and starts over as an LSD sort, with a second
                                     counting read, if the plan refuses; 1 (default) = adaptive: like 2 while the context's
                                     previous hybrid-capable sort of the same kind (keys / pairs) took the hybrid form, like 0 after a
                                     refusal (64-bit keys: always 2; after a refusal every 16th such sort tries again) */
    VRS_TUNE_FUSED_PLAN = 10,      /* 1: the last workgroup of the one-call sort's counting read turns the digit tables
                                     into the plan; 0 (default): a separate single-workgroup plan kernel (measured a
                                     tie at 10^7 and 10^8 keys) */
    VRS_TUNE_SINGLE_MAX_KEYS = 9,  /* vrs_sort_keys_u32 runs up to this many keys as ONE single_radixsort launch (one
                                     workgroup, four passes) instead of twelve launch-bound multi-block launches;
                                     0 = never.  Default 4096 (measured crossover, profiles/r02_small_n_crossover.csv) */
    VRS_TUNE_ASYNC_SORT = 14,      /* 1 (default on a context with its own stream): vrs_sort_keys_u32 / _pairs_u32 / _keys_u64 only
                                     enqueue and return at once; vrs_sort_settle (or any entry point that settles) finishes what the
                                     plan asks for.  0 (default on a borrowed stream): they return once the plan's head has reached
                                     the host and the whole sort is on the stream */
    VRS_TUNE_PLAN_WAIT_MS = 15,    /* longest wait for a plan's head in milliseconds (default 60000; 0 = no limit) */
    VRS_TUNE_MSD_RESERVE = 16,     /* the two MSD passes of the hybrid form over BARE keys reserve their output ranges with one L2-local atomic
                                      add per tile and digit instead of a decoupled look-back (the order inside a bucket is free there;
                                      payloads always take the stable look-back).  1 (default; 2 means the same): on; 0: look-back
                                      everywhere */
    VRS_TUNE_MSD_POOL = 17,        /* the hybrid form of BARE uint32 keys without its counting read (24 instead of 28 bytes per key): a sample of
                                      1/32 of the keys sizes a region of the partner buffer per (input slice, top byte), the first MSD
                                      pass reserves its output there, the second pass scatters by the next 6 or 7 bits into per-bucket
                                      regions of a context-owned slack buffer (about 1.5 n keys, sized from a sample of the first pass's output),
                                      the local sort reads every bucket in one piece and writes it to its final place.  A sort a verdict
                                      refuses (a region the sample misjudged, a bucket too large) starts over in the counted form with its input untouched.  1 (default) = adaptive: after a refusal the next 15
                                      such sorts of the context take the counted form; 2 = always tried; 0 = never.  Needs
                                      VRS_TUNE_MSD_RESERVE != 0. */
    VRS_TUNE_MSD_POOL_MIN_KEYS = 18, /* the pool form is considered from this many keys on (default and floor 2^22: with one wave per small bucket it beats the
                                        LSD passes from there on, profiles/labs/r05_pool_form.txt section 6) */
    VRS_TUNE_MSD_POOL_SUB_BITS = 20, /* S where a pool sort of bare keys has 256 << S buckets: 0 (default) = by size (6 while the buckets fit a 256-thread local sort, about
                                        1.1 * 10^8 uniform keys, else 7), 6, 7 or 8 (8 with VRS_TUNE_MSD_POOL_TOP_BITS 8: 65536 buckets of one wave each, a lab
                                        setting -- profiles/labs/r06_cut_8_8.txt) */
    VRS_TUNE_MSD_POOL_REUSE_LAYOUT = 22, /* (2: what follows; 1, the default: also the buckets' slack regions are kept -- the plan kernel of such a sort
                                       samples nothing; verified by the second pass like the first pass's regions by the first.)
                                       1 (default): a pool sort of the same size and key floor as the context's last TAKEN one runs its first
                                       pass in the regions that sort's sample laid out -- no sample and no layout kernel (13 us and two launch gaps
                                       at 10^8 keys).  Verified like any layout: keys it does not fit (another distribution, another key range)
                                       flag the sort, which then runs again with a sample of its own (vrs_one_call_pool_layouts counts both).
                                       0: every sort samples */
    VRS_TUNE_MSD_POOL_TOP_BITS = 24, /* how the pool form cuts a sort's 16384 buckets between its two passes: 7 (default) = 128 x 128, a first pass by 7 bits
                                        and a second by 7; 8 = 256 x 64 (the cut until late in round 5); 6 = 64 x 256.  Sorts whose second pass takes
                                        7 bits of 256 top bytes anyway (beyond about 1.1e8 keys) are not affected */
    VRS_TUNE_MSD_POOL_PAIRS = 23, /* 1 (default): uint32 key + uint32 payload pairs may take the pool form too -- its STABLE variant: a tile's place in
                                     a sampled region is its rank there (decoupled look-back, one chain per input slice / per top byte) instead
                                     of a reservation, so equal keys keep their input order; 48 instead of 52 bytes per pair.  0: pairs always
                                     take the counted form */
    VRS_TUNE_MSD_POOL_PAIRS_PACKED = 26, /* the local sort of a pool sort of pairs, per bucket: -1 (default) = by size, 1 = always, 0 = never in its PACKED form --
                                     inside a bucket a key's high bits are the bucket's, so a pair is sorted as ONE word (the key's low 18 bits | the
                                     pair's place in the bucket as read), the payloads wait in registers and take the words' LDS array once the words
                                     are sorted: 43 instead of 70 KB of LDS, three workgroups per CU instead of two.  5-9 % faster from 2.6e7 to 8e7
                                     pairs; level at 10^8 and 2e8 (buckets of 12-13 rows), where the form that carries the payloads through both
                                     passes stays (profiles/labs/r06_pairs_packed.txt) */
    VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS = 27, /* the segmented sorts hand a segment of this many elements or more to the one-call sort
                                       (vrs_sort_keys_u32 / vrs_sort_pairs_u32 on views); shorter ones beyond the LDS tiers are sorted by one
                                       workgroup each.  0 = never.  Default 2^20 */
    VRS_TUNE_TOPK_GRID_MIN_KEYS = 28, /* top-k: segments of this many keys or more take the grid tier (every phase one launch over all of
                                       them); shorter ones beyond the LDS tier are streamed by one workgroup each.  0 = never.  Default 2^17 (the measured
                                       crossover, DESIGN "K7") */
    VRS_TUNE_SEARCH_LDS_BYTES = 29, /* sorted-sequence search: a boundary row whose ranks (4 bytes each, 8 for int64 / float64) take up to this many
                                       bytes is staged and searched in LDS; also the room of the indexed tier's top level.  0 .. 163840.  Default
                                       65536 (DESIGN "K10") */
    VRS_TUNE_SEARCH_TABLE_MIN_QUERIES = 30, /* sorted-sequence search, 2-byte dtypes with one boundary row: from this many queries on every bit
                                       pattern is searched once and the queries are table lookups; 1-byte dtypes from 1/256 of it (at least 1).
                                       0 = never.  Default 65536 */
    VRS_TUNE_SEARCH_INDEX_MIN_QUERIES = 31, /* sorted-sequence search, rows beyond the LDS tier: from this many queries per boundary row on the call
                                       builds the sampled index first.  0 = never (plain lower / upper bound).  Default 65536 */
    VRS_TUNE_BINCOUNT_LDS_BYTES = 32, /* counting (vrs_bin_count): a call whose counters (num_bins x 4 bytes; x 8 with float64 weights) take up to this
                                       many bytes counts in every workgroup's LDS and flushes once; 0 = never.  0 .. 163840.  Default 65536 (two
                                       workgroups per CU): a first setting, not a measured one (DESIGN "K11") */
    VRS_TUNE_SELECT_GRID_MIN_KEYS = 33, /* one-rank selection: segments of this many keys or more take the grid tier (every phase one launch
                                         over all of them); 0 = never.  Default 2^17: top-k's measured crossover for the same walk shape,
                                         a first setting, not measured for this kernel (DESIGN "K12").  vrs_quantile_segments reads it
                                         too: its tiers are the same cuts (DESIGN "K16") */
    VRS_TUNE_SELECT_COMPACT_DIVISOR = 34, /* one-rank selection, grid tier: after a level whose chosen bin holds at most length / value keys
                                         (and at most 1024 per 16384 keys of the segment, what its area holds) the matching keys' ranks are
                                         copied once and the later levels read the copy; 0 = never.  Default 16, not measured (DESIGN "K12").
                                         vrs_quantile_segments reads it too: there the keys of all live groups together count (DESIGN "K16") */
    VRS_TUNE_REDUCE_CHUNK_ROWS = 35, /* segmented reduction: CH, the rows of one chunk (64 .. 4096).  Default 512, a split length known to even out
                                        skewed lists of 1- and 2-KB rows: a first setting (DESIGN "K13") */
    VRS_TUNE_REDUCE_LANE_ROWS = 36, /* segmented reduction, row_width < 64: chunks of up to this many rows (0 .. 64) are added by one lane per column.
                                       Default 16, not measured (DESIGN "K13") */
    VRS_TUNE_SCAN_TILE_ROWS = 37, /* prefix scan: T, the rows of one tile (a multiple of 256 in 256 .. 8192).  Part of the order: another T, other
                                     last bits of a float sum.  Default 2048, a first setting: in the one sweep taken (10^8 float32 along one row,
                                     profiles/labs/k14_scan.txt) the single pass is fastest at 8192, the three-launch form alike at every T (DESIGN "K14") */
    VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS = 38, /* prefix scan: the single pass runs from this many rows per call on where it applies; 0 = never.
                                                Default 1048576, a first setting: at the one size measured (10^8 float32, profiles/labs/k14_scan.txt) the
                                                single pass takes 0.37 ms against 0.26 ms for the three-launch form; other sizes are not measured (DESIGN "K14") */
    VRS_TUNE_SCAN_SPIN_BUDGET = 39, /* prefix scan, single pass: polls of an unpublished status word (0 .. 1048576) before the waiting wave
                                       computes it itself.  Default 4096, the run-length encode's; not measured (DESIGN "K14") */
    VRS_TUNE_COMPACT_TILE_ELEMS = 40, /* compaction: T, the elements of one tile (a multiple of 4096 in 4096 .. 65536): one uint32 of scratch and one
                                         workgroup of each phase per tile.  Default 16384, a first setting: the one sweep taken (10^8 bool flags,
                                         profiles/labs/k15_compact.txt) is flat from 8192 to 65536 (DESIGN "K15") */
    VRS_TUNE_DEBUG_POOL_NO_MEMORY = 25, /* test hook: the next `value` allocations of the pool form's scratch fail as if the device were full */
    VRS_TUNE_DEBUG_XCC_ROTATE = 21, /* test hook: run the placement probe again and rotate its result by `value` places (0 .. 7), as if the probe had
                                       run on another hardware queue than the sorts do (the dispatcher starts every queue's round-robin at its
                                       own XCC, and a stream may move between queues): the pool form's passes take their work lists by the XCC
                                       they run on and stay exact AND fast; the look-back streams and the counted form's reservations fall back
                                       to their placement-independent routes (exact, slower) */
    VRS_TUNE_DEBUG_XCC_STRAY_BLOCK = 19 /* test hook: run the placement probe again and pretend block `value` (0 .. 4095) of it ran on
                                       another XCC: block b -> XCC (b % 8) then holds for most blocks only, and every form that leans on
                                       it (the one-call sorts' look-back streams, reservation, the hybrid and pool forms, vrs_msd_*) is
                                       switched off -- the sorts run the contract stages, which share nothing between workgroups but
                                       agent-scope data.  A negative value probes again without pretending */
} vrs_tuning_key;
int vrs_set_tuning(vrs_context ctx, int key, int value);

/* ---- test hooks ----------------------------------------------------------------------------- */

/* Test hook: copies the per-workgroup offset table (uint32[W*256], multi_radixsort.comp:76's
 * global_offsets for every workgroup) computed by the most recent RADIX_SORT stage. */
int vrs_debug_download_offsets(vrs_context ctx, void *host_data, size_t size_bytes);

/* Test hook: checks on the device that one returning LDS atomic hands same-address lanes their
 * pre-values in ascending lane order (what the RANK_ATOMIC scatter variants rely on); returns the
 * number of lanes whose rank differs from the __ballot-based rank over `rounds` rounds per wave. */
int vrs_debug_atomic_rank_selftest(vrs_context ctx, uint32_t rounds, uint32_t seed, uint64_t *mismatches);

/* The forms of the one-call sorts that share L2-resident words between workgroups rest on where the blocks of a launch run
   ("block b on the XCC of place b % 8 of the probed order"), which the context probes when it is created.  Observed on MI355X: the
   dispatcher's round-robin starts at an XCC of the hardware queue's own, and a HIP stream may move to another queue -- the probed
   order is then rotated.  Every kernel checks (HW_REG_XCC_ID) and stays exact; the first workgroups that find themselves elsewhere
   say so, and the next vrs_sort_* call probes again.  *reprobes = how often that happened; *xcc_map = the probed order (byte x =
   the XCC of the blocks with index % 8 == x); *valid = the probe found the b % 8 rule intact.  Any pointer may be NULL. */
int vrs_debug_xcc_placement(vrs_context ctx, uint64_t *reprobes, uint64_t *xcc_map, int *valid);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* VKRADIXSORT_AMD_TUNE_H */
