/*
 * vkradixsort_amd_ops.h -- the operations built on the sort (build extensions; no reference counterpart).
 *
 * For callers that want more than a sort: segmented sorts, the torch.sort rank maps, top-k, one-rank and multi-rank
 * selection, sorted search, counting, segmented reduction, scan, compaction, run-length encode and unique.  Contexts,
 * buffers, status codes and the sorts themselves are in vkradixsort_amd.h; the VRS_TUNE_* settings the comments name are
 * in vkradixsort_amd_tune.h.
 */
#ifndef VKRADIXSORT_AMD_OPS_H
#define VKRADIXSORT_AMD_OPS_H

#include <stddef.h>
#include <stdint.h>

#include "vkradixsort_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/*
 * Segmented sorts (build extension; no reference counterpart -- the reference's callers sort per-tile or per-cell lists one
 * dispatch at a time): many independent segments of one buffer sorted by one call.  offsets: a device buffer of num_segments + 1
 * uint32; segment i = keys[offsets[i], offsets[i+1]).  Every segment ends up ascending in `keys` (and `values`); the pairs form is
 * stable (each segment == std::stable_sort by key), bare keys == std::sort.  Elements outside [offsets[0], offsets[num_segments])
 * and gaps no segment covers are not touched.  keys_tmp / values_tmp hold num_elements entries and are scratch.
 * num_elements == 0 or num_segments == 0: VRS_OK, nothing done.  NULL handles, buffers of fewer than 4 * num_elements bytes and an
 * offsets buffer of fewer than 4 * (num_segments + 1) bytes: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Malformed
 * offsets never cause an access out of bounds: the kernels clamp each segment to [min(b, n), min(max(b, e), n)) with the function
 * vrs_segment_tier_for exports; what overlapping clamped ranges hold afterwards is unspecified.
 * Tiers by segment length (VRS_SEGMENT_*): one wave per segment up to 1789 elements, one workgroup sorting inside LDS up to 14333
 * keys / 13312 pairs (both read and write each segment once: 8 bytes per key, 16 per pair), one workgroup per segment sorting through
 * keys_tmp below VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, and from there on the one-call sort (vrs_sort_keys_u32 / vrs_sort_pairs_u32) on
 * views of the buffers.  Blocking: below VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS elements in all (no segment can reach the one-call tier)
 * the call only enqueues; otherwise it waits (bounded by VRS_TUNE_PLAN_WAIT_MS) until the classification of the segments has reached
 * pinned host memory -- never for the sorts -- and enqueues the one-call sorts.  A pending one-call sort is settled first.
 * int32 / float32 keys: vrs_transform_keys before and after.
 */
typedef enum vrs_segment_tier {
    VRS_SEGMENT_WAVE = 0,    /* up to 1789 elements (segments of 0 or 1 element are counted here and never touched) */
    VRS_SEGMENT_BLOCK = 1,   /* up to 14333 keys / 13312 pairs */
    VRS_SEGMENT_GLOBAL = 2,  /* longer, below VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS */
    VRS_SEGMENT_ONE_CALL = 3 /* from VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS on */
} vrs_segment_tier;
/* offsets: device buffer of num_segments + 1 uint32; segment i = keys[offsets[i], offsets[i+1]). */
int vrs_sort_segments_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements,
                          vrs_buffer offsets, uint32_t num_segments);
int vrs_sort_segments_pairs_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values,
                                vrs_buffer values_tmp, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments);
/* cumulative per context: segments sorted by each tier (waits for the context's stream; any pointer may be NULL) */
int vrs_segmented_stats(vrs_context ctx, uint64_t *wave_segments, uint64_t *block_segments,
                        uint64_t *global_segments, uint64_t *one_call_segments);
/* the classification both the device and the tests use: a pure function, needs no device.  pairs != 0: key + payload pairs;
 * one_call_min_keys: VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS (0 = never the one-call tier); *tier = VRS_SEGMENT_*. */
int vrs_segment_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, int pairs, uint32_t one_call_min_keys,
                         int *tier, uint32_t *clamped_begin, uint32_t *clamped_end);
/* 64-bit keys: the same contract as the uint32 forms above (offsets, clamping, untouched gaps, NULL and size checks -- keys and
 * keys_tmp hold 8 * num_elements bytes, values and values_tmp 4 * num_elements --, blocking; the pairs form is stable).  Tiers: one
 * wave per segment up to 896 elements, one workgroup sorting inside LDS up to 13312 keys / 6656 pairs (16 bytes of traffic per key,
 * 24 per pair), one workgroup per segment through keys_tmp below VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, and from there on
 * vrs_sort_keys_u64 / vrs_sort_pairs_u64 on views of the buffers.  As in the uint32 forms only the bits that vary within a segment
 * are sorted.  Their segments count in vrs_segmented_stats' four counters. */
int vrs_sort_segments_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements,
                          vrs_buffer offsets, uint32_t num_segments);
int vrs_sort_segments_pairs_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values /* uint32 */,
                                vrs_buffer values_tmp, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments);
/* vrs_segment_tier_for with the 64-bit capacities (a pure function, needs no device) */
int vrs_segment_tier_for_u64(uint32_t begin, uint32_t end, uint32_t num_elements, int pairs, uint32_t one_call_min_keys,
                             int *tier, uint32_t *clamped_begin, uint32_t *clamped_end);

/*
 * torch.sort drop-in (build extension; no reference counterpart): the two streaming kernels around a stable segmented sort of ranks.
 * A tensor is seen as num_elements / row_len rows of row_len elements (num_elements a whole number of rows).
 * vrs_sort_rank_keys writes out_ranks[i] = r(src[i]) -- uint32 for every dtype of up to 4 bytes (the narrow ones zero-extended),
 * uint64 for INT64 / FLOAT64 (vrs_sort_rank_bytes) -- and out_positions[i] = i mod row_len (uint32; may be NULL).  r is torch's order:
 * unsigned as is, signed with the sign bit flipped, floats by the IEEE-754 total order except that -0.0 gets +0.0's rank and every NaN,
 * whatever its sign or payload, the largest rank of its width; VRS_SORT_DESCENDING: ~r.  A stable ascending sort of the ranks (with
 * the positions as payloads) is then torch.sort(x, dim=-1, descending, stable=True) of every row.
 * vrs_sort_restore writes out_values from the sorted ranks by inverting r -- an element of the merged ±0.0 or NaN class reads its bits
 * from src[row * row_len + position] -- and out_indices_i64[i] = positions[i] as int64.  Either output may be NULL; indices need
 * positions, and the values of a float dtype need src and positions.  src is never written.
 * NULL ctx or handles, an unknown dtype or flag bit, num_elements not a whole number of rows and undersized buffers:
 * VRS_ERROR_INVALID_ARGUMENT before anything is enqueued; num_elements == 0: VRS_OK, nothing done.  Stream-ordered on the context's
 * stream; both calls only enqueue (after settling a pending one-call sort).
 *
 * The mode form (torch.mode): vrs_sort_restore with VRS_SORT_MODE reduces every sorted row to its most frequent value and one place
 * where it sits in the input.  ranks: what vrs_sort_rank_keys (ascending, out_positions NULL) wrote, followed by a bare-key sort of
 * every row -- num_elements / row_len = num_rows rows, each sorted ascending; never written.  src: the unsorted input, required, never
 * written.  A run is a maximal stretch of equal ranks inside one row (runs never continue across a row boundary, even when the next
 * row begins with the same rank); the modal run of a row is its longest, among equally long ones the one that starts first -- the
 * smallest value, which is torch's rule.  out_indices_i64[row] = the highest i in [0, row_len) with r(src[row, i]) equal to the modal
 * rank: the last occurrence.  out_values[row] = src[row, that i], the element's own bits (a zero's sign and a NaN's payload are kept;
 * under r, -0.0 and +0.0 are one value and every NaN is one value, the largest).  out_values holds num_rows elements of dtype and
 * out_indices_i64 num_rows int64: both required, nothing beyond num_rows entries is written.
 * With VRS_SORT_MODE `positions` IS NOT POSITIONS BUT THE CALL'S SCRATCH: at least 8 * num_rows bytes on an 8-byte boundary, required,
 * its contents unspecified on entry and afterwards -- a caller that hands it the positions of a sort loses them.
 * The ranks (and the input) are read in tiles of 4096 consecutive elements, whatever the rows; the result does not depend on the tiles,
 * the grid or the run: the only communication between workgroups is an order-independent atomic maximum (a workgroup may read the
 * word first and skip a maximum that could not raise it; it never waits for one).
 * Refused with VRS_ERROR_INVALID_ARGUMENT before anything is enqueued: VRS_SORT_MODE | VRS_SORT_DESCENDING; a NULL src, ranks,
 * positions, out_values or out_indices_i64; undersized buffers; a scratch off an 8-byte boundary.  vrs_sort_rank_keys takes no
 * VRS_SORT_MODE (an unknown flag bit there); bit 4 and above are unknown flag bits for both calls.  Both calls look at their flags
 * before anything else, the context included.  num_elements == 0: VRS_OK, nothing done.  Stream-ordered and enqueue-only (two
 * memsets and three launches after settling a pending one-call sort); the call never waits for the device.
 */
typedef enum vrs_sort_dtype {
    VRS_SORT_INT8 = 0, VRS_SORT_UINT8 = 1, VRS_SORT_INT16 = 2, VRS_SORT_INT32 = 3, VRS_SORT_INT64 = 4,
    VRS_SORT_FLOAT16 = 5, VRS_SORT_BFLOAT16 = 6, VRS_SORT_FLOAT32 = 7, VRS_SORT_FLOAT64 = 8
} vrs_sort_dtype;
enum { VRS_SORT_DESCENDING = 1, VRS_SORT_MODE = 2 /* vrs_sort_restore only: the mode form */ }; /* flags */
int vrs_sort_rank_keys(vrs_context ctx, vrs_buffer src, uint32_t num_elements, uint32_t row_len, int dtype, int flags,
                       vrs_buffer out_ranks /* uint32 or uint64 */, vrs_buffer out_positions /* uint32, may be NULL */);
int vrs_sort_restore(vrs_context ctx, vrs_buffer src, vrs_buffer ranks, vrs_buffer positions /* may be NULL; VRS_SORT_MODE: scratch */,
                     uint32_t num_elements, uint32_t row_len, int dtype, int flags,
                     vrs_buffer out_values /* may be NULL */, vrs_buffer out_indices_i64 /* may be NULL */);
/* the bytes of one rank of dtype: 4 or 8 (a pure function, needs no device) */
int vrs_sort_rank_bytes(int dtype, int *rank_bytes);

/*
 * Top-k selection (build extension; no reference counterpart): the k smallest (or largest) keys of every segment of one buffer and
 * where they sat, by radix select, in one call.  offsets: a device buffer of num_segments + 1 uint32; segment i is
 * keys[offsets[i], offsets[i+1]) clamped exactly as vrs_segment_tier_for clamps it.  key_type (vrs_topk_key_type) fixes the rank of
 * a key x: r(x) = x (U32), x ^ 0x80000000 (I32), the VRS_KEYS_FLOAT32_TO_SORTABLE map (F32, IEEE-754 total order); VRS_TOPK_LARGEST
 * ranks by ~r(x).  The map is applied as the keys are read; `keys` and `offsets` are never written.
 * Segment i of length L and m = min(k, L): its selected set is the first m positions of the STABLE ascending order of r over the
 * segment (smallest r first; equal keys lowest index first).  out_keys[i*k + j] (j < m) holds a selected key's bit pattern and
 * out_indices[i*k + j] its position relative to the clamped begin; with VRS_TOPK_SORTED slot j holds the j-th entry of the stable
 * order, without it the same m entries in some order.  Slots j in [m, k) of both arrays get 0xFFFFFFFF.  out_indices may be NULL.
 * Bytes of the out buffers past 4 * num_segments * k are never written.  scratch: at least vrs_topk_scratch_bytes(...) bytes (at
 * most 4 n + 16 S k + 1 MiB) on an 8-byte boundary (its head holds a 64-bit counter; off it: VRS_ERROR_INVALID_ARGUMENT), contents
 * afterwards unspecified; given that much the call never fails for lack of memory.
 * k == 0 or num_segments == 0: VRS_OK, nothing done.  NULL handles other than out_indices, an unknown key_type or flag bit,
 * num_segments * k >= 2^32 and undersized buffers: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 * Tiers by clamped length (vrs_topk_tier): up to 8192 keys one workgroup per segment selects inside LDS; longer segments are streamed
 * by one workgroup each; from VRS_TUNE_TOPK_GRID_MIN_KEYS on every phase is one launch over all the grid tier's segments.  Stream-
 * ordered on the context's stream; the call only enqueues (after settling a pending one-call sort) -- except with VRS_TOPK_SORTED and
 * k > 4096, where the survivors are sorted by vrs_sort_segments_pairs_u32 (vrs_sort_segments_u32 without out_indices), which may wait
 * for the stream when its work lists grow; that sort's segments count in vrs_segmented_stats.
 *
 * TORCH'S ORDER: key_type VRS_TOPK_DTYPE(d), d a vrs_sort_dtype (I8, U8, I16, I32, I64, F16, BF16, F32, F64; another d:
 * VRS_ERROR_INVALID_ARGUMENT).  keys holds num_elements elements of d IN THEIR OWN WIDTH (1, 2, 4 or 8 bytes) and a segment may begin
 * at any element; out_keys holds num_segments * k elements of that width.  The rank is the one vrs_select_segments takes (torch.sort's:
 * every NaN the largest, -0.0 equal to +0.0, signed integers by value; VRS_TOPK_LARGEST its complement, so NaNs come first), applied
 * in registers as the elements are read; the result is what torch.sort(x, descending = largest, stable = True) puts first.
 * out_keys[i*k + j] holds the selected element's OWN BITS, fetched from keys at its position -- a NaN keeps its payload and a zero its
 * sign; slots [m, k) get all-ones bytes of the element's width (out_indices: 0xFFFFFFFF, as above), and bytes past num_segments * k *
 * width are never written.  The selection reads the rank's significant bits in digits of at most 11 from the top: 1 / 2 / 3 / 6 levels
 * for 8 / 16 / 32 / 64 bits.  The LDS tier holds 32 KB of ranks: 8192 elements of up to 4 bytes, 4096 of 8; the tier of a segment is
 * vrs_select_tier_for(begin, end, num_elements, d, VRS_TUNE_TOPK_GRID_MIN_KEYS) -- vrs_topk_tier_for has no dtype and keeps its meaning
 * for the three 32-bit key types (which it shares with every d of up to 4 bytes).  8-byte elements: flags must carry VRS_TOPK_RANK64
 * (and no other key type may: VRS_ERROR_INVALID_ARGUMENT either way), the same bit vrs_topk_scratch_bytes sizes 8-byte ranks by, and
 * keys and out_keys lie on 8-byte boundaries (VRS_ERROR_INVALID_ARGUMENT before anything is enqueued).  VRS_TOPK_SORTED with k > 4096
 * sorts (rank, position) by vrs_sort_segments_pairs_u32, or vrs_sort_segments_pairs_u64 for 8-byte elements, with or without
 * out_indices (without: the positions live in the scratch buffer), and fetches the own bits by position afterwards.  scratch: at most
 * 4 n + 24 S k + 1 MiB with VRS_TOPK_RANK64.
 */
typedef enum vrs_topk_key_type { VRS_TOPK_U32 = 0, VRS_TOPK_I32 = 1, VRS_TOPK_F32 = 2 } vrs_topk_key_type;
#define VRS_TOPK_DTYPE(d) (0x100 | (d)) /* key_type: an element of vrs_sort_dtype d, ranked in torch's order */
enum { VRS_TOPK_LARGEST = 1, VRS_TOPK_SORTED = 2, VRS_TOPK_RANK64 = 16 }; /* flags */
typedef enum vrs_topk_tier {
    VRS_TOPK_LDS = 0,   /* up to 8192 keys (empty segments included) */
    VRS_TOPK_BLOCK = 1, /* longer, below VRS_TUNE_TOPK_GRID_MIN_KEYS */
    VRS_TOPK_GRID = 2   /* from VRS_TUNE_TOPK_GRID_MIN_KEYS on */
} vrs_topk_tier;
int vrs_topk_segments(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments,
                      uint32_t k, int key_type, int flags, vrs_buffer out_keys, vrs_buffer out_indices /* may be NULL */,
                      vrs_buffer scratch);
/* the scratch vrs_topk_segments needs: a pure function, needs no device (0 for k == 0 or num_segments == 0).  flags: the call's;
 * VRS_TOPK_RANK64 sizes the sort area for 8-byte ranks (never less than without it) */
int vrs_topk_scratch_bytes(uint32_t num_elements, uint32_t num_segments, uint32_t k, int flags, uint64_t *bytes);
/* the classification both the device and the tests use: a pure function, needs no device.  grid_min_keys: VRS_TUNE_TOPK_GRID_MIN_KEYS
 * (0 = never the grid tier); *tier = VRS_TOPK_*. */
int vrs_topk_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, uint32_t grid_min_keys,
                      int *tier, uint32_t *clamped_begin, uint32_t *clamped_end);
/* cumulative per context: segments each tier was given by the classification (waits for the context's stream; any pointer may be
 * NULL).  Grid-tier segments beyond 4096 in one call -- only overlapping ranges get there -- count as grid and run in the BLOCK kernel. */
int vrs_topk_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments);

/*
 * One-rank selection (build extension; no reference counterpart): torch.kthvalue / torch.median / torch.nanmedian -- one entry of every
 * segment's sorted order, its own bits and where it sat, by radix select, in one call.  src: num_elements elements of `dtype` (a
 * vrs_sort_dtype); offsets: a device buffer of num_segments + 1 uint32; segment i is src[offsets[i], offsets[i+1]) clamped exactly as
 * vrs_segment_tier_for clamps it, L its length.  r is the rank vrs_sort_rank_keys gives (unsigned as is; signed with the sign bit
 * flipped; floats by value with -0.0 == +0.0 and every NaN the largest); VRS_SELECT_DESCENDING ranks by the complement of r.  The map is
 * applied in registers as the elements are read, element by element (a segment may begin at any element offset); src and offsets are
 * never written.
 * The call answers entry j (0-based) of the segment's STABLE ascending order of r -- the element sort(..., stable=True) puts at
 * position j: out_values[i] gets that element's own bits, read from src (a NaN's payload and a zero's sign are kept), out_indices[i]
 * (may be NULL) its position relative to the clamped begin as uint32.  A segment without such a j (L == 0; VRS_SELECT_KTH with k > L)
 * gets index 0xFFFFFFFF and all-zero value bits.  With nans = the segment's keys of the NaN class (0 for integer dtypes), counted by the
 * first read, `mode` (vrs_select_mode) fixes j -- the rule is vrs_select_target_for's:
 *   VRS_SELECT_KTH        j = k - 1 (1 <= k)
 *   VRS_SELECT_MEDIAN     j = (L - 1) / 2 when nans == 0, else the first NaN of the stable order (L - nans ascending, 0 descending):
 *                         torch's rule, a row with any NaN has median NaN
 *   VRS_SELECT_NANMEDIAN  j = (L - nans - 1) / 2 among the non-NaN keys when nans < L (they follow the NaNs when descending), else the
 *                         first NaN
 * scratch: at least vrs_select_scratch_bytes(...) bytes on an 8-byte boundary (whatever the dtype: its head holds a 64-bit counter),
 * contents afterwards unspecified; given that much the call never fails for
 * lack of memory.  num_segments == 0: VRS_OK, nothing done.  An unknown dtype, mode or flag bit, k == 0 with VRS_SELECT_KTH, a NULL
 * context, src, offsets, out_values or scratch, undersized buffers (src: num_elements elements; out_values: num_segments elements;
 * out_indices: num_segments uint32), 8-byte elements off an 8-byte boundary and a scratch off one: VRS_ERROR_INVALID_ARGUMENT before
 * anything is enqueued.
 * Digits of at most 11 bits from the top of the dtype's 8 / 16 / 32 / 64 bits (1 / 2 / 3 / 6 levels); a segment is done once the
 * chosen bin holds one key.  Tiers by clamped length (vrs_select_tier, decided by vrs_select_tier_for): ranks that fit 32 KB (8192 keys
 * of up to 4 bytes, 4096 of 8) are read once into the LDS of one workgroup; longer segments are streamed by one workgroup each, one read
 * per level; from VRS_TUNE_SELECT_GRID_MIN_KEYS on every phase is one launch over all the grid tier's segments, and after a level whose
 * chosen bin holds at most L / VRS_TUNE_SELECT_COMPACT_DIVISOR keys, with two levels or more still to come (the copy costs one read of
 * the segment, as a level does), the ranks of those keys are copied once into the scratch buffer (1024 ranks per 16384 keys of the
 * segment: a bin beyond that is not copied, whatever the divisor), where the later levels read them.
 * The index is found by counting the keys that match the final prefix in index order; nothing is emitted or sorted.
 * Stream-ordered on the context's stream; the call only enqueues (after settling a pending one-call sort) and never waits for the device.
 */
typedef enum vrs_select_mode { VRS_SELECT_KTH = 0, VRS_SELECT_MEDIAN = 1, VRS_SELECT_NANMEDIAN = 2 } vrs_select_mode;
enum { VRS_SELECT_DESCENDING = 1 }; /* flags */
typedef enum vrs_select_tier {
    VRS_SELECT_LDS = 0,   /* ranks of up to 32 KB (empty segments included) */
    VRS_SELECT_BLOCK = 1, /* longer, below VRS_TUNE_SELECT_GRID_MIN_KEYS */
    VRS_SELECT_GRID = 2   /* from VRS_TUNE_SELECT_GRID_MIN_KEYS on */
} vrs_select_tier;
int vrs_select_segments(vrs_context ctx, vrs_buffer src, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments,
                        int dtype /* vrs_sort_dtype */, int mode, uint32_t k, int flags, vrs_buffer out_values,
                        vrs_buffer out_indices /* may be NULL */, vrs_buffer scratch);
/* the scratch vrs_select_segments needs: a pure function, needs no device.  0 for num_segments == 0; with w = the bytes of the dtype's
 * rank (vrs_sort_rank_bytes) at most num_elements * w / 16 + 4 * num_elements + 4 * num_segments + 1 MiB; never shrinks as
 * num_elements grows. */
int vrs_select_scratch_bytes(uint32_t num_elements, uint32_t num_segments, int dtype, uint64_t *bytes);
/* the classification both the device and the tests use: a pure function, needs no device.  grid_min_keys: the value of
 * VRS_TUNE_SELECT_GRID_MIN_KEYS (0 = never the grid tier); *tier = VRS_SELECT_*. */
int vrs_select_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, int dtype, uint32_t grid_min_keys,
                        uint32_t *clamped_begin, uint32_t *clamped_end, int *tier);
/* the rule both the device and the tests use for the entry a mode asks for: a pure function, needs no device.  *valid = 0: the segment
 * has no such entry (*j = 0).  Refuses an unknown mode and nans > len. */
int vrs_select_target_for(int mode, uint32_t k, uint32_t len, uint32_t nans, int descending, uint32_t *j, int *valid);
/* cumulative per context: segments each tier was given by the classification, and grid-tier segments that compacted (waits for the
 * context's stream; any pointer may be NULL).  Grid-tier segments beyond the scratch buffer's slots -- num_elements / 8193, 4096 at the
 * most -- count as grid and run in the BLOCK kernel. */
int vrs_select_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments,
                     uint64_t *compacted_segments);

/*
 * Multi-rank selection (build extension; no reference counterpart): torch.quantile / torch.nanquantile -- for every segment and every q
 * the two neighbouring entries of the segment's ascending order, the weight between them and the interpolated quantile, by a radix
 * select that carries every target through one sequence of reads.  src: num_elements elements of `dtype` (VRS_SORT_F32 or VRS_SORT_F64,
 * as torch); offsets: a device buffer of num_segments + 1 uint32; segment i is src[offsets[i], offsets[i+1]) clamped exactly as
 * vrs_select_segments clamps it, L its length; a segment may begin at any element.  q: num_q doubles on the host, each in [0, 1] (they
 * are copied before the call returns).  flags: VRS_QUANTILE_IGNORE_NAN gives the nanquantile rule.
 * Outputs: [num_segments, num_q] elements of `dtype` each; out_values the quantile; out_lower, out_upper and out_weight (each may be NULL)
 * the two order statistics and the weight.  A segment with no answer -- L == 0, any NaN without the flag, NaNs alone with it -- gets the
 * quiet NaN in all four.  The rule (vrs_quantile_target_for; T the dtype, nans the segment's NaNs, counted by the first read):
 *   L' = L, or L - nans with the flag;  r = T(q) * T(L' - 1), one rounded multiply;  LOWER / HIGHER / NEAREST: r = floor / ceil /
 *   round-half-even of r;  lower = floor(r), upper = ceil(r), both clamped to L' - 1 (T(L' - 1) rounds up past the last index for float32
 *   segments longer than 2^24);  weight = r - floor(r), 0.5 for MIDPOINT, 0 for the three single-entry modes;
 *   value = weight < 0.5 ? a + weight * (b - a) : b - (b - a) * (1 - weight) for LINEAR and MIDPOINT (a, b the two entries' values; every
 *   operation rounded on its own, the same bits on the host and on the device; a NaN result is the quiet NaN), a for the rest.
 * The entries' values are rebuilt from their ranks: +0.0 for either zero (the NaN class is never an entry).
 * The selection: per segment the distinct entries asked for, ascending, 16 at the most (VRS_QUANTILE_MAX_TARGETS: num_q * 2 for LINEAR
 * and MIDPOINT, num_q for the rest, must not exceed it).  Levels as vrs_quantile_level_for gives them: the top 11 bits of the rank in one
 * histogram over every key, then 8 bits at a time (the last level: what is left; 4 levels for float32, 8 for float64) in one 256-bin
 * histogram per group of targets that share their prefix so far -- one read of its source per level, whatever the number of targets.
 * Tiers by clamped length exactly as vrs_select_tier_for decides them (the same VRS_TUNE_SELECT_GRID_MIN_KEYS): LDS, BLOCK and GRID; in
 * the GRID tier, after a level whose live groups together hold at most L / VRS_TUNE_SELECT_COMPACT_DIVISOR keys (and at most 1024 per
 * 16384 keys of the segment), with two levels or more still to come, the ranks of those keys are copied once into the scratch buffer,
 * where the later levels read them.
 * scratch: at least vrs_quantile_scratch_bytes(...) bytes on an 8-byte boundary, contents afterwards unspecified; given that much the
 * call never fails for lack of memory.  num_segments == 0 or num_q == 0: VRS_OK, nothing done.  Another dtype, an unknown interpolation
 * or flag bit, a q outside [0, 1] or NaN, more targets than VRS_QUANTILE_MAX_TARGETS, a NULL context, src, offsets, out_values or
 * scratch, undersized buffers and float64 off an 8-byte boundary: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 * Stream-ordered on the context's stream; the call only enqueues (after settling a pending one-call sort) and never waits for the device.
 */
typedef enum vrs_quantile_interpolation {
    VRS_QUANTILE_LINEAR = 0,
    VRS_QUANTILE_LOWER = 1,
    VRS_QUANTILE_HIGHER = 2,
    VRS_QUANTILE_MIDPOINT = 3,
    VRS_QUANTILE_NEAREST = 4
} vrs_quantile_interpolation;
enum { VRS_QUANTILE_IGNORE_NAN = 1 }; /* flags */
enum { VRS_QUANTILE_MAX_TARGETS = 16 };
int vrs_quantile_segments(vrs_context ctx, vrs_buffer src, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments,
                          int dtype /* VRS_SORT_F32 or VRS_SORT_F64 */, const double *q, uint32_t num_q, int interpolation, int flags,
                          vrs_buffer out_values, vrs_buffer out_lower /* may be NULL */, vrs_buffer out_upper /* may be NULL */,
                          vrs_buffer out_weight /* may be NULL */, vrs_buffer scratch);
/* the scratch vrs_quantile_segments needs: a pure function, needs no device.  0 for num_segments == 0; never shrinks as an argument grows:
 * 16 KiB of histograms and 512 bytes of state per grid slot (num_elements / 8193 slots, 4096 at the most), 4 bytes per segment, and
 * 1024 ranks per 16384 elements. */
int vrs_quantile_scratch_bytes(uint32_t num_elements, uint32_t num_segments, int dtype, uint64_t *bytes);
/* the rule both the device and the tests use for the entries a q asks for (above): a pure function, needs no device.  *weight: the
 * dtype's weight, widened.  *valid = 0: the segment has no answer (*lower = *upper = 0).  Refuses what vrs_quantile_segments refuses,
 * and nans > len. */
int vrs_quantile_target_for(int dtype, int interpolation, double q, uint32_t len, uint32_t nans, int ignore_nan, uint32_t *lower,
                            uint32_t *upper, double *weight, int *valid);
/* the level table of a rank of `bits` bits (32 or 64): *levels, and the digit of level `level` (0 = the top one) as rank >> *shift &
 * *mask.  32: 11, 8, 8, 5 bits; 64: 11, 8 x 6, 5.  A pure function, needs no device. */
int vrs_quantile_level_for(int bits, int level, uint32_t *shift, uint32_t *mask, int *levels);
/* vrs_quantile_segments evaluated on the host, every pointer in host memory: each segment's ranks sorted, then the same rule and the same
 * interpolation.  The device's outputs equal these bit for bit.  Refuses what vrs_quantile_segments refuses. */
int vrs_quantile_host(const void *src, uint32_t num_elements, const uint32_t *offsets, uint32_t num_segments, int dtype, const double *q,
                      uint32_t num_q, int interpolation, int flags, void *out_values, void *out_lower /* may be NULL */,
                      void *out_upper /* may be NULL */, void *out_weight /* may be NULL */);
/* cumulative per context, this call's own counters: segments each tier was given by the classification, and grid-tier segments that
 * sieved (waits for the context's stream; any pointer may be NULL).  Grid-tier segments beyond the scratch buffer's slots count as grid
 * and run in the BLOCK kernel. */
int vrs_quantile_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments,
                       uint64_t *sieved_segments);

/*
 * Sorted-sequence search (build extension; no reference counterpart): torch.searchsorted / torch.bucketize / numpy.searchsorted.
 * `boundaries`: num_boundaries elements of `dtype` (a vrs_sort_dtype) as rows of boundary_row_len, each ascending in r; `queries`:
 * num_queries elements of the same dtype as rows of query_row_len.  Either there is exactly one boundary row, which every query
 * searches (bucketize, 1-D searchsorted), or as many as query rows, query row i searching boundary row i (N-D searchsorted).
 * With r = the rank vrs_sort_rank_keys gives (unsigned as is; signed with the sign bit flipped; floats by value with -0.0 == +0.0 and
 * every NaN, whatever its sign or payload, equal to every other NaN and above +inf):
 *     out[q] = number of boundaries b of the query's row with r(b) <  r(queries[q])      (left, the default)
 *     out[q] = number of boundaries b of the query's row with r(b) <= r(queries[q])      (VRS_SEARCH_RIGHT)
 * as uint32 words (the bit patterns of int32 below 2^31), or int64 with VRS_SEARCH_OUT_INT64.  This is numpy.searchsorted's answer
 * always and torch.searchsorted's whenever the boundaries hold no NaN (NaN queries included); with NaN boundaries torch's answer
 * depends on the midpoints its binary search visits, this one does not.  Boundaries that are not ascending: some value in
 * [0, boundary_row_len] per query, no fault.  sorter: NULL, or num_boundaries int64 positions within the row -- boundary j of a row is
 * then row[sorter[j]] (an entry outside [0, boundary_row_len) reads the row's last element).  The rank map is applied as elements are
 * read; boundaries, queries and sorter are never written, nor are bytes of `out` past num_queries entries.
 * num_queries == 0: VRS_OK, nothing done.  num_boundaries == 0: every output 0.  A NULL context or out (boundaries, when
 * there are any; queries on a NULL context -- on a valid one NULL queries are the identity queries below), an unknown dtype or flag bit, element counts that are not whole rows, row counts that neither match nor equal one
 * and undersized buffers: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Both element counts are below 2^32.
 * Tiers (vrs_search_tier, decided by vrs_search_tier_for from the shape and three thresholds): a row whose ranks fit
 * VRS_TUNE_SEARCH_LDS_BYTES is staged in LDS by every workgroup and searched there; 1- and 2-byte dtypes with one boundary row and
 * VRS_TUNE_SEARCH_TABLE_MIN_QUERIES queries or more search every bit pattern once and then look every query up in that table;
 * longer rows with VRS_TUNE_SEARCH_INDEX_MIN_QUERIES queries or more per row are searched through a sampled index (the rank of the
 * last boundary of every 128-byte line, written by one pass per call; its top level in LDS): three or four dependent global line
 * fetches per query instead of about log2(boundary_row_len) - 5; everything else is a plain lower / upper bound in global memory.
 * scratch: at least the bytes vrs_search_plan (or vrs_search_scratch_bytes for the tier) reports, may be NULL when that is 0 (the LDS
 * and direct tiers); contents on entry unspecified, afterwards unspecified.  Stream-ordered on the context's stream; the call only
 * enqueues (after settling a pending one-call sort) and never waits for the device.
 * Identity queries (run-length decode; torch.repeat_interleave): queries == NULL with num_queries > 0 on a valid context means that
 * query row i holds the values 0, 1, ..., query_row_len - 1 as integers of `dtype`, every row starting again at 0, also when all rows
 * search the one boundary row.  The result is by definition what the same call writes when those queries are materialised, with
 * VRS_SEARCH_RIGHT, VRS_SEARCH_OUT_INT64 and one boundary row or one per query row as above; with the boundaries the ends of runs
 * (a cumulative sum of counts) and VRS_SEARCH_RIGHT, out[j] is the run of element j.  It is computed as a merge, not a search: per
 * 4096 outputs the two ends are found by a few rounds of evenly spaced probes, the boundaries between them are read once and the
 * outputs written once.  dtype is VRS_SORT_INT32 or VRS_SORT_INT64; any other dtype, VRS_SORT_INT32 with query_row_len above 2^31
 * (its queries would pass 2^31 - 1) and a sorter other than NULL: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  scratch may
 * be NULL: the form needs none.  num_boundaries == 0 gives zeros and num_queries == 0 returns VRS_OK as above; boundaries that are not
 * ascending give some value in [0, boundary_row_len] per output, and nothing outside out's num_queries entries is written.  The form
 * runs in no tier: it adds to none of the counters of vrs_search_stats, and vrs_search_plan, vrs_search_tier_for and
 * vrs_search_scratch_bytes, which take no queries, cannot express it -- their answers are those of the materialised call.
 * Membership (torch.isin / numpy.isin): with VRS_SEARCH_MEMBER `out` is ONE BYTE per query,
 *     out[q] = 1 when some boundary b of the query's row has r(b) == r(queries[q]) and queries[q] is not a NaN, 0 otherwise,
 * and with VRS_SEARCH_MEMBER_INVERT as well the two values are swapped.  So -0.0 is a member of a row that holds +0.0 (and the reverse),
 * and a NaN is a member of nothing, even of a row that holds NaNs: IEEE ==, numpy.isin's answer and torch.isin's.  Everything else is
 * the counting call's: the rank map applied as elements are read, the sorter, one boundary row or one per query row, the tier (the one
 * vrs_search_plan reports: these take no flags), its scratch (the table keeps its 4-byte entries and holds 0 / 1 in them) and its
 * counter of vrs_search_stats; stream-ordered, enqueue-only, never waits.  Nothing but out's num_queries bytes is written.
 * num_queries == 0: VRS_OK.  num_boundaries == 0: every output 0 (inverted: 1).  Boundaries that are not ascending: 0 or 1 per query,
 * no fault.  The left count c of a query is found as above, then boundary c is fetched once -- never when c == boundary_row_len.
 * VRS_SEARCH_MEMBER with VRS_SEARCH_RIGHT or VRS_SEARCH_OUT_INT64, VRS_SEARCH_MEMBER_INVERT without VRS_SEARCH_MEMBER,
 * VRS_SEARCH_MEMBER with queries == NULL (the identity queries) and an out of fewer than num_queries bytes:
 * VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 */
enum { VRS_SEARCH_RIGHT = 1, VRS_SEARCH_OUT_INT64 = 2, /* flags; bits 4 and 8 are none: they stay unknown flag bits and are refused */
       VRS_SEARCH_MEMBER = 16,       /* out: one byte per query, 1 = the query equals some boundary of its row */
       VRS_SEARCH_MEMBER_INVERT = 32 /* with VRS_SEARCH_MEMBER only: 0 = the query equals some boundary of its row */ };
typedef enum vrs_search_tier {
    VRS_SEARCH_LDS = 0,    /* the row's ranks fit VRS_TUNE_SEARCH_LDS_BYTES (no boundaries at all included) */
    VRS_SEARCH_TABLE = 1,  /* 1- / 2-byte dtype, one boundary row, VRS_TUNE_SEARCH_TABLE_MIN_QUERIES queries or more (1-byte: 1/256 of it) */
    VRS_SEARCH_DIRECT = 2, /* longer rows, fewer than VRS_TUNE_SEARCH_INDEX_MIN_QUERIES queries per boundary row */
    VRS_SEARCH_INDEXED = 3 /* longer rows, that many queries or more */
} vrs_search_tier;
int vrs_search_sorted(vrs_context ctx, vrs_buffer boundaries, uint32_t num_boundaries, uint32_t boundary_row_len, vrs_buffer queries,
                      uint32_t num_queries, uint32_t query_row_len, int dtype, int flags, vrs_buffer sorter /* may be NULL */,
                      vrs_buffer out, vrs_buffer scratch /* may be NULL when no scratch is needed */);
/* the classification both the device and the tests use: a pure function, needs no device.  The three thresholds are the values of
 * VRS_TUNE_SEARCH_LDS_BYTES, _TABLE_MIN_QUERIES and _INDEX_MIN_QUERIES (0 = never that tier; rows without boundaries are always
 * VRS_SEARCH_LDS).  Refuses what vrs_search_sorted refuses about the shape and the dtype.  *tier = VRS_SEARCH_*. */
int vrs_search_tier_for(uint32_t num_boundaries, uint32_t boundary_row_len, uint32_t num_queries, uint32_t query_row_len, int dtype,
                        uint32_t lds_bytes, uint32_t table_min_queries, uint32_t index_min_queries, int *tier);
/* the scratch a call in `tier` needs: a pure function, needs no device.  0 for VRS_SEARCH_LDS and VRS_SEARCH_DIRECT; the table: 4 bytes
 * per bit pattern (1 KiB / 256 KiB); the index: with e = the dtype's bytes and w = its rank's bytes (vrs_sort_rank_bytes), at most
 * (num_boundaries * e / 128) * w * 33 / 32 + (has_sorter ? num_boundaries * w : 0) + 1024 bytes. */
int vrs_search_scratch_bytes(uint32_t num_boundaries, uint32_t boundary_row_len, int dtype, int has_sorter, int tier, uint64_t *bytes);
/* the tier vrs_search_sorted will take on this context (its tuning as it stands) and the scratch that needs; no device work */
int vrs_search_plan(vrs_context ctx, uint32_t num_boundaries, uint32_t boundary_row_len, uint32_t num_queries, uint32_t query_row_len,
                    int dtype, int has_sorter, int *tier, uint64_t *scratch_bytes);
/* cumulative per context: calls each tier ran (calls without queries or without boundaries run none).  Counted on the host: does not
 * wait for the stream.  Any pointer may be NULL. */
int vrs_search_stats(vrs_context ctx, uint64_t *lds_calls, uint64_t *table_calls, uint64_t *direct_calls, uint64_t *indexed_calls);

/*
 * Counting (build extension; no reference counterpart): torch.bincount / torch.histc, and the count behind torch.histogram.
 * `values`: num_values elements of `dtype` (a vrs_sort_dtype).  `mode` says how an element x becomes a bin in [0, num_bins):
 *   VRS_BIN_INDEX   uint8, int8, int16, int32 or int64 elements: the element is the bin.  x < 0 and x >= num_bins have none.
 *   VRS_BIN_LINEAR  float16, bfloat16, float32 or float64 elements and a finite range lo < hi:
 *                       bin = (int)((x - lo) * num_bins / (hi - lo)),   bin == num_bins becomes num_bins - 1
 *                   in float32 (float64 elements: in float64; 16-bit elements are widened to float32 first; lo, hi and num_bins are
 *                   converted to that type), the three operations in this order, each rounded on its own -- torch.histc's rule,
 *                   and the definition of this mode (vrs_bin_linear_host evaluates the same function on the host).  x < lo, x > hi
 *                   and NaN have none.
 * Every element that has a bin adds 1 to it, or, with weight_dtype = VRS_SORT_FLOAT32 / VRS_SORT_FLOAT64 (otherwise
 * VRS_BIN_NO_WEIGHTS), its weight: `weights` holds num_values of them.  `out` takes num_bins results of out_dtype:
 *   counts        int64, or float16 / bfloat16 / float32 / float64.  Counts are accumulated as 32-bit integers (a call takes fewer
 *                 than 2^32 elements) and converted once: a float result is the correctly rounded count, where a sum of float ones
 *                 stops growing at 2^24 in float32 (as torch.histc's does).
 *   weighted sums out_dtype = weight_dtype; summed in that type by float atomics, in no specified order (as torch).
 * `skipped`: NULL, or two uint64 that receive the number of elements below the range (x < 0; x < lo) and at or beyond its end
 * (x >= num_bins; x > hi).  NaN counts in neither.
 * The library clears what it accumulates into (on the context's stream): `out` for int64 counts and weighted sums, otherwise 32-bit
 * counters in `scratch`, which a finish kernel converts.  scratch: at least the bytes vrs_bin_count_plan / vrs_bin_count_scratch_bytes
 * report (never 0: the two skip counters live there); contents on entry and afterwards unspecified.  values and weights are never
 * written, nor are bytes of `out` past num_bins entries.  num_values == 0: every output 0.
 * Tiers (vrs_bincount_tier, decided by vrs_bin_count_tier_for): counters of num_bins x 4 bytes (8 with float64 weights) that fit
 * VRS_TUNE_BINCOUNT_LDS_BYTES are kept in every workgroup's LDS and flushed once, the non-zero ones only; otherwise every add is a
 * global atomic.  In both a wave whose elements all fall into one bin adds once.
 * A NULL context, out or scratch (values / weights when there are elements), a dtype outside the mode's list, an unknown mode,
 * num_bins == 0, a range that is not finite, not lo < hi or whose width hi - lo overflows the type the rule is evaluated in (linear
 * mode; lo = -3e38, hi = 3e38 in float32), a weight dtype other than the two, an out dtype outside the list above and undersized
 * buffers (out: num_bins entries; values, weights: num_values; skipped: 16 bytes; scratch: what the plan reports):
 * VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Stream-ordered on the context's stream;
 * the call only enqueues (after settling a pending one-call sort) and never waits for the device.
 */
enum { VRS_BIN_INDEX = 0, VRS_BIN_LINEAR = 1 }; /* mode */
enum { VRS_BIN_NO_WEIGHTS = -1 };               /* weight_dtype of a count */
typedef enum vrs_bincount_tier {
    VRS_BINCOUNT_LDS = 0,   /* the counters fit VRS_TUNE_BINCOUNT_LDS_BYTES */
    VRS_BINCOUNT_GLOBAL = 1 /* every larger num_bins */
} vrs_bincount_tier;
int vrs_bin_count(vrs_context ctx, vrs_buffer values, uint32_t num_values, int dtype, int mode, double lo, double hi, uint32_t num_bins,
                  vrs_buffer weights /* NULL without weights */, int weight_dtype, int out_dtype, vrs_buffer out,
                  vrs_buffer skipped /* may be NULL */, vrs_buffer scratch);
/* the classification both the device and the tests use: a pure function, needs no device.  counter_bytes: 4, or 8 for float64
 * weights; lds_bytes: the value of VRS_TUNE_BINCOUNT_LDS_BYTES (0 = never the LDS tier; clamped to 163840).  *tier = VRS_BINCOUNT_*. */
int vrs_bin_count_tier_for(uint32_t num_bins, uint32_t counter_bytes, uint32_t lds_bytes, int *tier);
/* the scratch a call needs: a pure function, needs no device.  256 bytes, and 4 bytes per bin (rounded up to 256) more for counts
 * whose out dtype is not int64.  Refuses what vrs_bin_count refuses about num_bins and the two dtypes. */
int vrs_bin_count_scratch_bytes(uint32_t num_bins, int weight_dtype, int out_dtype, uint64_t *bytes);
/* the tier vrs_bin_count will take on this context (its tuning as it stands) and the scratch it needs; no device work */
int vrs_bin_count_plan(vrs_context ctx, uint32_t num_bins, int weight_dtype, int out_dtype, int *tier, uint64_t *scratch_bytes);
/* cumulative per context: calls each tier ran (calls without elements run none).  Counted on the host: does not wait for the stream.
 * Either pointer may be NULL. */
int vrs_bin_count_stats(vrs_context ctx, uint64_t *lds_calls, uint64_t *global_calls);
/* VRS_BIN_LINEAR's rule on the host, by the function the kernels compile: bins[i] = the bin of element i of `values` (host memory,
 * num_values elements of a float dtype), or -1 when it has none.  Needs no device. */
int vrs_bin_linear_host(const void *values, uint64_t num_values, int dtype, double lo, double hi, uint32_t num_bins, int64_t *bins);

/*
 * K13 -- segmented reduction over rows (build extension; no reference counterpart): torch.segment_reduce, and the sum behind
 * index_add / index_reduce / scatter_reduce once the contributions are sorted by destination.  `values`: num_rows rows of row_width
 * elements of `dtype` (int32, int64, float16, bfloat16, float32 or float64 of vrs_sort_dtype); element (row, column) sits at
 * (size_t)row * row_width + column.  `order`: NULL, or num_rows uint32 -- reduction row i is then values row order[i] (an entry beyond
 * num_rows - 1 reads row num_rows - 1).  `offsets`: num_segments + 1 uint32 that index reduction rows; segment s is the reduction rows
 * [offsets[s], offsets[s+1]) clamped exactly as vrs_segment_tier_for clamps it.  out row s = op over the segment's rows, column by
 * column; with `init` (num_segments rows) op(init row s, that); a segment without rows answers init's own bits, or without init the
 * op's identity: sum 0, prod 1, min +inf (the integer type's maximum), max -inf (the type's minimum).  min and max answer NaN when any
 * row holds one, as torch; integer sums and products wrap.
 * THE ORDER is fixed, so the same input gives the same bits on every run, device and grid; vrs_segment_reduce_host evaluates the same
 * functions on the host.  With CH = VRS_TUNE_REDUCE_CHUNK_ROWS and L rows: reduce(rows) = chunk(rows) when L <= CH, else reduce of the
 * list [chunk(rows[i * CH, min(L, (i + 1) * CH))) for i = 0 ..].  Partials are kept in the accumulator type: float32 for float16 and
 * bfloat16 values -- rounded to the value type once, at the end, to nearest even --, the value type otherwise.  chunk() starts every
 * accumulator at the identity and has three lane maps (vrs_reduce_map), chosen from the chunk's rows and row_width alone
 * (vrs_segment_reduce_map_for):
 *   VRS_REDUCE_MAP_LANE     row_width < 64, at most VRS_TUNE_REDUCE_LANE_ROWS rows: one accumulator, the rows added in order
 *   VRS_REDUCE_MAP_ROWS     row_width < 64, more rows: G = 64 / C' accumulators, C' the power of two at or above row_width; row t goes
 *                           to accumulator t mod G, in order; then for s = G/2, G/4 .. 1: acc[g] = op(acc[g], acc[g + s]) for g < s;
 *                           acc[0] answers.  An accumulator without a row keeps the identity, which changes nothing it meets
 *   VRS_REDUCE_MAP_COLUMNS  row_width >= 64: one accumulator per column, the rows added in order
 * Because every accumulator starts at +0.0, a float sum that is zero is +0.0 whatever the signs of the zeros that went in.
 * Kernels: a classify kernel writes the work lists into `scratch` (segments of the lane map; chunk items for every level); then one
 * launch for the lane map and one per level, whose grids are host-side bounds and whose workgroups read the real counts on the device.
 * Level k writes the partials level k + 1 reads into `scratch`.  No float atomics anywhere.  values, order, offsets and init are never
 * written; out may not overlap them, except that out == init is allowed; every element of out is written exactly once.
 * scratch: at least vrs_segment_reduce_scratch_bytes(...) bytes for the context's VRS_TUNE_REDUCE_CHUNK_ROWS, contents afterwards
 * unspecified.  The bound counts on segments that do not overlap; where clamped ranges overlap so far that it does not hold, the
 * segments that find no room answer as segments without rows (never an access out of bounds).
 * num_segments == 0: VRS_OK, nothing done.  A NULL context, values (when there are rows), offsets, out or scratch, an unknown dtype or
 * op, row_width == 0, undersized buffers (values: num_rows x row_width elements; order: num_rows uint32; offsets: num_segments + 1;
 * init, out: num_segments x row_width elements; scratch: the bound), 8-byte elements off an 8-byte boundary and an out that overlaps
 * an input: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Stream-ordered on the context's stream; the call only enqueues
 * (after settling a pending one-call sort) and never waits for the device.
 */
typedef enum vrs_reduce_op { VRS_REDUCE_SUM = 0, VRS_REDUCE_PROD = 1, VRS_REDUCE_MIN = 2, VRS_REDUCE_MAX = 3 } vrs_reduce_op;
typedef enum vrs_reduce_map { VRS_REDUCE_MAP_LANE = 0, VRS_REDUCE_MAP_ROWS = 1, VRS_REDUCE_MAP_COLUMNS = 2 } vrs_reduce_map;
int vrs_segment_reduce(vrs_context ctx, vrs_buffer values, uint32_t num_rows, uint32_t row_width, int dtype,
                       vrs_buffer order /* NULL, or num_rows uint32: reduction row i is values row order[i] */,
                       vrs_buffer offsets, uint32_t num_segments, int op,
                       vrs_buffer init /* NULL, or num_segments x row_width values */,
                       vrs_buffer out /* num_segments x row_width */, vrs_buffer scratch);
/* the scratch a call needs with chunk_rows = the context's VRS_TUNE_REDUCE_CHUNK_ROWS (64 .. 4096): a pure function, needs no device.
 * Never shrinks as num_rows grows, never grows with chunk_rows.  With a = the accumulator's bytes (8 for int64 / float64, else 4), about
 * 4 x num_segments + 16 x (num_rows / chunk_rows + num_segments) + 2 x a x row_width x num_rows / chunk_rows bytes. */
int vrs_segment_reduce_scratch_bytes(uint32_t num_rows, uint32_t row_width, uint32_t num_segments, int dtype, uint32_t chunk_rows,
                                     uint64_t *bytes);
/* the lane map of a chunk of chunk_len rows (lane_rows: VRS_TUNE_REDUCE_LANE_ROWS, 0 .. 64): a pure function, needs no device.
 * *map = VRS_REDUCE_MAP_*. */
int vrs_segment_reduce_map_for(uint32_t chunk_len, uint32_t row_width, uint32_t lane_rows, int *map);
/* levels a segment of len rows takes: 1 up to chunk_rows rows (an empty segment too), one more per factor of chunk_rows.  Pure. */
int vrs_segment_reduce_levels_for(uint32_t len, uint32_t chunk_rows, uint32_t *levels);
/* vrs_segment_reduce on the host, by the functions the kernels compile: host pointers, the same order, the same bits.  Needs no device. */
int vrs_segment_reduce_host(const void *values, uint64_t num_rows, uint32_t row_width, int dtype, const uint32_t *order,
                            const uint32_t *offsets, uint32_t num_segments, int op, const void *init,
                            uint32_t chunk_rows, uint32_t lane_rows, void *out);
/* cumulative per context: chunks each map was given by the classification, and the most levels any segment took (waits for the
 * context's stream; any pointer may be NULL) */
int vrs_segment_reduce_stats(vrs_context ctx, uint64_t *lane_chunks, uint64_t *row_chunks, uint64_t *column_chunks, uint64_t *max_levels);

/*
 * K14 -- inclusive prefix scan over rows (build extension; no reference counterpart): torch.cumsum, cumprod, cummax and cummin.
 * `values`: a dense [num_segments, num_rows, row_width] array of `dtype`; element (s, r, c) sits at ((size_t)s * num_rows + r) * row_width + c.
 * Every segment is scanned down its rows, every column on its own: out[s, r, c] = values[s, 0, c] (+) .. (+) values[s, r, c].  row_width
 * == 1 is the flat scan; a dim other than the last of a contiguous tensor is row_width > 1, without a transposed copy.  num_segments x
 * num_rows and row_width each fit 32 bits; their product may pass 2^32.  Ragged segments, exclusive and reverse scans, scans in place,
 * logcumsumexp and complex dtypes are not offered.
 * Ops and dtypes: VRS_SCAN_SUM and VRS_SCAN_PROD take int32, int64, float16, bfloat16, float32 or float64 into the same out_dtype, or
 * int8, uint8, int16 or int32 into int64 (torch's default promotion, done by the load); float16 and bfloat16 are accumulated in float32
 * and rounded once per output, to nearest even; integers wrap.  VRS_SCAN_MAX and VRS_SCAN_MIN take the nine dtypes of vrs_sort_dtype
 * (out_dtype == dtype) and also write int64 row numbers into out_indices; they combine (value, row) pairs by torch's CPU rule: a NaN
 * always replaces, a non-NaN replaces a non-NaN when it is >= (MIN: <=), so ties take the later row and its own bits, and after a NaN
 * the row follows the latest NaN.  That combine is associative and exact: these two ops equal torch bit for bit.
 * THE ORDER of sums and products is fixed: a function of (num_rows, row_width, dtype, op, T = VRS_TUNE_SCAN_TILE_ROWS) alone, never of
 * timing, the grid, num_segments or where a segment lies, so the same input gives the same bits on every run; vrs_scan_rows_host
 * evaluates the same functions on the host.  With F = 64 and every fold left to right from the op's identity (a float sum starts at
 * +0.0, so cumsum([-0.0]) is +0.0):
 *     A(0)_j = the aggregate of tile j (rows [jT, jT + T)) by the in-tile order;   A(k)_m = fold(A(k-1)_{mF} .. A(k-1)_{mF+F-1})
 *     P_j    = fold of, for k from the top level down to 0, A(k)_m for m in [F * floor(j / F^(k+1)), floor(j / F^k))
 *     out[i] = P_j (+) incl_j(i);   with num_rows <= T:  out[i] = incl_0(i)
 * The in-tile order has two maps, written down in csrc/vrs_scan_order.hpp: the flat map (row_width == 1: chunks of 256 rows, four per
 * lane, one six-step wave scan per chunk, the chunks in sequence) and the columns map (runs of 16 rows in sequence).
 * Tiers (vrs_scan_tier_for): VRS_SCAN_TILE, num_rows <= T: one launch, one wave per segment (flat) or one lane per segment and column;
 * VRS_SCAN_THREE_LAUNCH: an aggregates kernel, the carries (one small launch per level above the first, one for every P_j), an apply
 * kernel -- every dtype, op and row_width, no waiting anywhere; VRS_SCAN_SINGLE_PASS: row_width == 1, SUM or PROD into int32, float16,
 * bfloat16 or float32, from VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS rows per call on: one launch, tiles taken in order from a ticket, A(k)_m
 * published in 64-bit status words that are their own flag, waiting bounded by VRS_TUNE_SCAN_SPIN_BUDGET polls, after which the waiting
 * wave computes the missing word itself (the same bits).  All tiers give the same bits.
 * scratch: at least vrs_scan_scratch_bytes(...) bytes for the context's tuning (0 for the tile tier: scratch may then be NULL), on a
 * 16-byte boundary, contents afterwards unspecified.  values is never written; values, out, out_indices and scratch may not overlap.
 * num_segments == 0 or num_rows == 0: VRS_OK, nothing done.  A NULL context, values, out, out_indices (MAX, MIN) or scratch (when
 * needed), an unknown dtype / out_dtype / op triple, row_width == 0, num_segments x num_rows >= 2^32, undersized buffers and overlaps:
 * VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Stream-ordered on the context's stream; the call only enqueues (after
 * settling a pending one-call sort) and never waits for the device.
 */
typedef enum vrs_scan_op { VRS_SCAN_SUM = 0, VRS_SCAN_PROD = 1, VRS_SCAN_MAX = 2, VRS_SCAN_MIN = 3 } vrs_scan_op;
typedef enum vrs_scan_tier { VRS_SCAN_TILE = 0, VRS_SCAN_THREE_LAUNCH = 1, VRS_SCAN_SINGLE_PASS = 2 } vrs_scan_tier;
int vrs_scan_rows(vrs_context ctx, vrs_buffer values, uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype,
                  int op, vrs_buffer out, vrs_buffer out_indices /* MAX, MIN: int64, the shape of out; else NULL */, vrs_buffer scratch);
/* the tier a call takes with tile_rows = VRS_TUNE_SCAN_TILE_ROWS (a multiple of 256 in 256 .. 8192) and single_pass_min_rows =
 * VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS (0: never): a pure function, needs no device.  *tier = VRS_SCAN_*. */
int vrs_scan_tier_for(uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op, uint32_t tile_rows,
                      uint32_t single_pass_min_rows, int *tier);
/* levels of aggregates a segment of num_rows rows takes: 0 up to tile_rows rows, 1 up to F tiles, one more per factor of F.  Pure. */
int vrs_scan_levels_for(uint32_t num_rows, uint32_t tile_rows, uint32_t *levels);
/* the longest chain of combines behind any output of a segment (combines with the identity counted): the factor of the rounding-error
 * bound depth x u x cumsum(|x|), and at most tile_rows + F x (levels + 1).  Pure. */
int vrs_scan_depth_for(uint32_t num_rows, uint32_t row_width, uint32_t tile_rows, uint32_t *depth);
/* the scratch a call needs: a pure function, needs no device.  Three-launch: about 2 x a x row_width x num_segments x tiles bytes with
 * a the accumulator's bytes (4, 8, or 16 for MAX and MIN); single pass: 256 + about 8 x num_segments x tiles. */
int vrs_scan_scratch_bytes(uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op, uint32_t tile_rows,
                           uint32_t single_pass_min_rows, uint64_t *bytes);
/* vrs_scan_rows on the host, by the functions the kernels compile: host pointers, the same order, the same bits.  Needs no device. */
int vrs_scan_rows_host(const void *values, uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op,
                       uint32_t tile_rows, void *out, int64_t *out_indices);
/* cumulative per context: calls per tier, and the status words a waiting wave of the single pass computed itself (waits for the
 * context's stream; any pointer may be NULL) */
int vrs_scan_stats(vrs_context ctx, uint64_t *tile_calls, uint64_t *three_launch_calls, uint64_t *single_pass_calls, uint64_t *takeovers);

/*
 * K15 -- ordered stream compaction (build extension; no reference counterpart): "keep the elements whose flag is nonzero, in input
 * order, and say how many" -- torch.nonzero, argwhere, where(condition), masked_select, masked_scatter and count_nonzero.
 * `flags`: n elements of `dtype`, one of the nine of vrs_sort_dtype or VRS_COMPACT_BOOL (one byte), read in their own width.  THE
 * PREDICATE (csrc/vrs_compact_order.hpp, compiled by the kernels and by vrs_compact_host alike): an integer or bool is nonzero when its
 * bits are; a float when its bits without the sign are -- so -0.0 is zero, and NaNs, infinities and subnormals are nonzero.
 * The n elements are cut into tiles of T = VRS_TUNE_COMPACT_TILE_ELEMS elements.  Three phases, none of which polls, spins on or
 * otherwise waits for memory another workgroup writes:
 *   count    one workgroup per tile: 16-byte loads, the predicate's bits per lane, popcounts; one uint32 per tile into scratch
 *   carries  one workgroup: the exclusive scan of the tiles' counts in place, 4096 of them per step; the total R as a uint64
 *   emit     one workgroup per tile: the flags again, every survivor's rank in input order, the survivors of 4096 elements staged in LDS
 *            and written as dense runs in output order; a tile without survivors is not read again
 * vrs_compact_count enqueues count and carries; vrs_compact_emit enqueues emit against the offsets that call left in `scratch`.  THE
 * CONTRACT between the two: the same flags (unchanged), the same n and dtype, the same scratch, the same VRS_TUNE_COMPACT_TILE_ELEMS,
 * and no other compact call on that scratch in between.  Several emit calls may follow one count call.  outputs->num_selected is R as
 * the count call reported it: it sizes the checks of the output buffers, it is the leading dimension of the column layout, and whatever
 * `scratch` holds, no output row from num_selected on is written and no source element from there on is read.
 * Outputs of emit, in any combination (a NULL handle leaves one out):
 *   flat            R int64: the survivors' positions
 *   coords          R x ndim int64: their coordinates in a contiguous array of shape[0 .. ndim) (1 .. 8 sizes whose product is n), as
 *                   rows [R, ndim] (VRS_COMPACT_ROWS, torch.nonzero) or as columns [ndim, R] (VRS_COMPACT_COLUMNS, as_tuple=True)
 *   gather_out      R elements of value_bytes (1, 2, 4 or 8): gather_values[position], copied as bits (masked_select)
 *   scatter_out     n elements of value_bytes: out[i] = flag[i] ? scatter_source[rank(i)] : scatter_input[i], rank(i) the nonzero flags
 *                   in front of i (masked_scatter); scatter_source holds at least R elements, what lies behind R is never read
 * THE ROW FORM (x[mask] and index_put with a mask over the leading dims): outputs->row_elems = W >= 2 makes every flag stand for a dense
 * row of W elements of value_bytes; 0 and 1 both mean one element, the form above.  gather_values, scatter_input and scatter_out then
 * hold n x W elements, gather_out R x W and scatter_source at least R x W: gather_out row r = gather_values row position(r), and
 * scatter_out row i = flag[i] ? scatter_source row rank(i) : scatter_input row i.  flat and coords stay per flag and combine with the
 * row outputs in one call.  n x W x value_bytes may pass 2^32 (byte offsets are 64-bit; 2^62 and more is refused); nothing from row
 * num_selected on is written, no source row from there on is read; the size and overlap checks scale by W, the boundary stays the
 * element's.  Two kernels of their own move the rows (the element kernels are not touched): a chunk's rows are one contiguous span of
 * bytes that consecutive lanes copy word by word -- 16 bytes when the row's bytes and every base involved are multiples of 16, else the
 * largest of 8, 4, 2 and 1 that divides them all -- over a grid of (tiles, slices), every slice ranking its chunk's flags again and
 * copying its share of the span's words (csrc/vrs_compact_order.hpp: compact_row_word_bytes, compact_row_slices).
 * n < 2^32.  flags on its element's boundary (16-byte loads are used when it starts on a 16-byte boundary), scratch on a 16-byte
 * boundary and at least vrs_compact_scratch_bytes(n, T) bytes, value buffers on their element's boundary, int64 outputs on 8 bytes.
 * n == 0: VRS_OK, nothing enqueued but the count itself (0).  A NULL context, flags or scratch, an unknown dtype, layout or value_bytes,
 * ndim outside 1 .. 8, a shape whose product is not n, undersized buffers and an output that overlaps flags or scratch:
 * VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Stream-ordered on the context's stream; the calls only enqueue (after
 * settling a pending one-call sort), except that vrs_compact_count with host_count waits for the stream: the one host read torch's
 * own nonzero makes too.
 */
#define VRS_COMPACT_BOOL 9 /* after the nine of vrs_sort_dtype */
typedef enum vrs_compact_layout { VRS_COMPACT_ROWS = 0, VRS_COMPACT_COLUMNS = 1 } vrs_compact_layout;
typedef struct vrs_compact_outputs {
    uint64_t num_selected;     /* R, as vrs_compact_count reported it */
    vrs_buffer flat;           /* NULL, or R int64 */
    vrs_buffer coords;         /* NULL, or R x ndim int64 */
    int coords_layout;         /* VRS_COMPACT_ROWS or VRS_COMPACT_COLUMNS */
    uint32_t ndim;             /* with coords: 1 .. 8 */
    uint32_t shape[8];         /* with coords: sizes whose product is n */
    vrs_buffer gather_values;  /* with gather_out: n elements of value_bytes */
    vrs_buffer gather_out;     /* NULL, or R elements of value_bytes */
    uint32_t value_bytes;      /* of gather_* and scatter_*: 1, 2, 4 or 8 */
    uint32_t row_elems;        /* 0 or 1: a flag stands for one element; W >= 2: for a row of W elements (THE ROW FORM) */
    vrs_buffer scatter_input;  /* with scatter_out: n elements */
    vrs_buffer scatter_source; /* with scatter_out: at least R elements (may be NULL when R is 0) */
    vrs_buffer scatter_out;    /* NULL, or n elements */
} vrs_compact_outputs;
/* count and carries.  out_count_device: NULL, or 8 bytes that receive R as an int64 on the device; host_count: NULL, or where R goes
 * once the stream has been waited for. */
int vrs_compact_count(vrs_context ctx, vrs_buffer flags, uint64_t n, int dtype, vrs_buffer scratch, vrs_buffer out_count_device, uint64_t *host_count);
int vrs_compact_emit(vrs_context ctx, vrs_buffer flags, uint64_t n, int dtype, vrs_buffer scratch, const vrs_compact_outputs *outputs);
/* tiles of tile_elems (a multiple of 4096 in 4096 .. 65536) that cover n < 2^32 elements, and the scratch they take (256 bytes and 4 per
 * tile, rounded up to 256): pure functions, need no device */
int vrs_compact_tiles_for(uint64_t n, uint32_t tile_elems, uint32_t *tiles);
int vrs_compact_scratch_bytes(uint64_t n, uint32_t tile_elems, uint64_t *bytes);
/* the quotient and remainder of a 32-bit numerator by divisor >= 1 as the kernels form them (a multiplication by a constant made from
 * the divisor): pure, needs no device */
int vrs_compact_divide(uint32_t numerator, uint32_t divisor, uint32_t *quotient, uint32_t *remainder);
/* the same predicate, order and coordinate arithmetic on host pointers, by the functions the kernels compile.  Needs no device.  Every
 * output may be NULL; out_flat, out_coords and gather_out have room for every survivor (at most n); scatter_source holds
 * scatter_source_elems elements, of which the first R are read: fewer than R is VRS_ERROR_INVALID_ARGUMENT with nothing written to
 * scatter_out.  *out_count = R. */
typedef struct vrs_compact_host_outputs {
    int64_t *flat;
    int64_t *coords;
    int coords_layout;
    uint32_t ndim;
    uint32_t shape[8];
    const void *gather_values;
    void *gather_out;
    uint32_t value_bytes;
    uint32_t row_elems; /* as in vrs_compact_outputs; scatter_source_elems still counts elements: at least R x W of them */
    const void *scatter_input, *scatter_source;
    uint64_t scatter_source_elems;
    void *scatter_out;
} vrs_compact_host_outputs;
int vrs_compact_host(const void *flags, uint64_t n, int dtype, const vrs_compact_host_outputs *outputs, uint64_t *out_count);
/* cumulative per context: count calls, emit calls and the elements the count calls were given (any pointer may be NULL) */
int vrs_compact_stats(vrs_context ctx, uint64_t *count_calls, uint64_t *emit_calls, uint64_t *elements);

/*
 * Run-length encoding (build extension; no reference counterpart -- the reference's callers find each cell's or tile's [start, end)
 * in the sorted ids themselves): n keys of key_bytes (4 or 8) each, in any order, as maximal runs of bit-identical consecutive keys
 * (torch.unique_consecutive).  With R runs: out_keys[j] = the key of run j, out_offsets[j] = its first position and out_offsets[R] = n,
 * out_counts[j] = its length, out_run_ids[i] = the run of element i, and out_num_runs[0] = R, written on the device.  Every output but
 * out_num_runs may be NULL.  `keys` is never written; output entries past R (past R + 1 for out_offsets) are never written, nor are the
 * bytes of an output buffer beyond n (n + 1) entries.  n == 0: out_num_runs[0] = 0 and nothing else.
 * One pass over the keys: tiles of 4096 keys taken in order from a ticket, a head flag per key (i == 0 or k[i] != k[i-1]), ranks by
 * __ballot / mbcnt, the runs in front of a tile by decoupled look-back; the counts from the offsets by a second, short launch.
 * scratch: at least vrs_run_length_encode_scratch_bytes(n, key_bytes, flags) bytes, with VRS_RLE_COUNTS in flags whenever out_counts
 * is given and out_offsets is NULL (the offsets then live in the scratch): at most (VRS_RLE_COUNTS ? 4 n : 0) + n / 256 + 1024 bytes,
 * on an 8-byte boundary (the look-back's status words are 64 bits wide).
 * Contents on entry unspecified, afterwards unspecified.  NULL ctx, keys, out_num_runs or scratch, a key_bytes other than 4 or 8,
 * undersized buffers (n entries; n + 1 for out_offsets) and a scratch off an 8-byte boundary: VRS_ERROR_INVALID_ARGUMENT before
 * anything is enqueued.  Stream-ordered on the
 * context's stream; the call only enqueues (after settling a pending one-call sort).
 * THE ROW FORM: key_bytes = 4 or 8 | VRS_UNIQUE_COLUMNS(C) with C >= 2 (C of 0 or 1 is the form above, bit for bit) encodes maximal
 * runs of bit-identical consecutive rows (torch.unique_consecutive(x, dim=0)): num_elements counts rows, `keys` holds n x C words
 * row-major, out_keys has room for n x C words of which R x C are written (the R rows, by a short launch of its own), and out_offsets,
 * out_counts and out_run_ids count rows.  A lane compares a row's first 8 bytes with those in front as the word form compares keys and
 * reads the columns behind them only when these are equal.  scratch: always with room for the offsets (they serve the rows and the
 * counts when out_offsets is NULL), whatever `flags` says: at most 4 n + n / 256 + 2048 bytes.  n x C >= 2^32, a negative key_bytes
 * and an unknown low byte are refused like the other arguments.
 */
/* the columns per row of the row forms of vrs_run_length_encode (in key_bytes) and vrs_unique (in key_type): bits 8 and up */
#define VRS_UNIQUE_COLUMNS(c) ((int)(c) << 8)
enum { VRS_RLE_COUNTS = 1 }; /* scratch flag */
int vrs_run_length_encode(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, int key_bytes, vrs_buffer out_keys,
                          vrs_buffer out_offsets, vrs_buffer out_counts, vrs_buffer out_run_ids, vrs_buffer out_num_runs,
                          vrs_buffer scratch);
/* the scratch vrs_run_length_encode needs: a pure function, needs no device (0 for n == 0) */
int vrs_run_length_encode_scratch_bytes(uint32_t num_elements, int key_bytes, int flags, uint64_t *bytes);

/*
 * Unique (build extension; no reference counterpart): the distinct keys of n keys in ascending order, how often each occurs and which of
 * them each element is (torch.unique(x, sorted=True, return_inverse=True, return_counts=True)).  key_type (vrs_unique_key_type) fixes
 * the width and the order: the rank r(x) = x (U32, U64), x ^ 2^31 (I32), x ^ 2^63 (I64), the VRS_KEYS_FLOAT32_TO_SORTABLE map (F32)
 * and the same map widened (F64): IEEE-754 total order, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  Equality is equality of bit
 * patterns: -0.0 and +0.0 are two keys and NaNs of the same bits are one -- where torch.unique merges -0.0 into +0.0 and keeps every NaN
 * apart.  out_keys[j] = the j-th smallest distinct key (its bit pattern), out_counts[j] = its occurrences, out_inverse[i] = the j of
 * element i, out_num_runs[0] = R, written on the device.  out_counts and out_inverse may be NULL.  The same guarantees as
 * vrs_run_length_encode for `keys`, entries past R and bytes past n entries; n == 0: out_num_runs[0] = 0 and nothing else.
 * Pipeline: one kernel writes r(keys) (and, for the inverse, the positions 0 .. n-1 beside them) into the scratch, the stable one-call
 * sort sorts them there (vrs_sort_pairs_u32 / vrs_sort_pairs_u64 with the inverse, vrs_sort_keys_u32 / vrs_sort_keys_u64 without), and
 * the run-length encode runs over the sorted ranks, undoing r as it writes out_keys and scattering run ids through the sorted positions.
 * scratch: at least vrs_unique_scratch_bytes(n, key_type, flags) bytes with VRS_UNIQUE_INVERSE / VRS_UNIQUE_COUNTS set for the outputs
 * given: at most (2 * key bytes + (VRS_UNIQUE_INVERSE ? 8 : 0) + (VRS_UNIQUE_COUNTS ? 4 : 0)) * n + n / 256 + 2048 bytes, on an
 * 8-byte boundary (the encode's status words, and 64-bit keys sorted inside it).  Contents on
 * entry unspecified, afterwards unspecified.  NULL ctx, keys, out_keys, out_num_runs or scratch, an unknown key_type, undersized
 * buffers and a scratch off an 8-byte boundary: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 * Blocking, as the segmented sorts': after settling a pending one-call sort the call may wait for the inner sort's plan head (bounded by
 * VRS_TUNE_PLAN_WAIT_MS -> VRS_ERROR_TIMEOUT, the encode then not enqueued), never for the sort itself; the inner sort counts in the
 * one-call statistics.
 * THE ROW FORM: key_type = a vrs_unique_key_type | VRS_UNIQUE_COLUMNS(C) with C >= 2 (C of 0 or 1 is the form above, bit for bit) gives
 * the distinct rows of an n x C matrix (torch.unique(x, dim=0)): num_elements counts rows, `keys` holds n x C words row-major, rows are
 * ordered lexicographically by r of every word and are equal when bit-identical; out_keys has room for n x C words of which R x C are
 * written (the input's own bits), out_counts and out_inverse count rows.  Pipeline: the columns are grouped from the last backwards into
 * groups of at most 8 bytes of ranks (two 4-byte columns, the more significant in the high half, or one 8-byte column; a lone 4-byte
 * column left over is column 0 with a 32-bit key), ceil(C * word / 8) rounds; per round, least significant group first, one kernel
 * packs the group's ranks of the rows in their current order (round 1 reads them where they lie, later rounds gather through the
 * positions) and the stable vrs_sort_pairs_u64 / _u32 sorts (key, position); the encode then compares the top group's sorted keys and
 * fetches the remaining columns through the positions only for a pair whose top groups are equal; a last short launch gathers the R
 * rows.  The call may wait for every inner sort's plan head.  scratch: the same for every C, key type and flags: at most
 * 28 n + n / 256 + 4096 bytes (two key buffers of 8 bytes per row, the positions and their partner, the run offsets).
 * n x C >= 2^32, a negative key_type and an unknown low byte are refused like the other arguments.
 */
typedef enum vrs_unique_key_type {
    VRS_UNIQUE_U32 = 0, VRS_UNIQUE_I32 = 1, VRS_UNIQUE_F32 = 2,
    VRS_UNIQUE_U64 = 3, VRS_UNIQUE_I64 = 4, VRS_UNIQUE_F64 = 5
} vrs_unique_key_type;
enum { VRS_UNIQUE_INVERSE = 1, VRS_UNIQUE_COUNTS = 2 }; /* scratch flags */
int vrs_unique(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, int key_type, vrs_buffer out_keys,
               vrs_buffer out_counts /* may be NULL */, vrs_buffer out_inverse /* may be NULL */, vrs_buffer out_num_runs,
               vrs_buffer scratch);
/* the scratch vrs_unique needs: a pure function, needs no device (0 for n == 0) */
int vrs_unique_scratch_bytes(uint32_t num_elements, int key_type, int flags, uint64_t *bytes);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* VKRADIXSORT_AMD_OPS_H */
