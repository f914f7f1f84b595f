/*
 * vkradixsort_amd.h -- C ABI of the MI355X-native multi-block LSD radix sort.
 *
 * This is the drop-in boundary for VkRadixSort's `multi_radixsort` path.  The reference has no
 * FFI layer of its own: its boundary is the C++ class API (GPUContext / Buffer / ComputePass /
 * MultiRadixSortPass / MultiRadixSort).  The C++ host mirror under vkradixsort_amd/host keeps those
 * classes and calls ONLY the functions below; any other host language binds the same symbols
 * (see INTEGRATION.md).  Plain C types, opaque handles, no exceptions, 0 == success.
 *
 * Each entry point cites the reference interface it replaces (file:line in VkRadixSort @ v2).
 *
 * Threading: one HIP stream per context, a context is not thread-safe (the reference is single
 * threaded: one compute queue, one host thread).  Stage calls are ASYNCHRONOUS and stream-ordered;
 * the only blocking calls are vrs_queue_wait_idle, upload/download and the profile query.
 */
#ifndef VKRADIXSORT_AMD_H
#define VKRADIXSORT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRS_RADIX_SORT_BINS 256u /* multi_radixsort.comp:12 */
#define VRS_WORKGROUP_SIZE 256u  /* multi_radixsort.comp:11 -- the CONTRACT workgroup size that
                                    defines tiles and the [W][256] histogram layout */

typedef enum vrs_status {
    VRS_OK = 0,
    VRS_ERROR_INVALID_ARGUMENT = 1,
    VRS_ERROR_HIP = 2,          /* a HIP runtime call failed; see vrs_last_error */
    VRS_ERROR_NO_DEVICE = 3,    /* no gfx950-capable device / bad ordinal */
    VRS_ERROR_OUT_OF_MEMORY = 4,
    VRS_ERROR_UNBALANCED = 5,   /* vrs_dist_sort_keys_u32: too many equal keys -- no cut between key values balances the ranks */
    VRS_ERROR_PEER = 7,         /* vrs_dist_sort_keys_u32: another rank could not take part; every rank left the step together */
    VRS_ERROR_TIMEOUT = 6       /* a one-call sort's plan did not reach the host within VRS_TUNE_PLAN_WAIT_MS (the stream is held
                                   up by earlier work); the sort is still queued, vrs_sort_settle may be called again */
} vrs_status;

typedef struct vrs_context_t *vrs_context; /* replaces engine::GPUContext (GPUContext.h:15-111) */
typedef struct vrs_buffer_t *vrs_buffer;   /* replaces engine::Buffer     (Buffer.h:14-177)     */

/*
 * The 16-byte push-constant block shared by both stages, std430 order:
 * MultiRadixSortPass::PushConstantsHistograms (MultiRadixSortPass.h:17-22) and
 * MultiRadixSortPass::PushConstants           (MultiRadixSortPass.h:26-31), mirroring
 * multi_radixsort_histograms.comp:13-18 and multi_radixsort.comp:17-22.
 */
typedef struct vrs_push_constants {
    uint32_t g_num_elements;             /* N */
    uint32_t g_shift;                    /* 0, 8, 16, 24 -- set by the caller each pass
                                            (MultiRadixSort.cpp:57-58) */
    uint32_t g_num_workgroups;           /* W = ceil(ceil(N/B)/256)  (MultiRadixSort.cpp:13-20) */
    uint32_t g_num_blocks_per_workgroup; /* B = NUM_BLOCKS_PER_WORKGROUP (MultiRadixSort.cpp:12) */
} vrs_push_constants;

/* ---- device / context: GPUContext::init / shutdown (GPUContext.cpp:7-13) ------------------- */

int vrs_device_count(int *count);
/* Creates a context on `device_ordinal` with its own HIP stream.  Never prompts on stdin (the
 * reference does when >1 device: GPUContext.cpp:167-174). */
int vrs_context_create(int device_ordinal, vrs_context *out_ctx);
/* Same, but borrows a caller-owned hipStream_t (e.g. torch's current stream); never destroyed. */
int vrs_context_create_on_stream(int device_ordinal, void *hip_stream, vrs_context *out_ctx);
int vrs_context_destroy(vrs_context ctx);
/* Message of the last failure on this context (ctx may be NULL for creation failures). */
const char *vrs_last_error(vrs_context ctx);
/* hipStream_t of the context, for callers that interleave their own work. */
void *vrs_context_stream(vrs_context ctx);
int vrs_context_device(vrs_context ctx); /* the device ordinal the context was created on */
/* Device facts for reports: name, CU count, HBM bytes.  Any out pointer may be NULL. */
int vrs_device_info(vrs_context ctx, char *name, size_t name_cap, int *compute_units,
                    uint64_t *global_mem_bytes);

/* ---- buffers: Buffer ctor / release / staging copies (Buffer.h:25-72) ---------------------- */

/* Device-local allocation (VK_MEMORY_PROPERTY_DEVICE_LOCAL_BIT buffers of prepareBuffers,
 * MultiRadixSort.cpp:83-95).  size_t, not the reference's uint32 byte size (Buffer.h:17). */
int vrs_buffer_create(vrs_context ctx, size_t size_bytes, vrs_buffer *out_buf);
/* Wraps caller-owned device memory (hipMalloc / torch tensor); release does not free it.
 * `device_ptr` must be aligned to the element size (4 bytes; 8 for uint64 keys); 16-byte aligned bases
 * (every hipMalloc / torch allocation) take the fastest load path.  ("own usage", README.md:151-241.) */
int vrs_buffer_wrap(vrs_context ctx, void *device_ptr, size_t size_bytes, vrs_buffer *out_buf);
/* Idempotent (Buffer::release, Buffer.h:36-45).  Also frees the handle. */
int vrs_buffer_release(vrs_buffer buf);
/* Synchronous H2D copy of `size_bytes` (Buffer::fillDeviceWithStagingBuffer, Buffer.h:47-62). */
int vrs_buffer_upload(vrs_context ctx, vrs_buffer buf, const void *host_data, size_t size_bytes);
/* Synchronous D2H copy (Buffer::downloadWithStagingBuffer, Buffer.h:64-72). */
int vrs_buffer_download(vrs_context ctx, vrs_buffer buf, void *host_data, size_t size_bytes);
/* Stream-ordered device-to-device copy (used to re-arm the unsorted input between timed reps). */
int vrs_buffer_copy(vrs_context ctx, vrs_buffer dst, vrs_buffer src, size_t size_bytes);
void *vrs_buffer_device_ptr(vrs_buffer buf);
size_t vrs_buffer_size_bytes(vrs_buffer buf); /* Buffer::getSizeBytes, Buffer.h:103-105 */

/* ---- launch-shape arithmetic: ComputePass::setGlobalInvocationSize/getWorkGroupCount ------- */

/* gis = ceil(N/B) (MultiRadixSort.cpp:13-15); W = ceil(gis/256) (ComputePass.h:16-29). */
uint32_t vrs_global_invocation_size(uint32_t num_elements, uint32_t blocks_per_workgroup);
uint32_t vrs_workgroup_count(uint32_t num_elements, uint32_t blocks_per_workgroup);

/* ---- the two stages: MultiRadixSortPass::recordCommands (MultiRadixSortPass.cpp:10-20) ----- */

/*
 * Stage RADIX_SORT_HISTOGRAMS (multi_radixsort_histograms.comp:31-55).
 * bindings: set 0 b0 = keys_in (uint32[N]), set 0 b1 = histograms (uint32[W*256], layout
 * [workgroup][digit], every entry overwritten).  Asynchronous.
 */
int vrs_multi_radixsort_histograms(vrs_context ctx, vrs_buffer keys_in, vrs_buffer histograms,
                                   const vrs_push_constants *pc);
/*
 * Stage RADIX_SORT (multi_radixsort.comp:45-127): global digit prefix + per-workgroup offsets from
 * `histograms`, then the stable scatter keys_in -> keys_out.  bindings: set 1 b0 in, b1 out,
 * b2 histograms.  Stream-ordered after the histogram stage (replaces the W->R pipeline barrier,
 * MultiRadixSortPass.cpp:13-14).  keys_in and keys_out must not alias.  Asynchronous.
 */
int vrs_multi_radixsort(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out,
                        vrs_buffer histograms, const vrs_push_constants *pc);
/*
 * Key + payload variant of the RADIX_SORT stage (build extension, BASELINE.json config 4: the
 * reference has only g_elements_in/out, multi_radixsort.comp:24-30).  values follow their keys;
 * order among equal digits is the input order (stable), so four passes == std::stable_sort by key.
 */
int vrs_multi_radixsort_pairs(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out,
                              vrs_buffer values_in, vrs_buffer values_out, vrs_buffer histograms,
                              const vrs_push_constants *pc);
/*
 * Global exclusive digit prefix (uint32[256]) computed by the most recent RADIX_SORT stage on this
 * context -- the `global_histogram` of multi_radixsort.comp:74-75: position of the first key of each
 * digit in that stage's output.  Synchronous.  Used by the multi-GPU key-range exchange (build
 * extension) to cut the locally grouped shard into per-rank slices.
 */
int vrs_multi_radixsort_digit_offsets(vrs_context ctx, void *host_u32x256);
/* The same 256 words copied into a device buffer, asynchronously (no host round trip: the multi-GPU step feeds
 * them straight into its count all-gather). */
int vrs_multi_radixsort_digit_offsets_device(vrs_context ctx, vrs_buffer out_u32x256);
/* One-shot hook for the NEXT RADIX_SORT stage of the context: as soon as its offset table is complete -- before its scatter kernel --
 * the stage copies the 256 digit offsets to out_u32x256 (may be NULL) and records `event` (a hipEvent_t of the caller's, may be NULL)
 * on the context's stream.  Work on another stream that needs only the offsets (the multi-GPU step's all-gather) then runs beside
 * the scatter.  (The reference has no counterpart: its prefix lives inside multi_radixsort.comp:63-87.) */
int vrs_multi_radixsort_offsets_hook(vrs_context ctx, vrs_buffer out_u32x256, void *event);
/*
 * 64-bit keys: the reference's SORT_64_BIT switch (MultiRadixSort.h:10-18; NUM_ITERATIONS = 8,
 * MultiRadixSort.cpp:51-55), which it leaves as a stub ("requires changes in the two shaders").  Same two
 * stages, same [W][256] table and push constants; keys are uint64, g_shift is 0, 8, ..., 56, the caller runs
 * eight passes (even count: the result is in buffer 0 again).  Payloads of the pairs form stay uint32.
 */
int vrs_multi_radixsort_histograms_u64(vrs_context ctx, vrs_buffer keys_in, vrs_buffer histograms,
                                       const vrs_push_constants *pc);
int vrs_multi_radixsort_u64(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out,
                            vrs_buffer histograms, const vrs_push_constants *pc);
int vrs_multi_radixsort_pairs_u64(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out,
                                  vrs_buffer values_in, vrs_buffer values_out, vrs_buffer histograms,
                                  const vrs_push_constants *pc);
/*
 * Range partition (build extension for the multi-GPU key-range exchange; no reference counterpart): one
 * stable pass that groups uint32 keys by range instead of by digit.  `splitters` holds `num_splitters` <= 255
 * ascending uint32 values on the device; a key goes to range r = number of splitters <= key.  keys_out holds
 * range 0's keys, then range 1's, ... each in input order; vrs_multi_radixsort_digit_offsets then returns
 * the first position of every range (entries 0..num_splitters).  Asynchronous.
 */
int vrs_range_partition(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out, vrs_buffer splitters,
                        uint32_t num_splitters, uint32_t num_elements);
/* vkQueueWaitIdle on the compute queue (MultiRadixSort.cpp:62). */
int vrs_queue_wait_idle(vrs_context ctx);

/*
 * single_radixsort path (single_radixsort.comp:42-140, SingleRadixSort.cpp:5-47): one workgroup,
 * four passes in one launch, push constant {g_num_elements}; result in buffer0.  Asynchronous.
 */
int vrs_single_radixsort(vrs_context ctx, vrs_buffer buffer0, vrs_buffer buffer1,
                         uint32_t g_num_elements);

/*
 * One-call form of MultiRadixSort::execute's hot loop (MultiRadixSort.cpp:50-61): four passes with
 * g_shift = 0, 8, 16, 24 ping-ponging `keys` <-> `keys_tmp` (the reference's buffer0 / buffer1); the
 * library picks NUM_BLOCKS_PER_WORKGROUP (32) and owns the histogram table.  Result in `keys`.
 * The pairs form is stable (== std::stable_sort by key); `values` follow their keys.
 *
 * Up to VRS_TUNE_SINGLE_MAX_KEYS uint32 keys (default 4096) the whole sort is one single_radixsort launch (the
 * reference's guidance for small inputs, README.md:18-21).  Below VRS_TUNE_ONE_CALL_MIN_KEYS elements (default 2^13)
 * these are the four (eight) contract passes, fully asynchronous.  From there on -- the library owns all passes, so the per-pass [W][256] table of the
 * reference's interface is not needed -- the keys are read ONCE to count all four digits of a 32-bit word
 * and every pass is a stable scatter that finds its offsets by decoupled look-back (36 instead of 48 bytes
 * per 32-bit key, 136 instead of 192 per 64-bit key; DESIGN.md "K5").  That form enqueues everything, then waits on
 * the host ONCE per four passes until the plan kernel has written the plan's head (a few hundred bytes) into pinned
 * host memory -- i.e. until the counting read has run; it never waits for the sort itself, which still completes
 * asynchronously on the context's stream.  Passes whose digit is the same for every key (small keys, constant bytes)
 * are the identity and are left out.  Same result, bit for bit.
 * uint32 keys from 1.3 * 10^7 keys on, uint32 key + payload pairs from 2.5 * 10^7 pairs on (VRS_TUNE_HYBRID,
 * VRS_TUNE_HYBRID_MIN_KEYS):
 * the same counting read also histograms the top 14 bits of the key range, and when every such bucket fits one workgroup's
 * LDS (14333 keys, 13312 pairs or 64-bit keys; uniform input: up to about 2.2 * 10^8 keys, 2.1 * 10^8 pairs) the four LSD passes are
 * replaced by an MSD partition in two look-back scatter passes (8 + 6 bits) plus one pass in which every bucket is sorted
 * inside LDS -- 28 bytes per key instead of 36, 52 per pair instead of 68 (DESIGN.md "K5b").  The choice is made on the
 * device from that one read; either form gives the same bits, payloads of equal keys in input order included.
 * vrs_sort_keys_u64 takes the same form from 2 * 10^7 keys on (56 instead of 144 bytes per key; the local sort then needs
 * ceil(low bits / 9) LDS passes, up to six); its counting read never makes LSD tables, so a refused sort starts over.
 *
 * Blocking behaviour.  On a context with its OWN stream (vrs_context_create) these calls only ENQUEUE and return at once -- like
 * the reference's ComputePass::execute (ComputePass.h:31-56), whose only blocking call is the queue-idle wait
 * (MultiRadixSort.cpp:62): a sort the hybrid form is expected to take (the context's previous one of its kind did) is put on the
 * stream completely (second MSD pass and local sort with grids sized for the worst plan the form accepts; the pool form with
 * all six kernels), the LSD form as four speculative look-back passes.  What the plan may still ask for (a refused hybrid
 * form: the LSD sort; a pass with unbalanced or wide streams; the copy home after an odd number of passes) is enqueued by
 * vrs_sort_settle, which waits for the plan's head -- never for the sort; vrs_queue_wait_idle, the blocking buffer transfers,
 * vrs_verify_keys_u32, every stage / sort entry point and vrs_context_destroy settle a pending sort first.  Until then the
 * buffers must stay alive, and a caller who queues work of his own behind the sort (vrs_context_stream) calls vrs_sort_settle
 * before he does.  vrs_sort_pending tells whether a second half is outstanding (0 / 1).
 * On a BORROWED stream (vrs_context_create_on_stream) the caller waits with calls of his own (hipStreamSynchronize,
 * torch.cuda.synchronize), so the default there is the blocking form: the call returns once the plan's head has reached the
 * host and everything the plan asks for is on the stream (it spins briefly, then yields; never longer than
 * VRS_TUNE_PLAN_WAIT_MS -> VRS_ERROR_TIMEOUT) -- on a stream that still has earlier work queued that means waiting for that
 * work.  VRS_TUNE_ASYNC_SORT selects either form on either kind of context.
 */
int vrs_sort_keys_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements);
/* The same sort for keys the caller knows to lie in [key_floor, 2^32) -- a sub-range of a larger sort (the received key range
 * of a multi-GPU step): the hybrid form then takes its 16384 buckets from key - (key_floor rounded down to a multiple of 2^24),
 * as it would for a full key range, instead of finding almost all of them empty and the rest too large.  A hint only: a key
 * below the floor makes the plan refuse the hybrid form (the LSD passes run) -- the result is the same either way. */
int vrs_sort_keys_u32_ranged(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements, uint32_t key_floor);
int vrs_sort_settle(vrs_context ctx);
int vrs_sort_pending(vrs_context ctx);
int vrs_sort_pairs_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values,
                       vrs_buffer values_tmp, uint32_t num_elements);
int vrs_sort_keys_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements); /* 8 LSD passes, or the hybrid form */
/* uint64 keys with uint32 payloads: two groups of [counting read + four look-back scatter passes] from
 * VRS_TUNE_ONE_CALL_MIN_KEYS pairs on (2 x (8 + 4 x 24) = 208 instead of 8 x (8 + 24) = 256 bytes per pair), the eight contract passes
 * below; stable either way.  No hybrid form. */
int vrs_sort_pairs_u64(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, vrs_buffer values,
                       vrs_buffer values_tmp, uint32_t num_elements);

/*
 * The hybrid form of vrs_sort_keys_u32 in two halves, for callers that move the keys between its two MSD passes -- the
 * multi-GPU step (vrs_dist_*) puts the exchange between the GPUs there.  Both only enqueue.
 *   vrs_msd_partition_u32: counting read (histogram of the top 14 bits of the probed key range + top-byte counts) and the first
 *     MSD pass: `out` = the keys grouped by the top 8 bits of the range (in no particular order inside a group when the pass takes
 *     its places by reservation, VRS_TUNE_MSD_RESERVE: the default).  counts_out (VRS_MSD_COUNT_WORDS uint32):
 *     [0, 16384) the bucket histogram, [16384, 16384 + 8 * 256) the top-byte counts of the eight input slices,
 *     [VRS_MSD_SHIFT_WORD] the bucket shift (bucket = key >> shift; below 13 the key range is too narrow for the form: the
 *     histogram is empty and `out` is not a partition), [VRS_MSD_SHIFT_WORD + 1] != 0: a key above the probed range.
 *   vrs_msd_finish_u32: second MSD pass + local sort of n keys that ARE grouped by that top byte (`grouped`; clobbered as
 *     scratch), result in `out`.  counts: the same layout, [0, 16384) = the bucket histogram of exactly these n keys, the
 *     slice counts zero, the shift word set, the flag word zero; read in place by the plan kernel, which leaves the histogram zeroed.  bucket_hint: the largest bucket to expect (it picks the local
 *     sort's workgroup shape before the plan is known; 0 = num_elements / 16384 + 10 %).  The plan may refuse (a bucket beyond the local sort's
 *     capacity, top-byte buckets too unequal for the grid): vrs_msd_finish_status waits for the plan's head and tells
 *     (*took == 0: `out` holds nothing useful, `grouped` still holds the keys -- sort them with vrs_sort_keys_u32).
 *   A caller that enqueues several finishes before it looks (the rounds of the multi-GPU step: a wait per round would leave the
 *     GPU idle while the host enqueues the next) takes a ticket after each (vrs_msd_finish_ticket) and asks later:
 *     vrs_msd_finish_status_at(ticket) waits until THAT finish's plan has run.  The context keeps the last 32 decisions.
 */
#define VRS_MSD_COUNT_WORDS (16384u + 8u * 256u + 64u)
#define VRS_MSD_SHIFT_WORD (16384u + 8u * 256u)
int vrs_msd_partition_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer out, vrs_buffer counts_out, uint32_t num_elements);
/* The same; counts_ready_event (a hipEvent_t of the caller's, or NULL) is recorded on the context's stream as soon as counts_out is
 * complete -- before the first MSD pass -- so that work on ANOTHER stream that needs only the counts (the multi-GPU step's
 * collectives) runs beside that pass. */
int vrs_msd_partition_signal_u32(vrs_context ctx, vrs_buffer keys, vrs_buffer out, vrs_buffer counts_out, uint32_t num_elements,
                                 void *counts_ready_event);
int vrs_msd_finish_u32(vrs_context ctx, vrs_buffer grouped, vrs_buffer out, vrs_buffer counts, uint32_t num_elements,
                       uint32_t bucket_hint);
/* The same second half for keys that are grouped by their TOP BYTE and lie in top bytes [first_top_byte, first_top_byte + top_bytes)
 * -- what a rank of a large multi-GPU sort holds after the exchange -- with no histogram from the caller: one counting read of the
 * n keys (buckets = top byte and the next min(8, 14 - ceil(log2(top_bytes))) bits), then the second MSD pass by those bits and the
 * local sort: 20 bytes per key instead of the 28 of a whole sort.  Refused (ticket / status as above; `grouped` untouched) when a
 * bucket exceeds the local sort's capacity: about 3.6 * 10^6 keys per top byte. */
int vrs_msd_finish_grouped_u32(vrs_context ctx, vrs_buffer grouped, vrs_buffer out, uint32_t num_elements, uint32_t first_top_byte,
                               uint32_t top_bytes);
/* The same for a caller that KNOWS how many keys each of those top bytes holds (counts[0 .. top_bytes): host memory, read before the
 * call returns; their sum must be num_elements) -- the multi-GPU step does, from the exchange's own bookkeeping.  Nothing is read to
 * be counted: one workgroup per top byte samples 1/32 of its keys and sizes a region of the context's slack buffer per bucket (top byte
 * and the next 6 .. 8 bits), the second MSD pass scatters there, the local sort reads every bucket in one piece -- the second half of
 * the pool form (VRS_TUNE_MSD_POOL), 16 bytes per key instead of 20.  Refused (ticket / status as above; `grouped` untouched) when a
 * bucket outgrows its region or the local sort's capacity, or a key does not carry the top byte its place says.  Falls back to
 * vrs_msd_finish_grouped_u32 where the form cannot run (switched off, no workgroup shape for these buckets, fewer than 2^20 keys,
 * counts == NULL). */
int vrs_msd_finish_grouped_counts_u32(vrs_context ctx, vrs_buffer grouped, vrs_buffer out, uint32_t num_elements, uint32_t first_top_byte,
                                      uint32_t top_bytes, const uint32_t *counts);
/* The same with a part of every top byte's keys lying ELSEWHERE -- the keys a rank of the multi-GPU step keeps for itself stay where its
 * partition pass wrote them instead of being copied beside the received ones (1 / world of the exchange's 8 bytes per key): top byte a's
 * range of `grouped` is laid out for all counts[a] keys, its LAST own_counts[a] slots are a hole, and those keys are own_counts[a]
 * consecutive keys of `own`, the top bytes' own parts following each other from key own_offset on.  The second pass reads a top byte as
 * two pieces; nothing else changes (verdicts, ticket / status as above; `grouped` and `own` untouched by a refusal).  Where the pool
 * form's second half cannot run the own parts are copied into their holes and vrs_msd_finish_grouped_u32 runs.  own == NULL (and
 * own_counts == NULL): vrs_msd_finish_grouped_counts_u32. */
int vrs_msd_finish_grouped_split_u32(vrs_context ctx, vrs_buffer grouped, vrs_buffer own, uint64_t own_offset, vrs_buffer out,
                                     uint32_t num_elements, uint32_t first_top_byte, uint32_t top_bytes, const uint32_t *counts,
                                     const uint32_t *own_counts);
int vrs_msd_finish_status(vrs_context ctx, int *took);
int vrs_msd_finish_ticket(vrs_context ctx, uint32_t *ticket);
int vrs_msd_finish_status_at(vrs_context ctx, uint32_t ticket, int *took);

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
 */
typedef enum vrs_sort_dtype {
    VRS_SORT_INT8 = 0, VRS_SORT_UINT8 = 1, VRS_SORT_INT16 = 2, VRS_SORT_INT32 = 3, VRS_SORT_INT64 = 4,
    VRS_SORT_FLOAT16 = 5, VRS_SORT_BFLOAT16 = 6, VRS_SORT_FLOAT32 = 7, VRS_SORT_FLOAT64 = 8
} vrs_sort_dtype;
enum { VRS_SORT_DESCENDING = 1 }; /* flags */
int vrs_sort_rank_keys(vrs_context ctx, vrs_buffer src, uint32_t num_elements, uint32_t row_len, int dtype, int flags,
                       vrs_buffer out_ranks /* uint32 or uint64 */, vrs_buffer out_positions /* uint32, may be NULL */);
int vrs_sort_restore(vrs_context ctx, vrs_buffer src, vrs_buffer ranks, vrs_buffer positions /* may be NULL */,
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
 * most 4 n + 16 S k + 1 MiB), contents afterwards unspecified; given that much the call never fails for lack of memory.
 * k == 0 or num_segments == 0: VRS_OK, nothing done.  NULL handles other than out_indices, an unknown key_type or flag bit,
 * num_segments * k >= 2^32 and undersized buffers: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 * Tiers by clamped length (vrs_topk_tier): up to 8192 keys one workgroup per segment selects inside LDS; longer segments are streamed
 * by one workgroup each; from VRS_TUNE_TOPK_GRID_MIN_KEYS on every phase is one launch over all the grid tier's segments.  Stream-
 * ordered on the context's stream; the call only enqueues (after settling a pending one-call sort) -- except with VRS_TOPK_SORTED and
 * k > 4096, where the survivors are sorted by vrs_sort_segments_pairs_u32 (vrs_sort_segments_u32 without out_indices), which may wait
 * for the stream when its work lists grow; that sort's segments count in vrs_segmented_stats.
 */
typedef enum vrs_topk_key_type { VRS_TOPK_U32 = 0, VRS_TOPK_I32 = 1, VRS_TOPK_F32 = 2 } vrs_topk_key_type;
enum { VRS_TOPK_LARGEST = 1, VRS_TOPK_SORTED = 2 }; /* flags */
typedef enum vrs_topk_tier {
    VRS_TOPK_LDS = 0,   /* up to 8192 keys (empty segments included) */
    VRS_TOPK_BLOCK = 1, /* longer, below VRS_TUNE_TOPK_GRID_MIN_KEYS */
    VRS_TOPK_GRID = 2   /* from VRS_TUNE_TOPK_GRID_MIN_KEYS on */
} vrs_topk_tier;
int vrs_topk_segments(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments,
                      uint32_t k, int key_type, int flags, vrs_buffer out_keys, vrs_buffer out_indices /* may be NULL */,
                      vrs_buffer scratch);
/* the scratch vrs_topk_segments needs: a pure function, needs no device (0 for k == 0 or num_segments == 0) */
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
 * scratch: at least vrs_select_scratch_bytes(...) bytes, contents afterwards unspecified; given that much the call never fails for
 * lack of memory.  num_segments == 0: VRS_OK, nothing done.  An unknown dtype, mode or flag bit, k == 0 with VRS_SELECT_KTH, a NULL
 * context, src, offsets, out_values or scratch, undersized buffers (src: num_elements elements; out_values: num_segments elements;
 * out_indices: num_segments uint32) and 8-byte elements off an 8-byte boundary: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
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
 * num_queries == 0: VRS_OK, nothing done.  num_boundaries == 0: every output 0.  A NULL context, queries or out (boundaries, when
 * there are any), an unknown dtype or flag bit, element counts that are not whole rows, row counts that neither match nor equal one
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
 */
enum { VRS_SEARCH_RIGHT = 1, VRS_SEARCH_OUT_INT64 = 2 }; /* flags */
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
    uint32_t reserved;         /* 0 */
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
    uint32_t reserved;
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
 * is given and out_offsets is NULL (the offsets then live in the scratch): at most (VRS_RLE_COUNTS ? 4 n : 0) + n / 256 + 1024 bytes.
 * Contents on entry unspecified, afterwards unspecified.  NULL ctx, keys, out_num_runs or scratch, a key_bytes other than 4 or 8 and
 * undersized buffers (n entries; n + 1 for out_offsets): VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.  Stream-ordered on the
 * context's stream; the call only enqueues (after settling a pending one-call sort).
 */
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
 * given: at most (2 * key bytes + (VRS_UNIQUE_INVERSE ? 8 : 0) + (VRS_UNIQUE_COUNTS ? 4 : 0)) * n + n / 256 + 2048 bytes.  Contents on
 * entry unspecified, afterwards unspecified.  NULL ctx, keys, out_keys, out_num_runs or scratch, an unknown key_type and undersized
 * buffers: VRS_ERROR_INVALID_ARGUMENT before anything is enqueued.
 * Blocking, as the segmented sorts': after settling a pending one-call sort the call may wait for the inner sort's plan head (bounded by
 * VRS_TUNE_PLAN_WAIT_MS -> VRS_ERROR_TIMEOUT, the encode then not enqueued), never for the sort itself; the inner sort counts in the
 * one-call statistics.
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

/*
 * Key preprocessing the reference leaves to the integrator ("you have to preprocess negative numbers",
 * README.md:154-155): in-place, order-preserving maps between int32 / float32 bit patterns and the uint32
 * keys the sort orders.  Asynchronous.  Apply *_TO_SORTABLE before the four passes and the inverse after.
 */
typedef enum vrs_key_transform {
    VRS_KEYS_INT32 = 0,               /* int32 <-> sortable: flips the sign bit (self-inverse) */
    VRS_KEYS_FLOAT32_TO_SORTABLE = 1, /* IEEE-754 total order: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN */
    VRS_KEYS_SORTABLE_TO_FLOAT32 = 2
} vrs_key_transform;
int vrs_transform_keys(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, int mode);

/*
 * On-device counterpart of MultiRadixSort::verify / testSort (MultiRadixSort.cpp:97-102,148-161), for results too
 * many or too large to download and compare on the host: *descents = number of positions with keys[i] > keys[i+1]
 * (0 == ascending); *key_sum and *key_mix = order-independent fingerprints (plain sum, sum of a 64-bit mix of every
 * key) -- equal before and after a sort iff, up to hash collisions, the output is a permutation of the input.
 * Synchronous (one read of the keys).  Any of the three outputs may be NULL.
 */
int vrs_verify_keys_u32(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, uint64_t *descents, uint64_t *key_sum,
                        uint64_t *key_mix);

/* ---- multi-GPU: key-range sharded sort, one rank per GPU (BASELINE.json configs[4]) ---- */
/*
 * No reference counterpart (VkRadixSort is single-GPU); north_star defines the path: shard by key range across the
 * GPUs of one node, ONE all-to-all over xGMI between the local step and the local sorts.  A step on rank g, in its
 * default (hybrid) shape -- the single-GPU hybrid sort with the exchange between its two MSD passes, 28 B/key per GPU:
 *   1. vrs_msd_partition_u32 of the shard: one counting read + the first MSD pass -- the shard grouped by the top byte;
 *   2. one all-gather of every rank's row (top-byte counts, shard size, bucket shift, status) and one all-reduce of the
 *      16384-bin bucket histograms; every rank derives the same byte-aligned splitters (vrs_dist_plan_splitters), its
 *      send and receive counts and where every message lands;
 *   3. `rounds` rounds of grouped send / recv on a second stream (round r = the r-th sub-range of every rank), one
 *      message per (sender, top byte) landing in top-byte order;
 *   4. vrs_msd_finish_u32 (second MSD pass + LDS-local sort) of round r's keys while the later rounds are on the wire.
 *      The sub-ranges are disjoint and ascending: their concatenation is rank g's range in ascending order.
 * Key ranges below 27 bits, shards below 2^16 keys or ranks that probed different key ranges make ALL ranks take the byte
 * shape instead (contract partition pass by the top byte, one message per (sender, round), vrs_sort_keys_u32 per received
 * sub-range; also forced by the environment variable VRS_DIST_SHAPE=byte, which must then be set on every rank).
 * Every decision to leave a step is taken by all ranks from the same gathered rows: a rank that cannot take part (shard
 * above its capacity, a failed local stage) says so in its row, still joins the collectives, and all ranks return together
 * (that rank its own error, the others VRS_ERROR_PEER).  A rank whose step fails LOCALLY outside those stages (a HIP or
 * transport call) returns at once without the collectives it has not reached: over RCCL the caller aborts the
 * communicator, as after any failed rank; the loopback transport marks its hub broken whenever one of ITS calls fails
 * (HIP, mismatch or misuse), so the peers leave their next rendezvous with an error instead of waiting.
 * Keys whose top bytes are too concentrated for byte-aligned ranges (more than 15 % over the even share, or more than the
 * SMALLEST capacity of all ranks: small keys, clustered keys) are cut at SAMPLED key values instead: every rank adds 2048
 * keys of its shard to a pool (a second all-gather), the world * rounds - 1 cut keys are the pool's weighted quantiles,
 * the shard is grouped by range (vrs_range_partition, 12 B/key) and a third all-gather hands out the range prefixes; one
 * message per (sender, round), vrs_sort_keys_u32_ranged per received sub-range.  Only keys with massive ties -- one key
 * VALUE holding more than a rank's share -- still return VRS_ERROR_UNBALANCED (on every rank); so does every
 * concentrated input under VRS_DIST_SAMPLED_SPLITTERS=0 (tests).  The Python orchestration
 * (vkradixsort_amd/distributed.py) adds a gather path for small totals on top of the same entry points.  Blocking for
 * the count exchange and, per round, for the round's plan; the exchange and the sorts complete on the context's stream.
 *
 * The wire is a table of functions.  vrs_dist_create binds RCCL at run time (dlopen): `nccl_comm` is an ncclComm_t of the
 * RCCL copy already in the process; NULL at world size 1 (every transfer is then a device copy).
 * vrs_dist_create_with_transport takes any table: every function returns 0 on success, counts are in uint32 words, `peer`
 * is a rank, `hip_stream` the stream the operation is ordered on; all_gather / all_reduce (sum) are called by every rank
 * with equal counts (recv of all_gather: world * words, in rank order), send / recv only between group_start and
 * group_end, matched in posting order per pair of ranks (the RCCL contract).
 * vrs_dist_loopback_*: an in-process transport -- the ranks are host THREADS of one process sharing a hub, every transfer a
 * device-to-device copy ordered by events (same GPU or peer GPUs of the process).  One process driving several GPUs can
 * use it instead of RCCL; the tests use it to run two ranks on one GPU.
 */
typedef struct vrs_dist_t *vrs_dist;
typedef struct vrs_dist_transport {
    void *user; /* handed back as the first argument of every call */
    int (*all_gather)(void *user, const void *send, void *recv, size_t words, void *hip_stream);
    int (*all_reduce)(void *user, const void *send, void *recv, size_t words, void *hip_stream);
    int (*group_start)(void *user);
    int (*send)(void *user, const void *buf, size_t words, int peer, void *hip_stream);
    int (*recv)(void *user, void *buf, size_t words, int peer, void *hip_stream);
    int (*group_end)(void *user);
    const char *(*error_string)(void *user, int code); /* may be NULL */
} vrs_dist_transport;
int vrs_dist_create(vrs_context ctx, void *nccl_comm, int rank, int world, uint32_t capacity_keys, int rounds,
                    vrs_dist *out_dist);
/* capacity_keys: shard size and receive capacity (the smallest capacity of all ranks bounds every rank's range);
 * rounds: 1 .. 32 / world (clamped).  The table is copied; `user` must outlive the vrs_dist. */
int vrs_dist_create_with_transport(vrs_context ctx, const vrs_dist_transport *transport, int rank, int world,
                                   uint32_t capacity_keys, int rounds, vrs_dist *out_dist);
int vrs_dist_destroy(vrs_dist dist);
/* keys: this rank's shard (num_elements <= capacity_keys; untouched).  *out_keys: a library-owned buffer holding this
 * rank's key range ascending in its first *out_count keys (valid until the next step or vrs_dist_destroy). */
int vrs_dist_sort_keys_u32(vrs_dist dist, vrs_buffer keys, uint32_t num_elements, vrs_buffer *out_keys,
                           uint32_t *out_count);
/* bounds[0] = 0 <= ... <= bounds[parts] = 256: part q owns top bytes [bounds[q], bounds[q+1]); host only */
int vrs_dist_plan_splitters(const uint64_t *counts256, int parts, uint32_t *bounds);
/* The cut keys of a sampled-splitter step (host only): samples[q * per_rank + i] = the i-th of per_rank keys taken at evenly spaced
 * positions of rank q's shard; a sample of rank q stands for shard_sizes[q] / per_rank keys.  splitters[p - 1], 1 <= p < parts, = the
 * first sample in key order at which p / parts of all keys have gone by (ascending; range r = number of splitters <= key). */
int vrs_dist_plan_sampled_splitters(const uint32_t *samples, const uint64_t *shard_sizes, int world, uint32_t per_rank, int parts,
                                    uint32_t *splitters);
const char *vrs_dist_last_error(vrs_dist dist);
/* cumulative: received sub-ranges finished in the hybrid shape / sorted by vrs_sort_keys_u32 after a refused plan; steps
 * that took the byte shape.  Any pointer may be NULL. */
int vrs_dist_stats(vrs_dist dist, uint64_t *hybrid_rounds, uint64_t *fallback_rounds, uint64_t *byte_shape_steps);
/* rounds of byte-shape steps finished by vrs_msd_finish_grouped_u32 (one counting read + second MSD pass + local sort: 20 B/key)
 * instead of a whole ranged sort (28) */
int vrs_dist_grouped_rounds(vrs_dist dist, uint64_t *grouped_rounds);
/* steps that cut the key ranges at sampled key values (top bytes too concentrated for byte-aligned ranges) */
int vrs_dist_splitter_steps(vrs_dist dist, uint64_t *splitter_steps);
typedef struct vrs_dist_loopback_t *vrs_dist_loopback;
int vrs_dist_loopback_create(int world, vrs_dist_loopback *out_hub);
/* the same hub over HOST memory (buffers are host pointers, transfers memcpy, streams ignored, no HIP call): the hub's matching and
 * barriers on a machine without a GPU -- test infrastructure of the sanitizer builds, not a transport for vrs_dist_create_with_transport */
int vrs_dist_loopback_create_host(int world, vrs_dist_loopback *out_hub);
/* fills *out with rank `rank`'s end of the hub; call it on the thread that drives the rank, its device current */
int vrs_dist_loopback_transport(vrs_dist_loopback hub, int rank, vrs_dist_transport *out);
int vrs_dist_loopback_destroy(vrs_dist_loopback hub);
/* A wire that costs something (a model of xGMI's point-to-point links for the SCHEDULE's sake -- how much of the exchange a given number
 * of rounds exposes --, never a measurement): every group of sends / receives holds the receiving rank's stream for (the most bytes one peer
 * sends it in the group) / link_gbps [10^9 bytes per second and link direction] + latency_us, every all-gather / all-reduce for latency_us.
 * 0 / 0 (the default) = the free wire.  Also read from VRS_LOOPBACK_LINK_GBPS / VRS_LOOPBACK_LATENCY_US when the hub is made.  Call
 * between steps. */
int vrs_dist_loopback_set_wire(vrs_dist_loopback hub, double link_gbps, double latency_us);

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

/* Test hook: copies the per-workgroup offset table (uint32[W*256], multi_radixsort.comp:76's
 * global_offsets for every workgroup) computed by the most recent RADIX_SORT stage. */
int vrs_debug_download_offsets(vrs_context ctx, void *host_data, size_t size_bytes);

/* Test hook: checks on the device that one returning LDS atomic hands same-address lanes their
 * pre-values in ascending lane order (what the RANK_ATOMIC scatter variants rely on); returns the
 * number of lanes whose rank differs from the __ballot-based rank over `rounds` rounds per wave. */
int vrs_debug_atomic_rank_selftest(vrs_context ctx, uint32_t rounds, uint32_t seed, uint64_t *mismatches);

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
/* The pool form keeps its scratch -- the slack buffer and the first pass's overflow regions, about 1.55 n uint32 slots for the largest sort
   the context has taken in that form (616 MB at 10^8 keys), twice that once pairs took it (vrs_pool_form_shape reports it) -- until the
   context is destroyed.  vrs_context_trim_scratch gives it back to the device now (after settling and waiting for what is on the stream;
   *released_bytes may be NULL); the next pool sort allocates again.  A device with no room for it is no error of a sort: the sort takes a
   form that needs no such scratch (28 / 36 bytes per key instead of 24), vrs_one_call_pool_no_memory counts those sorts, and with the
   adaptive setting (VRS_TUNE_MSD_POOL = 1) the next 15 sorts of that size do not ask again. */
int vrs_context_trim_scratch(vrs_context ctx, uint64_t *released_bytes);
int vrs_one_call_pool_no_memory(vrs_context ctx, uint64_t *sorts);
/* VRS_TUNE_MSD_POOL_REUSE_LAYOUT: *reused = pool sorts that started in the regions of an earlier sort, *stale = those of them whose keys
   did not fit (run again with their own sample).  Either pointer may be NULL. */
int vrs_one_call_pool_layouts(vrs_context ctx, uint64_t *reused, uint64_t *stale);
/* The forms of the one-call sorts that share L2-resident words between workgroups rest on where the blocks of a launch run
   ("block b on the XCC of place b % 8 of the probed order"), which the context probes when it is created.  Observed on MI355X: the
   dispatcher's round-robin starts at an XCC of the hardware queue's own, and a HIP stream may move to another queue -- the probed
   order is then rotated.  Every kernel checks (HW_REG_XCC_ID) and stays exact; the first workgroups that find themselves elsewhere
   say so, and the next vrs_sort_* call probes again.  *reprobes = how often that happened; *xcc_map = the probed order (byte x =
   the XCC of the blocks with index % 8 == x); *valid = the probe found the b % 8 rule intact.  Any pointer may be NULL. */
int vrs_debug_xcc_placement(vrs_context ctx, uint64_t *reprobes, uint64_t *xcc_map, int *valid);

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

const char *vrs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VKRADIXSORT_AMD_H */
