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
 *
 * Beside this header: vkradixsort_amd_ops.h (operations built on the sort), vkradixsort_amd_dist.h (the
 * sort in halves, the multi-GPU step) and vkradixsort_amd_tune.h, which holds what the comments below
 * name but a sort does not need: the VRS_TUNE_* settings with vrs_set_tuning, the vrs_one_call_*
 * counters and the profile calls.  vrs_dist_* and vrs_sort_keys_u32_ranged are in the dist header.
 */
#ifndef VKRADIXSORT_AMD_H
#define VKRADIXSORT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

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
/* The pool form keeps its scratch -- the slack buffer and the first pass's overflow regions, about 1.55 n uint32 slots for the largest sort
   the context has taken in that form (616 MB at 10^8 keys), twice that once pairs took it (vrs_pool_form_shape reports it) -- until the
   context is destroyed.  vrs_context_trim_scratch gives it back to the device now (after settling and waiting for what is on the stream;
   *released_bytes may be NULL); the next pool sort allocates again.  A device with no room for it is no error of a sort: the sort takes a
   form that needs no such scratch (28 / 36 bytes per key instead of 24), vrs_one_call_pool_no_memory counts those sorts, and with the
   adaptive setting (VRS_TUNE_MSD_POOL = 1) the next 15 sorts of that size do not ask again. */
int vrs_context_trim_scratch(vrs_context ctx, uint64_t *released_bytes);

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

const char *vrs_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* VKRADIXSORT_AMD_H */
