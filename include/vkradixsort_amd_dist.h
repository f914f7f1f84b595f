/*
 * vkradixsort_amd_dist.h -- the sort in halves and the multi-GPU step (build extensions; no reference counterpart).
 *
 * For callers that move keys between the passes of a sort: the pieces the key-range exchange is made of (a ranged sort, the
 * range partition, the digit offsets on the device), the two MSD halves of the hybrid form (vrs_msd_*) and the multi-GPU
 * step itself (vrs_dist_*).  A comment that begins "The same" continues the declaration of the like-named call in
 * vkradixsort_amd.h.
 */
#ifndef VKRADIXSORT_AMD_DIST_H
#define VKRADIXSORT_AMD_DIST_H

#include <stddef.h>
#include <stdint.h>

#include "vkradixsort_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* The same sort for keys the caller knows to lie in [key_floor, 2^32) -- a sub-range of a larger sort (the received key range
 * of a multi-GPU step): the hybrid form then takes its 16384 buckets from key - (key_floor rounded down to a multiple of 2^24),
 * as it would for a full key range, instead of finding almost all of them empty and the rest too large.  A hint only: a key
 * below the floor makes the plan refuse the hybrid form (the LSD passes run) -- the result is the same either way. */
int vrs_sort_keys_u32_ranged(vrs_context ctx, vrs_buffer keys, vrs_buffer keys_tmp, uint32_t num_elements, uint32_t key_floor);
/*
 * Range partition (build extension for the multi-GPU key-range exchange; no reference counterpart): one
 * stable pass that groups uint32 keys by range instead of by digit.  `splitters` holds `num_splitters` <= 255
 * ascending uint32 values on the device; a key goes to range r = number of splitters <= key.  keys_out holds
 * range 0's keys, then range 1's, ... each in input order; vrs_multi_radixsort_digit_offsets then returns
 * the first position of every range (entries 0..num_splitters).  Asynchronous.
 */
int vrs_range_partition(vrs_context ctx, vrs_buffer keys_in, vrs_buffer keys_out, vrs_buffer splitters,
                        uint32_t num_splitters, uint32_t num_elements);
/* The same 256 words copied into a device buffer, asynchronously (no host round trip: the multi-GPU step feeds
 * them straight into its count all-gather). */
int vrs_multi_radixsort_digit_offsets_device(vrs_context ctx, vrs_buffer out_u32x256);
/* One-shot hook for the NEXT RADIX_SORT stage of the context: as soon as its offset table is complete -- before its scatter kernel --
 * the stage copies the 256 digit offsets to out_u32x256 (may be NULL) and records `event` (a hipEvent_t of the caller's, may be NULL)
 * on the context's stream.  Work on another stream that needs only the offsets (the multi-GPU step's all-gather) then runs beside
 * the scatter.  (The reference has no counterpart: its prefix lives inside multi_radixsort.comp:63-87.) */
int vrs_multi_radixsort_offsets_hook(vrs_context ctx, vrs_buffer out_u32x256, void *event);

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

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* VKRADIXSORT_AMD_DIST_H */
