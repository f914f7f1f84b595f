// vrs_capi_unique.hip -- the C ABI of run-length encoding (vrs_run_length_encode) and unique (vrs_unique): argument checks, the scratch
// layouts, the launches of vrs_unique.hip, and for unique the stable one-call sort of the mapped keys on views of the scratch.  The row
// form (VRS_UNIQUE_COLUMNS(C), C >= 2, in key_type / key_bytes): the same checks counted in rows, the LSD rounds over groups of columns
// (pack, stable pair sort, settle) and the launches of vrs_unique_rows.hip.
#include "vrs_host.hpp"
#include "vrs_unique.hpp"
#include "vrs_unique_rows_order.hpp"

using namespace vrsh;

namespace {

constexpr int kKnownRleFlags = vrs::kRleCounts;
constexpr int kKnownUniqueFlags = vrs::kUniqueInverse | vrs::kUniqueCounts;

bool known_key_type(int key_type) { return key_type >= vrs::kUniqueU32 && key_type <= vrs::kUniqueF64; }

// key_type / key_bytes with VRS_UNIQUE_COLUMNS(c) in bits 8 and up: the low byte and the columns (0 and 1: the word form).  A negative
// value has no known low byte.
struct Encoded {
    int low;
    uint32_t cols;
    bool rows() const { return cols >= 2u; }
};
Encoded decode(int encoded) { return encoded < 0 ? Encoded{-1, 0u} : Encoded{vrs::rows_low_byte(encoded), vrs::rows_columns(encoded)}; }
// n rows of cols words: fewer than 2^32 words
bool rows_fit(uint32_t n, uint32_t cols) { return static_cast<uint64_t>(n) * cols < (1ull << 32); }

// the look-back's status words are 64 bits wide and are their own flag: a word that straddles an 8-byte boundary could be seen half
// written (and 64-bit keys sorted inside unique's scratch sit behind them)
bool off_status_boundary(vrs_buffer scratch) { return (reinterpret_cast<uintptr_t>(scratch->ptr) & 7u) != 0u; }

// n == 0: R = 0 is the whole result
int write_no_runs(vrs_context ctx, vrs_buffer out_num_runs) {
    VRS_HIP(ctx, hipMemsetAsync(out_num_runs->ptr, 0, sizeof(uint32_t), ctx->stream));
    return VRS_OK;
}

// vrs_run_length_encode, row form: n rows of k.cols words of k.low bytes
int encode_rows(vrs_context ctx, vrs_buffer keys, uint32_t n, Encoded k, vrs_buffer out_keys, vrs_buffer out_offsets, vrs_buffer out_counts,
                vrs_buffer out_run_ids, vrs_buffer out_num_runs, vrs_buffer scratch) {
    if (!keys || !out_num_runs || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    if (!rows_fit(n, k.cols)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: rows x columns must be below 2^32");
    const size_t kb = static_cast<size_t>(n) * k.cols * static_cast<size_t>(k.low), wb = static_cast<size_t>(n) * sizeof(uint32_t);
    const vrs::RleLayout L = vrs::rle_rows_layout(n);
    int rc;
    if ((rc = check_buffer(ctx, keys, kb, "keys")) || (rc = check_buffer(ctx, out_num_runs, sizeof(uint32_t), "out_num_runs")) ||
        (out_keys && (rc = check_buffer(ctx, out_keys, kb, "out_keys"))) ||
        (out_offsets && (rc = check_buffer(ctx, out_offsets, wb + sizeof(uint32_t), "out_offsets"))) ||
        (out_counts && (rc = check_buffer(ctx, out_counts, wb, "out_counts"))) ||
        (out_run_ids && (rc = check_buffer(ctx, out_run_ids, wb, "out_run_ids"))) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    if (off_status_boundary(scratch)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (n == 0u) return write_no_runs(ctx, out_num_runs);
    char *s = static_cast<char *>(scratch->ptr);
    vrs::RleRowArgs r{};
    r.a.keys = nullptr;
    r.a.n = n;
    r.a.key_bytes = 8;
    r.a.key_type = -1;
    r.a.idx = nullptr;
    r.a.out_keys = out_keys ? out_keys->ptr : nullptr;
    r.a.out_offsets = out_offsets ? static_cast<uint32_t *>(out_offsets->ptr) : reinterpret_cast<uint32_t *>(s + L.offsets);
    r.a.out_counts = out_counts ? static_cast<uint32_t *>(out_counts->ptr) : nullptr;
    r.a.out_run_ids = out_run_ids ? static_cast<uint32_t *>(out_run_ids->ptr) : nullptr;
    r.a.out_num_runs = static_cast<uint32_t *>(out_num_runs->ptr);
    r.a.status = s + L.status;
    r.rows = keys->ptr;
    r.pos = nullptr;
    r.cols = k.cols;
    r.word = static_cast<uint32_t>(k.low);
    r.c0 = 8u / r.word;  // the columns behind a row's first 8 bytes
    VRS_HIP(ctx, vrs::launch_rle_rows(ctx->stream, r));
    return VRS_OK;
}

// vrs_unique, row form: n rows of k.cols words of key type k.low
int unique_rows(vrs_context ctx, vrs_buffer keys, uint32_t n, Encoded k, vrs_buffer out_keys, vrs_buffer out_counts, vrs_buffer out_inverse,
                vrs_buffer out_num_runs, vrs_buffer scratch) {
    if (!keys || !out_keys || !out_num_runs || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    if (!rows_fit(n, k.cols)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "unique: rows x columns must be below 2^32");
    const uint32_t word = static_cast<uint32_t>(vrs::unique_key_bytes(k.low));
    const size_t kb = static_cast<size_t>(n) * k.cols * word, wb = static_cast<size_t>(n) * sizeof(uint32_t);
    const vrs::UniqueRowsLayout L = vrs::unique_rows_layout(n);
    int rc;
    if ((rc = check_buffer(ctx, keys, kb, "keys")) || (rc = check_buffer(ctx, out_keys, kb, "out_keys")) ||
        (rc = check_buffer(ctx, out_num_runs, sizeof(uint32_t), "out_num_runs")) ||
        (out_counts && (rc = check_buffer(ctx, out_counts, wb, "out_counts"))) ||
        (out_inverse && (rc = check_buffer(ctx, out_inverse, wb, "out_inverse"))) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    if (off_status_boundary(scratch)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "unique: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (n == 0u) return write_no_runs(ctx, out_num_runs);

    // one round per group of columns, least significant first: the group's keys of the rows in their current order, then the stable
    // pair sort of (key, position) on views of the scratch, settled as the word form's sort is
    char *s = static_cast<char *>(scratch->ptr);
    auto *pos = reinterpret_cast<uint32_t *>(s + L.pos);
    const uint32_t rounds = vrs::rows_rounds(k.cols, word);
    uint32_t top_bytes = 8u;
    for (uint32_t g = 0; g < rounds; ++g) {
        top_bytes = vrs::rows_group(k.cols, word, g).count * word;
        VRS_HIP(ctx, vrs::launch_rows_pack(ctx->stream, keys->ptr, n, k.cols, word, k.low, g, s + L.keys, pos));
        const size_t gb = static_cast<size_t>(n) * top_bytes;
        vrs_buffer_t kv = stack_view(ctx, s + L.keys, gb), kt = stack_view(ctx, s + L.keys_tmp, gb);
        vrs_buffer_t vv = stack_view(ctx, s + L.pos, wb), vt = stack_view(ctx, s + L.pos_tmp, wb);
        rc = top_bytes == 8u ? vrs_sort_pairs_u64(ctx, &kv, &kt, &vv, &vt, n) : vrs_sort_pairs_u32(ctx, &kv, &kt, &vv, &vt, n);
        if (rc || (rc = settle_pending(ctx))) return rc;
    }
    vrs::RleRowArgs r{};
    r.a.keys = s + L.keys;
    r.a.n = n;
    r.a.key_bytes = static_cast<int>(top_bytes);
    r.a.key_type = k.low;
    r.a.idx = out_inverse ? pos : nullptr;
    r.a.out_keys = out_keys->ptr;
    r.a.out_offsets = reinterpret_cast<uint32_t *>(s + L.offsets);
    r.a.out_counts = out_counts ? static_cast<uint32_t *>(out_counts->ptr) : nullptr;
    r.a.out_run_ids = out_inverse ? static_cast<uint32_t *>(out_inverse->ptr) : nullptr;
    r.a.out_num_runs = static_cast<uint32_t *>(out_num_runs->ptr);
    r.a.status = s + L.status;
    r.rows = keys->ptr;
    r.pos = pos;
    r.cols = k.cols;
    r.word = word;
    r.c0 = top_bytes / word;  // the columns behind the top group
    VRS_HIP(ctx, vrs::launch_rle_rows(ctx->stream, r));
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_run_length_encode_scratch_bytes(uint32_t num_elements, int key_bytes, int flags, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    const Encoded k = decode(key_bytes);
    if (k.low != 4 && k.low != 8) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: key_bytes must be 4 or 8");
    if (flags & ~kKnownRleFlags) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: unknown flag bits");
    if (k.rows() && !rows_fit(num_elements, k.cols)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: rows x columns must be below 2^32");
    *bytes = k.rows() ? vrs::rle_rows_layout(num_elements).bytes : vrs::rle_layout(num_elements, flags).bytes;
    return VRS_OK;
}

int vrs_run_length_encode(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, int key_bytes, vrs_buffer out_keys, vrs_buffer out_offsets,
                          vrs_buffer out_counts, vrs_buffer out_run_ids, vrs_buffer out_num_runs, vrs_buffer scratch) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    const Encoded k = decode(key_bytes);
    if (k.low != 4 && k.low != 8) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: key_bytes must be 4 or 8");
    if (k.rows()) return encode_rows(ctx, keys, num_elements, k, out_keys, out_offsets, out_counts, out_run_ids, out_num_runs, scratch);
    key_bytes = k.low;
    if (!keys || !out_num_runs || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const uint32_t n = num_elements;
    const size_t kb = static_cast<size_t>(n) * key_bytes, wb = static_cast<size_t>(n) * sizeof(uint32_t);
    const vrs::RleLayout L = vrs::rle_layout(n, out_counts && !out_offsets ? vrs::kRleCounts : 0);
    int rc;
    if ((rc = check_buffer(ctx, keys, kb, "keys")) || (rc = check_buffer(ctx, out_num_runs, sizeof(uint32_t), "out_num_runs")) ||
        (out_keys && (rc = check_buffer(ctx, out_keys, kb, "out_keys"))) ||
        (out_offsets && (rc = check_buffer(ctx, out_offsets, wb + sizeof(uint32_t), "out_offsets"))) ||
        (out_counts && (rc = check_buffer(ctx, out_counts, wb, "out_counts"))) ||
        (out_run_ids && (rc = check_buffer(ctx, out_run_ids, wb, "out_run_ids"))) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    if (off_status_boundary(scratch)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "run-length encode: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (n == 0u) return write_no_runs(ctx, out_num_runs);
    char *s = static_cast<char *>(scratch->ptr);
    vrs::RleArgs a{};
    a.keys = keys->ptr;
    a.n = n;
    a.key_bytes = key_bytes;
    a.key_type = -1;
    a.idx = nullptr;
    a.out_keys = out_keys ? out_keys->ptr : nullptr;
    a.out_offsets = out_offsets ? static_cast<uint32_t *>(out_offsets->ptr) : out_counts ? reinterpret_cast<uint32_t *>(s + L.offsets) : nullptr;
    a.out_counts = out_counts ? static_cast<uint32_t *>(out_counts->ptr) : nullptr;
    a.out_run_ids = out_run_ids ? static_cast<uint32_t *>(out_run_ids->ptr) : nullptr;
    a.out_num_runs = static_cast<uint32_t *>(out_num_runs->ptr);
    a.status = s + L.status;
    VRS_HIP(ctx, vrs::launch_rle(ctx->stream, a));
    return VRS_OK;
}

int vrs_unique_scratch_bytes(uint32_t num_elements, int key_type, int flags, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    const Encoded k = decode(key_type);
    if (!known_key_type(k.low)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "unique: unknown key_type");
    if (flags & ~kKnownUniqueFlags) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "unique: unknown flag bits");
    if (k.rows() && !rows_fit(num_elements, k.cols)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "unique: rows x columns must be below 2^32");
    *bytes = k.rows() ? vrs::unique_rows_layout(num_elements).bytes : vrs::unique_layout(num_elements, k.low, flags).bytes;
    return VRS_OK;
}

int vrs_unique(vrs_context ctx, vrs_buffer keys, uint32_t num_elements, int key_type, vrs_buffer out_keys, vrs_buffer out_counts,
               vrs_buffer out_inverse, vrs_buffer out_num_runs, vrs_buffer scratch) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    const Encoded k = decode(key_type);
    if (!known_key_type(k.low)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "unique: unknown key_type");
    if (k.rows()) return unique_rows(ctx, keys, num_elements, k, out_keys, out_counts, out_inverse, out_num_runs, scratch);
    key_type = k.low;
    if (!keys || !out_keys || !out_num_runs || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const uint32_t n = num_elements;
    const int kbytes = vrs::unique_key_bytes(key_type);
    const size_t kb = static_cast<size_t>(n) * kbytes, wb = static_cast<size_t>(n) * sizeof(uint32_t);
    const int flags = (out_inverse ? vrs::kUniqueInverse : 0) | (out_counts ? vrs::kUniqueCounts : 0);
    const vrs::UniqueLayout L = vrs::unique_layout(n, key_type, flags);
    int rc;
    if ((rc = check_buffer(ctx, keys, kb, "keys")) || (rc = check_buffer(ctx, out_keys, kb, "out_keys")) ||
        (rc = check_buffer(ctx, out_num_runs, sizeof(uint32_t), "out_num_runs")) ||
        (out_counts && (rc = check_buffer(ctx, out_counts, wb, "out_counts"))) ||
        (out_inverse && (rc = check_buffer(ctx, out_inverse, wb, "out_inverse"))) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    if (off_status_boundary(scratch)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "unique: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (n == 0u) return write_no_runs(ctx, out_num_runs);

    // 1. ranks (and iota payloads) into the scratch; 2. the stable one-call sort on views of it, settled: everything it needs is on the
    // stream (it may wait for its plan's head, never for the sort); 3. the encode over the sorted ranks
    char *s = static_cast<char *>(scratch->ptr);
    auto *vals = out_inverse ? reinterpret_cast<uint32_t *>(s + L.vals) : nullptr;
    VRS_HIP(ctx, vrs::launch_unique_map(ctx->stream, keys->ptr, n, key_type, s + L.keys, vals));
    vrs_buffer_t kv = stack_view(ctx, s + L.keys, kb), kt = stack_view(ctx, s + L.keys_tmp, kb);
    vrs_buffer_t vv = stack_view(ctx, s + L.vals, wb), vt = stack_view(ctx, s + L.vals_tmp, wb);
    if (kbytes == 8)
        rc = out_inverse ? vrs_sort_pairs_u64(ctx, &kv, &kt, &vv, &vt, n) : vrs_sort_keys_u64(ctx, &kv, &kt, n);
    else
        rc = out_inverse ? vrs_sort_pairs_u32(ctx, &kv, &kt, &vv, &vt, n) : vrs_sort_keys_u32(ctx, &kv, &kt, n);
    if (rc || (rc = settle_pending(ctx))) return rc;
    vrs::RleArgs a{};
    a.keys = s + L.keys;
    a.n = n;
    a.key_bytes = kbytes;
    a.key_type = key_type;
    a.idx = vals;
    a.out_keys = out_keys->ptr;
    a.out_offsets = out_counts ? reinterpret_cast<uint32_t *>(s + L.offsets) : nullptr;
    a.out_counts = out_counts ? static_cast<uint32_t *>(out_counts->ptr) : nullptr;
    a.out_run_ids = out_inverse ? static_cast<uint32_t *>(out_inverse->ptr) : nullptr;
    a.out_num_runs = static_cast<uint32_t *>(out_num_runs->ptr);
    a.status = s + L.status;
    VRS_HIP(ctx, vrs::launch_rle(ctx->stream, a));
    return VRS_OK;
}

}  // extern "C"
