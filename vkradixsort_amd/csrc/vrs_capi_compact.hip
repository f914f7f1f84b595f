// vrs_capi_compact.hip -- the C ABI of the ordered stream compaction (vrs_compact_*): argument checks, the pure companions (tiles, scratch
// size, the division by a constant), the statistics, the rules restated on the host (vrs_compact_host) and the launches of vrs_compact.hip.
#include "vrs_host.hpp"
#include "vrs_compact.hpp"

using namespace vrsh;

namespace {

int check_span(vrs_context ctx, uint64_t n, uint32_t T) {
    if (!vrs::compact_tile_known(T)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: tile_elems must be a multiple of 4096 in 4096 .. 65536");
    if (n >= (1ull << 32)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: fewer than 2^32 elements");
    return VRS_OK;
}

int check_shape(vrs_context ctx, uint64_t n, uint32_t ndim, const uint32_t *shape) {
    if (ndim < 1u || ndim > vrs::kCompactMaxDims) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: coordinates take 1 .. 8 dims");
    uint64_t product = 1u;
    for (uint32_t k = 0; k < ndim; ++k) {
        product *= shape[k];
        if (product >= (1ull << 32)) break;  // (n is below 2^32: it cannot match, and nothing wraps)
    }
    if (product != n) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: the product of shape is not n");
    return VRS_OK;
}

bool overlap(const void *p, size_t pb, const void *q, size_t qb) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pb != 0u && qb != 0u && a < b + qb && b < a + pb;
}

bool off_boundary(const void *p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) != 0u; }

// flags, n, dtype and scratch as both device calls take them
int check_common(vrs_context ctx, vrs_buffer flags, uint64_t n, int dtype, vrs_buffer scratch, vrs::CompactLayout *layout) {
    if (!vrs::compact_dtype_known(dtype)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: dtype is one of vrs_sort_dtype or VRS_COMPACT_BOOL");
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (const int rc = check_span(ctx, n, ctx->tune.compact_tile_elems)) return rc;
    *layout = vrs::compact_layout(n, ctx->tune.compact_tile_elems);
    if (n == 0u) return VRS_OK;
    int rc;
    const size_t flag_bytes = static_cast<size_t>(n) * static_cast<size_t>(vrs::compact_dtype_bytes(dtype));
    if ((rc = check_buffer(ctx, flags, flag_bytes, "flags")) || (rc = check_buffer(ctx, scratch, layout->bytes, "scratch"))) return rc;
    if (off_boundary(flags->ptr, static_cast<size_t>(vrs::compact_dtype_bytes(dtype))) || off_boundary(scratch->ptr, 16u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: flags on their element's boundary, scratch on 16 bytes");
    if (overlap(flags->ptr, flag_bytes, scratch->ptr, layout->bytes)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: flags and scratch may not overlap");
    return VRS_OK;
}

template <class W>
uint64_t host_bits(const void *flags, uint64_t i) {
    return static_cast<const W *>(flags)[i];
}

// row `to` of dst = row `from` of src, rows of row_bytes (one element, or the row form's W elements), word by word as the kernels copy it
void host_copy(void *dst, uint64_t to, const void *src, uint64_t from, uint64_t row_bytes, uint32_t word_bytes) {
    char *d = static_cast<char *>(dst) + to * row_bytes;
    const char *s = static_cast<const char *>(src) + from * row_bytes;
    for (uint64_t w = 0; w < row_bytes; w += word_bytes) std::memcpy(d + w, s + w, word_bytes);
}

uint64_t address(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// the elements one flag stands for: row_elems, where 0 says what 1 says
uint64_t row_width(uint32_t row_elems) { return row_elems >= 2u ? row_elems : 1u; }

// n x W x value_bytes, or false when that passes 2^62 (no buffer is that large, and nothing wraps)
bool row_form_bytes(uint64_t n, uint64_t W, uint32_t value_bytes, uint64_t *row_bytes) {
    *row_bytes = W * value_bytes;  // (below 2^35)
    return (static_cast<unsigned __int128>(n) * *row_bytes >> 62) == 0u;
}

}  // namespace

extern "C" {

int vrs_compact_tiles_for(uint64_t n, uint32_t tile_elems, uint32_t *tiles) {
    if (!tiles) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "tiles is NULL");
    if (const int rc = check_span(nullptr, n, tile_elems)) return rc;
    *tiles = vrs::compact_tiles(n, tile_elems);
    return VRS_OK;
}

int vrs_compact_scratch_bytes(uint64_t n, uint32_t tile_elems, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (const int rc = check_span(nullptr, n, tile_elems)) return rc;
    *bytes = vrs::compact_layout(n, tile_elems).bytes;
    return VRS_OK;
}

int vrs_compact_divide(uint32_t numerator, uint32_t divisor, uint32_t *quotient, uint32_t *remainder) {
    if (divisor == 0u) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: the divisor must be 1 or more");
    const vrs::CompactDiv c = vrs::compact_div_make(divisor);
    if (quotient) *quotient = vrs::compact_div(numerator, c);
    if (remainder) *remainder = vrs::compact_mod(numerator, c);
    return VRS_OK;
}

int vrs_compact_stats(vrs_context ctx, uint64_t *count_calls, uint64_t *emit_calls, uint64_t *elements) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (count_calls) *count_calls = ctx->compact_calls[0];
    if (emit_calls) *emit_calls = ctx->compact_calls[1];
    if (elements) *elements = ctx->compact_elements;
    return VRS_OK;
}

int vrs_compact_host(const void *flags, uint64_t n, int dtype, const vrs_compact_host_outputs *outputs, uint64_t *out_count) {
    if (!vrs::compact_dtype_known(dtype)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: dtype is one of vrs_sort_dtype or VRS_COMPACT_BOOL");
    if (n >= (1ull << 32)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: fewer than 2^32 elements");
    if (n != 0u && !flags) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "flags is NULL");
    const vrs_compact_host_outputs none{};
    const vrs_compact_host_outputs &o = outputs ? *outputs : none;
    if (o.coords && o.coords_layout != VRS_COMPACT_ROWS && o.coords_layout != VRS_COMPACT_COLUMNS)
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: coords_layout is VRS_COMPACT_ROWS or VRS_COMPACT_COLUMNS");
    if (o.coords)
        if (const int rc = check_shape(nullptr, n, o.ndim, o.shape)) return rc;
    if ((o.gather_out || o.scatter_out) && !vrs::compact_value_bytes_known(o.value_bytes))
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: value_bytes is 1, 2, 4 or 8");
    if (n != 0u && ((o.gather_out && !o.gather_values) || (o.scatter_out && !o.scatter_input)))
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: gather_values or scatter_input is NULL");
    const uint64_t W = row_width(o.row_elems);
    uint64_t row_bytes = 0u;
    if ((o.gather_out || o.scatter_out) && !row_form_bytes(n, W, o.value_bytes, &row_bytes))
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: n x row_elems x value_bytes is below 2^62");
    const uint32_t gather_word = vrs::compact_row_word_bytes(row_bytes, address(o.gather_values) | address(o.gather_out));
    const uint32_t scatter_word = vrs::compact_row_word_bytes(row_bytes, address(o.scatter_input) | address(o.scatter_source) | address(o.scatter_out));
    const uint64_t keep = vrs::compact_keep_mask(dtype);
    const int bytes = vrs::compact_dtype_bytes(dtype);
    auto set = [&](uint64_t i) {
        const uint64_t bits = bytes == 1 ? host_bits<uint8_t>(flags, i) : bytes == 2 ? host_bits<uint16_t>(flags, i)
                              : bytes == 4 ? host_bits<uint32_t>(flags, i) : host_bits<uint64_t>(flags, i);
        return vrs::compact_nonzero(bits, keep);
    };
    uint64_t R = 0u;
    for (uint64_t i = 0; i < n; ++i) R += set(i) ? 1u : 0u;
    if (out_count) *out_count = R;
    if (o.scatter_out && (o.scatter_source_elems / W < R || (R != 0u && !o.scatter_source)))
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "compact: scatter_source holds fewer elements (rows of row_elems) than flags are nonzero");
    const vrs::CompactShape shape = o.coords && n != 0u ? vrs::compact_shape_make(o.ndim, o.shape) : vrs::CompactShape{};
    uint64_t row = 0u;
    for (uint64_t i = 0; i < n; ++i) {
        const bool s = set(i);
        if (o.scatter_out) host_copy(o.scatter_out, i, s ? o.scatter_source : o.scatter_input, s ? row : i, row_bytes, scatter_word);
        if (!s) continue;
        const uint32_t p = static_cast<uint32_t>(i);
        if (o.flat) o.flat[row] = static_cast<int64_t>(p);
        if (o.coords)
            for (uint32_t k = 0; k < o.ndim; ++k)
                o.coords[o.coords_layout == VRS_COMPACT_ROWS ? row * o.ndim + k : k * R + row] = static_cast<int64_t>(vrs::compact_coordinate(p, shape, k));
        if (o.gather_out) host_copy(o.gather_out, row, o.gather_values, i, row_bytes, gather_word);
        ++row;
    }
    return VRS_OK;
}

int vrs_compact_count(vrs_context ctx, vrs_buffer flags, uint64_t n, int dtype, vrs_buffer scratch, vrs_buffer out_count_device, uint64_t *host_count) {
    vrs::CompactLayout l{};
    int rc;
    if ((rc = check_common(ctx, flags, n, dtype, scratch, &l))) return rc;
    if (out_count_device) {
        if ((rc = check_buffer(ctx, out_count_device, sizeof(int64_t), "out_count_device"))) return rc;
        if (off_boundary(out_count_device->ptr, 8u)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: out_count_device on 8 bytes");
        if (n != 0u && (overlap(out_count_device->ptr, 8u, scratch->ptr, l.bytes) ||
                        overlap(out_count_device->ptr, 8u, flags->ptr, static_cast<size_t>(n) * static_cast<size_t>(vrs::compact_dtype_bytes(dtype)))))
            return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: out_count_device may not overlap flags or scratch");
    }
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (n == 0u) {
        if (out_count_device) VRS_HIP(ctx, hipMemsetAsync(out_count_device->ptr, 0, sizeof(int64_t), ctx->stream));
        if (host_count) *host_count = 0u;
        return VRS_OK;
    }
    vrs::CompactCountArgs a{};
    a.flags = flags->ptr;
    a.n = n;
    a.T = ctx->tune.compact_tile_elems;
    a.dtype = dtype;
    a.scratch = static_cast<char *>(scratch->ptr);
    a.out_count = out_count_device ? static_cast<long long *>(out_count_device->ptr) : nullptr;
    VRS_HIP(ctx, vrs::launch_compact_count(ctx->stream, a));
    ++ctx->compact_calls[0];
    ctx->compact_elements += n;
    if (host_count) {
        unsigned long long total = 0u;
        VRS_HIP(ctx, hipMemcpyAsync(&total, scratch->ptr, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
        VRS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *host_count = total;
    }
    return VRS_OK;
}

int vrs_compact_emit(vrs_context ctx, vrs_buffer flags, uint64_t n, int dtype, vrs_buffer scratch, const vrs_compact_outputs *outputs) {
    vrs::CompactLayout l{};
    int rc;
    if ((rc = check_common(ctx, flags, n, dtype, scratch, &l))) return rc;
    if (!outputs) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "outputs is NULL");
    const vrs_compact_outputs &o = *outputs;
    const uint64_t R = o.num_selected;
    if (R > n) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: num_selected is at most n");
    if (o.coords && o.coords_layout != VRS_COMPACT_ROWS && o.coords_layout != VRS_COMPACT_COLUMNS)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: coords_layout is VRS_COMPACT_ROWS or VRS_COMPACT_COLUMNS");
    if (o.coords && (rc = check_shape(ctx, n, o.ndim, o.shape))) return rc;
    if ((o.gather_out || o.scatter_out) && !vrs::compact_value_bytes_known(o.value_bytes))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: value_bytes is 1, 2, 4 or 8");
    uint64_t row_bytes = 0u;
    if ((o.gather_out || o.scatter_out) && !row_form_bytes(n, row_width(o.row_elems), o.value_bytes, &row_bytes))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: n x row_elems x value_bytes is below 2^62");
    if (n == 0u) return VRS_OK;
    const size_t vb = o.value_bytes, rb = row_bytes, flag_bytes = static_cast<size_t>(n) * static_cast<size_t>(vrs::compact_dtype_bytes(dtype));
    // every output: (buffer, bytes it must hold, its boundary); an output of no bytes (R == 0) needs no buffer and is left out
    struct Out {
        vrs_buffer buf;
        size_t bytes, boundary;
        const char *name;
    };
    const Out outs[4] = {{o.flat, static_cast<size_t>(R) * 8u, 8u, "flat"},
                         {o.coords, static_cast<size_t>(R) * 8u * (o.coords ? o.ndim : 0u), 8u, "coords"},
                         {o.gather_out, static_cast<size_t>(R) * rb, vb, "gather_out"},
                         {o.scatter_out, static_cast<size_t>(n) * rb, vb, "scatter_out"}};
    const Out ins[3] = {{o.gather_out ? o.gather_values : nullptr, static_cast<size_t>(n) * rb, vb, "gather_values"},
                        {o.scatter_out ? o.scatter_input : nullptr, static_cast<size_t>(n) * rb, vb, "scatter_input"},
                        {o.scatter_out ? o.scatter_source : nullptr, static_cast<size_t>(R) * rb, vb, "scatter_source"}};
    for (const Out &x : outs) {
        if (!x.buf || x.bytes == 0u) continue;
        if ((rc = check_buffer(ctx, x.buf, x.bytes, x.name))) return rc;
        if (off_boundary(x.buf->ptr, x.boundary)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, std::string("compact: ") + x.name + " is off its element's boundary");
        if (overlap(x.buf->ptr, x.bytes, flags->ptr, flag_bytes) || overlap(x.buf->ptr, x.bytes, scratch->ptr, l.bytes))
            return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, std::string("compact: ") + x.name + " may not overlap flags or scratch");
        for (const Out &y : outs)
            if (&y != &x && y.buf && y.bytes != 0u && overlap(x.buf->ptr, x.bytes, y.buf->ptr, y.bytes))
                return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "compact: outputs may not overlap each other");
    }
    for (const Out &x : ins) {
        const bool wanted = &x == &ins[0] ? (o.gather_out && R != 0u) : &x == &ins[1] ? o.scatter_out != nullptr : (o.scatter_out && R != 0u);
        if (!wanted) continue;
        if ((rc = check_buffer(ctx, x.buf, x.bytes, x.name))) return rc;
        if (off_boundary(x.buf->ptr, x.boundary)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, std::string("compact: ") + x.name + " is off its element's boundary");
        for (const Out &y : outs)
            if (y.buf && y.bytes != 0u && overlap(x.buf->ptr, x.bytes, y.buf->ptr, y.bytes))
                return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, std::string("compact: ") + x.name + " may not overlap an output");
    }
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    vrs::CompactEmitArgs a{};
    a.flags = flags->ptr;
    a.n = n;
    a.T = ctx->tune.compact_tile_elems;
    a.dtype = dtype;
    a.scratch = static_cast<const char *>(scratch->ptr);
    a.limit = R;
    if (R != 0u) {
        a.flat = o.flat ? static_cast<int64_t *>(o.flat->ptr) : nullptr;
        a.coords = o.coords ? static_cast<int64_t *>(o.coords->ptr) : nullptr;
        a.coords_layout = o.coords_layout;
        if (o.coords) a.shape = vrs::compact_shape_make(o.ndim, o.shape);
        a.gather_values = o.gather_out ? o.gather_values->ptr : nullptr;
        a.gather_out = o.gather_out ? o.gather_out->ptr : nullptr;
    }
    a.value_bytes = o.value_bytes;
    vrs::CompactRowForm rows{};
    rows.row_elems = o.row_elems;
    if (const char *v = std::getenv("VRS_COMPACT_ROW_SLICE_BYTES")) rows.slice_bytes = std::strtoull(v, nullptr, 10);  // (the timing tool's sweep)
    if (o.scatter_out) {
        a.scatter_input = o.scatter_input->ptr;
        a.scatter_source = R != 0u ? o.scatter_source->ptr : nullptr;
        a.scatter_out = o.scatter_out->ptr;
    }
    VRS_HIP(ctx, vrs::launch_compact_emit(ctx->stream, a, rows));
    ++ctx->compact_calls[1];
    return VRS_OK;
}

}  // extern "C"
