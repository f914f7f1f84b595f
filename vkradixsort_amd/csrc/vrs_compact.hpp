// vrs_compact.hpp -- what the compaction's kernels (vrs_compact.hip) and their host side (vrs_capi_compact.hip) share: the scratch layout
// and the launchers' argument structs.  The rules themselves: vrs_compact_order.hpp.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "vrs_compact_order.hpp"

namespace vrs {

// scratch: [0, 8) the total R as uint64 (the rest of the header unused), then one uint32 per tile -- the tile's count after the count
// phase, its exclusive offset after the carries.  The same function sizes it (vrs_compact_scratch_bytes) and cuts it.
struct CompactLayout {
    uint32_t tiles;
    size_t words, bytes;  // byte offset of the tiles' words, bytes in all
};
inline CompactLayout compact_layout(uint64_t n, uint32_t T) {
    CompactLayout l{};
    l.tiles = compact_tiles(n, T);
    l.words = kCompactHeaderBytes;
    l.bytes = kCompactHeaderBytes + ((static_cast<size_t>(l.tiles) * sizeof(uint32_t) + 255u) & ~static_cast<size_t>(255u));
    return l;
}

struct CompactCountArgs {
    const void *flags;  // n elements of dtype
    uint64_t n;
    uint32_t T;
    int dtype;
    char *scratch;
    long long *out_count;  // NULL, or where R goes as int64 as well
};

struct CompactEmitArgs {
    const void *flags;
    uint64_t n;
    uint32_t T;
    int dtype;
    const char *scratch;  // as the count call left it
    uint64_t limit;       // R as the caller knows it: no output row from here on is written, no source element from here on read
    int64_t *flat;        // NULL or [R]
    int64_t *coords;      // NULL or [R, ndim] (kCompactRows) / [ndim, R] (kCompactColumns)
    int coords_layout;
    CompactShape shape;
    const void *gather_values;  // NULL or n elements of value_bytes
    void *gather_out;           // [R]
    uint32_t value_bytes;
    const void *scatter_input, *scatter_source;  // NULL or n elements / at least R elements of value_bytes
    void *scatter_out;                           // [n]
};

// The row form, beside CompactEmitArgs (which the element kernels take as it always was): row_elems of 0 or 1 leaves everything to them;
// W >= 2 makes gather_* and scatter_* rows of W elements, moved by the row kernels.  slice_bytes: 0 for kCompactRowSliceBytes, or what
// stands in for it (the timing tool's sweep).
struct CompactRowForm {
    uint32_t row_elems, pad;
    uint64_t slice_bytes;
};

hipError_t launch_compact_count(hipStream_t stream, const CompactCountArgs &a);
hipError_t launch_compact_emit(hipStream_t stream, const CompactEmitArgs &a, const CompactRowForm &rows);

}  // namespace vrs
