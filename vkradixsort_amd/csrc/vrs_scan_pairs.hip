// vrs_scan_pairs.hip -- the prefix scan's MAX and MIN: the kernels of vrs_scan_kernels.hpp over (value, row) pairs, for the nine dtypes of
// vrs_sort_dtype.  A file of its own so that the two halves of the family compile side by side.
#include "vrs_scan_kernels.hpp"

namespace vrs {

hipError_t launch_scan_pairs(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units) {
    switch (a.dtype) {
        case kSortI8: return launch_scan_as<ScanPairs<int8_t, 0>>(stream, a, l, compute_units);
        case kSortU8: return launch_scan_as<ScanPairs<uint8_t, 0>>(stream, a, l, compute_units);
        case kSortI16: return launch_scan_as<ScanPairs<int16_t, 0>>(stream, a, l, compute_units);
        case kSortI32: return launch_scan_as<ScanPairs<int32_t, 0>>(stream, a, l, compute_units);
        case kSortI64: return launch_scan_as<ScanPairs<int64_t, 0>>(stream, a, l, compute_units);
        case kSortF16: return launch_scan_as<ScanPairs<uint16_t, 1>>(stream, a, l, compute_units);
        case kSortBF16: return launch_scan_as<ScanPairs<uint16_t, 2>>(stream, a, l, compute_units);
        case kSortF32: return launch_scan_as<ScanPairs<float, 0>>(stream, a, l, compute_units);
        default: return launch_scan_as<ScanPairs<double, 0>>(stream, a, l, compute_units);
    }
}

}  // namespace vrs
