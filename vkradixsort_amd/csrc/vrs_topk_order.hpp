// vrs_topk_order.hpp -- the rules of the top-k selection that its kernels (vrs_topk.hip) and the host program that checks them
// (host/test/topk_rank_host.cpp) share: which keys a selection state takes, and how a level's chosen digit advances it.  The rank map
// and the levels' digits are the one-rank selection's (vrs_select.hpp: select_rank, select_level).  Internal.
#pragma once
#include "vrs_select.hpp"

namespace vrs {

// r is below the selection's prefix in the bits fixed so far: taken whatever its index
template <typename R>
__host__ __device__ inline bool sel_less(R r, const TopkSel<R> &s) {
    return s.shift != kTopkNoShift && (r >> s.shift) < (s.prefix >> s.shift);
}
// r equals the prefix in the bits fixed so far: of these the first `need` in index order are taken
template <typename R>
__host__ __device__ inline bool sel_match(R r, const TopkSel<R> &s) {
    return s.shift == kTopkNoShift || (r >> s.shift) == (s.prefix >> s.shift);
}

// Level `level` of a rank of `bits` significant bits has counted the digits of the matching keys: d holds the need-th of them, `below`
// keys lie in smaller digits, `at` in d.  Done once every key at d is needed, or after the last level.
template <typename R>
__host__ __device__ inline void sel_apply(TopkSel<R> &sel, int bits, int level, uint32_t d, uint32_t below, uint32_t at) {
    uint32_t shift, mask;
    select_level(bits, level, &shift, &mask);
    sel.lt += below;
    sel.need -= below;
    sel.shift = shift;
    sel.prefix |= static_cast<R>(d) << shift;
    sel.done = (at == sel.need || level == select_levels(bits) - 1) ? 1u : 0u;
}

}  // namespace vrs
