// topk_rank_host.cpp -- the rules of the torch-order top-k selection (vrs_topk_segments with VRS_TOPK_DTYPE(d)) on the host, for all nine
// dtypes: EVERY bit pattern of the 8- and 16-bit dtypes, and a few thousand chosen 32- and 64-bit patterns (both NaN signs, payloads,
// zeros, infinities, subnormals, extremes, neighbours of each, seeded random ones):
//   the order of the ranks (select_rank) is torch's comparator -- NaN the largest and all NaNs equal, -0.0 == +0.0, integers by value --
//     against a set of probes, and the complement (VRS_TOPK_LARGEST) reverses it;
//   the digits of select_level tile the significant bits exactly, from the top, at most 11 bits each;
//   sort_unrank reports inexact for exactly the two merged classes (zeros, NaNs) and gives every other pattern back;
//   a serial evaluation of "select, then emit in index order" (the kernels' rules: vrs_topk_order.hpp) over the patterns as one row equals
//     std::stable_sort by the rank cut at k, for k = 1, 2, L/2, L-1 and L, smallest and largest -- positions and own bits.
// Exit status 0: every case equal; otherwise the first differences are printed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "vrs_topk_order.hpp"

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                 \
    do {                                                  \
        if (!(cond) && failures++ < 10) {                 \
            std::printf("%s:%d: ", __FILE__, __LINE__);   \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

using vrs::kSortBF16;
using vrs::kSortF16;
using vrs::kSortF32;
using vrs::kSortF64;

uint64_t inf_bits_of(int dtype) {
    return dtype == kSortF16 ? 0x7C00u : dtype == kSortBF16 ? 0x7F80u : dtype == kSortF32 ? 0x7F800000u : 0x7FF0000000000000ull;
}

// the value of a float pattern as a double (exact for all four formats); NaN for a NaN
double float_value(uint64_t u, int dtype) {
    if (dtype == kSortF64) {
        double d;
        std::memcpy(&d, &u, 8);
        return d;
    }
    if (dtype == kSortF32 || dtype == kSortBF16) {
        const uint32_t w = dtype == kSortBF16 ? static_cast<uint32_t>(u) << 16 : static_cast<uint32_t>(u);
        float f;
        std::memcpy(&f, &w, 4);
        return f;
    }
    const int sign = static_cast<int>(u >> 15) & 1, exp = static_cast<int>(u >> 10) & 31, man = static_cast<int>(u & 1023u);
    double v = exp == 31 ? (man ? std::nan("") : INFINITY) : exp == 0 ? std::ldexp(man, -24) : std::ldexp(1024 + man, exp - 25);
    return sign ? -v : v;
}

// torch's comparator on two patterns of the dtype: -1, 0, 1
int torch_compare(uint64_t a, uint64_t b, int dtype, int bits) {
    if (vrs::sort_dtype_float(dtype)) {
        const double x = float_value(a, dtype), y = float_value(b, dtype);
        const bool nx = std::isnan(x), ny = std::isnan(y);
        if (nx || ny) return nx == ny ? 0 : nx ? 1 : -1;  // every NaN above everything else, NaNs equal
        return x < y ? -1 : x > y ? 1 : 0;                // (-0.0 == +0.0)
    }
    if (dtype == vrs::kSortU8) return a < b ? -1 : a > b ? 1 : 0;
    const int64_t x = static_cast<int64_t>(a << (64 - bits)) >> (64 - bits), y = static_cast<int64_t>(b << (64 - bits)) >> (64 - bits);
    return x < y ? -1 : x > y ? 1 : 0;
}

template <typename R, int B>
R rank_of(uint64_t u, int dtype, bool largest) {
    return vrs::select_rank<R, B>(static_cast<R>(u), vrs::select_kind(dtype), static_cast<R>(inf_bits_of(dtype)), largest);
}

template <int B>
std::vector<uint64_t> patterns(int dtype) {
    std::vector<uint64_t> p;
    if (B <= 16) {
        for (uint64_t u = 0; u < (1ull << B); ++u) p.push_back(u);
        return p;
    }
    const uint64_t ones = B == 64 ? ~0ull : (1ull << B) - 1u, sign = 1ull << (B - 1), inf = inf_bits_of(dtype);
    std::vector<uint64_t> seeds = {0, 1, 2, ones, ones - 1, sign, sign - 1, sign + 1, sign | 1u, ones >> 1, 0x55555555u, 0x1234567u};
    if (vrs::sort_dtype_float(dtype)) {
        const uint64_t quiet = inf | ((inf & (~inf + 1)) >> 1), one = dtype == kSortF32 ? 0x3F800000ull : 0x3FF0000000000000ull;
        const uint64_t sub = (inf & (~inf + 1)) - 1u;  // the largest subnormal
        for (uint64_t s : {uint64_t{0}, sign})
            for (uint64_t v : {inf, quiet, quiet | 1u, quiet | 0x2A5u, inf | 1u, inf | (quiet - inf - 1u), uint64_t{0}, uint64_t{1}, sub, sub + 1u, one, one + 1u, inf - 1u})
                seeds.push_back(s | v);
    }
    for (uint64_t s : seeds)
        for (int d = -2; d <= 2; ++d) p.push_back((s + static_cast<uint64_t>(d)) & ones);
    std::mt19937_64 rng(static_cast<uint64_t>(dtype) * 7919u + 11u);
    for (int i = 0; i < 3000; ++i) p.push_back(rng() & ones);
    for (int i = 0; i < 400; ++i) p.push_back(p[rng() % p.size()]);  // ties
    for (int i = 0; i < 300; ++i) p.push_back((rng() & 0xFFu) | (p[0] & ~0xFFull));  // agree in every digit but the lowest
    return p;
}

template <typename R, int B>
void check_order(int dtype, const std::vector<uint64_t> &pats) {
    std::vector<uint64_t> probes;
    std::mt19937_64 rng(static_cast<uint64_t>(dtype) + 5u);
    const size_t step = std::max<size_t>(pats.size() / 150u, 1u);
    for (size_t i = 0; i < pats.size(); i += step) probes.push_back(pats[i]);
    for (int i = 0; i < 60; ++i) probes.push_back(pats[rng() % pats.size()]);
    const uint64_t inf = inf_bits_of(dtype), sign = 1ull << (B - 1);
    if (vrs::sort_dtype_float(dtype))
        for (uint64_t v : {uint64_t{0}, sign, inf, sign | inf, inf + 1u, (sign | inf) + 1u, uint64_t{1}, sign | 1u, inf - 1u}) probes.push_back(v);
    constexpr R ones = static_cast<R>(static_cast<R>(1) << (B - 1)) | static_cast<R>((static_cast<R>(1) << (B - 1)) - 1);
    for (uint64_t a : pats) {
        const R ra = rank_of<R, B>(a, dtype, false), da = rank_of<R, B>(a, dtype, true);
        EXPECT(ra <= ones && da == static_cast<R>(~ra & ones), "dtype %d pattern %llx: the complement is not the descending rank", dtype,
               static_cast<unsigned long long>(a));
        for (uint64_t b : probes) {
            const R rb = rank_of<R, B>(b, dtype, false), db = rank_of<R, B>(b, dtype, true);
            const int want = torch_compare(a, b, dtype, B), got = ra < rb ? -1 : ra > rb ? 1 : 0, rev = da < db ? -1 : da > db ? 1 : 0;
            EXPECT(got == want && rev == -want, "dtype %d: %llx against %llx ranks %d (descending %d), torch compares %d", dtype,
                   static_cast<unsigned long long>(a), static_cast<unsigned long long>(b), got, rev, want);
        }
    }
}

void check_levels(int bits) {
    const int levels = vrs::select_levels(bits);
    int top = bits;
    for (int level = 0; level < levels; ++level) {
        uint32_t shift, mask;
        vrs::select_level(bits, level, &shift, &mask);
        int width = 0;
        while ((mask >> width) & 1u) ++width;
        EXPECT(mask == (1u << width) - 1u && width >= 1 && width <= 11, "%d bits, level %d: mask %x", bits, level, mask);
        EXPECT(static_cast<int>(shift) + width == top, "%d bits, level %d: digit [%u, %u) does not end where the one above begins (%d)", bits, level, shift,
               shift + width, top);
        top = static_cast<int>(shift);
    }
    EXPECT(top == 0, "%d bits: the levels leave the low %d bits unread", bits, top);
}

template <typename R, int B, bool FLOAT, bool SIGNED>
void check_unrank(int dtype, const std::vector<uint64_t> &pats) {
    const R inf = static_cast<R>(inf_bits_of(dtype));
    for (uint64_t a : pats)
        for (bool descending : {false, true}) {
            const R r = vrs::sort_rank<R, B, FLOAT, SIGNED>(static_cast<R>(a), inf, descending);
            bool exact = false;
            const R back = vrs::sort_unrank<R, B, FLOAT, SIGNED>(r, descending, &exact);
            const double v = FLOAT ? float_value(a, dtype) : 1.0;
            const bool merged = FLOAT && (std::isnan(v) || v == 0.0);
            EXPECT(exact == !merged, "dtype %d pattern %llx: exact = %d", dtype, static_cast<unsigned long long>(a), static_cast<int>(exact));
            EXPECT(!exact || back == static_cast<R>(a), "dtype %d pattern %llx comes back as %llx", dtype, static_cast<unsigned long long>(a),
                   static_cast<unsigned long long>(back));
        }
}

// the kernels' selection, serially: per level the digit histogram of the matching keys and the digit that holds the need-th; then the
// emission in index order, each element's own bits fetched at its position
template <typename R, int B>
void select_and_emit(const std::vector<uint64_t> &row, int dtype, bool largest, uint32_t k, std::vector<uint64_t> &out_bits,
                     std::vector<uint32_t> &out_pos) {
    const uint32_t len = static_cast<uint32_t>(row.size()), m = std::min(k, len);
    vrs::TopkSel<R> sel = vrs::topk_sel_init<R>(len, m);
    for (int level = 0; level < vrs::select_levels(B) && !sel.done; ++level) {
        uint32_t shift, mask;
        vrs::select_level(B, level, &shift, &mask);
        std::vector<uint32_t> hist(vrs::kTopkBins, 0u);
        for (uint64_t u : row) {
            const R r = rank_of<R, B>(u, dtype, largest);
            if (vrs::sel_match(r, sel)) ++hist[static_cast<uint32_t>(r >> shift) & mask];
        }
        uint32_t d = 0, below = 0;
        while (below + hist[d] < sel.need) below += hist[d++];
        vrs::sel_apply(sel, B, level, d, below, hist[d]);
    }
    out_bits.assign(m, 0u);
    out_pos.assign(m, 0xFFFFFFFFu);
    uint32_t lt = 0, eq = 0;
    for (uint32_t p = 0; p < len; ++p) {
        const R r = rank_of<R, B>(row[p], dtype, largest);
        uint32_t slot = 0xFFFFFFFFu;
        if (vrs::sel_less(r, sel)) slot = lt++;
        else if (vrs::sel_match(r, sel) && eq < sel.need) slot = sel.lt + eq++;
        if (slot != 0xFFFFFFFFu) {
            EXPECT(slot < m && out_pos[slot] == 0xFFFFFFFFu, "dtype %d: slot %u of %u written twice or out of range", dtype, slot, m);
            if (slot < m) {
                out_bits[slot] = row[p];
                out_pos[slot] = p;
            }
        }
    }
    EXPECT(lt == sel.lt && sel.lt + eq == m, "dtype %d: %u below and %u equal for m = %u (lt %u)", dtype, lt, eq, m, sel.lt);
}

template <typename R, int B>
void check_selection(int dtype, std::vector<uint64_t> row) {
    std::mt19937_64 rng(static_cast<uint64_t>(dtype) + 99u);
    std::shuffle(row.begin(), row.end(), rng);
    const uint32_t len = static_cast<uint32_t>(row.size());
    for (bool largest : {false, true}) {
        std::vector<uint32_t> order(len);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t b) { return rank_of<R, B>(row[a], dtype, largest) < rank_of<R, B>(row[b], dtype, largest); });
        for (uint32_t k : {1u, 2u, len / 2u, len - 1u, len}) {
            std::vector<uint64_t> bits;
            std::vector<uint32_t> pos;
            select_and_emit<R, B>(row, dtype, largest, k, bits, pos);
            // the emission is in index order; the survivors' stable sort by rank is the stable order
            std::vector<uint32_t> by_rank(pos.size());
            std::iota(by_rank.begin(), by_rank.end(), 0u);
            std::stable_sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) {
                return rank_of<R, B>(bits[a], dtype, largest) < rank_of<R, B>(bits[b], dtype, largest);
            });
            bool same = pos.size() == std::min(k, len);
            for (size_t j = 0; same && j < by_rank.size(); ++j) same = pos[by_rank[j]] == order[j] && bits[by_rank[j]] == row[order[j]];
            EXPECT(same, "dtype %d largest %d k %u of %u: the selection differs from the stable sort cut at k", dtype, static_cast<int>(largest), k, len);
        }
    }
}

template <typename R, int B, bool FLOAT, bool SIGNED>
void check_dtype(int dtype) {
    const std::vector<uint64_t> pats = patterns<B>(dtype);
    check_order<R, B>(dtype, pats);
    check_unrank<R, B, FLOAT, SIGNED>(dtype, pats);
    check_selection<R, B>(dtype, pats);
}

}  // namespace

int main() {
    for (int bits : {8, 16, 32, 64}) check_levels(bits);
    check_dtype<uint32_t, 8, false, true>(vrs::kSortI8);
    check_dtype<uint32_t, 8, false, false>(vrs::kSortU8);
    check_dtype<uint32_t, 16, false, true>(vrs::kSortI16);
    check_dtype<uint32_t, 32, false, true>(vrs::kSortI32);
    check_dtype<uint64_t, 64, false, true>(vrs::kSortI64);
    check_dtype<uint32_t, 16, true, false>(vrs::kSortF16);
    check_dtype<uint32_t, 16, true, false>(vrs::kSortBF16);
    check_dtype<uint32_t, 32, true, false>(vrs::kSortF32);
    check_dtype<uint64_t, 64, true, false>(vrs::kSortF64);
    if (failures) {
        std::printf("topk_rank_host: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("topk_rank_host: ok\n");
    return 0;
}
