// search_member_host.cpp -- the membership decision of the sorted search (csrc/vrs_search.hpp: search_member and search_rank_is_nan,
// the code every query mode and the table kernel run behind their left count) on the host, against IEEE == / integer == over the
// decoded values: what numpy.isin and torch.isin answer.  The boundaries' ranks are a heap array of exact size and boundary `count` is
// fetched under the kernel's guard only, so with -fsanitize=address,undefined a fetch of boundary m is reported.
// Exit status 0: every case equal; otherwise the first differences are printed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vrs_search.hpp"

namespace {

int failures = 0;

double half_value(uint64_t u) {  // IEEE binary16
    const int e = static_cast<int>((u >> 10) & 31u);
    const double f = static_cast<double>(u & 1023u), s = (u & 0x8000u) ? -1.0 : 1.0;
    if (e == 31) return f != 0.0 ? std::nan("") : s * INFINITY;
    return s * (e == 0 ? std::ldexp(f, -24) : std::ldexp(1024.0 + f, e - 25));
}
double bfloat_value(uint64_t u) {
    const uint32_t w = static_cast<uint32_t>(u) << 16;
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}
double float_value(uint64_t u) {
    const uint32_t w = static_cast<uint32_t>(u);
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}
double double_value(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

// One dtype: B-bit patterns, ranks of type R.  equal(a, b): the reference's ==.
template <typename R, int B, bool FLOAT, bool SIGNED, typename Equal>
void check(const char *name, const std::vector<uint64_t> &boundaries, const std::vector<uint64_t> &queries, uint64_t inf_bits, Equal equal) {
    const R inf = static_cast<R>(inf_bits);
    const uint32_t m = static_cast<uint32_t>(boundaries.size());
    std::vector<R> ranks(m);  // exact size: ranks[m] does not exist
    for (uint32_t i = 0; i < m; ++i) ranks[i] = vrs::sort_rank<R, B, FLOAT, SIGNED>(static_cast<R>(boundaries[i]), inf, false);
    std::sort(ranks.begin(), ranks.end());
    for (uint64_t q : queries) {
        const R v = vrs::sort_rank<R, B, FLOAT, SIGNED>(static_cast<R>(q), inf, false);
        const uint32_t c = static_cast<uint32_t>(std::lower_bound(ranks.begin(), ranks.end(), v) - ranks.begin());  // the left count
        // the kernel's guard; where boundary c does not exist the function is handed the query's own rank, which it must not believe
        const R e = c < m ? ranks[c] : v;
        const uint32_t got = vrs::search_member<R>(c, m, e, v, vrs::search_rank_is_nan<R, B, FLOAT>(v));
        uint32_t want = 0u;
        for (uint64_t b : boundaries) want |= equal(b, q) ? 1u : 0u;
        if (got != want && failures++ < 10)
            std::printf("%s: m=%u query 0x%llx: got %u, want %u (count %u)\n", name, m, static_cast<unsigned long long>(q), got, want, c);
    }
}

template <typename R, int B>
void floats(const char *name, uint64_t inf_bits, double (*value)(uint64_t)) {
    const uint64_t sign = 1ull << (B - 1), one = inf_bits / 2u & ~((inf_bits / 2u) >> 1);  // (some finite exponent pattern)
    // +-0, +-inf, NaNs of both signs and with payloads, subnormals, the largest finite, ordinary values with duplicates
    const std::vector<uint64_t> special = {0u, sign, inf_bits, inf_bits | sign, inf_bits + 1u, (inf_bits + 1u) | sign, inf_bits | (inf_bits >> 3) | 5u,
                                           sign | (sign - 1u), sign - 1u, 1u, sign | 1u, 2u, inf_bits - 1u, (inf_bits - 1u) | sign,
                                           one, one | sign, one + 1u, one + 1u, one + 7u, (one + 7u) | sign};
    auto equal = [value](uint64_t a, uint64_t b) { return value(a) == value(b); };  // IEEE: NaN equals nothing, -0.0 == +0.0
    std::mt19937_64 rng(B);
    std::vector<std::vector<uint64_t>> rows = {{}, {0u}, {sign}, {inf_bits + 1u}, {inf_bits + 1u, (inf_bits + 9u) | sign}, {one}, {one, one}, special,
                                               {1u, one, inf_bits - 1u}};  // (the last: queries below and above every boundary)
    for (int r = 0; r < 6; ++r) {
        std::vector<uint64_t> row(1 + rng() % 300);
        for (uint64_t &x : row) x = rng() % 5 == 0 ? special[rng() % special.size()] : (one + rng() % 40) | (rng() % 2 ? sign : 0u);
        rows.push_back(row);
    }
    for (const auto &row : rows) {
        std::vector<uint64_t> q = special;
        q.insert(q.end(), row.begin(), row.end());  // a query row identical to the boundaries
        for (int i = 0; i < 200; ++i) q.push_back((one + rng() % 48) | (rng() % 2 ? sign : 0u));
        check<R, B, true, false>(name, row, q, inf_bits, equal);
        check<R, B, true, false>(name, row, std::vector<uint64_t>(5, row.empty() ? one : row[0]), inf_bits, equal);  // all queries equal
    }
}

template <typename R, int B, bool SIGNED>
void integers(const char *name) {
    const uint64_t ones = B == 64 ? ~0ull : (1ull << B) - 1u, sign = 1ull << (B - 1);
    auto equal = [](uint64_t a, uint64_t b) { return a == b; };
    const std::vector<uint64_t> special = {0u, 1u, ones, sign, sign - 1u, sign + 1u, ones - 1u, 40u, 41u, 41u};  // (ones: the largest rank, no NaN)
    std::mt19937_64 rng(B + SIGNED);
    std::vector<std::vector<uint64_t>> rows = {{}, {0u}, {ones}, {sign}, {sign - 1u}, {7u, 7u, 7u}, special, {10u, 20u, 30u}};
    for (int r = 0; r < 6; ++r) {
        std::vector<uint64_t> row(1 + rng() % 300);
        for (uint64_t &x : row) x = rng() % 5 == 0 ? special[rng() % special.size()] : (rng() % 80 - 40) & ones;
        rows.push_back(row);
    }
    for (const auto &row : rows) {
        std::vector<uint64_t> q = special;
        q.insert(q.end(), row.begin(), row.end());
        for (int i = 0; i < 200; ++i) q.push_back((rng() % 100 - 50) & ones);
        check<R, B, false, SIGNED>(name, row, q, 0u, equal);
        check<R, B, false, SIGNED>(name, row, std::vector<uint64_t>(5, row.empty() ? 3u : row[0]), 0u, equal);
    }
}

}  // namespace

int main() {
    floats<uint32_t, 16>("float16", 0x7C00ull, half_value);
    floats<uint32_t, 16>("bfloat16", 0x7F80ull, bfloat_value);
    floats<uint32_t, 32>("float32", 0x7F800000ull, float_value);
    floats<uint64_t, 64>("float64", 0x7FF0000000000000ull, double_value);
    integers<uint32_t, 8, true>("int8");
    integers<uint32_t, 8, false>("uint8");
    integers<uint32_t, 16, true>("int16");
    integers<uint32_t, 32, true>("int32");
    integers<uint64_t, 64, true>("int64");
    if (failures) {
        std::printf("search_member_host: %d difference(s)\n", failures);
        return 1;
    }
    std::printf("search_member_host: ok\n");
    return 0;
}
