// unique_rows_host.cpp -- the rules of the row form of vrs_unique / vrs_run_length_encode (csrc/vrs_unique_rows_order.hpp: the plan, the
// pack, the head rule with its guarded fetch) on the host, on seeded small matrices of all six key types and C = 1 .. 9:
//   the LSD rounds (std::stable_sort of the packed keys, least significant group first) give the permutation of one std::stable_sort
//     with a lexicographic comparator on the ranks;
//   heads, run ids, starts and counts from the head rule -- over the sorted rows with the top group's keys, and over the rows as they
//     lie with their first 8 bytes -- equal those from memcmp of adjacent rows.
// The matrices are heap arrays of exact size, so with -fsanitize=address,undefined a read past a row is reported.
// Exit status 0: every case equal; otherwise the first differences are printed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "vrs_unique_rows_order.hpp"

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

template <typename W> std::vector<W> specials(int key_type);
template <> std::vector<uint32_t> specials<uint32_t>(int key_type) {
    if (key_type == vrs::kUniqueF32) return {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7FC00001u, 0xFFC00000u, 0x3F800000u, 0xBF800000u};
    return {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0xFFFFFFFEu};
}
template <> std::vector<uint64_t> specials<uint64_t>(int key_type) {
    if (key_type == vrs::kUniqueF64)
        return {0ull, 1ull << 63, 0x7FF0000000000000ull, 0xFFF0000000000000ull, 0x7FF8000000000000ull, 0x7FF8000000000001ull, 0xFFF8000000000000ull,
                0x3FF0000000000000ull};
    return {0ull, 1ull, 2ull, 0x7FFFFFFFFFFFFFFFull, 1ull << 63, ~0ull, 0x00000001FFFFFFFFull, 0xFFFFFFFF00000000ull};
}

struct Runs {
    std::vector<uint32_t> ids, starts, counts;
};
template <typename Head>
Runs runs_of(uint32_t n, Head head) {
    Runs r;
    for (uint32_t i = 0; i < n; ++i) {
        if (i == 0u || head(i)) {
            r.starts.push_back(i);
            r.counts.push_back(0u);
        }
        r.ids.push_back(static_cast<uint32_t>(r.starts.size()) - 1u);
        ++r.counts.back();
    }
    return r;
}
bool same(const Runs &a, const Runs &b) { return a.ids == b.ids && a.starts == b.starts && a.counts == b.counts; }

template <typename W>
void check(int key_type, uint32_t n, uint32_t cols, uint32_t alphabet, uint32_t seed) {
    const uint32_t word = sizeof(W);
    std::mt19937_64 rng(seed * 7919u + cols * 131u + n);
    std::vector<W> pool = specials<W>(key_type);
    while (pool.size() < alphabet) pool.push_back(static_cast<W>(rng()));
    pool.resize(alphabet);
    std::vector<W> m(static_cast<size_t>(n) * cols);  // exact size
    for (W &w : m) w = pool[rng() % alphabet];
    if (n > 3u)  // rows that differ only in the last and only in the first column
        for (uint32_t c = 0; c < cols; ++c) m[1u * cols + c] = m[2u * cols + c] = m[3u * cols + c] = m[c];
    if (n > 3u) m[2u * cols + cols - 1u] = pool[1 % alphabet], m[3u * cols] = pool[2 % alphabet];
    const W *x = m.data();

    // the reference: one stable sort with a lexicographic comparator on the ranks
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
        for (uint32_t c = 0; c < cols; ++c) {
            const W ra = vrs::unique_rank(x[static_cast<size_t>(a) * cols + c], key_type), rb = vrs::unique_rank(x[static_cast<size_t>(b) * cols + c], key_type);
            if (ra != rb) return ra < rb;
        }
        return false;
    });

    // the plan's rounds
    const uint32_t rounds = vrs::rows_rounds(cols, word);
    EXPECT(rounds == (cols * word + 7u) / 8u, "rounds");
    std::vector<uint32_t> pos(n);
    std::iota(pos.begin(), pos.end(), 0u);
    std::vector<uint64_t> keys(n);
    uint32_t covered = cols, top_count = 0;
    for (uint32_t g = 0; g < rounds; ++g) {
        const vrs::RowsGroup group = vrs::rows_group(cols, word, g);
        EXPECT(group.first + group.count == covered && group.count >= 1u && group.count * word <= 8u, "group %u of C=%u word=%u: [%u, +%u)", g, cols, word,
               group.first, group.count);
        EXPECT(group.count * word == 8u || (group.first == 0u && g == rounds - 1u), "a short group that is not column 0");
        covered = group.first;
        top_count = group.count;
        std::vector<std::pair<uint64_t, uint32_t>> kv(n);
        for (uint32_t i = 0; i < n; ++i) {
            const W *row = x + static_cast<size_t>(pos[i]) * cols;
            uint64_t k;
            if constexpr (sizeof(W) == 4) {
                if (group.count == 2u)
                    k = vrs::rows_pack2(row, group.first, key_type);
                else
                    k = vrs::rows_pack1(row, group.first, key_type);
            } else {
                k = vrs::rows_pack1(row, group.first, key_type);
            }
            kv[i] = {k, pos[i]};
        }
        std::stable_sort(kv.begin(), kv.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (uint32_t i = 0; i < n; ++i) keys[i] = kv[i].first, pos[i] = kv[i].second;
    }
    EXPECT(covered == 0u, "the groups do not reach column 0");
    EXPECT(pos == want, "type %d n=%u C=%u: the LSD rounds' permutation differs", key_type, n, cols);

    // the head rule over the sorted rows (top keys, the rest through pos) against memcmp of adjacent sorted rows
    const uint32_t *p = pos.data();
    const Runs sorted_rule = runs_of(n, [&](uint32_t i) { return vrs::rows_head<W, uint64_t>(keys[i], keys[i - 1u], x, cols, p, i, top_count, cols); });
    const Runs sorted_ref = runs_of(n, [&](uint32_t i) {
        return std::memcmp(x + static_cast<size_t>(p[i]) * cols, x + static_cast<size_t>(p[i - 1u]) * cols, static_cast<size_t>(cols) * word) != 0;
    });
    EXPECT(same(sorted_rule, sorted_ref), "type %d n=%u C=%u: the sorted head rule differs from memcmp", key_type, n, cols);

    // the encode: rows as they lie, the first 8 bytes as the top key (C >= 2 for 4-byte words)
    if (cols * word >= 8u) {
        const uint32_t c0 = 8u / word;
        const Runs rule = runs_of(n, [&](uint32_t i) {
            return vrs::rows_head<W, uint64_t>(vrs::rows_front(x, cols, i), vrs::rows_front(x, cols, i - 1u), x, cols, nullptr, i, c0, cols);
        });
        const Runs ref = runs_of(n, [&](uint32_t i) {
            return std::memcmp(x + static_cast<size_t>(i) * cols, x + static_cast<size_t>(i - 1u) * cols, static_cast<size_t>(cols) * word) != 0;
        });
        EXPECT(same(rule, ref), "type %d n=%u C=%u: the encode's head rule differs from memcmp", key_type, n, cols);
    }
}

}  // namespace

int main() {
    uint32_t cases = 0;
    for (int key_type = vrs::kUniqueU32; key_type <= vrs::kUniqueF64; ++key_type)
        for (uint32_t cols = 1; cols <= 9u; ++cols)
            for (uint32_t n : {1u, 2u, 5u, 64u, 257u})
                for (uint32_t alphabet : {1u, 2u, 3u, 12u}) {
                    if (vrs::unique_key_bytes(key_type) == 8)
                        check<uint64_t>(key_type, n, cols, alphabet, cases);
                    else
                        check<uint32_t>(key_type, n, cols, alphabet, cases);
                    ++cases;
                }
    // the encoded argument
    EXPECT(vrs::rows_columns((7 << 8) | vrs::kUniqueF64) == 7u && vrs::rows_low_byte((7 << 8) | vrs::kUniqueF64) == vrs::kUniqueF64, "decode");
    EXPECT(vrs::rows_columns(8) == 0u && vrs::rows_low_byte(8) == 8, "decode of a plain width");
    if (failures) {
        std::printf("unique_rows_host: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("unique_rows_host: ok (%u cases)\n", cases);
    return 0;
}
