// sort_mode_host.cpp -- the rules of the mode form of vrs_sort_restore (csrc/vrs_sort_mode_order.hpp: the head rule, the word and its
// maximum, the tile that owns a run, the search for the end of a tile's last run, the tile and row arithmetic) on the host, against a
// brute-force count of every row.  The ranks are heap arrays of exact size, so with -fsanitize=address,undefined a read past a row's
// data is reported; the arithmetic near 2^32 runs on ranks given by a rule, without the data.
// Exit status 0: every case equal; otherwise the first differences are printed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "vrs_sort_mode_order.hpp"

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

using u64 = unsigned long long;

// every tile's runs merged per row by mode_better, as the kernel's atomicMax merges them; `runs`: how many words were emitted
template <typename R, typename At>
std::vector<uint64_t> reduce_all_tiles(At at, uint64_t n, uint32_t row_len, uint64_t *runs) {
    std::vector<uint64_t> scratch(n / row_len, 0u);
    *runs = 0u;
    for (uint32_t tile = 0; tile < vrs::mode_tiles(n); ++tile)
        vrs::mode_tile_host<R>(at, n, row_len, tile, [&](uint32_t row, uint64_t word) {
            ++*runs;
            scratch[row] = vrs::mode_better(scratch[row], word);
        });
    return scratch;
}

// rows x row_len sorted ranks against the brute force: per row, the count of every value; the largest count, the smallest value of it
template <typename R>
void check_rows(const char *name, const std::vector<R> &ranks, uint32_t row_len) {
    const uint64_t n = ranks.size();
    const R *data = ranks.data();  // exact size: data[n] does not exist
    uint64_t runs = 0u;
    const std::vector<uint64_t> got = reduce_all_tiles<R>([data](uint64_t i) { return data[i]; }, n, row_len, &runs);
    uint64_t want_runs = 0u;
    for (uint64_t row = 0; row < n / row_len; ++row) {
        std::map<R, uint32_t> counts, first;
        for (uint32_t k = 0; k < row_len; ++k) {
            const R v = data[row * row_len + k];
            if (!counts.count(v)) first[v] = k;
            ++counts[v];
        }
        want_runs += counts.size();
        R best = counts.begin()->first;
        for (const auto &c : counts)
            if (c.second > counts[best]) best = c.first;  // (ascending: the first of the largest is the smallest)
        const uint64_t want = vrs::mode_pack(counts[best], first[best]);
        EXPECT(got[row] == want, "%s: row_len %u row %llu: count %u start %u, want count %u start %u", name, row_len, static_cast<u64>(row),
               vrs::mode_word_count(got[row]), vrs::mode_word_start(got[row]), counts[best], first[best]);
    }
    EXPECT(runs == want_runs, "%s: row_len %u: %llu runs emitted, %llu exist (a run has one owner)", name, row_len, static_cast<u64>(runs),
           static_cast<u64>(want_runs));
}

template <typename R>
void data_cases(const char *name, R spread) {
    std::mt19937_64 rng(sizeof(R));
    for (uint32_t row_len : {1u, 2u, 4095u, 4096u, 4097u, 12289u}) {
        const uint32_t rows = row_len <= 2u ? 9001u : 3u;  // (more than two tiles of short rows)
        const uint64_t n = static_cast<uint64_t>(rows) * row_len;
        for (uint32_t alphabet : {1u, 2u, 3u, 40u, 100000u}) {
            // sorted rows whose ends and beginnings are equal values that touch: every row's smallest value is the largest of the row
            // before it (alphabet 1: all values are one)
            std::vector<R> ranks(n);
            R floor = 0;
            for (uint32_t row = 0; row < rows; ++row) {
                R *r = ranks.data() + static_cast<uint64_t>(row) * row_len;
                for (uint32_t k = 0; k < row_len; ++k) r[k] = floor + static_cast<R>(rng() % alphabet) * spread;
                if (rng() % 4u != 0u) r[0] = floor;
                std::sort(r, r + row_len);
                floor = row % 64u == 63u ? 0 : r[row_len - 1u];
            }
            check_rows<R>(name, ranks, row_len);
        }
        // runs against the tile boundary: one long run that ends at, just before and just behind multiples of the tile, ties included
        for (int shift : {-6, -1, 0, 1, 6}) {
            std::vector<R> ranks(n);
            for (uint32_t row = 0; row < rows; ++row)
                for (uint32_t k = 0; k < row_len; ++k) {
                    const uint64_t i = static_cast<uint64_t>(row) * row_len + k;
                    ranks[i] = static_cast<R>((i + static_cast<uint64_t>(vrs::kModeTile) + shift) / 1365u) * spread;  // (three runs per tile)
                }
            for (uint32_t row = 0; row < rows; ++row) std::sort(ranks.begin() + static_cast<uint64_t>(row) * row_len, ranks.begin() + static_cast<uint64_t>(row + 1u) * row_len);
            check_rows<R>(name, ranks, row_len);
        }
    }
}

void rules() {
    // the head rule
    EXPECT(vrs::mode_is_head<uint32_t>(0u, 5u, 5u), "a row's first element is a head whatever precedes it");
    EXPECT(!vrs::mode_is_head<uint32_t>(1u, 5u, 5u) && vrs::mode_is_head<uint32_t>(1u, 6u, 5u), "inside a row a head differs from its predecessor");
    EXPECT(vrs::mode_is_head<uint64_t>(7u, 1ull << 40, 1ull << 41) && !vrs::mode_is_head<uint64_t>(7u, 1ull << 40, 1ull << 40), "64-bit ranks");
    // pack and unpack
    for (uint32_t count : {1u, 2u, 4096u, 0x80000000u, 0xFFFFFFFFu})
        for (uint32_t start : {0u, 1u, 4095u, 0x7FFFFFFFu, 0xFFFFFFFEu}) {
            const uint64_t w = vrs::mode_pack(count, start);
            EXPECT(w != 0u && vrs::mode_word_count(w) == count && vrs::mode_word_start(w) == start, "pack(%u, %u) does not unpack", count, start);
        }
    // the better of two: the longer; of equally long ones the one that starts first; a cleared word never
    EXPECT(vrs::mode_better(vrs::mode_pack(3u, 100u), vrs::mode_pack(2u, 0u)) == vrs::mode_pack(3u, 100u), "the longer run wins");
    EXPECT(vrs::mode_better(vrs::mode_pack(3u, 100u), vrs::mode_pack(3u, 7u)) == vrs::mode_pack(3u, 7u), "a tie: the earlier start wins");
    EXPECT(vrs::mode_better(vrs::mode_pack(3u, 7u), vrs::mode_pack(3u, 100u)) == vrs::mode_pack(3u, 7u), "in either order");
    EXPECT(vrs::mode_better(0u, vrs::mode_pack(1u, 0xFFFFFFFEu)) != 0u, "a cleared word never wins");
    // the rows a tile can touch
    for (uint32_t row_len = 1u; row_len <= 13000u; ++row_len) {
        uint32_t most = 0u;
        for (uint32_t tile = 0; tile < 64u; ++tile) {
            const uint64_t b = vrs::mode_tile_base(tile);
            most = std::max<uint32_t>(most, static_cast<uint32_t>((b + vrs::kModeTile - 1u) / row_len - b / row_len + 1u));
        }
        EXPECT(most <= vrs::mode_tile_rows_max(row_len) && vrs::mode_tile_rows_max(row_len) <= vrs::kModeTile, "row_len %u: a tile touches %u rows, the table holds %u",
               row_len, most, vrs::mode_tile_rows_max(row_len));
    }
    // the end of a tile's last run: a heap array of exact size, the run's tail behind the tile 0, 1, 2, ... and up to the row's end
    for (uint32_t rest : {0u, 1u, 2u, 3u, 4u, 7u, 8u, 9u, 1000u, 4096u, 100001u}) {
        std::vector<uint32_t> tails = {rest / 2u, rest - std::min(rest, 1u), rest};
        for (uint32_t t = 0u; t <= std::min(rest, 70u); ++t) tails.push_back(t);
        for (uint32_t tail : tails) {
            std::vector<uint32_t> row(4096u + rest, 9u);
            std::fill(row.begin(), row.begin() + 4096 + tail, 5u);
            const uint32_t *data = row.data();
            uint32_t reads = 0u;
            const uint64_t end = vrs::mode_last_run_end<uint32_t>([&](uint64_t i) { ++reads; return data[i]; }, 4096u, row.size(), 5u);
            EXPECT(end == 4096u + tail && reads <= 64u, "a run that goes %u of %u behind its tile ends at %llu after %u reads", tail, rest, static_cast<u64>(end), reads);
        }
    }
    uint32_t reads = 0u;
    EXPECT(vrs::mode_last_run_end<uint32_t>([&](uint64_t) { ++reads; return 1u; }, 8192u, 8000u, 1u) == 8000u && reads == 0u, "a row that ends in its tile is not read");
}

// n = 2^32 - 1 without the data: tiles, rows and the division by a constant; where row_len divides n, whole tiles by a rule
void near_two_to_32() {
    const uint64_t n = 0xFFFFFFFFull;
    EXPECT(vrs::mode_tiles(n) == (1u << 20), "2^32 - 1 elements are 2^20 tiles");
    const uint32_t last = vrs::mode_tiles(n) - 1u;
    EXPECT(vrs::mode_tile_base(last) == 0xFFFFF000ull && vrs::mode_tile_end(last, n) == n && vrs::mode_tile_end(last - 1u, n) == 0xFFFFF000ull, "the last tile");
    std::mt19937_64 rng(32);
    for (uint32_t row_len : {1u, 3u, 0x80000000u, 0xFFFFFFFFu}) {
        const vrs::CompactDiv div = vrs::compact_div_make(row_len);
        std::vector<uint64_t> at = {0u, 1u, 2u, 3u, row_len - 1ull, row_len, row_len + 1ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFEFFFull, 0xFFFFF000ull, n - 2u, n - 1u};
        for (int k = 0; k < 2000; ++k) at.push_back(rng() % n);
        for (uint64_t i : at) {
            if (i >= n) continue;
            const uint32_t row = vrs::compact_div(static_cast<uint32_t>(i), div);
            EXPECT(row == i / row_len, "row of %llu at row_len %u: %u", static_cast<u64>(i), row_len, row);
            EXPECT(vrs::mode_row_begin(row, row_len) <= i && i < vrs::mode_row_end(row, row_len) && vrs::mode_row_end(row, row_len) - vrs::mode_row_begin(row, row_len) == row_len,
                   "the bounds of row %u at row_len %u", row, row_len);
        }
        if (n % row_len != 0u) continue;  // (2^31: the arithmetic alone; the call refuses rows that are not whole)
        // ranks by a rule: place-in-row >> 20, so runs of 2^20 (256 tiles) that rows of 1 and 3 never reach; every row the same ranks
        auto rank_at = [row_len](uint64_t i) { return static_cast<uint32_t>((i % row_len) >> 20); };
        for (uint32_t tile : {0u, 1u, 255u, 256u, 257u, (1u << 19), last - 256u, last - 255u, last - 1u, last}) {
            uint64_t emitted = 0u;
            vrs::mode_tile_host<uint32_t>(rank_at, n, row_len, tile, [&](uint32_t row, uint64_t word) {
                ++emitted;
                const uint64_t begin = vrs::mode_row_begin(row, row_len), head = begin + vrs::mode_word_start(word);
                const uint64_t stop = std::min<uint64_t>(vrs::mode_row_end(row, row_len), begin + ((((head - begin) >> 20) + 1u) << 20));
                EXPECT(head >= vrs::mode_tile_base(tile) && head < vrs::mode_tile_end(tile, n), "tile %u emits a run whose head is not its own", tile);
                EXPECT(((head - begin) & 0xFFFFFu) == 0u && vrs::mode_word_count(word) == stop - head, "row_len %u tile %u: run at %llu of %u, want %llu", row_len,
                       tile, static_cast<u64>(head), vrs::mode_word_count(word), static_cast<u64>(stop - head));
            });
            uint64_t want = 0u;  // the heads in the tile
            for (uint64_t i = vrs::mode_tile_base(tile); i < vrs::mode_tile_end(tile, n); ++i) want += (i % row_len) % (1u << 20) == 0u ? 1u : 0u;
            EXPECT(emitted == want, "row_len %u tile %u: %llu runs emitted, %llu heads", row_len, tile, static_cast<u64>(emitted), static_cast<u64>(want));
        }
    }
}

}  // namespace

int main() {
    rules();
    data_cases<uint32_t>("uint32 ranks", 1u);
    data_cases<uint64_t>("uint64 ranks", 1ull << 33);  // (values that differ only above bit 32)
    near_two_to_32();
    if (failures) {
        std::printf("sort_mode_host: %d difference(s)\n", failures);
        return 1;
    }
    std::printf("sort_mode_host: ok\n");
    return 0;
}
