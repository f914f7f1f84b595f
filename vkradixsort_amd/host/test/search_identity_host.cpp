// search_identity_host.cpp -- the chunk function of the identity search (csrc/vrs_search.hpp: search_identity_chunk, the code the merge
// kernel runs per workgroup) on the host, as a team of one, against a naive count per output.  Built for the host with
// -fsanitize=address,undefined: the marks and the outputs are heap arrays of their exact sizes, so an index outside a chunk is reported.
// Exit status 0: every pattern equal; otherwise the first difference is printed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "vrs_search.hpp"

namespace {

int failures = 0;

template <typename S>
uint32_t count_below(const std::vector<S> &b, int64_t v, int right) {
    uint32_t c = 0;
    for (S x : b) c += (static_cast<int64_t>(x) < v) || (right && static_cast<int64_t>(x) == v);
    return c;
}

// every chunk of Q outputs over ascending boundaries b, both sides
template <typename S>
void check(const char *name, const std::vector<S> &b, uint64_t q_len) {
    for (int right = 0; right < 2; ++right) {
        for (uint64_t j0 = 0; j0 < q_len; j0 += vrs::kSearchChunk) {
            const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(q_len - j0, vrs::kSearchChunk));
            const uint32_t a0 = count_below(b, static_cast<int64_t>(j0), right), a1 = count_below(b, static_cast<int64_t>(j0 + n - 1u), right);
            std::vector<uint32_t> marks(vrs::kSearchChunk, 0xDEADBEEFu), out(n, 0xDEADBEEFu);
            vrs::SearchIdentitySerial team;
            uint32_t *o = out.data();
            vrs::search_identity_chunk<S>(b.data(), a0, a1, j0, n, right, marks.data(), 0u, 1u, team,
                                          [o](uint32_t g, const uint32_t (&v)[vrs::kSearchItems], uint32_t k) {
                                              for (uint32_t i = 0; i < k; ++i) o[g + i] = v[i];
                                          });
            // the naive answers by one sweep: ascending boundaries
            size_t at = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const int64_t v = static_cast<int64_t>(j0 + k);
                while (at < b.size() && (static_cast<int64_t>(b[at]) < v || (right && static_cast<int64_t>(b[at]) == v))) ++at;
                if (out[k] != at) {
                    if (failures++ < 10)
                        std::printf("%s: right=%d output %llu: got %u, want %zu\n", name, right, static_cast<unsigned long long>(j0 + k), out[k], at);
                    break;
                }
            }
        }
    }
}

// boundaries in any order: every answer inside [0, m], nothing written outside the n outputs (the sanitizer's part)
template <typename S>
void check_unsorted(const std::vector<S> &b, uint64_t q_len, std::mt19937_64 &rng) {
    const uint32_t m = static_cast<uint32_t>(b.size());
    for (int right = 0; right < 2; ++right) {
        for (uint64_t j0 = 0; j0 < q_len; j0 += vrs::kSearchChunk) {
            const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(q_len - j0, vrs::kSearchChunk));
            const uint32_t a0 = static_cast<uint32_t>(rng() % (m + 1u)), a1 = static_cast<uint32_t>(rng() % (m + 1u));  // (any two ends)
            std::vector<uint32_t> marks(vrs::kSearchChunk), out(n, 0xDEADBEEFu);
            vrs::SearchIdentitySerial team;
            uint32_t *o = out.data();
            vrs::search_identity_chunk<S>(b.data(), a0, a1, j0, n, right, marks.data(), 0u, 1u, team,
                                          [o](uint32_t g, const uint32_t (&v)[vrs::kSearchItems], uint32_t k) {
                                              for (uint32_t i = 0; i < k; ++i) o[g + i] = v[i];
                                          });
            for (uint32_t k = 0; k < n; ++k)
                if (out[k] > m || out[k] < a0 || out[k] > std::max(a0, a1)) {
                    if (failures++ < 10) std::printf("unsorted: output %u = %u outside [%u, %u]\n", k, out[k], a0, std::max(a0, a1));
                    break;
                }
        }
    }
}

template <typename S>
void patterns(const char *type) {
    constexpr int64_t C = vrs::kSearchChunk;
    char name[96];
    auto run = [&](const char *what, const std::vector<S> &b, uint64_t q) {
        std::snprintf(name, sizeof name, "%s %s m=%zu Q=%llu", type, what, b.size(), static_cast<unsigned long long>(q));
        check<S>(name, b, q);
    };
    for (size_t m : {size_t(1), size_t(2), size_t(63), size_t(64), size_t(65), size_t(4095), size_t(4096), size_t(4097), size_t(3 * 4096 + 5)})
        for (uint64_t q : {uint64_t(1), uint64_t(4095), uint64_t(4096), uint64_t(4097), uint64_t(8192), uint64_t(100003)}) {
            std::vector<S> steps(m), equal(m, static_cast<S>(5000)), negative(m);
            for (size_t i = 0; i < m; ++i) steps[i] = static_cast<S>(i + 1), negative[i] = static_cast<S>(static_cast<int64_t>(i) * 3 - 100);
            run("steps of 1", steps, q);
            run("all equal", equal, q);
            run("negative leading", negative, q);
        }
    run("one run across three chunks", std::vector<S>{static_cast<S>(100), static_cast<S>(100 + 3 * C)}, 5 * C);
    {
        std::vector<S> b(10000, static_cast<S>(C + 77));
        b.insert(b.begin(), static_cast<S>(3));
        b.push_back(static_cast<S>(2 * C + 1));
        run("10000 equal inside one chunk", b, 3 * C);
    }
    run("chunk edges", std::vector<S>{static_cast<S>(C - 1), static_cast<S>(C), static_cast<S>(C + 4095), static_cast<S>(C + 4096)}, 3 * C);
    run("Q below the last boundary", std::vector<S>{static_cast<S>(10), static_cast<S>(20), static_cast<S>(1000000)}, 5000);
    run("Q above the last boundary", std::vector<S>{static_cast<S>(10), static_cast<S>(20), static_cast<S>(30)}, 5000);
    run("the type's ends", std::vector<S>{std::numeric_limits<S>::min(), static_cast<S>(0), static_cast<S>(0), std::numeric_limits<S>::max()}, 4097);
    std::mt19937_64 rng(sizeof(S));
    for (int round = 0; round < 20; ++round) {
        std::vector<S> b(1 + rng() % 20000);
        for (S &x : b) x = static_cast<S>(static_cast<int64_t>(rng() % 30000) - 5000);
        if (round == 0) b[0] = std::numeric_limits<S>::min(), b.back() = std::numeric_limits<S>::max();
        check_unsorted<S>(b, 1 + rng() % 20000, rng);
    }
}

}  // namespace

int main() {
    patterns<int32_t>("int32");
    patterns<int64_t>("int64");
    if (failures) {
        std::printf("search_identity_host: %d difference(s)\n", failures);
        return 1;
    }
    std::printf("search_identity_host: ok\n");
    return 0;
}
