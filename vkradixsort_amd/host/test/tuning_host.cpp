// tuning_host.cpp -- the table of the tuning settings (csrc/vrs_tuning.hpp) on the host, key by key from -1 to 41: a default-constructed
// vrs::Tuning holds an accepted value for every row; every finite bound is accepted and its outer neighbour refused; the rows without a
// bound take INT_MIN and INT_MAX; the sets of VRS_TUNE_DIGIT_TABLE_GROUPS and VRS_TUNE_MSD_POOL_SUB_BITS; what a store leaves in the
// member.  The defaults, bounds and refusal messages below are literals copied from vrs_set_tuning's switch as it stood before the
// table, NOT from the table under test.  Prints one line per key -- key default min max multiple, `-` = none -- for
// tests/test_tuning_cpu.py to compare the Python copies with, then "tuning_host: ok".  Exit status 0: every check held.
#include <climits>
#include <cstdio>
#include <cstring>

#include "vrs_tuning.hpp"

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                 \
    do {                                                  \
        if (!(cond) && failures++ < 20) {                 \
            std::printf("%s:%d: ", __FILE__, __LINE__);   \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

constexpr int NONE = INT_MIN + 7;  // no default (the key stores into no member of Tuning) / no bound
struct Expected {
    int key, def, min, max, multiple;
    const char *message;  // nullptr: the key refuses nothing
};
const Expected kExpected[] = {
    {VRS_TUNE_XCD_REMAP, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_SCATTER_VARIANT, NONE, NONE, NONE, 1, nullptr},
    {VRS_TUNE_FUSED_PREFIX, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_RANK_MODE, NONE, 0, 2, 1, "rank mode must be 0 (auto), 1 (ballot) or 2 (atomic)"},
    {VRS_TUNE_ONE_CALL_MIN_KEYS, 1 << 13, 0, NONE, 1, "one-call threshold must be >= 0"},
    {VRS_TUNE_DEBUG_MISPLACE_STREAMS, 0, NONE, NONE, 1, nullptr},
    {VRS_TUNE_LOOKBACK_SPIN_BUDGET, 4096, 0, NONE, 1, "spin budget must be >= 0"},
    {VRS_TUNE_DEBUG_HOLD_TILE, -1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_DIGIT_TABLE_GROUPS, 0, 0, 32, 1, "digit table groups must be 0 (by size), 8, 16 or 32"},
    {VRS_TUNE_SINGLE_MAX_KEYS, 4096, 0, NONE, 1, "single-launch threshold must be >= 0"},
    {VRS_TUNE_FUSED_PLAN, 0, NONE, NONE, 1, nullptr},
    {VRS_TUNE_HYBRID, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_HYBRID_MIN_KEYS, 0, 0, NONE, 1, "hybrid threshold must be >= 0"},
    {VRS_TUNE_HYBRID_FAST_COUNT, 1, 0, 2, 1, "fast count mode must be 0, 1 or 2"},
    {VRS_TUNE_ASYNC_SORT, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_PLAN_WAIT_MS, 60000, 0, NONE, 1, "the plan wait limit must be >= 0 ms"},
    {VRS_TUNE_MSD_RESERVE, 1, 0, 2, 1, "MSD reservation must be 0 (never) or 1 / 2 (bare keys of the hybrid form)"},
    {VRS_TUNE_MSD_POOL, 1, 0, 2, 1, "the pool form must be 0 (never), 1 (adaptive) or 2 (always tried)"},
    {VRS_TUNE_MSD_POOL_MIN_KEYS, 1 << 22, 1 << 22, NONE, 1, "the pool form takes 2^22 keys or more"},
    {VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, NONE, NONE, 4095, 1, "the probe has 4096 blocks (a negative value probes again without a stray one)"},
    {VRS_TUNE_MSD_POOL_SUB_BITS, 0, 0, 8, 1, "the pool form's second pass sorts by 6, 7 or 8 bits (0 = by size)"},
    {VRS_TUNE_DEBUG_XCC_ROTATE, NONE, 0, 7, 1, "rotate the probed placement by 0 .. 7 places"},
    {VRS_TUNE_MSD_POOL_REUSE_LAYOUT, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_MSD_POOL_PAIRS, 1, NONE, NONE, 1, nullptr},
    {VRS_TUNE_MSD_POOL_TOP_BITS, 7, 6, 8, 1, "the pool form's first pass sorts by 6, 7 (the default) or 8 bits"},
    {VRS_TUNE_DEBUG_POOL_NO_MEMORY, NONE, 0, NONE, 1, "allocations left to fail: 0 or more"},
    {VRS_TUNE_MSD_POOL_PAIRS_PACKED, -1, -1, 1, 1, "the pairs' packed local sort: -1 (by size), 0 (never) or 1 (always)"},
    {VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, 1 << 20, 0, NONE, 1, "the segmented sorts' one-call threshold must be >= 0"},
    {VRS_TUNE_TOPK_GRID_MIN_KEYS, 1 << 17, 0, NONE, 1, "the top-k grid tier's threshold must be >= 0"},
    {VRS_TUNE_SEARCH_LDS_BYTES, 64 * 1024, 0, 160 * 1024, 1, "the search's LDS capacity must be 0 .. 163840 bytes"},
    {VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, 1 << 16, 0, NONE, 1, "the search's table threshold must be >= 0"},
    {VRS_TUNE_SEARCH_INDEX_MIN_QUERIES, 1 << 16, 0, NONE, 1, "the search's index threshold must be >= 0"},
    {VRS_TUNE_BINCOUNT_LDS_BYTES, 64 * 1024, 0, 160 * 1024, 1, "the counting kernels' LDS capacity must be 0 .. 163840 bytes"},
    {VRS_TUNE_SELECT_GRID_MIN_KEYS, 1 << 17, 0, NONE, 1, "the selection's grid tier threshold must be >= 0"},
    {VRS_TUNE_SELECT_COMPACT_DIVISOR, 16, 0, NONE, 1, "the selection's compaction divisor must be >= 0"},
    {VRS_TUNE_REDUCE_CHUNK_ROWS, 512, 64, 4096, 1, "the reduction's chunk must be 64 .. 4096 rows"},
    {VRS_TUNE_REDUCE_LANE_ROWS, 16, 0, 64, 1, "the reduction's lane map takes 0 .. 64 rows"},
    {VRS_TUNE_SCAN_TILE_ROWS, 2048, 256, 8192, 256, "the scan's tile must be a multiple of 256 in 256 .. 8192 rows"},
    {VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, 1 << 20, 0, NONE, 1, "the scan's single pass starts at 0 (never) or more rows"},
    {VRS_TUNE_SCAN_SPIN_BUDGET, 4096, 0, 1 << 20, 1, "the scan's spin budget must be 0 .. 1048576 polls"},
    {VRS_TUNE_COMPACT_TILE_ELEMS, 16384, 4096, 65536, 4096, "the compaction's tile must be a multiple of 4096 in 4096 .. 65536 elements"},
};
// the keys whose switch case had no check at all
const int kUnbounded[] = {VRS_TUNE_XCD_REMAP, VRS_TUNE_SCATTER_VARIANT, VRS_TUNE_FUSED_PREFIX, VRS_TUNE_DEBUG_MISPLACE_STREAMS, VRS_TUNE_FUSED_PLAN,
                          VRS_TUNE_DEBUG_HOLD_TILE, VRS_TUNE_ASYNC_SORT, VRS_TUNE_HYBRID, VRS_TUNE_MSD_POOL_PAIRS, VRS_TUNE_MSD_POOL_REUSE_LAYOUT};

const Expected *expected(int key) {
    for (const Expected &e : kExpected)
        if (e.key == key) return &e;
    return nullptr;
}

bool accepted(int key, int value) { return vrs::tuning_refusal(key, value) == nullptr; }
// refused, and with the message the switch gave
void expect_refused(const Expected &e, int value) {
    const char *got = vrs::tuning_refusal(e.key, value);
    EXPECT(got != nullptr, "key %d accepts %d", e.key, value);
    if (got) EXPECT(e.message && std::strcmp(got, e.message) == 0, "key %d, value %d: \"%s\"", e.key, value, got);
}

// the member a row stores into, as an int (NONE: the row has no member)
int member_value(const vrs::Tuning &t, const vrs::TuneRow &r) {
    if (r.flag) return t.*r.flag ? 1 : 0;
    if (r.u32) return static_cast<int>(t.*r.u32);
    if (r.i32) return t.*r.i32;
    return NONE;
}

void print_field(int v, int none) { v == none ? std::printf(" -") : std::printf(" %d", v); }

void check_key(int key) {
    const Expected *e = expected(key);
    const vrs::TuneRow *r = vrs::tuning_row(key);
    if (!e) {  // outside the enum
        EXPECT(r == nullptr, "key %d has a row", key);
        for (int v : {INT_MIN, -1, 0, 1, INT_MAX}) {
            const char *got = vrs::tuning_refusal(key, v);
            EXPECT(got && std::strcmp(got, "unknown tuning key") == 0, "key %d, value %d: %s", key, v, got ? got : "accepted");
        }
        return;
    }
    EXPECT(r != nullptr && r->key == key, "key %d has no row of its own", key);
    if (!r) return;
    const vrs::Tuning fresh;
    const int def = member_value(fresh, *r);
    std::printf("%d", key);
    print_field(def, NONE);
    print_field(r->min, INT_MIN);
    print_field(r->max, INT_MAX);
    std::printf(" %d\n", r->multiple);
    EXPECT(def == e->def, "key %d: default %d, not %d", key, def, e->def);
    EXPECT(r->min == (e->min == NONE ? INT_MIN : e->min) && r->max == (e->max == NONE ? INT_MAX : e->max) && r->multiple == e->multiple,
           "key %d: range %d .. %d by %d", key, r->min, r->max, r->multiple);
    if (def != NONE) EXPECT(accepted(key, def), "key %d refuses its default %d", key, def);
    if (e->min != NONE) {
        EXPECT(accepted(key, e->min), "key %d refuses its minimum", key);
        expect_refused(*e, e->min - 1);
        expect_refused(*e, INT_MIN);
    } else {
        EXPECT(accepted(key, INT_MIN), "key %d refuses INT_MIN", key);
    }
    if (e->max != NONE) {
        EXPECT(accepted(key, e->max), "key %d refuses its maximum", key);
        expect_refused(*e, e->max + 1);
        expect_refused(*e, INT_MAX);
    } else {
        EXPECT(accepted(key, INT_MAX), "key %d refuses INT_MAX", key);
    }
    if (e->multiple > 1) {
        expect_refused(*e, e->min + 1);
        expect_refused(*e, e->max - 1);
        EXPECT(accepted(key, e->min + e->multiple), "key %d refuses the second multiple", key);
    }
    EXPECT((e->message == nullptr) == (r->refusal == nullptr), "key %d: a message without a check, or a check without one", key);
    // the store: what the switch's assignment left in the member
    if (def != NONE)
        for (int v : {e->min == NONE ? INT_MIN : e->min, e->max == NONE ? INT_MAX : e->max, def}) {
            vrs::Tuning t;
            vrs::tuning_store(t, key, v);
            const int want = r->flag || r->as_01 ? (v != 0 ? 1 : 0) : v;
            EXPECT(member_value(t, *r) == want, "key %d: %d stored as %d", key, v, member_value(t, *r));
        }
}

}  // namespace

int main() {
    EXPECT(vrs::kTuneKeys == 41 && sizeof(kExpected) / sizeof(kExpected[0]) == 41, "%d rows", vrs::kTuneKeys);
    for (int key = -1; key <= 41; ++key) check_key(key);
    for (int v = 0; v <= 33; ++v)
        EXPECT(accepted(VRS_TUNE_DIGIT_TABLE_GROUPS, v) == (v == 0 || v == 8 || v == 16 || v == 32), "digit table groups %d", v);
    for (int v = -1; v <= 9; ++v) EXPECT(accepted(VRS_TUNE_MSD_POOL_SUB_BITS, v) == (v == 0 || v == 6 || v == 7 || v == 8), "pool sub bits %d", v);
    expect_refused(*expected(VRS_TUNE_DIGIT_TABLE_GROUPS), 24);
    expect_refused(*expected(VRS_TUNE_MSD_POOL_SUB_BITS), 5);
    EXPECT(accepted(VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, -1) && accepted(VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, 4095) && !accepted(VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, 4096),
           "the stray block's range");
    for (int key : kUnbounded) EXPECT(accepted(key, INT_MIN) && accepted(key, INT_MAX) && accepted(key, 0), "key %d has a bound", key);
    {  // the one setting two members hold: the table's row stores the first, vrs_set_tuning's case the second
        const vrs::Tuning fresh;
        EXPECT(fresh.pool_reuse && fresh.pool_reuse_rooms, "the kept layout's defaults");
    }
    if (failures) {
        std::printf("tuning_host: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("tuning_host: ok\n");
    return 0;
}
