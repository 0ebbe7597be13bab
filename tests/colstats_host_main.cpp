// The host rules every column maker shares (sybil_amd/csrc/colstats.h: fit_storage, stats_fold, set_gather): built by
// tests/test_colstats_host.py with -fsanitize=address,undefined and run as a program of its own.  Every expectation is written
// out by hand or computed here with __int128 / a plain loop, never with the helper under test.  Prints one line per group of
// cases; exits 1 at the first value that differs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "colstats.h"

using namespace sybl;

static int g_failed = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                       \
            fprintf(stderr, "\n");                                              \
            g_failed = 1;                                                       \
            return;                                                             \
        }                                                                       \
    } while (0)

// ------------------------------------------------------------------ the storage rule

static void fit_is(int canon, bool any, int64_t lo, int64_t hi, int want_w, int64_t want_b, const char *what) {
    int w = -1;
    int64_t b = -1;
    fit_storage(canon, any, lo, hi, &w, &b);
    CHECK(w == want_w && b == want_b, "%s (canon %d): got (%d, %lld), expected (%d, %lld)", what, canon, w, (long long)b, want_w, (long long)want_b);
}

// the rule restated with 128-bit arithmetic: the bytes hi - lo needs
static int bytes_needed(int64_t lo, int64_t hi) {
    unsigned __int128 range = (unsigned __int128)((__int128)hi - (__int128)lo);
    int bytes = 1;
    while (bytes < 16 && (range >> (8 * bytes)) != 0) bytes++;
    return bytes <= 1 ? 1 : bytes <= 2 ? 2 : bytes <= 4 ? 4 : 8;  // (the range of two int64 needs at most 8 bytes)
}

static void storage_cases() {
    const int64_t two32 = (int64_t)1 << 32;
    struct {
        int64_t d;
        int w4, w8;  // the width at canonical width 4 / 8
    } const spans[] = {{0, 1, 1}, {255, 1, 1}, {256, 2, 2}, {65535, 2, 2}, {65536, 4, 4}, {two32 - 1, 4, 4}, {two32, 4, 8}};
    const int64_t los[] = {0, -7, 1000000007, INT64_MIN, INT64_MAX - two32};
    for (const auto &s : spans)
        for (int64_t lo : los) {
            const int64_t hi = (int64_t)((__int128)lo + s.d);
            // below the canonical width: offsets from lo; at it: base 0
            fit_is(4, true, lo, hi, s.w4, s.w4 < 4 ? lo : 0, "span, canonical 4");
            if (g_failed) return;
            fit_is(8, true, lo, hi, s.w8, s.w8 < 8 ? lo : 0, "span, canonical 8");
            if (g_failed) return;
            CHECK(bytes_needed(lo, hi) == s.w8, "the table of spans itself: %lld needs %d bytes", (long long)s.d, bytes_needed(lo, hi));
        }
    // a range that needs 128 bits to state
    fit_is(8, true, INT64_MIN, INT64_MAX, 8, 0, "the whole int64 range");
    if (g_failed) return;
    fit_is(4, true, INT64_MIN, INT64_MAX, 4, 0, "the whole int64 range");
    if (g_failed) return;
    fit_is(8, true, INT64_MIN, INT64_MIN, 1, INT64_MIN, "one value at INT64_MIN");
    if (g_failed) return;
    fit_is(4, true, INT64_MIN, INT64_MIN, 1, INT64_MIN, "one value at INT64_MIN");
    if (g_failed) return;
    fit_is(8, true, INT64_MAX, INT64_MAX, 1, INT64_MAX, "one value at INT64_MAX");
    if (g_failed) return;
    // nothing populated: (1, 0) whatever the extrema say
    for (int canon : {4, 8}) {
        fit_is(canon, false, 0, 0, 1, 0, "nothing populated");
        if (g_failed) return;
        fit_is(canon, false, INT64_MAX, INT64_MIN, 1, 0, "nothing populated, untouched extrema");
        if (g_failed) return;
        fit_is(canon, false, -5, two32 * 4, 1, 0, "nothing populated, stale extrema");
        if (g_failed) return;
    }
    // canonical width 4 never goes wider, and has base 0 there
    fit_is(4, true, 5, 5 + two32, 4, 0, "canonical 4 at a range of 2^32");
    if (g_failed) return;
    fit_is(4, true, -two32 * 8, two32 * 8, 4, 0, "canonical 4 at a range of 2^36");
}

// ------------------------------------------------------------------ the fold

struct Col {
    std::vector<int64_t> mn, mx, pop;
    int64_t emin = INT64_MAX, emax = INT64_MIN, n_pop = 0, stats_blocks = 0;
    bool missing = false;
    ColStats ref(bool with_missing) { return ColStats{mn, mx, pop, emin, emax, n_pop, stats_blocks, with_missing ? &missing : nullptr}; }
};

static bool same(const std::vector<int64_t> &a, std::initializer_list<int64_t> b) { return a == std::vector<int64_t>(b); }

static void fold_cases() {
    {  // nb = 0: nothing moves (h may be anything: it is not read)
        Col c;
        stats_fold(c.ref(false), nullptr, 0, 0, 0);
        CHECK(c.mn.empty() && c.mx.empty() && c.pop.empty(), "nb = 0 wrote blocks");
        CHECK(c.emin == INT64_MAX && c.emax == INT64_MIN && c.n_pop == 0 && c.stats_blocks == 0 && !c.missing, "nb = 0 moved a scalar");
    }
    {  // one block without a populated row carries the identity elements: recorded, but the extrema stay
        Col c;
        c.emin = 3, c.emax = 9, c.n_pop = 2;
        const int64_t h[3] = {INT64_MAX, INT64_MIN, 0};
        stats_fold(c.ref(false), h, 1, 0, 1);
        CHECK(same(c.mn, {INT64_MAX}) && same(c.mx, {INT64_MIN}) && same(c.pop, {0}), "the empty block's entries");
        CHECK(c.emin == 3 && c.emax == 9 && c.n_pop == 2 && c.stats_blocks == 1, "an empty block moved the extrema: %lld %lld", (long long)c.emin, (long long)c.emax);
    }
    {  // ... also with garbage instead of the identity elements, and on a fresh column
        Col c;
        const int64_t h[3] = {-100, 100, 0};
        stats_fold(c.ref(false), h, 1, 0, 1);
        CHECK(c.emin == INT64_MAX && c.emax == INT64_MIN && c.n_pop == 0, "an empty block moved fresh extrema");
    }
    {  // b0 > 0: appended behind existing entries, from the FRONT of each third of h (stride nb, here 5; 3 blocks given)
        Col c;
        c.mn = {1, 2}, c.mx = {10, 20}, c.pop = {4, 5};
        c.emin = 1, c.emax = 20, c.n_pop = 9, c.stats_blocks = 2;
        const int64_t h[15] = {-3, 7, INT64_MAX, 111, 111, /**/ 5, 30, INT64_MIN, 222, 222, /**/ 2, 6, 0, 333, 333};
        stats_fold(c.ref(false), h, 5, 2, 3);
        CHECK(same(c.mn, {1, 2, -3, 7, INT64_MAX}), "blk_min behind existing entries");
        CHECK(same(c.mx, {10, 20, 5, 30, INT64_MIN}), "blk_max behind existing entries");
        CHECK(same(c.pop, {4, 5, 2, 6, 0}), "blk_pop behind existing entries");
        CHECK(c.emin == -3 && c.emax == 30 && c.n_pop == 17 && c.stats_blocks == 5, "scalars: %lld %lld %lld %lld", (long long)c.emin, (long long)c.emax,
              (long long)c.n_pop, (long long)c.stats_blocks);
        CHECK(!c.missing, "has_missing moved without being asked");
    }
    {  // extrema at the int64 edges
        Col c;
        const int64_t h[6] = {INT64_MIN, INT64_MAX, /**/ INT64_MIN, INT64_MAX, /**/ 1, 1};
        stats_fold(c.ref(false), h, 2, 0, 2);
        CHECK(c.emin == INT64_MIN && c.emax == INT64_MAX && c.n_pop == 2, "extrema at the edges");
        CHECK(same(c.mn, {INT64_MIN, INT64_MAX}) && same(c.mx, {INT64_MIN, INT64_MAX}), "entries at the edges");
    }
    // has_missing: on and off, with pop < rows, pop == rows and rows == 0
    struct {
        int64_t pop, rows;
        bool want;
    } const cases[] = {{3, 4, true}, {4, 4, false}, {0, 0, false}, {0, 1, true}};
    for (const auto &k : cases)
        for (int on = 0; on < 2; on++) {
            Col c;
            const int64_t h[3] = {k.pop ? 5 : INT64_MAX, k.pop ? 6 : INT64_MIN, k.pop};
            stats_fold(c.ref(on != 0), h, 1, 0, 1, &k.rows);
            CHECK(c.missing == (on && k.want), "has_missing %s, pop %lld of %lld rows: %d", on ? "on" : "off", (long long)k.pop, (long long)k.rows, (int)c.missing);
            CHECK(c.n_pop == k.pop && same(c.pop, {k.pop}), "pop with has_missing %s", on ? "on" : "off");
        }
    {  // has_missing is only ever set: a full block behind a short one leaves it
        Col c;
        const int64_t h[6] = {1, 1, /**/ 2, 2, /**/ 1, 8}, rows[2] = {2, 8};
        stats_fold(c.ref(true), h, 2, 0, 2, rows);
        CHECK(c.missing, "a short block before a full one");
    }
}

// ------------------------------------------------------------------ the set gather

struct Csr {
    std::vector<int64_t> off;
    std::vector<int32_t> vals;
};

// the loop written out: row by row, member by member
static Csr gather_loop(const Csr &src, const std::vector<uint32_t> &map, Csr out) {
    if (out.off.empty()) out.off.push_back(0);
    const int64_t src_rows = (int64_t)src.off.size() - 1;  // (-1 for a CSR of size 0: no row is inside)
    for (uint32_t m : map) {
        if (m != 0xFFFFFFFFu && (int64_t)m < src_rows)
            for (int64_t j = src.off[m]; j < src.off[m + 1]; j++) out.vals.push_back(src.vals[(size_t)j]);
        out.off.push_back((int64_t)out.vals.size());
    }
    return out;
}

static void gather_is(const Csr &src, const std::vector<uint32_t> &map, const Csr &before, const char *what) {
    Csr got = before;
    set_gather(src.off, src.vals, map.data(), (int64_t)map.size(), got.off, got.vals);
    const Csr want = gather_loop(src, map, before);
    CHECK(got.off == want.off && got.vals == want.vals, "%s: differs from the loop", what);
    const size_t had = before.off.empty() ? 1 : before.off.size();
    CHECK(got.off.size() == had + map.size(), "%s: %zu offsets", what, got.off.size());
    for (size_t i = 1; i < got.off.size(); i++) CHECK(got.off[i - 1] <= got.off[i], "%s: offsets fall at %zu", what, i);
    CHECK(got.off.back() == (int64_t)got.vals.size(), "%s: the last offset is not the member count", what);
}

static void gather_cases() {
    const uint32_t none = 0xFFFFFFFFu;
    const Csr empty{{}, {}}, one{{0}, {}};  // size 0: never uploaded; size 1: no row
    // 5 rows: {7, 8}, {}, {9}, {1, 2, 3}, {}
    const Csr five{{0, 2, 2, 3, 6, 6}, {7, 8, 9, 1, 2, 3}};
    for (const Csr *src : {&empty, &one}) {
        gather_is(*src, {}, {}, "no source row, no output row");
        if (g_failed) return;
        gather_is(*src, {0, none, 1, 0}, {}, "no source row: every set is empty");
        if (g_failed) return;
    }
    {
        Csr got;
        const uint32_t map[3] = {0, none, 4};
        set_gather(empty.off, empty.vals, map, 3, got.off, got.vals);
        CHECK(got.off == std::vector<int64_t>({0, 0, 0, 0}) && got.vals.empty(), "a CSR of size 0, by hand");
    }
    gather_is(five, {none, none, none}, {}, "all none");
    if (g_failed) return;
    gather_is(five, {5, 0, 6, none, 1000000}, {}, "a source row at off.size() - 1 and beyond");
    if (g_failed) return;
    {
        Csr got;
        const uint32_t map[2] = {5, 3};  // (row 5 = off.size() - 1: outside)
        set_gather(five.off, five.vals, map, 2, got.off, got.vals);
        CHECK(got.off == std::vector<int64_t>({0, 0, 3}) && got.vals == std::vector<int32_t>({1, 2, 3}), "the first row outside, by hand");
    }
    gather_is(five, {3, 3, 0, 3, 0, 0}, {}, "repeated source rows");
    if (g_failed) return;
    gather_is(five, {4, 2, 0, 3, 1}, {}, "a permutation");
    if (g_failed) return;
    {
        Csr got;
        const uint32_t map[5] = {4, 2, 0, 3, 1};
        set_gather(five.off, five.vals, map, 5, got.off, got.vals);
        CHECK(got.off == std::vector<int64_t>({0, 0, 1, 3, 6, 6}) && got.vals == std::vector<int32_t>({9, 7, 8, 1, 2, 3}), "the permutation, by hand");
    }
    gather_is(five, {0, none, 3}, Csr{{0, 1, 1}, {42}}, "appended behind rows that are there");
    if (g_failed) return;
    gather_is(five, {}, Csr{{0, 1}, {42}}, "nothing appended");
    if (g_failed) return;
    // blocks padded to 32 rows: the padding maps to none
    std::vector<uint32_t> padded(64, none);
    for (uint32_t i = 0; i < 33; i++) padded[i < 32 ? i : 32] = i % 5;
    gather_is(five, padded, {}, "padding rows");
}

int main() {
    storage_cases();
    if (g_failed) return 1;
    printf("storage rule ok\n");
    fold_cases();
    if (g_failed) return 1;
    printf("fold ok\n");
    gather_cases();
    if (g_failed) return 1;
    printf("set gather ok\n");
    return 0;
}
