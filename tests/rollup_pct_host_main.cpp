// The host plan of the rollup's percentiles (sybil_amd/csrc/rollup_plan.h: the bits of the cell and of the value span, the sort
// variant, the forced variants, the tokens, the rank) as a program of its own, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_rollup_pct_host.py and run as a child process.  Expected values are written out by
// hand or computed with __int128 here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rollup_plan.h"

using namespace sybl;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static void vbits() {
    // spans 0, 1, 2^32 - 1, 2^32, 2^63 from bases at both int64 edges
    struct {
        unsigned __int128 span;
        int bits;
    } cases[5] = {{0, 0}, {1, 1}, {((unsigned __int128)1 << 32) - 1, 32}, {(unsigned __int128)1 << 32, 33}, {(unsigned __int128)1 << 63, 64}};
    for (auto &c : cases) {
        const int64_t lo = INT64_MIN, hi = (int64_t)((__int128)lo + (__int128)c.span);
        CHECK(ru_pct_vbits(lo, hi) == c.bits);
        const int64_t hi2 = INT64_MAX, lo2 = (int64_t)((__int128)hi2 - (__int128)c.span);
        CHECK(ru_pct_vbits(lo2, hi2) == c.bits);
    }
    CHECK(ru_pct_vbits(INT64_MIN, INT64_MAX) == 64);  // the whole int64 range
    CHECK(ru_pct_vbits(INT64_MIN, INT64_MAX - 1) == 64 && ru_pct_vbits(INT64_MIN, -1) == 63 && ru_pct_vbits(0, INT64_MAX) == 63);
    CHECK(ru_pct_vbits(-1, 0) == 1 && ru_pct_vbits(-2, 1) == 2 && ru_pct_vbits(7, 7) == 0 && ru_pct_vbits(100, 355) == 8 && ru_pct_vbits(100, 356) == 9);
}

static void cbits() {
    CHECK(ru_pct_cbits(1) == 0 && ru_pct_cbits(2) == 1 && ru_pct_cbits(3) == 2 && ru_pct_cbits(4) == 2 && ru_pct_cbits(5) == 3);
    CHECK(ru_pct_cbits(64) == 6 && ru_pct_cbits(1600) == 11 && ru_pct_cbits(kRuMaxCells) == 27 && ru_pct_cbits(kRuMaxCells - 1) == 27);
    CHECK(ru_pct_cbits((int64_t)1 << 26) == 26 && ru_pct_cbits(0) == 0);
}

static void variants() {
    // both sides of 32 and of 64 total bits
    CHECK(ru_pct_variant(0, 0, kRuPctNone) == kRuPct32 && ru_pct_variant(27, 5, kRuPctNone) == kRuPct32 && ru_pct_variant(0, 32, kRuPctNone) == kRuPct32);
    CHECK(ru_pct_variant(27, 6, kRuPctNone) == kRuPct64 && ru_pct_variant(1, 32, kRuPctNone) == kRuPct64 && ru_pct_variant(0, 33, kRuPctNone) == kRuPct64);
    CHECK(ru_pct_variant(0, 64, kRuPctNone) == kRuPct64 && ru_pct_variant(27, 37, kRuPctNone) == kRuPct64);
    CHECK(ru_pct_variant(1, 64, kRuPctNone) == kRuPctPairs && ru_pct_variant(27, 38, kRuPctNone) == kRuPctPairs && ru_pct_variant(27, 64, kRuPctNone) == kRuPctPairs);
    // from the quantities themselves
    CHECK(ru_pct_variant(ru_pct_cbits(1), ru_pct_vbits(INT64_MIN, INT64_MAX), kRuPctNone) == kRuPct64);
    CHECK(ru_pct_variant(ru_pct_cbits(2), ru_pct_vbits(INT64_MIN, INT64_MAX), kRuPctNone) == kRuPctPairs);
    CHECK(ru_pct_variant(ru_pct_cbits(1600), ru_pct_vbits(0, 999999), kRuPctNone) == kRuPct32);  // 11 + 20
    CHECK(ru_pct_variant(ru_pct_cbits(1600), ru_pct_vbits(0, (1 << 21)), kRuPctNone) == kRuPct64);  // 11 + 22
}

static void forced() {
    // a forced variant holds the bits or is refused (kRuPctNone)
    CHECK(ru_pct_variant(10, 10, kRuPct32) == kRuPct32 && ru_pct_variant(10, 10, kRuPct64) == kRuPct64 && ru_pct_variant(10, 10, kRuPctPairs) == kRuPctPairs);
    CHECK(ru_pct_variant(16, 16, kRuPct32) == kRuPct32 && ru_pct_variant(16, 17, kRuPct32) == kRuPctNone);
    CHECK(ru_pct_variant(16, 17, kRuPct64) == kRuPct64 && ru_pct_variant(16, 17, kRuPctPairs) == kRuPctPairs);
    CHECK(ru_pct_variant(27, 37, kRuPct64) == kRuPct64 && ru_pct_variant(27, 38, kRuPct64) == kRuPctNone && ru_pct_variant(27, 38, kRuPct32) == kRuPctNone);
    CHECK(ru_pct_variant(27, 64, kRuPctPairs) == kRuPctPairs && ru_pct_variant(0, 0, kRuPctPairs) == kRuPctPairs);
}

static int tok(const char *s) { return ru_pct_token(s, strlen(s)); }

static void tokens() {
    CHECK(tok("p1") == 1 && tok("p9") == 9 && tok("p10") == 10 && tok("p50") == 50 && tok("p99") == 99);
    CHECK(tok("p0") == 0 && tok("p100") == 0 && tok("p05") == 0 && tok("p5.5") == 0 && tok("p") == 0 && tok("") == 0);
    CHECK(tok("P50") == 0 && tok("p-1") == 0 && tok("p5x") == 0 && tok("q50") == 0 && tok("p 5") == 0 && tok("50") == 0 && tok("p00") == 0);
    CHECK(ru_pct_token("p50,p99", 3) == 50);  // (a token inside a longer string: the length bounds it)
    // the rank: (k * n + 99) / 100
    CHECK(ru_pct_rank(1, 4) == 1 && ru_pct_rank(50, 4) == 2 && ru_pct_rank(51, 4) == 3 && ru_pct_rank(99, 4) == 4);
    CHECK(ru_pct_rank(66, 3) == 2 && ru_pct_rank(67, 3) == 3 && ru_pct_rank(50, 101) == 51 && ru_pct_rank(99, 101) == 100);
    CHECK(ru_pct_rank(1, 200) == 2 && ru_pct_rank(50, 200) == 100 && ru_pct_rank(99, 200) == 198 && ru_pct_rank(1, 1) == 1 && ru_pct_rank(99, 1) == 1);
    for (int k = 1; k <= 99; k++) {
        CHECK(ru_pct_rank(k, 100) == k);
        const int64_t n = (int64_t)1 << 56;  // more rows than a table holds: no overflow, and the rank stays within 1 .. n
        const unsigned __int128 want = ((unsigned __int128)k * (unsigned __int128)n + 99) / 100;
        CHECK((unsigned __int128)ru_pct_rank(k, n) == want && ru_pct_rank(k, n) >= 1 && ru_pct_rank(k, n) <= n);
    }
}

int main() {
    vbits();
    puts("vbits ok");
    cbits();
    puts("cbits ok");
    variants();
    puts("variants ok");
    forced();
    puts("forced ok");
    tokens();
    puts("tokens ok");
    return 0;
}
