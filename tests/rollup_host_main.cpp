// The host plan of sybl_table_rollup (sybil_amd/csrc/rollup_plan.h) as a program of its own, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_rollup_host.py and run as a child process.  Expected values are written out by hand
// or computed with __int128 here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rollup_plan.h"

using namespace sybl;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static const ru_u128 one = 1;

static void radices() {
    // a range of 0, 2^16 - 1, 2^16, 2^61 values apart, with and without the MISSING digit
    const int64_t spans[4] = {0, (1 << 16) - 1, 1 << 16, (int64_t)1 << 61};
    const int64_t los[4] = {0, -5, INT64_MIN, INT64_MAX - ((int64_t)1 << 61)};
    for (int64_t span : spans)
        for (int64_t lo : los) {
            const int64_t hi = (int64_t)((__int128)lo + span);
            const ru_u128 want = (ru_u128)((__int128)hi - (__int128)lo) + 1;
            CHECK(ru_radix(true, lo, hi, false) == want);
            CHECK(ru_radix(true, lo, hi, true) == want + 1);
        }
    CHECK(ru_radix(false, 0, 0, false) == 0 && ru_radix(false, 7, 3, true) == 1);
    // INT64_MIN / INT64_MAX as bounds: the whole range is 2^64 values, one more with the MISSING digit
    CHECK(ru_radix(true, INT64_MIN, INT64_MAX, false) == one << 64);
    CHECK(ru_radix(true, INT64_MIN, INT64_MAX, true) == (one << 64) + 1);
    CHECK(ru_radix(true, INT64_MIN, INT64_MIN, false) == 1 && ru_radix(true, INT64_MAX, INT64_MAX, true) == 2);
    CHECK(ru_radix(true, INT64_MIN, -1, false) == one << 63 && ru_radix(true, 0, INT64_MAX, false) == one << 63);
}

static void composites() {
    uint64_t stride[kRuMaxKeys];
    ru_u128 product = 0;
    {
        const ru_u128 r[3] = {24, 101, 7};
        CHECK(ru_composite(r, 3, stride, &product) && product == 24 * 101 * 7);
        CHECK(stride[0] == 101 * 7 && stride[1] == 7 && stride[2] == 1);
    }
    {
        CHECK(ru_composite(nullptr, 0, stride, &product) && product == 1);  // no key: one cell
        const ru_u128 r[2] = {0, 5};  // a column without values or bitmap counts as one digit
        CHECK(ru_composite(r, 2, stride, &product) && product == 5 && stride[0] == 5 && stride[1] == 1);
    }
    {
        const ru_u128 r[1] = {one << 62};  // exactly 2^62 combinations: the largest composite is 2^62 - 1
        CHECK(ru_composite(r, 1, stride, &product) && product == one << 62);
        const ru_u128 r1[1] = {(one << 62) + 1};
        CHECK(!ru_composite(r1, 1, stride, &product));
        const ru_u128 r2[2] = {one << 61, 2};
        CHECK(ru_composite(r2, 2, stride, &product) && product == one << 62 && stride[0] == 2);
        const ru_u128 r3[2] = {(one << 61) + 1, 2};
        CHECK(!ru_composite(r3, 2, stride, &product));
        const ru_u128 r4[1] = {one << 64};  // a key over the whole int64 range
        CHECK(!ru_composite(r4, 1, stride, &product));
        const ru_u128 r5[5] = {one << 62, one << 62, one << 62, one << 62, one << 62};  // no overflow of the running product
        CHECK(!ru_composite(r5, 5, stride, &product));
        const ru_u128 r6[2] = {(one << 64) + 1, (one << 64) + 1};
        CHECK(!ru_composite(r6, 2, stride, &product));
    }
    CHECK(ru_key_bits(1) == 1 && ru_key_bits(2) == 1 && ru_key_bits(3) == 2 && ru_key_bits(256) == 8 && ru_key_bits(257) == 9);
    CHECK(ru_key_bits(one << 62) == 62 && ru_key_bits((one << 61) + 1) == 62 && ru_key_bits(one << 61) == 61);
}

static void buckets() {
    int64_t qlo = 0, qhi = 0;
    ru_bucket_range(-1, 1, 3600, &qlo, &qhi);
    CHECK(qlo == 0 && qhi == 0);  // -1 and 1 both fall into bucket 0
    ru_bucket_range(-3600, 3599, 3600, &qlo, &qhi);
    CHECK(qlo == -1 && qhi == 0);
    ru_bucket_range(-7201, -3601, 3600, &qlo, &qhi);
    CHECK(qlo == -2 && qhi == -1);
    ru_bucket_range(INT64_MIN, INT64_MAX, 1, &qlo, &qhi);
    CHECK(qlo == INT64_MIN && qhi == INT64_MAX);
    ru_bucket_range(INT64_MIN, INT64_MAX, 2, &qlo, &qhi);
    CHECK(qlo == INT64_MIN / 2 && qhi == INT64_MAX / 2 && ru_radix(true, qlo, qhi, false) == one << 63);
    ru_bucket_range(INT64_MIN, INT64_MAX, INT64_MAX, &qlo, &qhi);
    CHECK(qlo == -1 && qhi == 1);
    for (int64_t v = -10; v <= 10; v++) {
        const __int128 q = (__int128)v / 3;  // (C++ division truncates, as Go's)
        CHECK(ru_trunc_div(v, 3) == (int64_t)q && ru_trunc_div(v, 3) * 3 == v - v % 3);
    }
}

static void paths() {
    const int64_t k64 = 64 * 1024;
    // both sides of 2^16 with few rows
    CHECK(ru_choose_path(1 << 16, 100, 1, kRuForceNone) == kRuPathGlobal);
    CHECK(ru_choose_path((1 << 16) + 1, 100, 1, kRuForceNone) == kRuPathHash);
    CHECK(ru_choose_path((1 << 16) + 1, 16384, 1, kRuForceNone) == kRuPathHash);
    CHECK(ru_choose_path((1 << 16) + 1, 16385, 1, kRuForceNone) == kRuPathGlobal);
    // both sides of 4 x rows
    CHECK(ru_choose_path(80000, 20000, 1, kRuForceNone) == kRuPathGlobal && ru_choose_path(80001, 20000, 1, kRuForceNone) == kRuPathHash);
    // both sides of 2^27, whatever the rows
    CHECK(ru_choose_path(one << 27, INT64_MAX, 1, kRuForceNone) == kRuPathGlobal);
    CHECK(ru_choose_path((one << 27) + 1, INT64_MAX, 1, kRuForceNone) == kRuPathHash);
    CHECK(ru_choose_path(one << 62, INT64_MAX, 33, kRuForceNone) == kRuPathHash);
    // the LDS rule one cell either side, at 1, 5 and 33 fields
    const int fields[3] = {1, 5, 33};
    for (int f : fields) {
        const int64_t top = k64 / (8 * f);
        CHECK(ru_choose_path((ru_u128)top, 10, f, kRuForceNone) == kRuPathLds);
        CHECK(ru_choose_path((ru_u128)top + 1, 10, f, kRuForceNone) == kRuPathGlobal);
        CHECK(ru_choose_path((ru_u128)top, 10, f, kRuForceDirect) == kRuPathLds);
        CHECK(ru_choose_path((ru_u128)top, 10, f, kRuForceGlobal) == kRuPathGlobal);
    }
    CHECK(ru_choose_path(1, 0, 1, kRuForceNone) == kRuPathLds);
    // forced
    CHECK(ru_choose_path(100, 10, 1, kRuForceHash) == kRuPathHash);
    CHECK(ru_choose_path(one << 40, 10, 1, kRuForceDirect) == kRuPathNone && ru_choose_path((one << 27) + 1, 10, 1, kRuForceGlobal) == kRuPathNone);
    CHECK(ru_choose_path(one << 27, 10, 1, kRuForceDirect) == kRuPathGlobal);
}

static void slots() {
    CHECK(ru_slots(10, one << 40, 0) == 64 && ru_slots(0, 1, 0) == 64);
    CHECK(ru_slots(32, one << 40, 0) == 64 && ru_slots(33, one << 40, 0) == 128);
    CHECK(ru_slots(1000, 40, 0) == 128);  // min(rows, product)
    CHECK(ru_slots(INT64_MAX, one << 62, 0) == kRuMaxCells && ru_slots((int64_t)1 << 26, one << 62, 0) == kRuMaxCells);
    CHECK(ru_slots(((int64_t)1 << 26) - 1, one << 62, 0) == kRuMaxCells && ru_slots((int64_t)1 << 25, one << 62, 0) == (int64_t)1 << 26);
    CHECK(ru_slots(1000, one << 40, 32) == 32 && ru_slots(1000, one << 40, 33) == 64 && ru_slots(5, 5, 1) == 1);
    CHECK(ru_slots(5, 5, INT64_MAX) == kRuMaxCells);
}

int main() {
    radices();
    puts("radices ok");
    composites();
    puts("composites ok");
    buckets();
    puts("buckets ok");
    paths();
    puts("paths ok");
    slots();
    puts("slots ok");
    return 0;
}
