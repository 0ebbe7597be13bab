// rollup_plan.h -- what sybl_table_rollup (rollup.hip) decides on the host before any kernel runs: the digit of every key
// column, the mixed-radix composite key, the path and the size of the hash table, and for percentiles the sort key's bits and
// the sort variant.  Host only, no HIP, as colstats.h; tests/rollup_host_main.cpp and tests/rollup_pct_host_main.cpp run it under
// sanitizers.  Every quantity that can leave int64 is carried in 128 bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sybl {

typedef unsigned __int128 ru_u128;

constexpr int kRuMaxKeys = 5;                          // the time part + 4 group columns
constexpr int kRuMaxAggs = 8;
constexpr int64_t kRuMaxCells = (int64_t)1 << 27;      // direct cells, and hash slots (plan.h: kHashMaxSlots)
constexpr int64_t kRuMinSlots = 64;
constexpr int64_t kRuDirectFloor = (int64_t)1 << 16;   // a product up to here is direct whatever the row count
constexpr int64_t kRuLdsBytes = 64 * 1024;             // the LDS body: cells x fields x 8 B up to here
constexpr ru_u128 kRuMaxComposite = (ru_u128)1 << 62;  // composites stay below: kHashEmpty and the sort's bits

enum RuPath { kRuPathNone = 0, kRuPathLds = 1, kRuPathGlobal = 2, kRuPathHash = 3 };
enum RuForce { kRuForceNone = 0, kRuForceDirect = 1, kRuForceGlobal = 2, kRuForceHash = 3 };

// Go's truncating division (aggregate.go:174): -1 / B and 1 / B are both 0.  b > 0.
inline int64_t ru_trunc_div(int64_t v, int64_t b) { return v / b; }

// The digits of a key column whose populated values lie in [lo, hi] (any = false: no populated value): hi - lo + 1 value
// digits, and one more -- digit 0, the MISSING digit, before every value -- when the column has a bitmap.
inline ru_u128 ru_radix(bool any, int64_t lo, int64_t hi, bool missing) {
    ru_u128 r = any ? (ru_u128)((__int128)hi - (__int128)lo) + 1 : 0;
    return r + (missing ? 1 : 0);
}

// The time part: the buckets of values in [lo, hi] are the quotients trunc(lo / B) .. trunc(hi / B).
inline void ru_bucket_range(int64_t lo, int64_t hi, int64_t B, int64_t *qlo, int64_t *qhi) {
    *qlo = ru_trunc_div(lo, B);
    *qhi = ru_trunc_div(hi, B);
}

// The composite: digit k has stride[k] = the product of the radices behind it (key 0 is the most significant), so ascending
// composites are the output order.  false: the product exceeds 2^62 (a key column over the whole int64 range does so alone).
// A radix of 0 (a column without values or bitmap: a table without rows) counts as 1.
inline bool ru_composite(const ru_u128 *radix, int n, uint64_t *stride, ru_u128 *product) {
    ru_u128 p = 1;
    for (int k = n - 1; k >= 0; k--) {
        stride[k] = (uint64_t)p;
        const ru_u128 r = radix[k] ? radix[k] : 1;
        if (r > kRuMaxComposite || p * r > kRuMaxComposite) {  // (p, r <= 2^62: the product fits 128 bits)
            *product = kRuMaxComposite + 1;
            return false;
        }
        p *= r;
    }
    *product = p;
    return true;
}

// direct: product <= max(2^16, 4 x live rows) and <= 2^27; the LDS body where cells x fields x 8 B <= 64 KiB.
// force: SYBL_ROLLUP_PATH.  kRuPathNone: direct / global was forced and the product exceeds 2^27.
inline int ru_choose_path(ru_u128 product, int64_t live_rows, int fields, int force) {
    const ru_u128 by_rows = live_rows > 0 ? (ru_u128)live_rows * 4 : 0;
    const ru_u128 limit = by_rows > (ru_u128)kRuDirectFloor ? by_rows : (ru_u128)kRuDirectFloor;
    const bool fits = product <= (ru_u128)kRuMaxCells;
    const bool lds = fits && product * (ru_u128)fields * 8 <= (ru_u128)kRuLdsBytes;
    switch (force) {
    case kRuForceDirect: return !fits ? kRuPathNone : lds ? kRuPathLds : kRuPathGlobal;
    case kRuForceGlobal: return !fits ? kRuPathNone : kRuPathGlobal;
    case kRuForceHash: return kRuPathHash;
    default: break;
    }
    if (!fits || product > limit) return kRuPathHash;
    return lds ? kRuPathLds : kRuPathGlobal;
}

inline int64_t ru_pow2_at_least(ru_u128 x) {
    int64_t s = 1;
    while ((ru_u128)s < x && s < kRuMaxCells) s <<= 1;
    return s;
}

// Slots of the hash table: the power of two >= 2 x min(live rows, product), at least 64, at most 2^27.  asked > 0
// (SYBL_ROLLUP_SLOTS): that many, rounded up to a power of two, at most 2^27 -- a table smaller than its keys fills and the call
// returns SYBL_E_NOMEM.
inline int64_t ru_slots(int64_t live_rows, ru_u128 product, int64_t asked) {
    if (asked > 0) return ru_pow2_at_least((ru_u128)asked);
    const ru_u128 keys = (ru_u128)(live_rows > 0 ? live_rows : 0) < product ? (ru_u128)(live_rows > 0 ? live_rows : 0) : product;
    const int64_t s = ru_pow2_at_least(keys * 2);
    return s < kRuMinSlots ? kRuMinSlots : s;
}

// the bits of the largest composite, product - 1: what the radix sort of the hash path orders by
inline int ru_key_bits(ru_u128 product) {
    int bits = 1;
    const ru_u128 top = product > 0 ? product - 1 : 0;
    while (bits < 64 && (top >> bits) != 0) bits++;
    return bits;
}

// ------------------------------------------------------------------ percentiles (p<k> in `ops`)
// Per aggregated column with percentiles the populated values of the matching rows are sorted by the key
// cell << vbits | (v - lo): cell the direct path's cell or the hash path's slot, [lo, hi] the column's tracked extrema.  A group's
// values are then contiguous, ascending, and start at the exclusive sum of n over the cells before its own.

constexpr int kRuMaxPcts = 8;  // percentile tokens per aggregated column

enum RuPctVariant { kRuPctNone = 0, kRuPct32 = 1, kRuPct64 = 2, kRuPctPairs = 3 };

// A token p<k>: k a decimal integer 1..99 without a leading zero.  0: not such a token.
inline int ru_pct_token(const char *p, size_t len) {
    if (len < 2 || len > 3 || p[0] != 'p' || p[1] < '1' || p[1] > '9') return 0;
    if (len == 2) return p[1] - '0';
    if (p[2] < '0' || p[2] > '9') return 0;
    return (p[1] - '0') * 10 + (p[2] - '0');
}

inline int ru_bits_of(ru_u128 x) {
    int bits = 0;
    while (bits < 128 && (x >> bits) != 0) bits++;
    return bits;
}

// the bits of n_cells - 1: one cell needs none
inline int ru_pct_cbits(int64_t n_cells) { return n_cells > 1 ? ru_bits_of((ru_u128)(n_cells - 1)) : 0; }

// the bits of hi - lo, carried in 128 bits: 0 for one value, 64 for the whole int64 range
inline int ru_pct_vbits(int64_t lo, int64_t hi) { return hi > lo ? ru_bits_of((ru_u128)((__int128)hi - (__int128)lo)) : 0; }

// 32: cbits + vbits <= 32, uint32 keys; 64: <= 64, uint64 keys; pairs: beyond -- the values sorted with the cell as payload, then
// stably by cell.  force: SYBL_ROLLUP_PCT, kRuPctNone = the rule.  kRuPctNone: the forced variant does not hold the bits.
inline int ru_pct_variant(int cbits, int vbits, int force) {
    const int bits = cbits + vbits;
    const int fit = bits <= 32 ? kRuPct32 : bits <= 64 ? kRuPct64 : kRuPctPairs;
    if (force == kRuPctNone) return fit;
    return force >= fit ? force : kRuPctNone;
}

// nearest rank: the 1-based rank of p<k> among n > 0 ascending values, ceil(k * n / 100) (n counts rows: k * n stays in int64)
inline int64_t ru_pct_rank(int k, int64_t n) { return ((int64_t)k * n + 99) / 100; }

}  // namespace sybl
