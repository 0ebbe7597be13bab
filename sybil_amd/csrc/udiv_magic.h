// udiv_magic.h -- the constants of an exact multiply-shift quotient floor(n / d) for n < 2^24 and 1 <= d < 2^24: what
// FastPlan::lean's kLeanProved proves of every bucket numerator and bucket size (scan_fast.h; planner.cpp: plan_lean).
// Host code only, all of it constexpr: the planner fills FastPlan::qmul / qshift with it, and the PROVED row bodies of
// k_scan_packed (scan_packed.h: packed_row) spell the same three operations out on the device.
//
//   s = floor(log2 d),  M = ceil(2^(31 + s) / d)  (2^30 < M <= 2^31),  q = umulhi(2 n, M) >> s = floor(n M / 2^(31 + s))
//
// Exact: M d = 2^(31 + s) + e with 0 <= e < d < 2^(s + 1), so n M / 2^(31 + s) = n / d + n e / (d 2^(31 + s)), and
// n e < 2^24 2^(s + 1) <= 2^(31 + s) keeps the second term below 1 / d -- too little to carry n / d past the next integer.
// The DOUBLED numerator is what keeps d = 1 inside 32 bits (M = 2^31, q = n); 2 n < 2^25 cannot wrap.
#pragma once
#include <cstdint>

namespace sybl {

constexpr uint32_t kUdivMagicLimit = 1u << 24;  // n and d are below it

struct UdivMagic {
    uint32_t mul, shift;
};

// (d outside 1 .. 2^24 - 1: {0, 0}, a quotient of zero -- no PROVED body is launched with such a bucket size)
constexpr UdivMagic udiv_magic(uint32_t d) {
    if (d < 1 || d >= kUdivMagicLimit) return UdivMagic{0, 0};
    uint32_t s = 0;
    while ((d >> (s + 1)) != 0) s++;
    const uint64_t p = (uint64_t)1 << (31 + s);
    return UdivMagic{(uint32_t)((p + d - 1) / d), s};
}

// the quotient as the device computes it: the high dword of (2 n) * mul, shifted
constexpr uint32_t udiv_magic_apply(uint32_t n, UdivMagic m) { return (uint32_t)(((uint64_t)(n << 1) * m.mul) >> 32) >> m.shift; }

namespace udiv_magic_check {
constexpr bool at(uint32_t n, uint32_t d) { return n >= kUdivMagicLimit || udiv_magic_apply(n, udiv_magic(d)) == n / d; }
// n = 2^24 - 1, and k d - 1, k d for the first, a middle and the last multiple of d below 2^24
constexpr bool edges(uint32_t d) {
    const uint32_t top = kUdivMagicLimit - 1, kmax = top / d, kmid = kmax / 2 + 1;
    return udiv_magic(d).mul > (1u << 30) && udiv_magic(d).mul <= (1u << 31) && at(top, d) && at(0, d) && at(d - 1, d) && at(d, d) &&
           at(kmid * d - 1, d) && at(kmid * d, d) && at(kmax * d - 1, d) && at(kmax * d, d);
}
static_assert(udiv_magic(1).mul == (1u << 31) && udiv_magic(1).shift == 0, "d = 1: q = (2 n * 2^31) >> 32 = n");
static_assert(udiv_magic(1000).shift == 9 && udiv_magic(1000).mul == 1099511628u, "ceil(2^40 / 1000)");
static_assert(edges(1) && edges(2) && edges(3), "the smallest bucket sizes");
static_assert(edges(999) && edges(1000) && edges(4096), "bucket sizes of the benchmark's kind, a power of two");
static_assert(edges((1u << 23) - 1) && edges(1u << 23) && edges((1u << 23) + 1), "around the last power of two");
static_assert(edges((1u << 24) - 2) && edges((1u << 24) - 1), "the largest bucket sizes");
static_assert(udiv_magic(0).mul == 0 && udiv_magic(1u << 24).mul == 0, "outside the proof: no constants");
}  // namespace udiv_magic_check

}  // namespace sybl
