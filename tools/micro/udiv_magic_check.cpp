// udiv_magic_check.cpp -- sybil_amd/csrc/udiv_magic.h against n / d for EVERY numerator below 2^24, host code only.
//
//   g++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -Isybil_amd/csrc
//       -o /tmp/udiv_magic_check tools/micro/udiv_magic_check.cpp && /tmp/udiv_magic_check
//
// Divisors: the edges of the range and of the powers of two inside it, the bucket sizes the benchmark's columns get, and
// `n_random` seeded ones (argv[1], default 300), spread over the bit lengths 1 .. 24.  For each: the multiplier recomputed in
// 64 bits (it is at most 2^31, so it fits the 32-bit field), and udiv_magic_apply(n, m) == n / d for n = 0 .. 2^24 - 1 -- the
// expected quotient is carried along as a counter, so no division is trusted on either side.
// Prints `ok divisors=.. numerators=..` and returns 0, or the first mismatch and 1.  tests/test_udiv_magic.py builds and runs it.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "udiv_magic.h"

using namespace sybl;

static std::atomic<int> failures{0};

static void check(uint32_t d) {
    const UdivMagic m = udiv_magic(d);
    uint32_t s = 0;
    while (((uint64_t)2 << s) <= d) s++;
    const uint64_t p = (uint64_t)1 << (31 + s), want_mul = p / d + (p % d ? 1 : 0);
    if (m.shift != s || (uint64_t)m.mul != want_mul || want_mul > ((uint64_t)1 << 31)) {
        if (failures++ == 0) fprintf(stderr, "d=%u: mul=%u shift=%u, expected mul=%llu shift=%u\n", d, m.mul, m.shift, (unsigned long long)want_mul, s);
        return;
    }
    uint32_t q = 0, r = 0;  // n = q * d + r
    for (uint32_t n = 0; n < kUdivMagicLimit; n++) {
        if (udiv_magic_apply(n, m) != q) {
            if (failures++ == 0) fprintf(stderr, "d=%u n=%u: got %u, expected %u\n", d, n, udiv_magic_apply(n, m), q);
            return;
        }
        if (++r == d) r = 0, q++;
    }
}

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 300;
    std::vector<uint32_t> ds = {1,     2,     3,     7,     641,           999,     1000,          1001,          4095,         4096,
                                4097,  65535, 65536, 65537, (1u << 23) - 1, 1u << 23, (1u << 23) + 1, (1u << 24) - 2, (1u << 24) - 1};
    uint64_t x = 0x9E3779B97F4A7C15ull;  // splitmix64, fixed seed
    for (int i = 0; i < n_random; i++) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const uint32_t bits = 1 + (uint32_t)(i % 24);  // a divisor of exactly `bits` bits
        const uint32_t top = 1u << (bits - 1);
        ds.push_back(top | ((uint32_t)z & (top - 1)));
    }
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t i = next++; i < ds.size(); i = next++) check(ds[i]);
    };
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nt; i++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    if (failures.load()) {
        fprintf(stderr, "FAILED: %d divisors\n", failures.load());
        return 1;
    }
    printf("ok divisors=%zu numerators=%u\n", ds.size(), (unsigned)kUdivMagicLimit);
    return 0;
}
