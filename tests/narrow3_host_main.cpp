// The 3-byte layout of a narrow twin (sybil_amd/csrc/narrow3.h) on the host: built by tests/test_narrow3_host.py with
// -fsanitize=address,undefined and run as a program of its own.  Prints one line per group of cases; exits 1 at the first
// property that does not hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "narrow3.h"

using namespace sybl;

static int g_failed = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
            g_failed = 1;                     \
            return;                           \
        }                                     \
    } while (0)

// the twelve bytes of d[0..2] as memory holds them on the little-endian machines the library runs on
static void bytes_of(const uint32_t (&d)[3], uint8_t (&b)[12]) {
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 4; j++) b[4 * k + j] = (uint8_t)(d[k] >> (8 * j));
}

// round trip, and the byte image against a plain 3-bytes-per-row little-endian write
static void check_quad(const uint32_t (&u)[4]) {
    uint32_t d[3], back[4];
    pack3(u, d);
    unpack3(d, back);
    for (int k = 0; k < 4; k++) CHECK(back[k] == u[k], "row %d: %06x -> %06x (quad %06x %06x %06x %06x)", k, u[k], back[k], u[0], u[1], u[2], u[3]);
    uint8_t got[12], want[12];
    bytes_of(d, got);
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 3; j++) want[3 * k + j] = (uint8_t)(u[k] >> (8 * j));
    CHECK(memcmp(got, want, 12) == 0, "byte image of quad %06x %06x %06x %06x", u[0], u[1], u[2], u[3]);
    // (the dwords in memory ARE those bytes: what the kernels store and load)
    uint8_t mem[12];
    memcpy(mem, d, 12);
    CHECK(memcmp(mem, want, 12) == 0, "this host is not little-endian");
}

static void edge_values() {
    const uint32_t vals[5] = {0u, 1u, (1u << 24) - 1u, 0x010203u, 0xFDFEFFu};
    // every value in every row position, against every value in the other three
    for (int pos = 0; pos < 4; pos++)
        for (int v = 0; v < 5; v++)
            for (int o = 0; o < 5; o++) {
                uint32_t u[4] = {vals[o], vals[o], vals[o], vals[o]};
                u[pos] = vals[v];
                check_quad(u);
                if (g_failed) return;
            }
    // four distinct values at once, in every rotation
    for (int rot = 0; rot < 4; rot++) {
        const uint32_t u[4] = {vals[(1 + rot) % 5], vals[(2 + rot) % 5], vals[(3 + rot) % 5], vals[(4 + rot) % 5]};
        check_quad(u);
        if (g_failed) return;
    }
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next24() {  // splitmix64, top 24 bits
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 40);
}

static void random_quads() {
    for (int i = 0; i < 1000000; i++) {
        const uint32_t u[4] = {next24(), next24(), next24(), next24()};
        check_quad(u);
        if (g_failed) return;
    }
}

// a column of n rows written quad by quad reads back row by row at byte 3 * i (the last quad partial: its tail rows are zeros)
static void whole_column() {
    const int n = 1234 + 3;
    uint8_t *img = (uint8_t *)calloc((size_t)(n + 3) / 4 * 12, 1);
    uint32_t *src = (uint32_t *)calloc((size_t)(n + 3) / 4 * 4, 4);
    CHECK(img && src, "out of memory");
    for (int i = 0; i < n; i++) src[i] = next24();
    for (int q = 0; q < (n + 3) / 4; q++) {
        const uint32_t u[4] = {src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]};
        uint32_t d[3];
        pack3(u, d);
        memcpy(img + 12 * q, d, 12);
    }
    for (int i = 0; i < n && !g_failed; i++) {
        const uint32_t v = (uint32_t)img[3 * i] | ((uint32_t)img[3 * i + 1] << 8) | ((uint32_t)img[3 * i + 2] << 16);
        if (v != src[i]) {
            fprintf(stderr, "FAILED row %d: %06x, wrote %06x\n", i, v, src[i]);
            g_failed = 1;
        }
    }
    free(img);
    free(src);
}

int main() {
    edge_values();
    if (g_failed) return 1;
    printf("edge values ok\n");
    random_quads();
    if (g_failed) return 1;
    printf("random quads ok\n");
    whole_column();
    if (g_failed) return 1;
    printf("whole column ok\n");
    return 0;
}
