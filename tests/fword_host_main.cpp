// The layout of a filter word (sybil_amd/csrc/fword.h) on the host: built by tests/test_fword_host.py with
// -fsanitize=address,undefined and run as a program of its own.  Prints one line per group of cases; exits 1 at the first
// property that does not hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fword.h"

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

struct Layout {
    int n;
    int32_t bits[kFwordMaxFields], shift[kFwordMaxFields];
    uint32_t top[kFwordMaxFields];  // all ones in the field
};

// the layout of fields whose largest offsets have the given bit lengths, through fword_layout as the table builds it
static Layout layout_of(int n, const int *want_bits, int want_total) {
    Layout L;
    memset(&L, 0, sizeof(L));
    L.n = n;
    for (int i = 0; i < n; i++) L.top[i] = want_bits[i] == 32 ? 0xFFFFFFFFu : (1u << want_bits[i]) - 1u;
    const int total = fword_layout(L.top, n, L.bits, L.shift);
    int sum = 0;
    for (int i = 0; i < n; i++) {
        if (L.bits[i] != want_bits[i] || L.shift[i] != sum || total != want_total) {
            fprintf(stderr, "FAILED layout: field %d bits %d shift %d total %d, want bits %d shift %d total %d\n", i, L.bits[i], L.shift[i], total,
                    want_bits[i], sum, want_total);
            g_failed = 1;
        }
        sum += want_bits[i];
    }
    return L;
}

// pack, then every field back; the word against a plain sum of shifted offsets; nothing above the last field
static void check_row(const Layout &L, const uint32_t *off) {
    const uint32_t w = fword_pack(off, L.n, L.shift);
    uint64_t plain = 0;
    for (int i = 0; i < L.n; i++) plain += (uint64_t)off[i] << L.shift[i];
    CHECK((uint64_t)w == plain, "word %08x, plain sum %llx", w, (unsigned long long)plain);
    for (int i = 0; i < L.n; i++) {
        const uint32_t back = fword_field(w, L.shift[i], L.bits[i]);
        CHECK(back == off[i], "field %d of %d: %x -> %x (word %08x)", i, L.n, off[i], back, w);
    }
    const int used = L.shift[L.n - 1] + L.bits[L.n - 1];
    CHECK(used == 32 || (w >> used) == 0, "bits above the last field: word %08x uses %d bits", w, used);
}

// 0, 1 and all ones in every field position, against 0, 1 and all ones in every other field at once
static void edge_values(const Layout &L) {
    for (int pos = 0; pos < L.n; pos++)
        for (int v = 0; v < 3; v++)
            for (int o = 0; o < 3; o++) {
                uint32_t off[kFwordMaxFields];
                for (int i = 0; i < L.n; i++) {
                    const int which = i == pos ? v : o;
                    off[i] = which == 0 ? 0u : which == 1 ? 1u : L.top[i];
                }
                check_row(L, off);
                if (g_failed) return;
            }
}

// a field changed alone changes no other field: every single bit of every field set and cleared under all-ones and all-zero neighbours
static void no_bleed(const Layout &L) {
    for (int pos = 0; pos < L.n; pos++)
        for (int bit = 0; bit < L.bits[pos]; bit++)
            for (int others = 0; others < 2; others++) {
                uint32_t off[kFwordMaxFields];
                for (int i = 0; i < L.n; i++) off[i] = others ? L.top[i] : 0u;
                const uint32_t before = fword_pack(off, L.n, L.shift);
                off[pos] ^= 1u << bit;
                const uint32_t after = fword_pack(off, L.n, L.shift);
                CHECK((before ^ after) == (1u << (L.shift[pos] + bit)), "field %d bit %d: words %08x -> %08x", pos, bit, before, after);
                for (int i = 0; i < L.n; i++)
                    if (i != pos) CHECK(fword_field(after, L.shift[i], L.bits[i]) == (others ? L.top[i] : 0u), "field %d moved with field %d bit %d", i, pos, bit);
                check_row(L, off);
                if (g_failed) return;
            }
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next32() {  // splitmix64, top 32 bits
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}

static void random_rows(const Layout &L) {
    for (int r = 0; r < 1000000; r++) {
        uint32_t off[kFwordMaxFields];
        for (int i = 0; i < L.n; i++) off[i] = next32() & L.top[i];
        check_row(L, off);
        if (g_failed) return;
    }
}

static void bit_lengths() {
    const uint32_t v[] = {0u, 1u, 2u, 3u, 999u, 1023u, 1024u, 2047u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const int want[] = {1, 1, 2, 2, 10, 10, 11, 11, 16, 17, 31, 32, 32};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) CHECK(fword_bits(v[i]) == want[i], "fword_bits(%u) = %d, want %d", v[i], fword_bits(v[i]), want[i]);
    // 33 bits: the layout says so and no word is built (2047 / 2047 / 2047)
    const uint32_t top3[3] = {2047u, 2047u, 2047u};
    int32_t bits[3], shift[3];
    CHECK(fword_layout(top3, 3, bits, shift) == 33, "three 11-bit fields need %d bits", fword_layout(top3, 3, bits, shift));
}

int main() {
    const int sets[4][kFwordMaxFields] = {{10, 10, 10, 0}, {11, 11, 10, 0}, {1, 1, 0, 0}, {16, 8, 8, 0}};
    const int counts[4] = {3, 3, 2, 3}, totals[4] = {30, 32, 2, 32};
    bit_lengths();
    if (g_failed) return 1;
    printf("bit lengths ok\n");
    for (int s = 0; s < 4; s++) {
        const Layout L = layout_of(counts[s], sets[s], totals[s]);
        if (g_failed) return 1;
        edge_values(L);
        if (g_failed) return 1;
        no_bleed(L);
        if (g_failed) return 1;
    }
    printf("edge values ok\n");
    for (int s = 0; s < 4; s++) {
        const Layout L = layout_of(counts[s], sets[s], totals[s]);
        random_rows(L);
        if (g_failed) return 1;
    }
    printf("random rows ok\n");
    return 0;
}
