// The piece table of k_scan_packed's dynamic dealing (sybil_amd/csrc/pieces.h) on the host: built by tests/test_pieces_host.py
// with -fsanitize=address,undefined and run as a program of its own.  Prints one line per group of cases; exits 1 at the first
// property that does not hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pieces.h"

using namespace sybl;

struct Run {
    int64_t start, n;
};

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

// every row of every run in exactly one piece; table order; no piece across a run's end or a multiple of 2^28 rows from the
// run's start; only a run's last piece partial; no piece above piece_tiles tiles
static void check(const std::vector<Run> &runs, int piece_tiles, const char *what) {
    std::vector<Piece> pieces;
    deal_pieces(runs, piece_tiles, pieces);
    const int64_t piece_rows = (int64_t)piece_tiles * kPieceTileRows;
    size_t pi = 0;
    int64_t prev_end = INT64_MIN;
    for (size_t ri = 0; ri < runs.size(); ri++) {
        const Run &r = runs[ri];
        int64_t at = r.start;  // the next row of this run that no piece has covered yet
        while (at < r.start + r.n) {
            CHECK(pi < pieces.size(), "%s: run %zu: rows from %lld are in no piece", what, ri, (long long)at);
            const Piece &p = pieces[pi];
            CHECK(p.n >= 1, "%s: piece %zu is empty", what, pi);
            CHECK(p.start == at, "%s: piece %zu starts at %lld, expected %lld (gap, overlap or order)", what, pi, (long long)p.start, (long long)at);
            CHECK(p.start >= prev_end, "%s: piece %zu is not in table order", what, pi);
            const int64_t end = p.start + (int64_t)p.n;
            CHECK(end <= r.start + r.n, "%s: piece %zu crosses the end of run %zu", what, pi, ri);
            CHECK((int64_t)p.n <= piece_rows, "%s: piece %zu has %u rows > %lld", what, pi, p.n, (long long)piece_rows);
            CHECK((p.start - r.start) / kPieceChunkRows == (end - 1 - r.start) / kPieceChunkRows, "%s: piece %zu crosses a 2^28 boundary", what, pi);
            CHECK((p.start - r.start) % kPieceTileRows == 0, "%s: piece %zu does not start on a tile of its run", what, pi);
            if (end < r.start + r.n) CHECK(p.n % kPieceTileRows == 0, "%s: piece %zu is partial but not its run's last", what, pi);
            prev_end = end;
            at = end;
            pi++;
        }
    }
    CHECK(pi == pieces.size(), "%s: %zu pieces beyond the runs", what, pieces.size() - pi);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64: seeded, the same everywhere
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const int tiles[] = {1, 2, 16, 32, 64, 65536};
    // single runs: 1 row, around one tile, around the 2^28-row chunk; at row 0 and at a 32-row boundary far into the table
    const int64_t lens[] = {1, 4095, 4096, 4097, ((int64_t)1 << 28) - 1, (int64_t)1 << 28, ((int64_t)1 << 28) + 1};
    for (int pt : tiles)
        for (int64_t n : lens)
            for (int64_t start : {(int64_t)0, (int64_t)32 * 1234567, ((int64_t)1 << 33) + 64}) {
                check({{start, n}}, pt, "single run");
                if (g_failed) return 1;
            }
    printf("single runs ok\n");
    // many runs with gaps (blocks that start on padded 32-row boundaries; some runs shorter than a tile)
    for (int pt : tiles) {
        std::vector<Run> runs;
        int64_t at = 0;
        const int64_t ns[] = {65536, 5, 4096, 100000, 4097, 1, 8191, 8192, 300001, 31};
        for (int rep = 0; rep < 30; rep++)
            for (int64_t n : ns) {
                runs.push_back({at, n});
                at += (n + 31) / 32 * 32 + 32 * (int64_t)(rep % 3) * 1000;  // (rep % 3 == 0: the next run touches the padding)
            }
        check(runs, pt, "runs with gaps");
        if (g_failed) return 1;
    }
    printf("runs with gaps ok\n");
    // 200 random seeded run lists
    for (int it = 0; it < 200; it++) {
        g_rng = 1000 + (uint64_t)it;
        std::vector<Run> runs;
        int64_t at = (int64_t)(rnd() % 100) * 32;
        const int n_runs = (int)(rnd() % 40);
        for (int r = 0; r < n_runs; r++) {
            const uint64_t kind = rnd() % 8;
            int64_t n = kind == 0 ? 1 + (int64_t)(rnd() % 64) : kind == 1 ? kPieceTileRows * (1 + (int64_t)(rnd() % 70)) : 1 + (int64_t)(rnd() % 3000000);
            if (kind == 7 && it % 50 == 0) n = kPieceChunkRows + (int64_t)(rnd() % 10000) - 5000;
            runs.push_back({at, n});
            at += (n + 31) / 32 * 32 + 32 * (int64_t)(rnd() % 4 == 0 ? 0 : rnd() % 5000);
        }
        const int pt = tiles[rnd() % 5];
        check(runs, pt, "random runs");
        if (g_failed) {
            fprintf(stderr, "(seed %d)\n", 1000 + it);
            return 1;
        }
    }
    printf("random runs ok\n");
    // the cap: n_wg workgroups at their caps have drawn at least n_pieces tickets
    for (int64_t n_wg : {1, 16, 256, 304})
        for (int64_t n_pieces : {(int64_t)0, (int64_t)1, n_wg - 1, n_wg, n_wg + 1, 10 * n_wg + 3})
            for (int64_t pct : {100, 125}) {
                const int64_t cap = piece_cap(n_pieces, n_wg, pct);
                if (!(cap >= 0 && n_wg * cap >= n_pieces)) {
                    fprintf(stderr, "FAILED: n_wg %lld x cap %lld < %lld pieces (pct %lld)\n", (long long)n_wg, (long long)cap, (long long)n_pieces, (long long)pct);
                    return 1;
                }
                if (pct == 125 && cap != (n_pieces * 5 + n_wg * 4 - 1) / (n_wg * 4) + 2) {
                    fprintf(stderr, "FAILED: cap %lld is not ceil(n_pieces / n_wg * 5 / 4) + 2 (n_wg %lld, n_pieces %lld)\n", (long long)cap, (long long)n_wg, (long long)n_pieces);
                    return 1;
                }
            }
    printf("cap ok\n");
    return 0;
}
