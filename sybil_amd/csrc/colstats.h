// colstats.h -- what every maker of a column decides on the host: the stored (width, base), the block statistics and tracked
// extrema, the CSR of a set column gathered through a row map.  Host only, no HIP: table.cpp (appended blocks) and the derived
// tables (derived.h: digest, select, concat, lookup, compute) share these, so a derived column is stored and tracked exactly as
// an appended one.  tests/colstats_host_main.cpp runs them under sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

namespace sybl {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// The storage rule: the (width, base) of a compact column whose tracked extrema are [lo, hi] -- the narrowest of 1 / 2 / 4 / 8
// bytes that holds hi - lo as offsets from lo, never wider than the canonical width `canon`, which has base 0.  any = false: no
// populated row, the stored bits are never looked at -- width 1, base 0.
inline void fit_storage(int canon, bool any, int64_t lo, int64_t hi, int *width, int64_t *base) {
    *width = canon;
    *base = 0;
    if (!any) {
        *width = 1;
        return;
    }
    const unsigned __int128 range = (unsigned __int128)((__int128)hi - (__int128)lo);
    const int fit = range < 256 ? 1 : range < 65536 ? 2 : range < ((unsigned __int128)1 << 32) ? 4 : 8;
    if (fit < *width) {
        *width = fit;
        *base = lo;
    }
}

// the statistics a column tracks (Column's fields of the same names, engine.h)
struct ColStats {
    std::vector<int64_t> &blk_min, &blk_max, &blk_pop;
    int64_t &exact_min, &exact_max, &n_pop, &stats_blocks;
    bool *has_missing;  // nullptr: left alone
};

// The fold.  h: what k_block_minmax left, [min x nb | max x nb | pop x nb]; entry k < n of each third is block b0 + k of the
// column.  The extrema move only with blocks that have a populated row (an empty block carries INT64_MAX / INT64_MIN).
// rows[k]: the rows of block b0 + k, looked at only where has_missing is given: a block with fewer populated rows sets it.
inline void stats_fold(ColStats c, const int64_t *h, int64_t nb, int64_t b0, int64_t n, const int64_t *rows = nullptr) {
    c.blk_min.resize((size_t)(b0 + n));
    c.blk_max.resize((size_t)(b0 + n));
    c.blk_pop.resize((size_t)(b0 + n));
    for (int64_t k = 0; k < n; k++) {
        const int64_t mn = h[k], mx = h[nb + k], pop = h[2 * nb + k];
        c.blk_min[(size_t)(b0 + k)] = mn;
        c.blk_max[(size_t)(b0 + k)] = mx;
        c.blk_pop[(size_t)(b0 + k)] = pop;
        if (pop > 0) {
            if (mn < c.exact_min) c.exact_min = mn;
            if (mx > c.exact_max) c.exact_max = mx;
        }
        c.n_pop += pop;
        if (c.has_missing && pop < rows[k]) *c.has_missing = true;
    }
    c.stats_blocks = b0 + n;
}

// The set-column gather.  (off, vals): the source CSR over its physical rows.  map[p], p < n: the source row of output physical
// row p, or kSetNoRow.  Appends n rows to the output CSR (out_off ends with the members so far: {0} when new).  kSetNoRow -- a
// padding row, a row without a match -- and a source row the CSR does not reach (>= off.size() - 1) give an empty set.
constexpr uint32_t kSetNoRow = 0xFFFFFFFFu;
inline void set_gather(const std::vector<int64_t> &off, const std::vector<int32_t> &vals, const uint32_t *map, int64_t n,
                       std::vector<int64_t> &out_off, std::vector<int32_t> &out_vals) {
    if (out_off.empty()) out_off.push_back(0);
    out_off.reserve(out_off.size() + (size_t)n);
    for (int64_t p = 0; p < n; p++) {
        const size_t s = map[p];
        if (map[p] != kSetNoRow && s + 1 < off.size()) out_vals.insert(out_vals.end(), vals.begin() + off[s], vals.begin() + off[s + 1]);
        out_off.push_back((int64_t)out_vals.size());
    }
}

}  // namespace sybl
