// rollup.hip -- a group-by whose result is again a resident table: one row per group, aggregated on the GPU.  The semantics are
// restated in include/sybilgpu.h ("rollup") and DESIGN.md 3.14; the host plan -- digits, composite key, path, slots -- is
// rollup_plan.h.  This file is the device work and the host code that drives it.
//
//   filter        k_prefilter (kernels.hip) over the slots the planner lowered, into a zeroed bitmap indexed by physical row, as
//                 select.hip runs it.  Without filters there is no bitmap.
//   k_ru_accum    the hot path.  A lane owns FOUR consecutive physical rows of one block and reads every key and value column
//                 at its stored width as whole dwords (the column table arrives by value and stays scalar; the switch on the
//                 width is wave-uniform); a tile is 1024 rows of ONE block, workgroups take tiles grid-stride and find the
//                 block by a scalar bisection.  Cells are [field][cell] int64: count and, per aggregated column, n, sum, max
//                 and ~min -- every field is an add or a signed max.
//                   <LDS>     direct path, cells x fields x 8 B <= 64 KiB: the workgroup's cells live in LDS (64-bit LDS
//                             atomics); at the end each workgroup flushes its occupied cells with agent-scope atomics.
//                   <global>  per row the cell (direct: the composite) or the slot (hash: find-or-claim), agent-scope atomics.
//                 In both a lane first folds its consecutive rows of equal cell, and a wave whose active rows all fall into
//                 ONE cell reduces every field by shuffles and lets one lane issue the atomics (SYBL_ROLLUP_MERGE=0: off).
//                 matched / rows_no_time / table-full leave as one atomic per workgroup.
//   order         direct: the occupied cells in cell order (hipcub::DeviceSelect::Flagged over count > 0: cell order is key
//                 order, nothing is sorted).  hash: the claimed slots compacted likewise, their composites fetched, and
//                 hipcub::DeviceRadixSort::SortPairs over exactly the composite's bits.  One readback brings G and the counters.
//   percentiles   once per aggregated column with p<k> tokens, between order and emit, every column in the same pool buffers:
//                 the exclusive sum of the column's n field over the cells (where each cell's values start); k_ru_pct_keys --
//                 k_ru_accum's row front end, the cell found and never claimed -- writes one sort key cell << vbits | (v - lo)
//                 per matching populated value, compacted with wave ballots and one cursor atomic per workgroup and tile;
//                 hipcub::DeviceRadixSort over exactly the key's bits (uint32 keys, uint64 keys, or -- beyond 64 bits -- by value
//                 with the cell as payload and then stably by cell: rollup_plan.h); k_ru_pct_pick takes the value of rank
//                 (k * n + 99) / 100 for every (output row, percentile).  One sort serves all percentiles of a column.  The
//                 item counts travel with the order phase's readback: no further wait.
//   k_ru_emit     a lane owns four consecutive OUTPUT physical rows of one column: it decodes the composite into the column's
//                 digit, reads the cell's field, or reads an array by output row (a percentile).  <false, 0>: the range pass -- min / max / populated, one set of atomics per
//                 workgroup --, read back once for all columns; the host fits (width, base) with the storage rule.  <true, W>:
//                 the store pass -- (v - base) at width W as whole dwords, 0 in padding and where unpopulated; validity words
//                 OR-ed together from the 8 lanes that hold a word's 32 rows.
//   statistics    derived_block_stats (derived.h): one readback, one wait.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "derived.h"
#include "hash_table.h"
#include "rollup_plan.h"

namespace sybl {

constexpr int kRuThreads = 256;
constexpr int kRuRows = 4;                         // per lane
constexpr int kRuTileRows = kRuThreads * kRuRows;  // 1024
constexpr int kRuWgPerCu = 8;
constexpr int kRuMaxFilterCols = 8;  // k_prefilter is instantiated for 1..8 slots

struct RuCol {
    const void *data;       // nullptr: no row was ever written -- every row unpopulated
    const uint32_t *valid;  // nullptr: every row populated
    int64_t base;
    int32_t width;
    int32_t missing;  // a key column: 1 = digit 0 is the MISSING digit
};

struct RuArgs {
    RuCol keys[kRuMaxKeys];  // keys[0] is the time part when has_time
    int64_t key_lo[kRuMaxKeys];
    uint64_t key_stride[kRuMaxKeys];
    RuCol vals[kRuMaxAggs];
    const RowBlk *blk;  // base: the tiles before a block
    const uint32_t *bits;
    int64_t *cells;    // [fields][n_cells]
    uint64_t *hkeys;   // hash: [n_cells] slot -> composite
    long long *ctr;    // matched, rows_no_time, rows that found the table full
    int64_t n_tiles, n_cells, time_bucket;
    uint32_t hmask;
    int32_t nb, n_keys, n_vals, has_time, merge;
};

// field f of a cell: 0 = count; 1 + 4a .. 4 + 4a = n, sum, max, ~min of aggregated column a.  max and ~min start at INT64_MIN
// and grow by signed max, the others start at 0 and grow by add.
__host__ __device__ __forceinline__ bool ru_is_max(int f) { return f > 0 && ((f - 1) & 3) >= 2; }

// rows p0 .. p0 + 3 of a column (p0 a multiple of 4 inside a block's padded rows): the values of the rows in `want` that are
// populated, and their bits
__device__ __forceinline__ uint32_t ru_load(const RuCol &c, int64_t p0, uint32_t want, int64_t v[kRuRows]) {
#pragma unroll
    for (int k = 0; k < kRuRows; k++) v[k] = 0;
    if (c.data == nullptr || want == 0) return 0;
    uint32_t pop = want;
    if (c.valid != nullptr) pop &= c.valid[p0 >> 5] >> (p0 & 31);
    uint64_t raw[kRuRows];
    switch (c.width) {
    case 8: {
        const ulonglong2 *p = (const ulonglong2 *)c.data + (p0 >> 1);
        const ulonglong2 a = p[0], b = p[1];
        raw[0] = a.x, raw[1] = a.y, raw[2] = b.x, raw[3] = b.y;
        break;
    }
    case 4: {
        const uint4 a = ((const uint4 *)c.data)[p0 >> 2];
        raw[0] = a.x, raw[1] = a.y, raw[2] = a.z, raw[3] = a.w;
        break;
    }
    case 2: {
        const uint2 a = ((const uint2 *)c.data)[p0 >> 2];
        raw[0] = a.x & 0xFFFFu, raw[1] = a.x >> 16, raw[2] = a.y & 0xFFFFu, raw[3] = a.y >> 16;
        break;
    }
    default: {
        const uint32_t a = ((const uint32_t *)c.data)[p0 >> 2];
        raw[0] = a & 0xFFu, raw[1] = (a >> 8) & 0xFFu, raw[2] = (a >> 16) & 0xFFu, raw[3] = a >> 24;
        break;
    }
    }
#pragma unroll
    for (int k = 0; k < kRuRows; k++) v[k] = (pop >> k) & 1u ? (int64_t)((uint64_t)c.base + raw[k]) : 0;
    return pop;
}

// The slot of a composite: found, or claimed by a 64-bit compare-and-swap against kHashEmpty (composites are below 2^62).
// Linear probing from splitmix64(key) >> 32 & mask; the walk is bounded -- -1: the table is full.
__device__ __forceinline__ int32_t ru_find_or_claim(uint64_t *keys, uint32_t mask, uint64_t key) {
    uint32_t h = (uint32_t)(splitmix64(key) >> 32) & mask;
    const uint32_t limit = mask + 1u < kHashMaxProbes ? mask + 1u : kHashMaxProbes;
    for (uint32_t probe = 0; probe < limit; probe++) {
        uint64_t k = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kHashEmpty) {
            unsigned long long expect = kHashEmpty;
            if (__hip_atomic_compare_exchange_strong((unsigned long long *)keys + h, &expect, (unsigned long long)key, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                k = key;
            else
                k = expect;
        }
        if (k == key) return (int32_t)h;
        h = (h + 1) & mask;
    }
    return -1;
}

template <bool LDS>
__device__ __forceinline__ void ru_add(int64_t *g, int64_t *l, int64_t ix, int64_t v) {
    if (LDS) __hip_atomic_fetch_add(l + ix, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(g + ix, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void ru_max(int64_t *g, int64_t *l, int64_t ix, int64_t v) {
    if (LDS) __hip_atomic_fetch_max(l + ix, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_max(g + ix, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n, sum, max, ~min of one aggregated column into a cell (n > 0)
template <bool LDS>
__device__ __forceinline__ void ru_put(int64_t *g, int64_t *l, int64_t n_cells, int a, uint32_t cell, int64_t n, uint64_t s, int64_t mx, int64_t nm) {
    const int64_t at = (int64_t)(1 + 4 * a) * n_cells + cell;
    ru_add<LDS>(g, l, at, n);
    ru_add<LDS>(g, l, at + n_cells, (int64_t)s);
    ru_max<LDS>(g, l, at + 2 * n_cells, mx);
    ru_max<LDS>(g, l, at + 3 * n_cells, nm);
}

__device__ __forceinline__ int64_t ru_wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int64_t ru_wave_max(int64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// A composite's slot in a table that is complete: found, or -1 -- nothing is claimed.  The walk is bounded as above.
__device__ __forceinline__ int32_t ru_find(const uint64_t *keys, uint32_t mask, uint64_t key) {
    uint32_t h = (uint32_t)(splitmix64(key) >> 32) & mask;
    const uint32_t limit = mask + 1u < kHashMaxProbes ? mask + 1u : kHashMaxProbes;
    for (uint32_t probe = 0; probe < limit; probe++) {
        const uint64_t k = keys[h];
        if (k == key) return (int32_t)h;
        if (k == kHashEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// The row front end of a tile, shared by k_ru_accum and k_ru_pct_keys: the lane's four rows p0 .. p0 + 3 of the tile's block, the
// returned mask of those that are live, pass the filters and have a key (a row without a time value is dropped and counted),
// and their cells -- the composite, or its slot: find-or-claim (<CLAIM>) or find-only.  *lost counts rows whose composite found
// no slot; find-only also those whose composite is not below n_cells (cannot be; never an address).
template <bool HASH, bool CLAIM>
__device__ __forceinline__ uint32_t ru_rows(const RuArgs &A, int64_t tile, int tid, int64_t *p0_out, uint32_t cell[kRuRows], long long *matched,
                                            long long *no_time, long long *lost) {
    const RowBlk B = A.blk[block_of(A.blk, A.nb, tile, &RowBlk::base)];  // (uniform, scalar)
    const int64_t p0 = B.start + (tile - B.base) * kRuTileRows + (int64_t)tid * kRuRows;
    const int64_t left = B.start + B.n - p0;
    uint32_t m = left <= 0 ? 0u : left >= kRuRows ? 0xFu : (1u << (int)left) - 1u;  // the lane's live rows ...
    if (A.bits != nullptr && m != 0) m &= A.bits[p0 >> 5] >> (p0 & 31);               // ... that pass the filters
    *matched += __popc(m);

    // ---- the composite key
    uint64_t comp[kRuRows] = {0, 0, 0, 0};
    for (int g = 0; g < A.n_keys; g++) {
        int64_t v[kRuRows];
        const uint32_t pop = ru_load(A.keys[g], p0, m, v);
        const int64_t lo = A.key_lo[g];
        const uint64_t stride = A.key_stride[g];
        if (g == 0 && A.has_time) {
            *no_time += __popc(m & ~pop);
            m &= pop;
#pragma unroll
            for (int k = 0; k < kRuRows; k++)
                if ((m >> k) & 1u) comp[k] += (uint64_t)(v[k] / A.time_bucket - lo) * stride;
        } else {
            const uint64_t miss = (uint64_t)A.keys[g].missing;
            if (!miss) m &= pop;  // (a column without a bitmap has every row populated)
#pragma unroll
            for (int k = 0; k < kRuRows; k++)
                if ((pop >> k) & 1u) comp[k] += ((uint64_t)v[k] - (uint64_t)lo + miss) * stride;
        }
    }

    // ---- the cell: the composite itself, or its slot; a lane's consecutive rows of one key probe once
#pragma unroll
    for (int k = 0; k < kRuRows; k++) cell[k] = 0;
#pragma unroll
    for (int k = 0; k < kRuRows; k++) {
        if (!((m >> k) & 1u)) continue;
        if (HASH) {
            if (k > 0 && ((m >> (k - 1)) & 1u) && comp[k] == comp[k - 1]) {
                cell[k] = cell[k - 1];
                continue;
            }
            const int32_t s = CLAIM ? ru_find_or_claim(A.hkeys, A.hmask, comp[k]) : ru_find(A.hkeys, A.hmask, comp[k]);
            if (s < 0) {
                (*lost)++;
                m &= ~(1u << k);
            } else {
                cell[k] = (uint32_t)s;
            }
        } else if (comp[k] >= (uint64_t)A.n_cells) {
            m &= ~(1u << k);  // (beyond the tracked extrema: cannot be; never an address)
            if (!CLAIM) (*lost)++;
        } else {
            cell[k] = (uint32_t)comp[k];
        }
    }
    *p0_out = p0;
    return m;
}

template <bool LDS, bool HASH>
__global__ __launch_bounds__(kRuThreads) void k_ru_accum(const RuArgs A) {
    extern __shared__ int64_t ru_lds[];  // <LDS>: [fields][n_cells]
    __shared__ long long red[3 * (kRuThreads / 64)];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int fields = 1 + 4 * A.n_vals;
    const int64_t n_cells = A.n_cells;
    int64_t *const G = A.cells;
    if (LDS) {
        for (int64_t i = tid; i < (int64_t)fields * n_cells; i += kRuThreads) ru_lds[i] = ru_is_max((int)(i / n_cells)) ? INT64_MIN : 0;
        __syncthreads();
    }
    long long matched = 0, no_time = 0, full = 0;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        int64_t p0;
        uint32_t cell[kRuRows];
        const uint32_t m = ru_rows<HASH, true>(A, tile, tid, &p0, cell, &matched, &no_time, &full);
        const unsigned long long act = __ballot(m != 0);
        if (act == 0) continue;  // (the whole wave filtered out; no barrier inside the loop)

        // ---- do the wave's active rows all fall into ONE cell?
        uint32_t c_first = 0;
        bool lane_same = true;
#pragma unroll
        for (int k = kRuRows - 1; k >= 0; k--)
            if ((m >> k) & 1u) c_first = cell[k];
#pragma unroll
        for (int k = 0; k < kRuRows; k++)
            if (((m >> k) & 1u) && cell[k] != c_first) lane_same = false;
        const int leader = __ffsll(act) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)c_first, leader, 64);
        const bool uni = A.merge != 0 && __all(m == 0 || (lane_same && c_first == c0));

        if (uni) {
            const int64_t cnt = ru_wave_sum((int64_t)__popc(m));
            if (lane == leader) ru_add<LDS>(G, ru_lds, c0, cnt);
        } else {
            int64_t run = 0;
            uint32_t rc = 0;
#pragma unroll
            for (int k = 0; k < kRuRows; k++) {
                if (!((m >> k) & 1u)) continue;
                if (run > 0 && cell[k] != rc) {
                    ru_add<LDS>(G, ru_lds, rc, run);
                    run = 0;
                }
                rc = cell[k];
                run++;
            }
            if (run > 0) ru_add<LDS>(G, ru_lds, rc, run);
        }

        for (int a = 0; a < A.n_vals; a++) {
            int64_t v[kRuRows];
            const uint32_t pop = ru_load(A.vals[a], p0, m, v);
            if (uni) {
                int64_t n = 0, mx = INT64_MIN, nm = INT64_MIN;
                uint64_t s = 0;
#pragma unroll
                for (int k = 0; k < kRuRows; k++)
                    if ((pop >> k) & 1u) {
                        n++;
                        s += (uint64_t)v[k];
                        mx = v[k] > mx ? v[k] : mx;
                        nm = ~v[k] > nm ? ~v[k] : nm;
                    }
                n = ru_wave_sum(n);
                s = (uint64_t)ru_wave_sum((int64_t)s);
                mx = ru_wave_max(mx);
                nm = ru_wave_max(nm);
                if (lane == leader && n > 0) ru_put<LDS>(G, ru_lds, n_cells, a, c0, n, s, mx, nm);
            } else {
                int64_t n = 0, mx = INT64_MIN, nm = INT64_MIN;
                uint64_t s = 0;
                uint32_t rc = 0;
                bool have = false;
#pragma unroll
                for (int k = 0; k < kRuRows; k++) {
                    if (!((m >> k) & 1u)) continue;
                    if (have && cell[k] != rc) {
                        if (n > 0) ru_put<LDS>(G, ru_lds, n_cells, a, rc, n, s, mx, nm);
                        n = 0, s = 0, mx = INT64_MIN, nm = INT64_MIN;
                    }
                    rc = cell[k];
                    have = true;
                    if ((pop >> k) & 1u) {
                        n++;
                        s += (uint64_t)v[k];
                        mx = v[k] > mx ? v[k] : mx;
                        nm = ~v[k] > nm ? ~v[k] : nm;
                    }
                }
                if (n > 0) ru_put<LDS>(G, ru_lds, n_cells, a, rc, n, s, mx, nm);
            }
        }
    }

    // ---- <LDS>: the workgroup's occupied cells leave with agent-scope atomics
    if (LDS) {
        __syncthreads();
        for (int64_t c = tid; c < n_cells; c += kRuThreads) {
            if (ru_lds[c] <= 0) continue;
            for (int f = 0; f < fields; f++) {
                const int64_t v = ru_lds[(int64_t)f * n_cells + c];
                if (ru_is_max(f)) {
                    if (v != INT64_MIN) __hip_atomic_fetch_max(G + (int64_t)f * n_cells + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (v != 0) {
                    __hip_atomic_fetch_add(G + (int64_t)f * n_cells + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }

    // ---- the counters: one atomic each per workgroup
    matched = ru_wave_sum(matched);
    no_time = ru_wave_sum(no_time);
    full = ru_wave_sum(full);
    if (lane == 0) {
        red[3 * (tid >> 6)] = matched;
        red[3 * (tid >> 6) + 1] = no_time;
        red[3 * (tid >> 6) + 2] = full;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kRuThreads / 64; k++) {
            matched += red[3 * k];
            no_time += red[3 * k + 1];
            full += red[3 * k + 2];
        }
        if (matched) __hip_atomic_fetch_add(A.ctr, matched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (no_time) __hip_atomic_fetch_add(A.ctr + 1, no_time, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (full) __hip_atomic_fetch_add(A.ctr + 2, full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- every field of every cell at its start value
__global__ __launch_bounds__(kRuThreads) void k_ru_init(int64_t *cells, int64_t n_cells, int fields) {
    const int64_t i = (int64_t)blockIdx.x * kRuThreads + threadIdx.x;
    if (i >= n_cells) return;
    for (int f = 0; f < fields; f++) cells[(int64_t)f * n_cells + i] = ru_is_max(f) ? INT64_MIN : 0;
}

// ---- hash: the composites of the claimed slots
__global__ __launch_bounds__(kRuThreads) void k_ru_slot_keys(const uint64_t *__restrict__ hkeys, const uint32_t *__restrict__ slots, int64_t n,
                                                             uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kRuThreads + threadIdx.x;
    if (i < n) out[i] = hkeys[slots[i]];
}

// ---- percentiles: the sort keys of one aggregated column.  The front end is k_ru_accum's; a matching row whose value is
// populated is an item.  Items are compacted: per row slot a wave ballot ranks the lanes, the workgroup's four wave totals meet in
// LDS and ONE cursor atomic per workgroup and tile reserves the tile's range -- the order of items before the sort is free, the
// keys alone determine the result.  The buffers hold M items: an item at or beyond M is dropped and counted, as is a row whose
// composite is not in the table (neither can be; neither becomes an address).
struct RuPct {
    RuCol val;
    uint64_t lo, vmask;  // key = cell << vbits | ((v - lo) & vmask)
    int32_t vbits;
    void *keys;          // [M] uint32 (V = 32) or uint64; <pairs>: (v - lo) & vmask alone
    uint32_t *cells;     // <pairs>: [M] the payload
    long long *cursor;   // zeroed
    long long *dropped;
    int64_t M;
};

template <bool HASH, int V>
__global__ __launch_bounds__(kRuThreads) void k_ru_pct_keys(const RuArgs A, const RuPct P) {
    __shared__ int wsum[kRuThreads / 64];
    __shared__ long long sbase;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long matched = 0, no_time = 0, dropped = 0;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {  // (uniform: every wave reaches both barriers)
        int64_t p0;
        uint32_t cell[kRuRows];
        const uint32_t m = ru_rows<HASH, false>(A, tile, tid, &p0, cell, &matched, &no_time, &dropped);
        int64_t v[kRuRows];
        const uint32_t pop = ru_load(P.val, p0, m, v);
        int rank[kRuRows], wtotal = 0;
#pragma unroll
        for (int k = 0; k < kRuRows; k++) {
            const unsigned long long b = __ballot((pop >> k) & 1u);
            rank[k] = wtotal + __popcll(b & below);
            wtotal += __popcll(b);
        }
        if (lane == 0) wsum[wave] = wtotal;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kRuThreads / 64; w++) {
            const int s = wsum[w];
            before += w < wave ? s : 0;
            total += s;
        }
        if (tid == 0) sbase = total > 0 ? __hip_atomic_fetch_add(P.cursor, (long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        __syncthreads();
        const int64_t base = (int64_t)sbase + before;
#pragma unroll
        for (int k = 0; k < kRuRows; k++) {
            if (!((pop >> k) & 1u)) continue;
            const int64_t at = base + rank[k];
            if (at < 0 || at >= P.M) {
                dropped++;
                continue;
            }
            const uint64_t d = ((uint64_t)v[k] - P.lo) & P.vmask;
            const uint64_t major = P.vbits < 64 ? (uint64_t)cell[k] << P.vbits : 0;  // (64 value bits: one cell, cell 0)
            if (V == 32) {
                ((uint32_t *)P.keys)[at] = (uint32_t)(major | d);
            } else if (V == 64) {
                ((uint64_t *)P.keys)[at] = major | d;
            } else {
                ((uint64_t *)P.keys)[at] = d;
                P.cells[at] = cell[k];
            }
        }
    }
    dropped = ru_wave_sum(dropped);
    if (lane == 0 && dropped) __hip_atomic_fetch_add(P.dropped, dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- percentiles: the pick.  A lane per (output row g, percentile): c the g-th occupied cell of the order phase, n = n[c] its
// populated values, off = offsets[c] where they start in the sorted array; the value of 1-based rank (k * n + 99) / 100, as
// lo + (key & vmask) with wrapping unsigned addition, into [percentile][G].  n = 0: 0 (the emit leaves it unpopulated).
struct RuPick {
    const uint32_t *cell;  // [G]
    const int64_t *n;      // [n_cells] the column's n field
    const int64_t *off;    // [n_cells] its exclusive sum
    const void *sorted;    // [M] uint32 / uint64 (wide)
    int64_t *out;          // [np][G]
    long long *dropped;
    int64_t G, M;
    uint64_t lo, vmask;
    int32_t np, wide;
    int32_t k[kRuMaxPcts];
};

__global__ __launch_bounds__(kRuThreads) void k_ru_pct_pick(const RuPick P) {
    const int64_t i = (int64_t)blockIdx.x * kRuThreads + threadIdx.x;
    if (i >= P.G * P.np) return;
    const int p = (int)(i / P.G);
    const int64_t g = i - (int64_t)p * P.G;
    const uint32_t c = P.cell[g];
    const int64_t n = P.n[c];
    int64_t r = 0;
    if (n > 0) {
        const int64_t at = P.off[c] + ((int64_t)P.k[p] * n + 99) / 100 - 1;
        if (at < 0 || at >= P.M) {
            __hip_atomic_fetch_add(P.dropped, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (cannot be; never an address)
        } else {
            const uint64_t key = P.wide ? ((const uint64_t *)P.sorted)[at] : (uint64_t)((const uint32_t *)P.sorted)[at];
            r = (int64_t)(P.lo + (key & P.vmask));
        }
    }
    P.out[i] = r;
}

struct RuOccupied {
    __host__ __device__ __forceinline__ bool operator()(const int64_t &count) const { return count > 0; }
};
struct RuClaimed {
    __host__ __device__ __forceinline__ bool operator()(const uint64_t &key) const { return key != kHashEmpty; }
};

// ---- emit
enum RuKind { kRuTime = 0, kRuGroup = 1, kRuField = 2, kRuFieldIfN = 3, kRuMinIfN = 4, kRuArrayIfN = 5 };

struct RuEmit {
    const uint32_t *cell;   // [G] the cell / slot of output row i, in key order
    const uint64_t *comp;   // [G] its composite; nullptr: the cell is the composite (direct)
    const int64_t *cells;
    int64_t G, block_rows, stride_rows, n_out;
    int32_t kind, missing;
    uint64_t kstride, radix;  // a key column: digit = composite / kstride % radix
    int64_t lo, bucket;
    int64_t f_off, n_off;  // a field: its offset in `cells`, and that of the column's n
    const int64_t *arr;    // an array by output row (a percentile): [G]
    void *out;             // store pass
    uint32_t *out_valid;   // ... nullptr: the column has no bitmap
    int64_t out_base;
    long long *acc;        // range pass: min, max, populated count
};

__device__ __forceinline__ bool ru_value(const RuEmit &E, int64_t i, int64_t *v) {
    const uint32_t cell = E.cell[i];
    if (E.kind <= kRuGroup) {
        const uint64_t comp = E.comp != nullptr ? E.comp[i] : (uint64_t)cell;
        const uint64_t digit = comp / E.kstride % E.radix;
        if (E.kind == kRuTime) {
            *v = (E.lo + (int64_t)digit) * E.bucket;
            return true;
        }
        if (E.missing && digit == 0) return false;
        *v = (int64_t)((uint64_t)E.lo + digit - (uint64_t)E.missing);
        return true;
    }
    if (E.kind != kRuField && E.cells[E.n_off + cell] <= 0) return false;
    if (E.kind == kRuArrayIfN) {
        *v = E.arr[i];
        return true;
    }
    const int64_t f = E.cells[E.f_off + cell];
    *v = E.kind == kRuMinIfN ? ~f : f;
    return true;
}

template <bool STORE, int W>
__global__ __launch_bounds__(kRuThreads) void k_ru_emit(const RuEmit E) {
    __shared__ long long red[3 * (kRuThreads / 64)];
    const int tid = (int)threadIdx.x;
    const int64_t p0 = ((int64_t)blockIdx.x * kRuThreads + tid) * kRuRows;
    const bool active = p0 < E.n_out;  // (n_out is a multiple of 32: the 8 lanes of a validity word are active together)
    int64_t v[kRuRows] = {0, 0, 0, 0};
    uint32_t pop = 0;
    if (active) {
#pragma unroll
        for (int k = 0; k < kRuRows; k++) {
            const int64_t p = p0 + k, j = p / E.stride_rows, r = p - j * E.stride_rows, i = j * E.block_rows + r;
            if (r < E.block_rows && i < E.G && ru_value(E, i, &v[k])) pop |= 1u << k;
        }
    }
    if (STORE) {
        if (active) {
            uint64_t e[kRuRows];
#pragma unroll
            for (int k = 0; k < kRuRows; k++) e[k] = (pop >> k) & 1u ? (uint64_t)v[k] - (uint64_t)E.out_base : 0;
            if (W == 8) {
                ulonglong2 *o = (ulonglong2 *)E.out + (p0 >> 1);
                o[0] = make_ulonglong2(e[0], e[1]);
                o[1] = make_ulonglong2(e[2], e[3]);
            } else if (W == 4) {
                ((uint4 *)E.out)[p0 >> 2] = make_uint4((uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]);
            } else if (W == 2) {
                ((uint2 *)E.out)[p0 >> 2] = make_uint2(((uint32_t)e[0] & 0xFFFFu) | ((uint32_t)e[1] << 16), ((uint32_t)e[2] & 0xFFFFu) | ((uint32_t)e[3] << 16));
            } else {
                ((uint32_t *)E.out)[p0 >> 2] =
                    ((uint32_t)e[0] & 0xFFu) | (((uint32_t)e[1] & 0xFFu) << 8) | (((uint32_t)e[2] & 0xFFu) << 16) | ((uint32_t)e[3] << 24);
            }
        }
        if (E.out_valid != nullptr) {  // (uniform; every lane takes part in the shuffles)
            uint32_t word = pop << (4 * (tid & 7));
            word |= (uint32_t)__shfl_xor((int)word, 1, 64);
            word |= (uint32_t)__shfl_xor((int)word, 2, 64);
            word |= (uint32_t)__shfl_xor((int)word, 4, 64);
            if (active && (tid & 7) == 0) E.out_valid[p0 >> 5] = word;
        }
    } else {
        long long mn = INT64_MAX, mx = INT64_MIN, cnt = 0;
#pragma unroll
        for (int k = 0; k < kRuRows; k++)
            if ((pop >> k) & 1u) {
                mn = v[k] < mn ? v[k] : mn;
                mx = v[k] > mx ? v[k] : mx;
                cnt++;
            }
        for (int d = 32; d > 0; d >>= 1) {
            const long long omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64), oc = __shfl_xor(cnt, d, 64);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            cnt += oc;
        }
        if ((tid & 63) == 0) {
            red[3 * (tid >> 6)] = mn;
            red[3 * (tid >> 6) + 1] = mx;
            red[3 * (tid >> 6) + 2] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < kRuThreads / 64; k++) {
                mn = red[3 * k] < mn ? red[3 * k] : mn;
                mx = red[3 * k + 1] > mx ? red[3 * k + 1] : mx;
                cnt += red[3 * k + 2];
            }
            if (cnt > 0) {  // one set of atomics per workgroup
                __hip_atomic_fetch_min(E.acc, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(E.acc + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(E.acc + 2, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

namespace {

constexpr const char *kWho = "sybl_table_rollup";

// an aggregated column and what is asked of it
struct AggPlan {
    Column *c = nullptr;
    bool want[4] = {false, false, false, false};  // n, sum, min, max
    std::vector<int> pcts;                        // the k of its p<k> tokens, ascending
    // percentiles: what the host plan decided (variant 0: no populated value, nothing to sort) and where the values land
    int variant = kRuPctNone, cbits = 0, vbits = 0;
    int64_t M = 0;
    int64_t *picked = nullptr;  // [pcts][G]
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// an output column: where its values come from
struct OutCol {
    Column *n = nullptr;
    bool is_key = false;  // a group column: the source's (width, base)
    RuEmit E{};
};

bool parse_ops(const char *ops, bool want[4], std::vector<int> *pcts) {
    static const char *const names[4] = {"n", "sum", "min", "max"};
    if (!ops || !ops[0]) return false;
    const char *p = ops;
    for (;;) {
        const char *e = strchr(p, ',');
        const size_t len = e ? (size_t)(e - p) : strlen(p);
        int hit = -1;
        for (int k = 0; k < 4; k++)
            if (strlen(names[k]) == len && !strncmp(names[k], p, len)) hit = k;
        if (hit >= 0) {
            if (want[hit]) return false;
            want[hit] = true;
        } else {
            const int k = ru_pct_token(p, len);
            if (k == 0 || std::find(pcts->begin(), pcts->end(), k) != pcts->end() || pcts->size() >= (size_t)kRuMaxPcts) return false;
            pcts->push_back(k);
        }
        if (!e) break;
        p = e + 1;
    }
    std::sort(pcts->begin(), pcts->end());
    return true;
}

RuCol col_view(const Column *c, bool missing) {
    return RuCol{c->d_data, c->d_data ? c->d_valid : nullptr, c->vbase, c->elem, missing ? 1 : 0};
}

// the bytes one pass over a column reads, from the shapes
int64_t col_bytes(const Column *c, int64_t N) { return (c->d_data ? N * (int64_t)c->elem : 0) + (c->d_valid ? (N + 7) / 8 : 0); }

void launch_accum(int path, const RuArgs &A, unsigned grid, size_t lds, hipStream_t st) {
    const dim3 g(grid), b(kRuThreads);
    if (path == kRuPathLds) hipLaunchKernelGGL((k_ru_accum<true, false>), g, b, lds, st, A);
    else if (path == kRuPathGlobal) hipLaunchKernelGGL((k_ru_accum<false, false>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_ru_accum<false, true>), g, b, 0, st, A);
}

void launch_emit(bool store, int width, const RuEmit &E, hipStream_t st) {
    const dim3 g(grid_for(E.n_out / kRuRows, kRuThreads)), b(kRuThreads);
    if (!store) hipLaunchKernelGGL((k_ru_emit<false, 0>), g, b, 0, st, E);
    else by_width(width, [&](auto W) { hipLaunchKernelGGL((k_ru_emit<true, decltype(W)::value>), g, b, 0, st, E); });
}

int run(Table *t, const sybl_rollup_desc *d, int64_t block_rows, Table *o, sybl_rollup_stats *S, sybl_rollup_pct_stats *PS) {
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;

    // ---- the arguments: everything that can be refused is refused before anything is made
    if (d->n_filters < 0 || (d->n_filters > 0 && !d->filters)) return fail(SYBL_E_INVAL, "%s: bad filter list", kWho);
    if (d->n_groups < 0 || (d->n_groups > 0 && !d->groups)) return fail(SYBL_E_INVAL, "%s: bad group list", kWho);
    if (d->n_aggs < 0 || (d->n_aggs > 0 && !d->aggs)) return fail(SYBL_E_INVAL, "%s: bad aggregation list", kWho);
    if (d->n_groups > kRuMaxKeys - 1) return fail(SYBL_E_INVAL, "%s: %d group columns; the limit is %d", kWho, (int)d->n_groups, kRuMaxKeys - 1);
    if (d->n_aggs > kRuMaxAggs) return fail(SYBL_E_INVAL, "%s: %d aggregated columns; the limit is %d", kWho, (int)d->n_aggs, kRuMaxAggs);
    if (d->time_bucket < 0) return fail(SYBL_E_INVAL, "%s: time_bucket %lld is negative", kWho, (long long)d->time_bucket);
    std::vector<std::string> out_names;
    auto claim = [&](const std::string &name) {
        if (std::find(out_names.begin(), out_names.end(), name) != out_names.end()) return false;
        out_names.push_back(name);
        return true;
    };
    Column *tc = nullptr;
    if (d->time_bucket > 0) {
        const char *name = d->time_col && d->time_col[0] ? d->time_col : "time";
        tc = t->find(name);
        if (!tc) return fail(SYBL_E_INVAL, "%s: unknown time column '%s'", kWho, name);
        if (tc->type != SYBL_INT_VAL) return fail(SYBL_E_INVAL, "%s: time column '%s' is a %s column; buckets are cut from an int column", kWho, name, type_name(tc->type));
        claim(tc->name);
    }
    std::vector<Column *> gcols;
    for (int i = 0; i < d->n_groups; i++) {
        const char *name = d->groups[i];
        Column *c = name ? t->find(name) : nullptr;
        if (!c) return fail(SYBL_E_INVAL, "%s: unknown group column '%s'", kWho, name ? name : "(null)");
        if (c->type == SYBL_SET_VAL) return fail(SYBL_E_INVAL, "%s: group column '%s' is a set column; keys are int or str columns", kWho, name);
        if (!claim(c->name)) return fail(SYBL_E_INVAL, "%s: column '%s' is named twice in the key", kWho, name);
        gcols.push_back(c);
    }
    const std::string count_name = d->count_name && d->count_name[0] ? d->count_name : "count";
    if (!claim(count_name)) return fail(SYBL_E_INVAL, "%s: column '%s': the output already holds a column of that name", kWho, count_name.c_str());
    std::vector<AggPlan> aggs((size_t)d->n_aggs);
    static const char *const suffix[4] = {"_n", "_sum", "_min", "_max"};
    for (int i = 0; i < d->n_aggs; i++) {
        const char *name = d->aggs[i].col;
        Column *c = name ? t->find(name) : nullptr;
        if (!c) return fail(SYBL_E_INVAL, "%s: unknown aggregated column '%s'", kWho, name ? name : "(null)");
        if (c->type != SYBL_INT_VAL) return fail(SYBL_E_INVAL, "%s: aggregated column '%s' is a %s column; n, sum, min and max are taken of int columns", kWho, name, type_name(c->type));
        aggs[(size_t)i].c = c;
        if (!parse_ops(d->aggs[i].ops, aggs[(size_t)i].want, &aggs[(size_t)i].pcts))
            return fail(SYBL_E_INVAL, "%s: column '%s': ops '%s' are not a non-empty subset of n, sum, min, max and at most %d of p1 .. p99", kWho, name,
                        d->aggs[i].ops ? d->aggs[i].ops : "(null)", kRuMaxPcts);
        for (int k = 0; k < 4; k++)
            if (aggs[(size_t)i].want[k] && !claim(c->name + suffix[k]))
                return fail(SYBL_E_INVAL, "%s: column '%s%s': the output already holds a column of that name", kWho, name, suffix[k]);
        for (int k : aggs[(size_t)i].pcts)
            if (!claim(c->name + "_p" + std::to_string(k)))
                return fail(SYBL_E_INVAL, "%s: column '%s_p%d': the output already holds a column of that name", kWho, name, k);
        if (!aggs[(size_t)i].pcts.empty()) {
            PS->columns++;
            PS->percentiles += (int32_t)aggs[(size_t)i].pcts.size();
        }
    }
    int pct_force = kRuPctNone;
    if (const char *e = env("SYBL_ROLLUP_PCT")) {
        pct_force = !strcmp(e, "32") ? kRuPct32 : !strcmp(e, "64") ? kRuPct64 : !strcmp(e, "pairs") ? kRuPctPairs : -1;
        if (pct_force < 0) return fail(SYBL_E_INVAL, "%s: SYBL_ROLLUP_PCT=%s is none of 32, 64, pairs", kWho, e);
    }
    int force = kRuForceNone;
    if (const char *e = env("SYBL_ROLLUP_PATH")) {
        force = !strcmp(e, "direct") ? kRuForceDirect : !strcmp(e, "global") ? kRuForceGlobal : !strcmp(e, "hash") ? kRuForceHash : -1;
        if (force < 0) return fail(SYBL_E_INVAL, "%s: SYBL_ROLLUP_PATH=%s is none of direct, global, hash", kWho, e);
    }
    int64_t asked_slots = 0;
    if (const char *e = env("SYBL_ROLLUP_SLOTS")) asked_slots = std::max<long long>(0, atoll(e));
    const char *merge_env = env("SYBL_ROLLUP_MERGE");
    const bool merge = !(merge_env && !strcmp(merge_env, "0"));
    if ((rc = load_sync_all(ctx))) return rc;
    if ((rc = table_ensure_stats(t))) return rc;  // (the key columns' extrema; the table's version does not move)

    // ---- filters, lowered by the planner
    struct FilterPlan {
        Query q;
        ~FilterPlan() {
            for (void *p : q.d_idmasks) (void)hipFree(p);
        }
    };
    auto fp = std::make_unique<FilterPlan>();
    fp->q.t = t;
    fp->q.ctx = ctx;
    if ((rc = plan_filter_slots(t, d->filters, d->n_filters, &fp->q))) return rc;
    ScanPlan &plan = fp->q.plan;
    const int n_slots = plan.n_slots;
    if (n_slots > kRuMaxFilterCols) return fail(SYBL_E_INVAL, "%s: filters on %d distinct columns; the limit is %d", kWho, n_slots, kRuMaxFilterCols);

    // ---- the output's columns.  New columns: INT, no IntInfo, no dictionary; canonical until the range is known
    o->compact_mode = t->compact_mode;
    std::vector<OutCol> outs;
    auto add_col = [&](const std::string &name, const Column *like) {
        auto n = std::make_unique<Column>();
        n->name = name;
        if (like) {  // a group column, by digest's rules
            n->type = like->type;
            n->elem = like->elem;
            n->vbase = like->vbase;
            n->info_given = like->info_given;
            n->info_min = like->info_min;
            n->info_max = like->info_max;
            n->dict = like->dict;  // id for id
            n->dict_ix = like->dict_ix;
        } else {
            n->type = SYBL_INT_VAL;
            n->elem = n->canon();
            if (o->compact_mode) fit_storage(n->canon(), false, 0, 0, &n->elem, &n->vbase);
        }
        OutCol oc;
        oc.n = n.get();
        oc.is_key = like != nullptr;
        o->col_ix[n->name] = (int)o->cols.size();
        o->cols.push_back(std::move(n));
        outs.push_back(oc);
        return outs.size() - 1;
    };
    const int n_keys = (tc ? 1 : 0) + (int)gcols.size(), n_vals = (int)aggs.size(), fields = 1 + 4 * n_vals;
    if (tc) outs[add_col(tc->name, nullptr)].E.kind = kRuTime;
    for (Column *c : gcols) outs[add_col(c->name, c)].E.kind = kRuGroup;
    const size_t count_at = add_col(count_name, nullptr);
    outs[count_at].E.kind = kRuField;
    std::vector<std::pair<size_t, int>> pct_outs;  // (output column, aggregated column): the percentiles, in output order
    for (int a = 0; a < n_vals; a++) {
        for (int k = 0; k < 4; k++) {
            if (!aggs[(size_t)a].want[k]) continue;
            RuEmit &E = outs[add_col(aggs[(size_t)a].c->name + suffix[k], nullptr)].E;
            // want: n, sum, min, max; fields: n, sum, max, ~min
            E.kind = k == 0 ? kRuField : k == 2 ? kRuMinIfN : kRuFieldIfN;
            E.f_off = 1 + 4 * a + (k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 3 : 2);  // (a field number until the cells are sized)
            E.n_off = 1 + 4 * a;
        }
        for (int k : aggs[(size_t)a].pcts) {  // after the column's four, ascending k
            const size_t at = add_col(aggs[(size_t)a].c->name + "_p" + std::to_string(k), nullptr);
            outs[at].E.kind = kRuArrayIfN;
            outs[at].E.n_off = 1 + 4 * a;
            pct_outs.emplace_back(at, a);
        }
    }

    // ---- the source rows: the live blocks, a tile = 1024 rows of one block
    std::vector<RowBlk> blk;
    std::vector<Segment> runs;
    int64_t N = 0, n_tiles = 0, row_hi = 0;
    for (const Segment &b : t->blocks) {
        if (b.n <= 0) continue;  // (a dead block, sybl_table_refresh)
        blk.push_back(RowBlk{b.start, b.n, n_tiles});
        n_tiles += (round_up(b.n, 32) + kRuTileRows - 1) / kRuTileRows;
        N += b.n;
        row_hi = std::max(row_hi, b.start + b.n);
        if (!runs.empty() && runs.back().start + runs.back().n == b.start) runs.back().n += b.n;
        else runs.push_back(Segment{b.start, b.n});
    }
    S->rows_in = N;
    S->fields = fields;
    if (blk.size() > (size_t)INT32_MAX) return fail(SYBL_E_INVAL, "%s: more blocks than a launch counts", kWho);

    // ---- the host plan: digits, composite, path
    RuArgs A{};
    ru_u128 radix[kRuMaxKeys];
    int kk = 0;
    if (tc) {
        int64_t qlo = 0, qhi = 0;
        const bool any = tc->n_pop > 0;
        if (any) ru_bucket_range(tc->exact_min, tc->exact_max, d->time_bucket, &qlo, &qhi);
        radix[kk] = ru_radix(any, qlo, qhi, false);
        A.keys[kk] = col_view(tc, false);
        A.key_lo[kk] = qlo;
        kk++;
    }
    for (Column *c : gcols) {
        const bool any = c->n_pop > 0, missing = c->d_valid != nullptr || c->d_data == nullptr;
        radix[kk] = ru_radix(any, any ? c->exact_min : 0, any ? c->exact_max : 0, missing);
        A.keys[kk] = col_view(c, missing);
        A.key_lo[kk] = any ? c->exact_min : 0;
        kk++;
    }
    ru_u128 product = 1;
    if (!ru_composite(radix, n_keys, A.key_stride, &product))
        return fail(SYBL_E_INVAL, "%s: the key columns span more than 2^62 combinations; the composite key does not hold them", kWho);
    if (N == 0 || fp->q.never_matches) return SYBL_OK;  // (the columns and no blocks; no kernel runs)
    const int path = ru_choose_path(product, N, fields, force);
    if (path == kRuPathNone)
        return fail(SYBL_E_INVAL, "%s: SYBL_ROLLUP_PATH=%s needs a cell per key combination; there are more than 2^27", kWho, env("SYBL_ROLLUP_PATH"));
    const int64_t n_cells = path == kRuPathHash ? ru_slots(N, product, asked_slots) : (int64_t)product;
    S->path = path;
    S->cells_or_slots = n_cells;
    for (int a = 0; a < n_vals; a++) A.vals[a] = col_view(aggs[(size_t)a].c, false);
    // percentiles: the sort key of every column that has a populated value -- cell above, v - lo below -- and its variant
    for (AggPlan &ap : aggs) {
        if (ap.pcts.empty() || ap.c->n_pop <= 0) continue;  // (no populated value: nothing to sort, every percentile unpopulated)
        ap.cbits = ru_pct_cbits(n_cells);
        ap.vbits = ru_pct_vbits(ap.c->exact_min, ap.c->exact_max);
        ap.variant = ru_pct_variant(ap.cbits, ap.vbits, pct_force);
        if (ap.variant == kRuPctNone)
            return fail(SYBL_E_INVAL, "%s: SYBL_ROLLUP_PCT=%s holds fewer bits than the %d + %d of the cell and the values of column '%s'", kWho,
                        env("SYBL_ROLLUP_PCT"), ap.cbits, ap.vbits, ap.c->name.c_str());
    }

    GatherPool pool;
    hipEvent_t ev[5];
    RowBlk *d_blk = nullptr;
    // matched, rows_no_time, full, G; percentiles: items dropped, then per aggregated column its items M and its cursor
    constexpr int kCtrDropped = 4, kCtrM = 5, kCtrCursor = kCtrM + kRuMaxAggs, kCtrs = kCtrCursor + kRuMaxAggs;
    long long *d_ctr = nullptr;
    int64_t *cells = nullptr;
    uint64_t *hkeys = nullptr;
    uint32_t *bits = nullptr;
    if ((rc = pool.alloc(&d_blk, blk.size(), "rollup blocks"))) return rc;
    if ((rc = pool.alloc(&d_ctr, kCtrs, "rollup counters"))) return rc;
    if ((rc = pool.alloc(&cells, (size_t)fields * (size_t)n_cells, "rollup cells"))) return rc;
    if (path == kRuPathHash && (rc = pool.alloc(&hkeys, (size_t)n_cells, "rollup hash keys"))) return rc;
    if ((rc = host_to_device(ctx, d_blk, blk.data(), blk.size() * sizeof(RowBlk), "rollup blocks"))) return rc;
    SYBL_HIP(hipMemsetAsync(d_ctr, 0, kCtrs * sizeof(long long), st));

    // ---- filter
    if ((rc = pool.event(&ev[0], st))) return rc;
    if (n_slots > 0) {
        const int n_wg = ctx->n_cus > 0 ? ctx->n_cus : 256;
        const int64_t n_words = (row_hi + 31) >> 5;
        ScanPlan *d_plan = nullptr;
        Segment *d_segs = nullptr;
        int32_t *d_wgb = nullptr;
        std::vector<Segment> segs;
        std::vector<int32_t> wg_seg_begin;
        deal_tiles(runs, n_wg, segs, wg_seg_begin);
        if ((rc = pool.alloc(&bits, (size_t)n_words, "rollup bitmap"))) return rc;
        if ((rc = pool.alloc(&d_plan, 1, "rollup filter plan"))) return rc;
        if ((rc = pool.alloc(&d_segs, segs.size(), "rollup segments"))) return rc;
        if ((rc = pool.alloc(&d_wgb, wg_seg_begin.size(), "rollup segments"))) return rc;
        if ((rc = host_to_device(ctx, d_segs, segs.data(), segs.size() * sizeof(Segment), "rollup segments"))) return rc;
        if ((rc = host_to_device(ctx, d_wgb, wg_seg_begin.data(), wg_seg_begin.size() * sizeof(int32_t), "rollup segments"))) return rc;
        plan.segs = d_segs;
        plan.wg_seg_begin = d_wgb;
        static_assert(sizeof(ScanPlan) % 4 == 0, "host_to_device copies whole words");
        if ((rc = host_to_device(ctx, d_plan, &plan, sizeof(ScanPlan), "rollup filter plan"))) return rc;
        if ((rc = pool.event(&ev[0], st))) return rc;
        SYBL_HIP(hipMemsetAsync(bits, 0, (size_t)n_words * 4, st));  // (zeroed: the padding to 32 rows and dead blocks read 0)
        hipError_t e = launch_prefilter(d_plan, n_slots, bits, n_wg, st);
        if (e != hipSuccess) return hip_fail(e, "k_prefilter");
        std::vector<const Column *> fcols;  // (a slot per distinct filter column)
        for (int i = 0; i < d->n_filters; i++) {
            const Column *c = d->filters[i].col ? t->find(d->filters[i].col) : nullptr;
            if (c && std::find(fcols.begin(), fcols.end(), c) == fcols.end()) fcols.push_back(c);
        }
        for (const Column *c : fcols)
            S->filter_bytes += c->type == SYBL_SET_VAL ? N * 8 + (int64_t)c->h_set_vals.size() * 4 + (c->d_valid ? (N + 7) / 8 : 0) : col_bytes(c, N);
        S->filter_bytes += 2 * n_words * 4;  // (the bitmap: zeroed, written)
        S->accumulate_bytes += n_words * 4;
    }

    // ---- accumulate
    if ((rc = pool.event(&ev[1], st))) return rc;
    hipLaunchKernelGGL(k_ru_init, dim3(grid_for(n_cells, kRuThreads)), dim3(kRuThreads), 0, st, cells, n_cells, fields);
    SYBL_HIP(hipGetLastError());
    if (hkeys) SYBL_HIP(hipMemsetAsync(hkeys, 0xFF, (size_t)n_cells * 8, st));  // (kHashEmpty)
    A.blk = d_blk;
    A.bits = bits;
    A.cells = cells;
    A.hkeys = hkeys;
    A.ctr = d_ctr;
    A.n_tiles = n_tiles;
    A.n_cells = n_cells;
    A.time_bucket = d->time_bucket;
    A.hmask = (uint32_t)(n_cells - 1);
    A.nb = (int32_t)blk.size();
    A.n_keys = n_keys;
    A.n_vals = n_vals;
    A.has_time = tc ? 1 : 0;
    A.merge = merge ? 1 : 0;
    const size_t lds = path == kRuPathLds ? (size_t)fields * (size_t)n_cells * 8 : 0;
    // (LDS body: as many workgroups per CU as its cells leave room for -- every one of them flushes its occupied cells)
    const int wg_per_cu = path == kRuPathLds ? (int)std::min<size_t>(kRuWgPerCu, std::max<size_t>(1, (size_t)(160 * 1024) / (lds + 1024))) : kRuWgPerCu;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)std::max(ctx->n_cus, 1) * wg_per_cu));
    if (lds > 0) SYBL_HIP(hipFuncSetAttribute((const void *)k_ru_accum<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    launch_accum(path, A, grid, lds, st);
    SYBL_HIP(hipGetLastError());
    if ((rc = pool.event(&ev[2], st))) return rc;
    for (int k = 0; k < n_keys; k++) S->accumulate_bytes += col_bytes(k == 0 && tc ? tc : gcols[(size_t)(k - (tc ? 1 : 0))], N);
    for (const AggPlan &a : aggs) S->accumulate_bytes += col_bytes(a.c, N);
    S->accumulate_bytes += (int64_t)fields * n_cells * 8 + (hkeys ? n_cells * 8 : 0);  // (the cells: written once)

    // ---- order: the occupied cells / claimed slots in ascending order, G behind the counters
    uint32_t *d_cell = nullptr, *d_cell2 = nullptr;
    uint64_t *d_comp = nullptr, *d_comp2 = nullptr;
    char *tmp = nullptr;
    size_t tmp_bytes = 0;
    if ((rc = pool.alloc(&d_cell, (size_t)n_cells, "rollup order"))) return rc;
    hipcub::CountingInputIterator<uint32_t> idx(0u);
    hipcub::TransformInputIterator<bool, RuOccupied, const int64_t *> occupied((const int64_t *)cells, RuOccupied());
    hipcub::TransformInputIterator<bool, RuClaimed, const uint64_t *> claimed((const uint64_t *)hkeys, RuClaimed());
    if (hkeys) SYBL_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, idx, claimed, d_cell, d_ctr + 3, (int)n_cells, st));
    else SYBL_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, idx, occupied, d_cell, d_ctr + 3, (int)n_cells, st));
    if ((rc = pool.alloc(&tmp, tmp_bytes, "rollup order"))) return rc;
    if (hkeys) SYBL_HIP(hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, idx, claimed, d_cell, d_ctr + 3, (int)n_cells, st));
    else SYBL_HIP(hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, idx, occupied, d_cell, d_ctr + 3, (int)n_cells, st));
    // percentiles: the items of every column to sort, M = the sum of its n field over the cells, travel with the same readback
    for (int a = 0; a < n_vals; a++) {
        if (aggs[(size_t)a].variant == kRuPctNone) continue;
        const int64_t *n_field = cells + (int64_t)(1 + 4 * a) * n_cells;
        size_t red_bytes = 0;
        char *red_tmp = nullptr;
        SYBL_HIP(hipcub::DeviceReduce::Sum(nullptr, red_bytes, n_field, d_ctr + kCtrM + a, (int)n_cells, st));
        if ((rc = pool.alloc(&red_tmp, red_bytes, "rollup percentile items"))) return rc;
        SYBL_HIP(hipcub::DeviceReduce::Sum(red_tmp, red_bytes, n_field, d_ctr + kCtrM + a, (int)n_cells, st));
    }
    long long ctr[kCtrCursor] = {0};
    SYBL_HIP(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));  // the one readback: the counters and G
    SYBL_HIP(hipStreamSynchronize(st));
    S->rows_matched = ctr[0];
    S->rows_no_time = ctr[1];
    if (ctr[2] > 0)
        return fail(SYBL_E_NOMEM, "%s: the hash table of %lld slots is full (%lld rows found no slot)", kWho, (long long)n_cells, ctr[2]);
    const int64_t G = ctr[3];
    S->order_bytes += n_cells * 8 + G * 4;
    if (G < 0 || G > n_cells) return fail(SYBL_E_STATE, "%s: %lld groups in %lld cells", kWho, (long long)G, (long long)n_cells);
    if (G > 0 && hkeys) {
        const int key_bits = ru_key_bits(product);
        if ((rc = pool.alloc(&d_cell2, (size_t)G, "rollup order"))) return rc;
        if ((rc = pool.alloc(&d_comp, (size_t)G, "rollup order"))) return rc;
        if ((rc = pool.alloc(&d_comp2, (size_t)G, "rollup order"))) return rc;
        hipLaunchKernelGGL(k_ru_slot_keys, dim3(grid_for(G, kRuThreads)), dim3(kRuThreads), 0, st, (const uint64_t *)hkeys, (const uint32_t *)d_cell, G, d_comp);
        SYBL_HIP(hipGetLastError());
        size_t sort_bytes = 0;
        char *sort_tmp = nullptr;
        SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_comp, d_comp2, d_cell, d_cell2, (int)G, 0, key_bits, st));
        if ((rc = pool.alloc(&sort_tmp, sort_bytes, "rollup sort"))) return rc;
        SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, d_comp, d_comp2, d_cell, d_cell2, (int)G, 0, key_bits, st));
        // (an LSD pass per 8 bits reads and writes every pair; the histogram pass reads the keys once more)
        S->order_bytes += G * 12 + (int64_t)((key_bits + 7) / 8) * 2 * G * 12 + G * 8;
    }
    if ((rc = pool.event(&ev[3], st))) return rc;
    S->groups = G;
    float f = 0;
    if (G == 0) {  // (nothing matched: the columns and no blocks)
        SYBL_HIP(hipEventSynchronize(ev[3]));
        SYBL_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
        S->filter_ms = f;
        SYBL_HIP(hipEventElapsedTime(&f, ev[1], ev[2]));
        S->accumulate_ms = f;
        SYBL_HIP(hipEventElapsedTime(&f, ev[2], ev[3]));
        S->order_ms = f;
        return SYBL_OK;
    }

    // ---- percentiles, once per aggregated column that has some: offsets, keys, sort, pick.  Every column uses the same buffers;
    // one sort serves all percentiles of a column.
    const uint32_t *out_cell = hkeys ? d_cell2 : d_cell;
    hipEvent_t ev_emit = ev[3];
    {
        size_t key_bytes = 0, pay_bytes = 0, work_bytes = 0;
        int64_t *d_off = nullptr;
        char *keys_a = nullptr, *keys_b = nullptr, *work = nullptr;
        uint32_t *pay_a = nullptr, *pay_b = nullptr;
        bool any = false;
        // what the hipcub calls below need, at their largest over the columns
        for (int a = 0; a < n_vals; a++) {
            AggPlan &ap = aggs[(size_t)a];
            if (ap.pcts.empty()) continue;
            if ((rc = pool.alloc(&ap.picked, ap.pcts.size() * (size_t)G, "rollup percentiles"))) return rc;
            ap.M = ap.variant == kRuPctNone ? 0 : ctr[kCtrM + a];
            if (ap.M < 0 || ap.M > N) return fail(SYBL_E_STATE, "%s: %lld values to sort among %lld rows", kWho, (long long)ap.M, (long long)N);
            if (ap.M > (int64_t)INT32_MAX)
                return fail(SYBL_E_INVAL, "%s: column '%s': %lld values to sort; the percentile sort takes at most 2^31 - 1", kWho, ap.c->name.c_str(), (long long)ap.M);
            if (ap.M == 0) continue;
            any = true;
            const int M = (int)ap.M, kbits = std::max(1, ap.cbits + ap.vbits);
            size_t need = 0;
            SYBL_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const int64_t *)nullptr, (int64_t *)nullptr, (int)n_cells, st));
            work_bytes = std::max(work_bytes, need);
            if (ap.variant == kRuPct32) {
                SYBL_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, M, 0, kbits, st));
                work_bytes = std::max(work_bytes, need);
            } else if (ap.variant == kRuPct64) {
                SYBL_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const uint64_t *)nullptr, (uint64_t *)nullptr, M, 0, kbits, st));
                work_bytes = std::max(work_bytes, need);
            } else {
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                                            (uint32_t *)nullptr, M, 0, std::max(1, ap.vbits), st));
                work_bytes = std::max(work_bytes, need);
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint64_t *)nullptr,
                                                            (uint64_t *)nullptr, M, 0, std::max(1, ap.cbits), st));
                work_bytes = std::max(work_bytes, need);
                pay_bytes = std::max(pay_bytes, (size_t)M * 4);
            }
            key_bytes = std::max(key_bytes, (size_t)M * (ap.variant == kRuPct32 ? 4 : 8));
        }
        if (any) {
            if ((rc = pool.alloc(&d_off, (size_t)n_cells, "rollup percentile offsets"))) return rc;
            if ((rc = pool.alloc(&keys_a, key_bytes, "rollup percentile keys"))) return rc;
            if ((rc = pool.alloc(&keys_b, key_bytes, "rollup percentile keys"))) return rc;
            if (pay_bytes > 0 && (rc = pool.alloc(&pay_a, pay_bytes / 4, "rollup percentile keys"))) return rc;
            if (pay_bytes > 0 && (rc = pool.alloc(&pay_b, pay_bytes / 4, "rollup percentile keys"))) return rc;
            if ((rc = pool.alloc(&work, work_bytes, "rollup percentile sort"))) return rc;
        }
        int64_t key_cols_bytes = bits ? ((row_hi + 31) >> 5) * 4 : 0;
        for (int k = 0; k < n_keys; k++) key_cols_bytes += col_bytes(k == 0 && tc ? tc : gcols[(size_t)(k - (tc ? 1 : 0))], N);
        for (int a = 0; a < n_vals; a++) {
            AggPlan &ap = aggs[(size_t)a];
            if (ap.pcts.empty()) continue;
            if (ap.M == 0) {  // (no value passed: every percentile is unpopulated, the emit reads none of them)
                SYBL_HIP(hipMemsetAsync(ap.picked, 0, ap.pcts.size() * (size_t)G * 8, st));
                continue;
            }
            const int M = (int)ap.M, kbits = std::max(1, ap.cbits + ap.vbits);
            const int64_t *n_field = cells + (int64_t)(1 + 4 * a) * n_cells;
            const int64_t item = ap.variant == kRuPct32 ? 4 : ap.variant == kRuPct64 ? 8 : 12;
            // -- offsets and keys
            if ((rc = pool.event(&ap.ev[0], st))) return rc;
            size_t need = work_bytes;
            SYBL_HIP(hipcub::DeviceScan::ExclusiveSum(work, need, n_field, d_off, (int)n_cells, st));
            RuPct P{};
            P.val = A.vals[a];
            P.lo = (uint64_t)ap.c->exact_min;
            P.vbits = ap.vbits;
            P.vmask = ap.vbits >= 64 ? ~0ull : (1ull << ap.vbits) - 1ull;
            P.keys = keys_a;
            P.cells = pay_a;
            P.cursor = d_ctr + kCtrCursor + a;
            P.dropped = d_ctr + kCtrDropped;
            P.M = ap.M;
            {
                const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)std::max(ctx->n_cus, 1) * kRuWgPerCu))), b(kRuThreads);
                const bool hash = hkeys != nullptr;
                if (ap.variant == kRuPct32) {
                    if (hash) hipLaunchKernelGGL((k_ru_pct_keys<true, 32>), g, b, 0, st, A, P);
                    else hipLaunchKernelGGL((k_ru_pct_keys<false, 32>), g, b, 0, st, A, P);
                } else if (ap.variant == kRuPct64) {
                    if (hash) hipLaunchKernelGGL((k_ru_pct_keys<true, 64>), g, b, 0, st, A, P);
                    else hipLaunchKernelGGL((k_ru_pct_keys<false, 64>), g, b, 0, st, A, P);
                } else {
                    if (hash) hipLaunchKernelGGL((k_ru_pct_keys<true, 0>), g, b, 0, st, A, P);
                    else hipLaunchKernelGGL((k_ru_pct_keys<false, 0>), g, b, 0, st, A, P);
                }
                SYBL_HIP(hipGetLastError());
            }
            if ((rc = pool.event(&ap.ev[1], st))) return rc;
            // -- sort: exactly the key's bits
            const void *sorted = keys_b;
            int64_t passes = (kbits + 7) / 8;
            need = work_bytes;
            if (ap.variant == kRuPct32) {
                SYBL_HIP(hipcub::DeviceRadixSort::SortKeys(work, need, (const uint32_t *)keys_a, (uint32_t *)keys_b, M, 0, kbits, st));
            } else if (ap.variant == kRuPct64) {
                SYBL_HIP(hipcub::DeviceRadixSort::SortKeys(work, need, (const uint64_t *)keys_a, (uint64_t *)keys_b, M, 0, kbits, st));
            } else {
                // by value with the cell as payload, then by cell carrying the value: the radix sort is STABLE, so within a cell the
                // values keep the ascending order of the first sort
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(work, need, (const uint64_t *)keys_a, (uint64_t *)keys_b, (const uint32_t *)pay_a, pay_b, M, 0,
                                                            std::max(1, ap.vbits), st));
                need = work_bytes;
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(work, need, (const uint32_t *)pay_b, pay_a, (const uint64_t *)keys_b, (uint64_t *)keys_a, M, 0,
                                                            std::max(1, ap.cbits), st));
                sorted = keys_a;
                passes = (std::max(1, ap.vbits) + 7) / 8 + (std::max(1, ap.cbits) + 7) / 8;
            }
            if ((rc = pool.event(&ap.ev[2], st))) return rc;
            // -- pick
            RuPick K{};
            K.cell = out_cell;
            K.n = n_field;
            K.off = d_off;
            K.sorted = sorted;
            K.out = ap.picked;
            K.dropped = d_ctr + kCtrDropped;
            K.G = G;
            K.M = ap.M;
            K.lo = P.lo;
            K.vmask = ap.variant == kRuPctPairs ? ~0ull : P.vmask;
            K.np = (int32_t)ap.pcts.size();
            K.wide = ap.variant == kRuPct32 ? 0 : 1;
            for (size_t k = 0; k < ap.pcts.size(); k++) K.k[k] = ap.pcts[k];
            hipLaunchKernelGGL(k_ru_pct_pick, dim3(grid_for(G * K.np, kRuThreads)), dim3(kRuThreads), 0, st, K);
            SYBL_HIP(hipGetLastError());
            if ((rc = pool.event(&ap.ev[3], st))) return rc;
            ev_emit = ap.ev[3];
            // -- the counts, and the bytes from the shapes
            PS->items += ap.M;
            PS->key_bits_max = std::max<int32_t>(PS->key_bits_max, ap.cbits + ap.vbits);
            (ap.variant == kRuPct32 ? PS->variant32 : ap.variant == kRuPct64 ? PS->variant64 : PS->variant_pairs)++;
            PS->keys_bytes += 2 * n_cells * 8 + key_cols_bytes + col_bytes(ap.c, N) + ap.M * item;
            // (an LSD pass per 8 bits reads and writes every item; the histogram pass reads the keys once more)
            PS->sort_bytes += passes * 2 * ap.M * item + ap.M * (item == 12 ? 12 : item);
            PS->pick_bytes += G * 4 + (int64_t)K.np * G * (8 + 8 + (K.wide ? 8 : 4) + 8);
        }
    }

    // ---- emit: the output's layout, block j at physical row j * stride
    const int64_t stride = round_up(block_rows, 32);
    const int64_t nb_out = (G + block_rows - 1) / block_rows;
    const int64_t last_n = G - (nb_out - 1) * block_rows;
    const int64_t phys_out = (nb_out - 1) * stride + last_n;
    const int64_t n_out = round_up(phys_out, 32);
    const size_t nc = outs.size();
    long long *d_acc = nullptr;
    if ((rc = pool.alloc(&d_acc, 3 * nc, "rollup extrema"))) return rc;
    std::vector<long long> h_acc(3 * nc, 0);
    for (size_t c = 0; c < nc; c++) h_acc[3 * c] = INT64_MAX, h_acc[3 * c + 1] = INT64_MIN;
    if ((rc = host_to_device(ctx, d_acc, h_acc.data(), h_acc.size() * sizeof(long long), "rollup extrema"))) return rc;
    {
        std::vector<size_t> seen((size_t)n_vals, 0);  // percentile output columns are in (column, ascending k) order
        for (const auto &po : pct_outs) outs[po.first].E.arr = aggs[(size_t)po.second].picked + (int64_t)(seen[(size_t)po.second]++) * G;
    }
    kk = 0;
    for (size_t c = 0; c < nc; c++) {
        RuEmit &E = outs[c].E;
        E.cell = out_cell;
        E.comp = hkeys ? d_comp2 : nullptr;
        E.cells = cells;
        E.G = G;
        E.block_rows = block_rows;
        E.stride_rows = stride;
        E.n_out = n_out;
        E.acc = d_acc + 3 * c;
        if (E.kind <= kRuGroup) {
            E.kstride = A.key_stride[kk];
            E.radix = (uint64_t)std::max<ru_u128>(radix[kk], 1);
            E.lo = A.key_lo[kk];
            E.bucket = d->time_bucket;
            E.missing = A.keys[kk].missing;
            kk++;
        } else {
            E.f_off *= n_cells;
            E.n_off *= n_cells;
        }
        launch_emit(false, 0, E, st);
        SYBL_HIP(hipGetLastError());
    }
    SYBL_HIP(hipMemcpyAsync(h_acc.data(), d_acc, h_acc.size() * sizeof(long long), hipMemcpyDeviceToHost, st));  // read back once
    long long pct_dropped = 0;  // (with the same wait)
    if (!pct_outs.empty()) SYBL_HIP(hipMemcpyAsync(&pct_dropped, d_ctr + kCtrDropped, sizeof(long long), hipMemcpyDeviceToHost, st));
    SYBL_HIP(hipStreamSynchronize(st));
    if (pct_dropped != 0)
        return fail(SYBL_E_STATE, "%s: internal error: %lld percentile items had no place in the sorted values", kWho, pct_dropped);
    std::vector<Column *> made;
    for (size_t c = 0; c < nc; c++) {
        OutCol &oc = outs[c];
        Column *n = oc.n;
        const int64_t populated = h_acc[3 * c + 2];
        const bool missing = populated < G;
        if (!oc.is_key && o->compact_mode)
            fit_storage(n->canon(), populated > 0, populated > 0 ? h_acc[3 * c] : 0, populated > 0 ? h_acc[3 * c + 1] : 0, &n->elem, &n->vbase);
        n->has_missing = missing;
        // (the table has no rows yet: a bitmap reserved now starts zeroed, the store pass writes every word of the output)
        if ((rc = table_reserve(o, n, phys_out))) return rc;
        if (missing && (rc = valid_reserve(o, n, phys_out))) return rc;
        oc.E.out = n->d_data;
        oc.E.out_valid = missing ? n->d_valid : nullptr;
        oc.E.out_base = n->vbase;
        launch_emit(true, n->elem, oc.E, st);
        SYBL_HIP(hipGetLastError());
        S->emit_bytes += 2 * G * 12 + n_out * (int64_t)n->elem + (missing ? n_out / 8 : 0);
        made.push_back(n);
    }

    // ---- the blocks, and their statistics
    for (int64_t j = 0; j < nb_out; j++) o->blocks.push_back(Segment{j * stride, j + 1 < nb_out ? block_rows : last_n});
    o->phys_rows = phys_out;
    o->logical_rows = G;
    if ((rc = table_upload_blocks(o))) return rc;
    // (the ONE wait for the statistics of every block of every column)
    if ((rc = derived_block_stats(o, made, o->d_blocks, nb_out, pool, "rollup statistics", &ev[4]))) return rc;
    o->version++;
    S->blocks_out = nb_out;
    SYBL_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
    S->filter_ms = f;
    SYBL_HIP(hipEventElapsedTime(&f, ev[1], ev[2]));
    S->accumulate_ms = f;
    SYBL_HIP(hipEventElapsedTime(&f, ev[2], ev[3]));
    S->order_ms = f;
    SYBL_HIP(hipEventElapsedTime(&f, ev_emit, ev[4]));
    S->emit_ms = f;
    for (const AggPlan &ap : aggs) {
        if (ap.ev[3] == nullptr) continue;
        SYBL_HIP(hipEventElapsedTime(&f, ap.ev[0], ap.ev[1]));
        PS->keys_ms += f;
        SYBL_HIP(hipEventElapsedTime(&f, ap.ev[1], ap.ev[2]));
        PS->sort_ms += f;
        SYBL_HIP(hipEventElapsedTime(&f, ap.ev[2], ap.ev[3]));
        PS->pick_ms += f;
    }
    return SYBL_OK;
}

}  // namespace

int rollup_run(Table *t, const sybl_rollup_desc *d, sybl_table **out) {
    if (d->block_rows < 0 || d->block_rows > SYBL_BLOCK_ROWS)
        return fail(SYBL_E_INVAL, "%s: block_rows %d is outside 0 .. %d", kWho, d->block_rows, SYBL_BLOCK_ROWS);
    const int64_t br = d->block_rows ? d->block_rows : SYBL_BLOCK_ROWS;
    TableOwner O;
    int rc = derived_new_table(t->ctx, t->name, kWho, O);
    if (rc) return rc;
    rc = derived_call(t->ctx, kWho, O, out, [&] { return run(t, d, br, O.t, &O.t->rollup_stats, &O.t->rollup_pct_stats); });
    if (rc) {  // (what the planner, the table and the runtime say on the way is this call's error too)
        const std::string msg = sybl_last_error();
        if (msg.compare(0, strlen(kWho), kWho) != 0) return fail(rc, "%s: %s", kWho, msg.c_str());
    }
    return rc;
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_rollup(sybl_table *t, const sybl_rollup_desc *d, sybl_table **out) {
    SYBL_API_GUARD(t);
    if (out) *out = nullptr;
    if (!t || !d || !out) return fail(SYBL_E_INVAL, "sybl_table_rollup: NULL argument");
    return rollup_run(t, d, out);
}

int sybl_table_rollup_stats(const sybl_table *t, sybl_rollup_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_rollup_stats: NULL argument");
    *out = t->rollup_stats;
    return SYBL_OK;
}

int sybl_table_rollup_pct_stats(const sybl_table *t, sybl_rollup_pct_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_rollup_pct_stats: NULL argument");
    *out = t->rollup_pct_stats;
    return SYBL_OK;
}

}  // extern "C"
