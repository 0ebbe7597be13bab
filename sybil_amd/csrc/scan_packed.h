// scan_packed.h -- the role-specialised scan over COMPACT storage (sybl_table_compact).
//
// Columns stored as 1 / 2 / 4-byte unsigned offsets from the column minimum make the scan of the
// common shape 2-4x lighter on HBM, which moves the bound from the memory system to instruction
// issue and LDS atomics.  k_scan_packed therefore works in the 32-bit OFFSET domain end to end:
//   * four consecutive rows per lane and tile: one 4 / 8 / 16-byte load per column (1 / 2 / 4-byte
//     values), fully coalesced across the wave, next tile in flight while this one is consumed;
//   * filters compare the raw offset against bounds the planner rebased (filter.go:171-195);
//   * the group digit is offset + (base - gmin), one 24-bit multiply-add per key column
//     (aggregate.go:125-143 as a direct-mapped cell index);
//   * the histogram bucket is (offset + (base - h.Min)) / BucketSize (hist_basic.go:130); the 64-bit
//     value is only rebuilt for the exact sum.
// Cell table, LDS layout, publication and fold are those of k_scan_fast (scan_fast.h), so the
// all-reduce and finalize do not care which kernel ran.
#pragma once
#include "narrow3.h"
#include "fword.h"
#include "scan_fast.h"

namespace sybl {

constexpr int kPackedRows = 4;                                // rows per lane and tile
constexpr int kPackedTileRows = kWgThreads * kPackedRows;

hipError_t launch_scan_packed(const FastPlan &P, int nf, int ng, int na, int mode, bool time, int n_wg, size_t lds_bytes,
                              hipStream_t st);
hipError_t launch_emit_packed(const EmitPlan &E, int nf, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_count_packed_nf0(const EmitPlan &E, int ng, int n_wg, hipStream_t st);
hipError_t launch_count_packed_nf1(const EmitPlan &E, int ng, int n_wg, hipStream_t st);
hipError_t launch_count_packed_nf2(const EmitPlan &E, int ng, int n_wg, hipStream_t st);
hipError_t launch_count_packed_nf3(const EmitPlan &E, int ng, int n_wg, hipStream_t st);
hipError_t launch_count_packed_nf4(const EmitPlan &E, int ng, int n_wg, hipStream_t st);
hipError_t launch_emit_packed_nf0(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_emit_packed_nf1(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_emit_packed_nf2(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_emit_packed_nf3(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_emit_packed_nf4(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st);
hipError_t launch_scan_packed_nf0(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st);
hipError_t launch_scan_packed_nf1(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st);
hipError_t launch_scan_packed_nf2(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st);
hipError_t launch_scan_packed_nf3(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st);
hipError_t launch_scan_packed_nf4(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st);

#ifdef __HIPCC__

typedef unsigned int pu32x4 __attribute__((ext_vector_type(4)));

template <int N>
struct PackedTile {
    uint32_t u[N > 0 ? N : 1][kPackedRows];  // stored offsets (value - column base), zero-extended
    uint32_t pop[N > 0 ? N : 1];             // NUL kernels: validity bits of the four rows
};

template <int N>
struct PackedRaw {
    pu32x4 v[N > 0 ? N : 1];     // the loaded bytes of four rows: 1 / 2 / 4 dwords are meaningful
    uint32_t pw[N > 0 ? N : 1];  // NUL kernels: the validity word holding the four rows' bits
};

// Issues the load of four consecutive rows of one column.  The instruction is the same 16-byte
// buffer load for every stored width, so issuing needs no branch and nothing here waits for the
// data (the width only matters when the registers are decoded).  A narrower column would over-read
// into its neighbours' rows; the buffer descriptor is therefore set to exactly the wave's 256 rows
// (`col` = wave-uniform address of the wave's first row, `voff` = the lane's byte offset inside
// them), and the hardware range check drops the out-of-range dwords without touching memory --
// HBM traffic stays at the stored bytes.
constexpr uint32_t kBufferRsrcWord3 = 0x00020000;  // raw buffer, 32-bit data format (gfx9 family)

__device__ __forceinline__ void packed_issue(const uint8_t *col, int wshift, uint32_t voff, pu32x4 &raw) {
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)col, 0, (int)((64u * kPackedRows) << wshift), (int)kBufferRsrcWord3);
    raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 2);  // aux 2 = nt: streamed once
}
// The same for k_scan_packed, where an aggregation column may be a narrow twin (narrow3.h: 3 bytes a row): address, record
// count and lane offset are PRODUCTS of the width -- every lane's offset stays a multiple of 4 bytes, the wave's 256 rows are
// 768, and the last lane's fourth dword is out of range and dropped like a 2-byte column's upper half.
__device__ __forceinline__ void packed_issue_w(const uint8_t *col, uint32_t width, uint32_t voff, pu32x4 &raw) {
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)col, 0, (int)((64u * kPackedRows) * width), (int)kBufferRsrcWord3);
    raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 2);  // aux 2 = nt: streamed once
}

__device__ __forceinline__ void packed_decode(int width, const pu32x4 &raw, uint32_t (&u)[kPackedRows]) {
    if (width == 4) {
        u[0] = raw.x;
        u[1] = raw.y;
        u[2] = raw.z;
        u[3] = raw.w;
    } else if (width == 2) {
        u[0] = raw.x & 0xFFFFu;
        u[1] = raw.x >> 16;
        u[2] = raw.y & 0xFFFFu;
        u[3] = raw.y >> 16;
    } else if (width == kNarrowWidth) {
        const uint32_t d[3] = {raw.x, raw.y, raw.z};
        unpack3(d, u);
    } else {
        u[0] = raw.x & 0xFFu;
        u[1] = (raw.x >> 8) & 0xFFu;
        u[2] = (raw.x >> 16) & 0xFFu;
        u[3] = raw.x >> 24;
    }
}

// chunk-relative column addresses (wave-uniform)
template <int NF, int NG, int NA>
struct PackedBases {
    const uint8_t *f[NF > 0 ? NF : 1], *g[NG > 0 ? NG : 1], *a[NA > 0 ? NA : 1], *t;
    int64_t first;  // physical row of the chunk's first row (validity bitmaps are indexed by physical row)
};

// 1-byte columns: four rows are ONE dword.  Loaded with the 16-byte instruction they cost the address
// pipeline as much as a 4-byte column for a quarter of the data (loads-only: 4.0 TB/s against 6.1), and
// the instruction cannot depend on a run-time width (see packed_issue) -- so "every group column is one
// byte wide" (low-cardinality keys: the common case) is a compile-time property of the kernel (G1) and
// those columns are read with 4-byte loads.
__device__ __forceinline__ void packed_issue1(const uint8_t *col, uint32_t voff, pu32x4 &raw) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)col, 0, (int)(64u * kPackedRows), (int)kBufferRsrcWord3);
    raw.x = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, 0, 2);
}

// r: the lane's first row inside the chunk; the wave's first row is that of its first lane
template <int NF, int NG, int NA, bool TIME, bool G1, bool NUL, bool FRESH = false>
__device__ __forceinline__ void packed_issue_all(const FastPlan &P0, const PackedBases<NF, NG, NA> &B, uint32_t r, PackedRaw<NF> &f,
                                                 PackedRaw<NG> &g, PackedRaw<NA> &a, PackedRaw<1> &t) {
    const FastPlan &P = plan_fresh<FRESH>(P0);  // (FRESH: the plan words a stage uses are reloaded there, scan_fast.h)
    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
    const uint32_t lane_row = r - r0;
    if (NUL) {
        // validity words of the lane's four rows (nullptr: every row populated)
        const int64_t w = (B.first + r) >> 5;
        if (TIME) t.pw[0] = P.tvalid ? P.tvalid[w] : 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < NF; c++) f.pw[c] = P.fvalid[c] ? P.fvalid[c][w] : 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < NG; c++) g.pw[c] = P.gvalid[c] ? P.gvalid[c][w] : 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < NA; c++) a.pw[c] = P.avalid[c] ? P.avalid[c][w] : 0xFFFFFFFFu;
    }
    auto issue = [&](const uint8_t *col, int width, pu32x4 &raw) {
        const uint32_t w = (uint32_t)width;  // (r0 < 2^28 + 2^14 rows of at most 4 bytes: the products fit 32 bits)
        packed_issue_w(col + (size_t)(r0 * w), w, __umul24(lane_row, w), raw);
    };
    if (TIME) issue(B.t, P.twid, t.v[0]);
#pragma unroll
    for (int c = 0; c < NF; c++) issue(B.f[c], P.fwid[c], f.v[c]);
#pragma unroll
    for (int c = 0; c < NG; c++) {
        if (G1) {
            packed_issue1(B.g[c] + (size_t)r0, lane_row, g.v[c]);
        } else {
            issue(B.g[c], P.gwid[c], g.v[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < NA; c++) issue(B.a[c], P.awid[c], a.v[c]);
}

// The same loads for the staged kernels (k_count_packed / k_emit_packed), which keep several tiles in flight:
// every lane ALWAYS issues them -- a tile (or the lanes of a wave) beyond the end of the chunk gets a
// descriptor that ends at row n, so the range check returns zeros without touching memory.  Loads issued
// under a condition make the compiler assume the younger ones may not exist, and it then waits for all but
// the newest whenever it needs the oldest (s_waitcnt vmcnt(1) instead of vmcnt(6)).
template <int NF, int NG, int NA>
__device__ __forceinline__ void packed_issue_always(const FastPlan &P, const PackedBases<NF, NG, NA> &B, uint32_t r, uint32_t n,
                                                    PackedRaw<NF> &f, PackedRaw<NG> &g, PackedRaw<NA> &a) {
    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
    const uint32_t lane_row = r - r0;
    // wave-uniform; whole lanes (4 rows: at least one dword at any width -- the range check drops a dword that is
    // only partly inside), which never reaches past the padding every block ends with
    const uint32_t rows = r0 < n ? (n - r0 < 64u * kPackedRows ? (n - r0 + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows) : 0u;
    auto issue = [&](const uint8_t *col, int width, pu32x4 &raw) {
        const uint32_t w = (uint32_t)width;  // (products of the width: packed_issue_w)
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void *)(col + (size_t)((rows ? r0 : 0u) * w)), 0, (int)(rows * w), (int)kBufferRsrcWord3);
        raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24(lane_row, w)), 0, 2);  // aux 2 = nt: streamed once
    };
#pragma unroll
    for (int c = 0; c < NF; c++) issue(B.f[c], P.fwid[c], f.v[c]);
#pragma unroll
    for (int c = 0; c < NG; c++) issue(B.g[c], P.gwid[c], g.v[c]);
#pragma unroll
    for (int c = 0; c < NA; c++) issue(B.a[c], P.awid[c], a.v[c]);
}

// packed_issue_all for a ring of tiles in flight (k_scan_packed without NUL): like packed_issue_always every lane ALWAYS
// issues -- the descriptor ends at row n, so a tile (or the lanes of a wave) past the end of the chunk loads nothing --
// and the load count between a tile's loads and their use is the same on every path: the compiler's vmcnt is exact.
template <int NF, int NG, int NA, bool TIME, bool G1>
__device__ __forceinline__ void packed_issue_ring(const FastPlan &P, const PackedBases<NF, NG, NA> &B, uint32_t r, uint32_t n,
                                                  PackedRaw<NF> &f, PackedRaw<NG> &g, PackedRaw<NA> &a, PackedRaw<1> &t) {
    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
    const uint32_t lane_row = r - r0;
    const uint32_t rows = r0 < n ? (n - r0 < 64u * kPackedRows ? (n - r0 + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows) : 0u;
    const uint32_t base_row = rows ? r0 : 0u;
    auto issue = [&](const uint8_t *col, int width, pu32x4 &raw) {
        const uint32_t w = (uint32_t)width;  // (products of the width: packed_issue_w)
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void *)(col + (size_t)(base_row * w)), 0, (int)(rows * w), (int)kBufferRsrcWord3);
        raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24(lane_row, w)), 0, 2);  // aux 2 = nt: streamed once
    };
    if (TIME) issue(B.t, P.twid, t.v[0]);
#pragma unroll
    for (int c = 0; c < NF; c++) issue(B.f[c], P.fwid[c], f.v[c]);
#pragma unroll
    for (int c = 0; c < NG; c++) {
        if (G1) {
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(B.g[c] + (size_t)base_row), 0, (int)rows, (int)kBufferRsrcWord3);
            g.v[c].x = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)lane_row, 0, 2);
        } else {
            issue(B.g[c], P.gwid[c], g.v[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < NA; c++) issue(B.a[c], P.awid[c], a.v[c]);
}

// Tiles of loads a lane keeps in flight in k_scan_packed: ONE (the next tile is requested before the current one is
// consumed).  A ring of two or three tiles (RING > 1: the k_emit structure, every lane always issuing) was measured on one
// box against it (tools/bench_ring.py, round 3): config 2 (three columns) 0.177 ms with one tile, 0.180 with two, 0.182
// with three; the seven-column headline 2.81 / 2.92 / 2.92 ms; the time rollup 1.74 ms whichever -- the row bodies cover the
// latency of one tile, and the ring's clamped descriptors cost scalar work per load.  (Round 2 had found the same for
// queries of <= 3 columns.)  SYBL_PACKED_RING keeps the variants reachable for the BASELINE shapes.
constexpr int packed_depth(int) { return 1; }

template <int NF, int NG, int NA, bool TIME, bool G1, bool NUL, bool FRESH = false>
__device__ __forceinline__ void packed_decode_all(const FastPlan &P0, const PackedRaw<NF> &rf, const PackedRaw<NG> &rg,
                                                  const PackedRaw<NA> &ra, const PackedRaw<1> &rt, PackedTile<NF> &f,
                                                  PackedTile<NG> &g, PackedTile<NA> &a, PackedTile<1> &t, uint32_t bit0) {
    const FastPlan &P = plan_fresh<FRESH>(P0);
    if (NUL) {  // bit0 = (physical row of the lane's first row) & 31, a multiple of 4
        if (TIME) t.pop[0] = (rt.pw[0] >> bit0) & 0xFu;
#pragma unroll
        for (int c = 0; c < NF; c++) f.pop[c] = (rf.pw[c] >> bit0) & 0xFu;
#pragma unroll
        for (int c = 0; c < NG; c++) g.pop[c] = (rg.pw[c] >> bit0) & 0xFu;
#pragma unroll
        for (int c = 0; c < NA; c++) a.pop[c] = (ra.pw[c] >> bit0) & 0xFu;
    }
    if (TIME) packed_decode(P.twid, rt.v[0], t.u[0]);
#pragma unroll
    for (int c = 0; c < NF; c++) packed_decode(P.fwid[c], rf.v[c], f.u[c]);
#pragma unroll
    for (int c = 0; c < NG; c++) packed_decode(G1 ? 1 : P.gwid[c], rg.v[c], g.u[c]);
#pragma unroll
    for (int c = 0; c < NA; c++) packed_decode(P.awid[c], ra.v[c], a.u[c]);
}

// floor(n / d) for 32-bit n, d >= 1.  inv_lo is 1/d scaled down by (1 - 2^-40), so the product never
// exceeds the true quotient and is at most 1 short of it: one one-sided correction step is exact.
__device__ __forceinline__ uint32_t packed_udiv(uint32_t n, uint32_t d, double inv_lo) {
    uint32_t q = (uint32_t)((double)n * inv_lo);
    if (n - q * d >= d) q += 1;
    return q;
}

// Aggregation c's bucket number of the stored offset u: (u + adoff) / bucket_size.  PROVED (kLeanProved: numerator and bucket
// size below 2^24): udiv_magic.h's exact multiply-shift on the planner's constants -- a shift-add, a high multiply and a shift,
// no f64 -- where packed_udiv converts, multiplies and converts in f64 and corrects once.
template <bool PROVED>
__device__ __forceinline__ uint32_t packed_bucket(const FastPlan &P, const int c, const uint32_t u) {
    if (PROVED) return __umulhi((u << 1) + P.qoff2[c], P.qmul[c]) >> P.qshift[c];
    return packed_udiv(u + P.adoff[c], P.bucket_size[c], P.pinv_bucket[c]);
}

// Wave-uniform operands of the PROVED and lean row bodies that a loop may hold in VECTOR registers of its own (packed_scan_dyn:
// a VOP3 instruction of gfx950 takes one scalar operand, so a second uniform one is otherwise moved into a vector register in
// front of every use).  kfold: FastPlan::kfold - FastLds::cell_base; chi / zero: the high halves of the lean body's addends.
struct PackedRowRegs {
    uint32_t kfold, chi, zero;
};

// (OUT: the plain body with the outlier test -- a value beyond the last bucket is clipped and remembered, hist_basic.go:132-135:
// what a fully populated tile of a NUL kernel runs when outliers are the only thing its plan asks of the NUL body)
// (MAX32: avg mode's maxima as 32-bit OFFSETS -- see the kFastAvgMax branch; the caller has checked !ext_general once per tile)
// (LEAN, PROVED: FastPlan::lean's kLeanMoments / kLeanProved -- properties of the kernel, see k_scan_packed)
// matched / overflow: per lane.  (COUNTED: the caller has counted the tile's matched rows itself.  DERIVED: a kernel without NUL,
// where a matched row either adds one to its cell's Count or is out of bounds -- fast_finish derives the workgroup's overflow
// from the two, and the row counts nothing.)
template <int NF, int NG, int NA, int MODE, bool TIME, bool NUL, bool FRESH = false, bool OUT = false, bool MAX32 = false, bool LEAN = false,
          bool PROVED = false, bool COUNTED = false, bool DERIVED = false>
__device__ __forceinline__ void packed_row(const FastPlan &P0, const PackedTile<NF> &f, const PackedTile<NG> &g,
                                           const PackedTile<NA> &a, const PackedTile<1> &t, const int r, bool pass, int64_t *lds,
                                           const FastLds &L, uint32_t &matched, uint32_t &overflow, const uint32_t xpop = 0xFu,
                                           const PackedRowRegs *X = nullptr) {
    static_assert(!LEAN || (MODE == kFastMoments && !NUL && !OUT && NA >= 1), "the lean layout is the plain moments body's");
    static_assert(!PROVED || (!NUL && !OUT), "proofs cover fully populated rows");
    static_assert(!DERIVED || (!NUL && !OUT), "only a row that counts in exactly one place can have its overflow derived");
    if (NUL) pass = pass & ((xpop >> r) & 1u);  // the filter pre-pass's verdict (FastPlan::xvalid; all ones without one)
    // no short-circuit anywhere: one predicate, one exec-masked region per row
#pragma unroll
    for (int c = 0; c < NF; c++) {
        const FastPlan &P = plan_fresh<FRESH>(P0);
        const uint32_t u = f.u[c][r];
        bool ok = (u >= P.plo[c]) & (u <= P.phi[c]);  // filter.go:171-195, folded to a range of offsets
        if (NUL) {
            if (P.fmask[c]) {
                // StrFilter eq / neq / re / nre, evaluated per dictionary id on the host (filter.go:199-250)
                const uint32_t id = u + (uint32_t)P.fbase[c];
                ok = id < (uint32_t)P.fmask_bits[c];
                if (ok) ok = (P.fmask[c][id >> 5] >> (id & 31)) & 1u;
            }
            for (int k = 0; k < P.npneq[c]; k++) ok = ok & (u != P.pneq[c][k]);  // int neq, rebased
            ok = ok & ((f.pop[c] >> r) & 1u);  // an unpopulated value fails every filter
        }
        pass = pass & ok;
    }
    // (PROVED: the sum starts from the folded constant and runs over the stored offsets -- FastPlan::kfold; `cell` is then the
    // position inside this workgroup's LDS table from the start)
    uint32_t cell = PROVED ? (X ? X->kfold : plan_fresh<FRESH>(P0).kfold - L.cell_base) : 0u;
    bool inb = true;
#pragma unroll
    for (int c = 0; c < NG; c++) {
        const FastPlan &P = plan_fresh<FRESH>(P0);
        const uint32_t d = PROVED ? g.u[c][r] : g.u[c][r] + P.gdoff[c];  // value - gmin (PROVED: the stored offset)
        if (NUL) {
            // MISSING_VALUE key (aggregate.go:138): its own digit, or the digit of the value -1
            const bool p = (g.pop[c] >> r) & 1u;
            inb = inb & (p ? d < (uint32_t)P.gvalues[c] : P.gmissing[c] >= 0);
            cell += p ? __umul24(d, (uint32_t)P.gstride[c]) : (uint32_t)P.gmissing[c];
        } else {
            // (PROVED: the column's exact extrema lie inside the declared range, its stored offsets are below 2^24 and the table
            // is not windowed -- `lcell < ncell` below still keeps a wrong proof from ever writing outside the table)
            if (!PROVED) inb = inb & (d < P.gcard[c]);
            cell += __umul24(d, (uint32_t)P.gstride[c]);  // aggregate.go:125-143 as a direct-mapped index
        }
    }
    bool live = pass;
    const FastPlan &P = plan_fresh<FRESH>(P0);
    if (TIME) {
        // int(val) / TimeBucket (aggregate.go:174) for val >= 0, relative to the first bucket
        const uint32_t tb = packed_udiv(t.u[0][r] + P.tdoff, (uint32_t)P.time_bucket, P.pinv_time);
        if (NUL) {
            // no time value: the row was matched, then dropped (aggregate.go:147-153)
            const bool tp = (t.pop[0] >> r) & 1u;
            live = live & tp;
            inb = inb & (tb < (uint32_t)P.n_tb || !tp);
        } else {
            inb = inb & (tb < (uint32_t)P.n_tb);
        }
        cell += __umul24(tb, (uint32_t)P.tb_stride);
    }
    const uint32_t ncell = L.tab_cells;
    const uint32_t lcell = PROVED ? cell : cell - L.cell_base;  // position inside this workgroup's LDS table
    inb = inb & (lcell < ncell);
    if (!COUNTED) matched += pass ? 1u : 0u;  // aggregate.go:117
    if (!DERIVED) overflow += (live & !inb) ? 1u : 0u;
    if (!(live & inb)) return;
    const uint32_t rs = (uint32_t)P.rep_shift;
    if (LEAN) {
        // kLeanMoments (scan_fast.h): NA + ceil(NA / 2) + NA words, every addend a register or a register pair as it stands --
        // S_0 takes {u, 1 << (cshift - 32)}, B_j takes {b_even, b_odd}
        // The words of a (cell, replica) are NEIGHBOURS here (scan_fast.h): one address per row, every atomic a constant offset.
        constexpr uint32_t kB = NA, kQ = NA + (NA + 1) / 2, kW = (uint32_t)lean_sum_fields(NA);
        const uint32_t chi = X ? X->chi : 1u << ((uint32_t)P.cshift - 32u), zero = X ? X->zero : 0u;
        char *const lean_p = (char *)lds + __umul24((lcell << rs) + L.rep, kW * 8u);
        auto add = [&](uint32_t field, int64_t v) {
            __hip_atomic_fetch_add((int64_t *)(lean_p + field * 8u), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        uint32_t b[NA > 0 ? NA : 1];
#pragma unroll
        for (int c = 0; c < NA; c++) {
            const uint32_t u = a.u[c][r];
            add((uint32_t)c, (int64_t)(((uint64_t)(c == 0 ? chi : zero) << 32) | u));  // sum of OFFSETS (c == 0: and Count++)
            b[c] = packed_bucket<PROVED>(P, c, u);
            add(kQ + (uint32_t)c, (int64_t)(((uint64_t)zero << 32) | (uint32_t)__umul24(b[c], b[c])));
        }
#pragma unroll
        for (int j = 0; j < (NA + 1) / 2; j++)
            add(kB + (uint32_t)j, (int64_t)(((uint64_t)(2 * j + 1 < NA ? b[2 * j + 1 < NA ? 2 * j + 1 : 0] : zero) << 32) | b[2 * j]));
        return;
    }
    // byte address of the cell's Count word; every other field of the cell is a wave-uniform byte
    // offset away (one VALU add per atomic)
    char *const cell_p = (char *)lds + (((lcell << rs) + L.rep) << 3);
    const uint32_t fstep = (ncell << rs) << 3;  // bytes between consecutive fields
    auto add = [&](uint32_t field, int64_t v) {
        __hip_atomic_fetch_add((int64_t *)(cell_p + field * fstep), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    // avg modes with every value populated: Result.Count rides in the high bits of aggregation 0's sum word (FastPlan::cshift,
    // wave-uniform; 0 = it has a word of its own) -- one LDS atomic less per row
    const uint32_t cshift = ((MODE == kFastAvg || MODE == kFastAvgMax) && !NUL && !OUT && NA > 0) ? (uint32_t)P.cshift : 0u;
    if (!cshift) add(0, 1);  // Result.Count++ (aggregate.go:203)
#pragma unroll
    for (int c = 0; c < NA; c++) {
        const FastPlan &P = plan_fresh<FRESH>(P0);
        const uint32_t u = a.u[c][r];
        if (NUL) {
            if (!((a.pop[c] >> r) & 1u)) continue;  // no value: no hist for this row
            if (P.f_pop[c] >= 0) add((uint32_t)P.f_pop[c], 1);
            if (P.f_cnt[c] >= 0) {
                if (u < P.alo[c] || u > P.ahi[c]) continue;  // hist_basic.go:104, rebased
                add((uint32_t)P.f_cnt[c], 1);                // h.Count++
            }
        }
        const int64_t x = (int64_t)((uint64_t)P.abase[c] + u);
        if (c == 0 && cshift) add((uint32_t)P.f_sum[0], (int64_t)(((uint64_t)1 << cshift) + u));  // Count++ and sum of OFFSETS
        else add((uint32_t)P.f_sum[c], x);
        if (MODE == kFastAvgMax) {
            if (MAX32) {
                // BasicHist.Max (hist_basic.go:118-120) in the offset domain: max(v) = base + max(offset), so the lane's replica
                // of the MAX word holds the largest OFFSET in its low half -- one ds_max_u32 that returns nothing, where the
                // 64-bit form read the word, waited for it, compared and branched around a ds_max_i64 (two of those round trips
                // per row of config 2).  (A gate read of an unreplicated uint32 table in front of a rare atomic measured SLOWER
                // than the blind atomic: tools/micro/ldsrate.hip, profiles/r06_ldsrate.txt.)  A cell's maximum exists iff its
                // Count is not zero: fast_finish rebuilds the value.
                __hip_atomic_fetch_max((uint32_t *)(cell_p + ((uint32_t)P.n_sum_fields + (uint32_t)P.m_max[c]) * fstep), u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if (!P.ext_general) {
                int64_t *m = (int64_t *)(cell_p + ((uint32_t)P.n_sum_fields + (uint32_t)P.m_max[c]) * fstep);
                if (x > *m) __hip_atomic_fetch_max(m, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                // (FastPlan::ext_general: a minimum is tracked as well -- negative values in avg mode --, or not every maximum)
                if (P.m_max[c] >= 0) {
                    int64_t *m = (int64_t *)(cell_p + ((uint32_t)P.n_sum_fields + (uint32_t)P.m_max[c]) * fstep);
                    if (x > *m) __hip_atomic_fetch_max(m, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (P.m_nmin[c] >= 0) {
                    int64_t *m = (int64_t *)(cell_p + ((uint32_t)P.n_sum_fields + (uint32_t)P.m_nmin[c]) * fstep);
                    const int64_t nx = ~x;
                    if (nx > *m) __hip_atomic_fetch_max(m, nx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (MODE == kFastMoments || MODE == kFastHist) {
            // bucket_value := (value - h.Min) / BucketSize, hist_basic.go:130; the planner guarantees
            // 0 <= value - h.Min < 2^32 and that no value reaches len(Values)
            uint32_t b = packed_bucket<PROVED>(P, c, u);
            if ((NUL || OUT) && b >= (uint32_t)P.n_values[c]) {
                // Outlier (hist_basic.go:132-135; BucketSize = size / 1000 truncates, so the top of many a column's range
                // lies beyond the last bucket): clipped into the last bucket AND remembered as exact n, sum(o), sum(o^2)
                // in four 32-bit limbs (+ the value itself in the log when bucket arrays are kept); a cold path
                if (P.f_out[c] >= 0) {
                    const unsigned __int128 sq = (unsigned __int128)((__int128)x * (__int128)x);
                    const uint32_t fo = (uint32_t)P.f_out[c];
                    add(fo, 1);
                    add(fo + 1, x);
                    add(fo + 2, (int64_t)(uint64_t)(sq & 0xFFFFFFFFu));
                    add(fo + 3, (int64_t)(uint64_t)((sq >> 32) & 0xFFFFFFFFu));
                    add(fo + 4, (int64_t)(uint64_t)((sq >> 64) & 0xFFFFFFFFu));
                    add(fo + 5, (int64_t)(uint64_t)(sq >> 96));
                    if (P.out_log) log_outlier(P.out_log, P.out_cap, (int64_t)cell, c, x);
                } else {
                    overflow += 1;
                }
                b = (uint32_t)P.n_values[c] - 1;
            }
            if (MODE == kFastMoments) {
                add((uint32_t)P.f_sb[c], (int64_t)(uint64_t)b);
                add((uint32_t)P.f_sb2[c], (int64_t)(uint64_t)(uint32_t)__umul24(b, b));
            } else if (P.hist_lds) {
                __hip_atomic_fetch_add(L.hist32 + lcell * (uint32_t)P.hist_stride + (uint32_t)P.hist_agg_off[c] + b, 1u,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                __hip_atomic_fetch_add(P.sum_out + P.hist_off + (int64_t)(PROVED ? cell + L.cell_base : cell) * P.hist_stride + P.hist_agg_off[c] + b,
                                       (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// The four rows of a tile of a kernel without NUL (overflow is derived, see packed_row) through its plain body.  pass(k): row
// k's predicate so far.  max32: kFastAvgMax && !ext_general (wave-uniform, once per tile); LEANV: the kernel's (k_scan_packed).
// COUNTED: the caller counts the tile's matched rows per lane (where that is one instruction per tile).
template <int NF, int NG, int NA, int MODE, bool TIME, bool FRESH, bool COUNTED, int LEANV, class PASS>
__device__ __forceinline__ void packed_plain_tile(const FastPlan &P, const PackedTile<NF> &f, const PackedTile<NG> &g, const PackedTile<NA> &a,
                                                  const PackedTile<1> &t, PASS pass, int64_t *lds, const FastLds &L, const bool max32,
                                                  uint32_t &matched, uint32_t &overflow, const PackedRowRegs *X = nullptr) {
    constexpr bool kLean = (LEANV & kLeanMoments) != 0, kProved = (LEANV & kLeanProved) != 0;
    if (MODE == kFastAvgMax && max32) {
#pragma unroll
        for (int k = 0; k < kPackedRows; k++)
            packed_row<NF, NG, NA, MODE, TIME, false, FRESH, false, true, false, false, COUNTED, true>(P, f, g, a, t, k, pass(k), lds, L, matched, overflow);
    } else {
#pragma unroll
        for (int k = 0; k < kPackedRows; k++)
            packed_row<NF, NG, NA, MODE, TIME, false, FRESH, false, false, kLean, kProved, COUNTED, true>(P, f, g, a, t, k, pass(k), lds, L, matched, overflow,
                                                                                                          0xFu, X);
    }
}

constexpr int64_t kPackedChunkRows = (int64_t)1 << 28;  // rows addressed with one 32-bit byte offset (x4 bytes)

// SYBL_PACKED_LATE=0 at build time: k_scan_packed without late materialisation (same-box A/B builds)
#ifndef SYBL_PACKED_LATE
#define SYBL_PACKED_LATE 1
#endif
constexpr bool kPackedLate = SYBL_PACKED_LATE != 0;
#ifndef SYBL_PACKED_LATE_BRANCH
#define SYBL_PACKED_LATE_BRANCH 1
#endif
constexpr bool kPackedLateBranch = SYBL_PACKED_LATE_BRANCH != 0;
// (A late path inside the NUL variants was built and measured in round 6 and taken out again: in one body with the plain loop it
// cost the variant 268 B of scratch and its plain path 3.3 -> 4.05 ms per 1e9 rows of config 3, for 2.95 -> 2.79 ms at 0.1 %
// selectivity -- the NUL row body's own floor; profiles/r06_late_path_ab.txt.  As a kernel of its own it would be ~390 more
// instantiations of this template.)

#ifndef SYBL_PACKED_WAVES_PER_EU
#define SYBL_PACKED_WAVES_PER_EU 4
#endif

// ---- dynamic dealing (FastPlan::dyn; pieces.h) ----------------------------------------------------------------------------
// The loops of k_scan_packed without NUL over the workgroup's sequence of TILES across the pieces it draws, instead of over its
// share of segments.  A tile is the 64-bit physical row of its first row and its number of rows (1 .. 4096; 0 = past the
// workgroup's last piece: descriptors of zero records, rows that fail `k < left`); both are wave-uniform, and the descriptor of
// a column is (column + (R + the wave's row) * width, the wave's rows * width) -- the static loops' per-tile 64-bit add with R
// in place of the chunk's first row plus the row inside it.  Nothing drains at a piece's end: the loops below never see pieces.
static_assert(kPackedTileRows == kPieceTileRows, "pieces.h counts k_scan_packed's tiles");
struct DynTile {
    int64_t R;
    uint32_t rows;
};
constexpr uint32_t kNoTicket = 0xFFFFFFFFu;

// The workgroup's cursor over its pieces.  Thread 0 draws the tickets -- one returning agent-scope increment each, ONE piece
// ahead of the piece being entered, so the atomic's latency is a piece long in the past when its value is wanted -- and hands
// them to the other waves through a ring of LDS words and the one barrier a piece costs.  Every decision below is taken from
// those words, so it is the same in all 16 waves: they enter the same pieces, meet at the same barriers and leave together.  A
// workgroup never waits for another one (no flag, no spinning): it cannot hang.  (piece_cap, pieces.h: why every piece is
// scanned exactly once.)
// (The increment is atomic_inc with a bound of 2^32 - 1, not fetch_add: the compiler rewrites a fetch_add into a wave-wide
// reduction whose result it waits for on the spot -- s_waitcnt vmcnt(0) right behind the atomic.  The piece itself is read
// through the constant address space: one scalar 16-byte load, counted apart from the vector loads.)
static_assert(sizeof(Piece) == 16 && offsetof(Piece, start) == 0 && offsetof(Piece, n) == 8, "enter_piece reads a piece as four dwords");
struct DynCursor {
    const FastPlan &P;
    uint32_t *ring;          // LDS, 4 words: ring[k & 3] = the ticket of the k-th piece this workgroup enters
    uint32_t k = 0;          // pieces entered
    int64_t R = 0;           // next tile's first row
    uint32_t left = 0;       // rows of the entered piece not yet handed out
    bool done = false;       // a ticket past the table (or the cap): no more pieces
    uint32_t pend = kNoTicket, drawn = 0;  // (thread 0) the ticket drawn ahead; tickets drawn
    bool pend_ok = false;                  // (thread 0) ... and whether one was drawn at all
    bool want_draw = false;                // (thread 0) the next ticket is still to be drawn: draw_ahead()

    __device__ __forceinline__ DynCursor(const FastPlan &P_, uint32_t *ring_) : P(P_), ring(ring_) {
        if (threadIdx.x == 0) {
            draw();
            ring[0] = pend_ok ? pend : kNoTicket;
            draw();
        }
        __syncthreads();
    }
    __device__ __forceinline__ void draw() {
        pend_ok = drawn < (uint32_t)P.piece_cap;
        if (pend_ok) {
            pend = __builtin_amdgcn_atomic_inc32(P.piece_queue, 0xFFFFFFFFu, __ATOMIC_RELAXED, "agent");
            drawn++;
        }
    }
    // Called where the loops have just waited for their youngest loads (the decode of a tile): waiting for `pend` there
    // holds no load back.  ring[(k + 1) & 3] was last read when piece k - 3 was entered, three barriers ago.
    __device__ __forceinline__ void enter_piece() {
        if (threadIdx.x == 0) {
            if (want_draw) draw();  // (two pieces entered within one iteration: the draw has had no chance yet)
            const uint32_t ahead = pend_ok ? pend : kNoTicket;
            if (ahead >= (uint32_t)P.n_pieces) drawn = (uint32_t)P.piece_cap;  // the table has been dealt: draw no more
            ring[(k + 1) & 3u] = ahead;
            want_draw = true;
        }
        __syncthreads();
        const uint32_t ticket = __builtin_amdgcn_readfirstlane(ring[k & 3u]);
        k++;
        const bool have = ticket < (uint32_t)P.n_pieces;  // (the table read is bounded here; n_pieces >= 1)
        typedef const __attribute__((address_space(4))) pu32x4 *piece_words;
        const pu32x4 pc = *(piece_words)(uintptr_t)(P.pieces + (have ? ticket : 0u));
        R = (int64_t)(((uint64_t)pc.y << 32) | pc.x);
        left = have ? pc.z : 0u;
        done = !have;
    }
    // The draw that entering a piece asks for, issued BEHIND the iteration's loads: in front of them its return would be waited
    // for before they are issued (the compiler's next vmcnt(0)); behind them it comes back with them.
    __device__ __forceinline__ void draw_ahead() {
        if (threadIdx.x == 0 && want_draw) {
            draw();
            want_draw = false;
        }
    }
    __device__ __forceinline__ DynTile next() {
        if (left == 0 && !done) enter_piece();
        DynTile T;
        T.R = ((int64_t)__builtin_amdgcn_readfirstlane((int)(R >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)R);
        left = __builtin_amdgcn_readfirstlane(left);
        T.rows = left < (uint32_t)kPackedTileRows ? left : (uint32_t)kPackedTileRows;
        R = T.R + kPackedTileRows;
        left -= T.rows;
        return T;
    }
};

// FW: the filter columns' offsets come from one filter word per row (FastPlan::fword, fword.h) -- ONE full 16-byte load per lane
// and tile into rf.v[0] where the columns take NF, and a bit-field extract per column and row where they take a width decode.
// A property of the kernel like LEANV and DYN (the launcher picks it from P.fword): nothing in the loop asks which it is.
// KW: the key columns' and aggregation 0's offsets come from one key word per row (FastPlan::kword, a filter word in layout) --
// ONE full 16-byte load per lane and tile into ra.v[0] where they take NG + 1, and a bit-field extract per field and row.
// Likewise a property of the kernel (the launcher picks it from P.kword).
template <int NF, int NG, int NA, int MODE, bool TIME, bool G1, int LEANV, bool FW, bool KW>
__device__ __forceinline__ void packed_scan_dyn(const FastPlan &P, int64_t *lds, const FastLds &L, const bool max32, uint32_t &matched,
                                                uint32_t &overflow) {
    static_assert(!FW || NF >= kFwordMinFields, "a filter word holds at least two columns");
    static_assert(kFwordMaxFields == kFastMaxF, "one field per filter column of a FastPlan");
    static_assert(!KW || (!TIME && !G1 && NF >= 1 && NG >= 1 && NA >= 1), "a key word holds the keys and aggregation 0 of the late loop");
    static_assert(!KW || kPackedLate, "a key word is read by the late loop");
    static_assert(!KW || NG + 1 <= kFwordMaxFields, "one field per key column and one for aggregation 0");
    __shared__ uint32_t ring[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave_row = __builtin_amdgcn_readfirstlane((tid & ~63u) * kPackedRows);  // the wave's first row inside a tile
    const uint32_t lane_row = (tid & 63u) * kPackedRows;                                  // the lane's inside the wave's 256
    DynCursor cur(P, ring);
    PackedRaw<NF> rf;
    PackedRaw<NG> rg;
    PackedRaw<NA> ra;
    PackedRaw<1> rt;
    PackedTile<NF> f;
    PackedTile<NG> g;
    PackedTile<NA> a;
    PackedTile<1> t;
    // Wave-uniform operands of the loops' vector instructions, held in vector registers of their own from here on: the field
    // widths of the words (a v_bfe_u32 takes the shift as its one scalar operand; the width beside it would be moved into a
    // vector register in front of every extract) and PackedRowRegs for the PROVED bodies.  The empty asm makes each an opaque
    // vector value the compiler cannot re-materialise from its scalar source per use.  Only the kernels that read a word or
    // hold a PROVED body carry them: every other instantiation is what it was.
    auto pinned = [](uint32_t x) -> uint32_t {
        asm volatile("" : "+v"(x));
        return x;
    };
    uint32_t fbits_v[NF > 0 ? NF : 1] = {}, gbits_v[NG > 0 ? NG : 1] = {}, kabits_v = 0;
    if constexpr (FW) {
#pragma unroll
        for (int c = 0; c < NF; c++) fbits_v[c] = pinned((uint32_t)P.fbits[c]);
    }
    if constexpr (KW) {
#pragma unroll
        for (int c = 0; c < NG; c++) gbits_v[c] = pinned((uint32_t)P.gbits[c]);
        kabits_v = pinned((uint32_t)P.kabits);
    }
    constexpr bool kRowRegs = (LEANV & kLeanProved) != 0;
    PackedRowRegs regs = {0, 0, 0};
    if constexpr (kRowRegs) {
        regs.kfold = pinned(P.kfold - L.cell_base);
        if constexpr ((LEANV & kLeanMoments) != 0) {
            regs.chi = pinned(1u << ((uint32_t)P.cshift - 32u));
            regs.zero = pinned(0u);
        }
    }
    const PackedRowRegs *const X = kRowRegs ? &regs : nullptr;
    // one column's four rows for this lane: whole lanes up to the tile's end, like packed_issue_ring (`wanted` false, wave-
    // uniform: a descriptor of zero records -- the range check answers without touching memory)
    auto issue = [&](const void *col, int width, const DynTile &T, bool wanted, pu32x4 &raw, bool one_dword) {
        const uint32_t rows = wanted && T.rows > wave_row
                                  ? (T.rows - wave_row < 64u * kPackedRows ? (T.rows - wave_row + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows)
                                  : 0u;
        const int64_t base = rows ? T.R + wave_row : 0;
        const uint32_t w = (uint32_t)width;  // (products of the width, packed_issue_w; the base is a physical row: 64 bits)
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void *)((const uint8_t *)col + (size_t)base * w), 0, (int)(rows * w), (int)kBufferRsrcWord3);
        if (one_dword) raw.x = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)lane_row, 0, 2);  // (G1: width 1, see packed_issue1)
        else raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24(lane_row, w)), 0, 2);       // aux 2 = nt: streamed once
    };
    auto issue_filters = [&](const DynTile &T) {
        if constexpr (FW) {
            issue(P.fword, 4, T, true, rf.v[0], false);
        } else {
#pragma unroll
            for (int c = 0; c < NF; c++) issue(P.fcol[c], P.fwid[c], T, true, rf.v[c], false);
        }
    };
    auto decode_filters = [&]() {
        if constexpr (FW) {
            const uint32_t wd[kPackedRows] = {rf.v[0].x, rf.v[0].y, rf.v[0].z, rf.v[0].w};
#pragma unroll
            for (int c = 0; c < NF; c++) {
#pragma unroll
                for (int k = 0; k < kPackedRows; k++) f.u[c][k] = __builtin_amdgcn_ubfe(wd[k], (uint32_t)P.fshift[c], fbits_v[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < NF; c++) packed_decode(P.fwid[c], rf.v[c], f.u[c]);
        }
    };
    auto issue_rest = [&](const DynTile &T, bool wanted) {
        if (TIME) issue(P.tcol, P.twid, T, wanted, rt.v[0], false);
        if constexpr (KW) {
            issue(P.kword, 4, T, wanted, ra.v[0], false);
        } else {
#pragma unroll
            for (int c = 0; c < NG; c++) issue(P.gcol[c], G1 ? 1 : P.gwid[c], T, wanted, rg.v[c], G1);
        }
#pragma unroll
        for (int c = KW ? 1 : 0; c < NA; c++) issue(P.acol[c], P.awid[c], T, wanted, ra.v[c], false);
    };
    auto decode_rest = [&]() {
        if (TIME) packed_decode(P.twid, rt.v[0], t.u[0]);
        if constexpr (KW) {
            const uint32_t wd[kPackedRows] = {ra.v[0].x, ra.v[0].y, ra.v[0].z, ra.v[0].w};
#pragma unroll
            for (int c = 0; c < NG; c++) {
#pragma unroll
                for (int k = 0; k < kPackedRows; k++) g.u[c][k] = __builtin_amdgcn_ubfe(wd[k], (uint32_t)P.gshift[c], gbits_v[c]);
            }
#pragma unroll
            for (int k = 0; k < kPackedRows; k++) a.u[0][k] = __builtin_amdgcn_ubfe(wd[k], (uint32_t)P.kashift, kabits_v);
        } else {
#pragma unroll
            for (int c = 0; c < NG; c++) packed_decode(G1 ? 1 : P.gwid[c], rg.v[c], g.u[c]);
        }
#pragma unroll
        for (int c = KW ? 1 : 0; c < NA; c++) packed_decode(P.awid[c], ra.v[c], a.u[c]);
    };
    auto lane_left = [&](const DynTile &T) -> uint32_t { return T.rows > tid * kPackedRows ? T.rows - tid * kPackedRows : 0u; };
    if (kPackedLate && NF > 0 && NG + NA + (TIME ? 1 : 0) > 0) {
        // late materialisation as in k_scan_packed's static loop: filters of tile t + 2 and keys / values of t + 1 in flight
        // while the rows of t are consumed
        PackedTile<0> f0;
        auto filter_bits = [&](const DynTile &T) -> uint32_t {
            decode_filters();
            const uint32_t left = lane_left(T);
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < kPackedRows; k++) {
                bool pass = (uint32_t)k < left;
#pragma unroll
                for (int c = 0; c < NF; c++) pass = pass & (f.u[c][k] >= P.plo[c]) & (f.u[c][k] <= P.phi[c]);
                bits |= pass ? 1u << k : 0u;
            }
            return bits;
        };
        DynTile T0 = cur.next();
        issue_filters(T0);
        uint32_t bits = filter_bits(T0);
        DynTile T1 = cur.next();
        issue_rest(T0, __builtin_amdgcn_ballot_w64(bits != 0) != 0);
        issue_filters(T1);
        cur.draw_ahead();
        while (T0.rows) {
            decode_rest();  // keys / values / time of T0 (zeros if nothing was wanted)
            const uint32_t next_bits = filter_bits(T1);
            const DynTile T2 = cur.next();  // (every load issued so far has been waited for)
            if (kPackedLateBranch) {
                if (__builtin_amdgcn_ballot_w64(next_bits != 0) != 0) issue_rest(T1, true);
            } else {
                issue_rest(T1, __builtin_amdgcn_ballot_w64(next_bits != 0) != 0);
            }
            issue_filters(T2);
            cur.draw_ahead();
            matched += (uint32_t)__builtin_popcount(bits);
            packed_plain_tile<0, NG, NA, MODE, TIME, false, true, LEANV>(P, f0, g, a, t, [&](int k) -> bool { return (bits >> k) & 1u; }, lds, L, max32,
                                                                         matched, overflow, X);
            bits = next_bits;
            T0 = T1;
            T1 = T2;
        }
        return;
    }
    // the plain loop: every column of tile t + 1 in flight while the rows of t are consumed
    DynTile T0 = cur.next();
    issue_filters(T0);
    issue_rest(T0, true);
    cur.draw_ahead();
    while (T0.rows) {
        decode_filters();
        decode_rest();
        const DynTile T1 = cur.next();  // (every load issued so far has been waited for)
        issue_filters(T1);
        issue_rest(T1, true);
        cur.draw_ahead();
        const uint32_t left = lane_left(T0);
        if (NF == 0) matched += left < (uint32_t)kPackedRows ? left : (uint32_t)kPackedRows;  // no filter: every row of the tile
        packed_plain_tile<NF, NG, NA, MODE, TIME, false, NF == 0, LEANV>(P, f, g, a, t, [&](int k) { return (uint32_t)k < left; }, lds, L, max32,
                                                                        matched, overflow, X);
        T0 = T1;
    }
}
// LEANV: what the planner proved for this launch (FastPlan::lean: kLeanMoments | kLeanProved) as a property of the KERNEL -- the
// launcher picks the instantiation, and a lean kernel holds the lean body only.  (Two bodies chosen per tile inside one loop
// cost the loop 20 more spilled scalar registers; DESIGN 3.6 has the same finding for two loops in one kernel.)
// DYN: FastPlan::dyn, likewise a property of the kernel -- the dynamic loops instead of the static ones (packed_scan_dyn).
// FW: the dynamic loops read a filter word in the filter columns' place (packed_scan_dyn).
// KW: the dynamic late loop reads a key word in the place of the key columns and aggregation 0 (packed_scan_dyn).  G1 only
// shapes the key loads a key word replaces: the KW kernels are the G1 = false ones.
template <int NF, int NG, int NA, int MODE, bool TIME, bool G1, bool NUL, int RING = 0, int LEANV = 0, bool DYN = false, bool FW = false,
          bool KW = false>
__global__ __launch_bounds__(kWgThreads, SYBL_PACKED_WAVES_PER_EU) void k_scan_packed(const FastPlan P) {
    static_assert(LEANV == 0 || !NUL, "the NUL kernels mix row bodies: no proofs");
    static_assert(!DYN || (!NUL && RING == 0), "dynamic dealing is the plain kernels'");
    static_assert(!FW || (DYN && NF >= kFwordMinFields), "filter words are the dynamic loops', for two filter columns and more");
    static_assert(!KW || (DYN && !TIME && !G1 && NG >= 1 && NA >= 1 && FW == (NF >= kFwordMinFields) && NF >= 1),
                  "key words are the dynamic late loop's: keys and an aggregation, one filter column or a filter word");
    static_assert(!(LEANV & kLeanMoments) || (MODE == kFastMoments && NA >= 1), "the lean layout is moments mode's");
    static_assert(!(LEANV & kLeanProved) || MODE == kFastMoments || MODE == kFastHist, "the proved bodies are the bucket modes'");
    extern __shared__ int64_t lds[];
    const uint32_t tid = threadIdx.x;
    // avg mode, every value populated (the NUL kernels mix row bodies: they keep 64-bit maxima): maxima as 32-bit offsets
    constexpr bool kMax32 = MODE == kFastAvgMax && !NUL;
    constexpr bool lean_layout = (LEANV & kLeanMoments) != 0;
    const FastLds L = fast_begin<MODE>(P, lds, kMax32 && !P.ext_general, lean_layout);

    uint32_t matched = 0, overflow = 0;
    const uint64_t clock_in = P.wg_clock ? wall_clock64() : 0;  // (SYBL_WG_CLOCKS=1: when this workgroup's loop began and ended)
    if constexpr (DYN) packed_scan_dyn<NF, NG, NA, MODE, TIME, G1, LEANV, FW, KW>(P, lds, L, kMax32 && !P.ext_general, matched, overflow);
    // (DYN: no segments -- the static loops below compile to nothing)
    const int s0 = DYN ? 0 : P.wg_seg_begin[blockIdx.x], s1 = DYN ? 0 : P.wg_seg_begin[blockIdx.x + 1];
    for (int si = s0; si < s1; si++) {
        const Segment seg = P.segs[si];
        for (int64_t c0 = 0; c0 < seg.n; c0 += kPackedChunkRows) {
            const int64_t first = seg.start + c0;
            const uint32_t n = (uint32_t)(seg.n - c0 < kPackedChunkRows ? seg.n - c0 : kPackedChunkRows);
            PackedBases<NF, NG, NA> B;
#pragma unroll
            for (int c = 0; c < NF; c++) B.f[c] = (const uint8_t *)P.fcol[c] + first * P.fwid[c];
#pragma unroll
            for (int c = 0; c < NG; c++) B.g[c] = (const uint8_t *)P.gcol[c] + first * P.gwid[c];
#pragma unroll
            for (int c = 0; c < NA; c++) B.a[c] = (const uint8_t *)P.acol[c] + first * P.awid[c];
            B.t = TIME ? (const uint8_t *)P.tcol + first * P.twid : nullptr;
            B.first = first;

            PackedTile<NF> f;
            PackedTile<NG> g;
            PackedTile<NA> a;
            PackedTile<1> t;
            constexpr bool FRESH = RING == 4;  // (A/B: plan words reloaded per stage instead of spilled scalar registers)
            constexpr int D = NUL ? 1 : (RING > 0 && RING < 4 ? RING : packed_depth(NF + NG + NA + (TIME ? 1 : 0)));
            if (D > 1) {
                // a ring of D tiles of loads in flight, consumed oldest first; no exit inside a round (a tile past the end
                // loads nothing and its rows fail `k < left`)
                PackedRaw<NF> rf[D];
                PackedRaw<NG> rg[D];
                PackedRaw<NA> ra[D];
                PackedRaw<1> rt[D];
                const uint32_t n_tiles = (n + kPackedTileRows - 1) / kPackedTileRows;
                const uint32_t r_first = tid * kPackedRows;
#pragma unroll
                for (int d = 0; d < D; d++) {
                    packed_issue_ring<NF, NG, NA, TIME, G1>(P, B, r_first + (uint32_t)d * kPackedTileRows, n, rf[d], rg[d], ra[d], rt[d]);
                    __builtin_amdgcn_sched_barrier(0);  // oldest tile first: the ring is consumed in this order
                }
                for (uint32_t it0 = 0; it0 < n_tiles; it0 += D) {
#pragma unroll
                    for (int d = 0; d < D; d++) {
                        const uint32_t r = r_first + (it0 + d) * kPackedTileRows;  // (< 2^28 + 2^14: no wrap)
                        packed_decode_all<NF, NG, NA, TIME, G1, false>(P, rf[d], rg[d], ra[d], rt[d], f, g, a, t, 0u);
                        packed_issue_ring<NF, NG, NA, TIME, G1>(P, B, r + (uint32_t)D * kPackedTileRows, n, rf[d], rg[d], ra[d], rt[d]);
                        const uint32_t left = r < n ? n - r : 0u;
                        packed_plain_tile<NF, NG, NA, MODE, TIME, false, false, LEANV>(P, f, g, a, t, [&](int k) { return (uint32_t)k < left; }, lds, L,
                                                                                kMax32 && !P.ext_general, matched, overflow);
                    }
                }
                continue;
            }
            PackedRaw<NF> rf;
            PackedRaw<NG> rg;
            PackedRaw<NA> ra;
            PackedRaw<1> rt;
            // (NUL) the filter pre-pass's bitmap (FastPlan::xvalid): the lane's four bits for the tile being consumed, and
            // the word of the tile after it -- fetched a tile early, so that a wave none of whose 256 rows passed the
            // pre-pass issues no load at all for that tile
            uint32_t xpop = 0xFu, xw_n = 0xFFFFFFFFu;
            const bool xv = NUL && P.xvalid != nullptr;
            // The NUL row body costs twice the plain one (config 3 forced through it: 5.8 against 2.85 ms per 1e9 rows) --
            // validity bits, the MISSING digit, per-aggregation counts, the outlier test, each a branch per row and column.
            // Most tiles of most tables need none of it: a str group column, or a bitmap that is all ones where it is read.
            // `light` (wave-uniform, once): the plan itself asks for nothing the plain body lacks; a tile all of whose
            // values are populated (and pass the pre-pass) then runs the plain body.
            bool light = NUL, outliers = false;
            if (NUL) {
#pragma unroll
                for (int c = 0; c < NF; c++) light = light && P.fmask[c] == nullptr && P.npneq[c] == 0;
#pragma unroll
                for (int c = 0; c < NG; c++) light = light && (uint32_t)P.gvalues[c] == P.gcard[c];
#pragma unroll
                for (int c = 0; c < NA; c++) {
                    light = light && P.f_pop[c] < 0 && P.f_cnt[c] < 0;
                    outliers = outliers || P.f_out[c] >= 0;  // (BucketSize = size / 1000 truncates: an ordinary column's top values)
                }
            }
            if (kPackedLate && !NUL && NF > 0 && NG + NA + (TIME ? 1 : 0) > 0) {
                // Late materialisation (the reference's row loop leaves a row at its first failing filter, aggregate.go:105-116):
                // the filter columns run one tile ahead of the key / aggregation / time columns, the tile's predicate is
                // evaluated as soon as they arrive, and a WAVE none of whose 256 rows passes does not read the other columns
                // of that tile.  The load instructions are still issued -- a fixed count per iteration keeps the compiler's
                // vmcnt exact (packed_issue_always) -- but through a descriptor of zero records: the range check answers
                // without touching memory, so the skipped lines are never fetched (a wave's tile of 256 rows is whole 128-byte
                // lines at every stored width: 256, 512 or 1024 bytes).
                // Iteration t: decode keys / values of tile t and the filters of t + 1, issue keys / values of t + 1 (or
                // nothing) and the filters of t + 2, then the rows of t with the predicate bits kept from last time.
                const uint32_t r_first = tid * kPackedRows;
                const uint32_t n_tiles = (n + kPackedTileRows - 1) / kPackedTileRows;
                PackedTile<0> f0;
                auto issue_filters = [&](uint32_t r) {
                    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r), lane_row = r - r0;
                    const uint32_t rows = r0 < n ? (n - r0 < 64u * kPackedRows ? (n - r0 + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows) : 0u;
                    const uint32_t base_row = rows ? r0 : 0u;
#pragma unroll
                    for (int c = 0; c < NF; c++) {
                        const int ws = P.fwid[c] >> 1;
                        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(B.f[c] + ((size_t)base_row << ws)), 0, (int)(rows << ws), (int)kBufferRsrcWord3);
                        rf.v[c] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane_row << ws), 0, 2);
                    }
                };
                auto issue_rest = [&](uint32_t r, bool wanted) {
                    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r), lane_row = r - r0;
                    uint32_t rows = r0 < n ? (n - r0 < 64u * kPackedRows ? (n - r0 + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows) : 0u;
                    rows = wanted ? rows : 0u;  // (wave-uniform: nothing of this tile is wanted -> a descriptor of zero records)
                    const uint32_t base_row = rows ? r0 : 0u;
                    auto issue = [&](const uint8_t *col, int width, pu32x4 &raw) {
                        const uint32_t w = (uint32_t)width;  // (products of the width: packed_issue_w)
                        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(col + (size_t)(base_row * w)), 0, (int)(rows * w), (int)kBufferRsrcWord3);
                        raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24(lane_row, w)), 0, 2);
                    };
                    if (TIME) issue(B.t, P.twid, rt.v[0]);
#pragma unroll
                    for (int c = 0; c < NG; c++) {
                        if (G1) {
                            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(B.g[c] + (size_t)base_row), 0, (int)rows, (int)kBufferRsrcWord3);
                            rg.v[c].x = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)lane_row, 0, 2);
                        } else {
                            issue(B.g[c], P.gwid[c], rg.v[c]);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NA; c++) issue(B.a[c], P.awid[c], ra.v[c]);
                };
                auto filter_bits = [&](uint32_t r) -> uint32_t {
                    // (decodes rf: the first use of the filter loads issued an iteration ago)
#pragma unroll
                    for (int c = 0; c < NF; c++) packed_decode(P.fwid[c], rf.v[c], f.u[c]);
                    const uint32_t left = r < n ? n - r : 0u;
                    uint32_t bits = 0;
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        bool pass = (uint32_t)k < left;
#pragma unroll
                        for (int c = 0; c < NF; c++) pass = pass & (f.u[c][k] >= P.plo[c]) & (f.u[c][k] <= P.phi[c]);
                        bits |= pass ? 1u << k : 0u;
                    }
                    return bits;
                };
                issue_filters(r_first);
                uint32_t bits = filter_bits(r_first);
                issue_rest(r_first, __builtin_amdgcn_ballot_w64(bits != 0) != 0);
                issue_filters(r_first + kPackedTileRows);
                for (uint32_t it = 0; it < n_tiles; it++) {
                    const uint32_t r = r_first + it * kPackedTileRows;  // (< 2^28 + 2^13: no wrap)
                    // keys / values / time of tile `it` (their loads were issued an iteration ago; zeros if nothing was wanted)
                    if (TIME) packed_decode(P.twid, rt.v[0], t.u[0]);
#pragma unroll
                    for (int c = 0; c < NG; c++) packed_decode(G1 ? 1 : P.gwid[c], rg.v[c], g.u[c]);
#pragma unroll
                    for (int c = 0; c < NA; c++) packed_decode(P.awid[c], ra.v[c], a.u[c]);
                    const uint32_t next_bits = filter_bits(r + kPackedTileRows);
                    if (kPackedLateBranch) {
                        if (__builtin_amdgcn_ballot_w64(next_bits != 0) != 0) issue_rest(r + kPackedTileRows, true);
                    } else {
                        issue_rest(r + kPackedTileRows, __builtin_amdgcn_ballot_w64(next_bits != 0) != 0);
                    }
                    issue_filters(r + 2u * kPackedTileRows);
                    matched += (uint32_t)__builtin_popcount(bits);  // aggregate.go:117, the lane's rows of this tile at once
                    packed_plain_tile<0, NG, NA, MODE, TIME, false, true, LEANV>(P, f0, g, a, t, [&](int k) -> bool { return (bits >> k) & 1u; }, lds, L,
                                                                                 kMax32 && !P.ext_general, matched, overflow);
                    bits = next_bits;
                }
                continue;
            }
            uint32_t r = tid * kPackedRows;
            if (r < n) {
                packed_issue_all<NF, NG, NA, TIME, G1, NUL, FRESH>(P, B, r, rf, rg, ra, rt);
                if (xv) {
                    xpop = (P.xvalid[(first + r) >> 5] >> ((uint32_t)(first + r) & 31u)) & 0xFu;
                    if (r + kPackedTileRows < n) xw_n = P.xvalid[(first + r + kPackedTileRows) >> 5];
                }
                packed_decode_all<NF, NG, NA, TIME, G1, NUL, FRESH>(P, rf, rg, ra, rt, f, g, a, t, (uint32_t)(first + r) & 31u);
            }
            for (; r < n; r += kPackedTileRows) {
                // the next tile's loads are in flight while this one is consumed; they are decoded
                // (the first use of the loaded registers) only after the rows below
                const uint32_t rn = r + kPackedTileRows;
                const uint32_t xpop_n = xv ? (xw_n >> ((uint32_t)(first + rn) & 31u)) & 0xFu : 0xFu;
                const bool more = rn < n && (!xv || __builtin_amdgcn_ballot_w64(xpop_n != 0) != 0);  // (wave-uniform)
                if (more) packed_issue_all<NF, NG, NA, TIME, G1, NUL, FRESH>(P, B, rn, rf, rg, ra, rt);
                if (xv && rn + kPackedTileRows < n) xw_n = P.xvalid[(first + rn + kPackedTileRows) >> 5];
                const uint32_t left = n - r;
                bool plain_tile = false;
                if (NUL && light) {
                    uint32_t allpop = xpop;
                    if (TIME) allpop &= t.pop[0];
#pragma unroll
                    for (int c = 0; c < NF; c++) allpop &= f.pop[c];
#pragma unroll
                    for (int c = 0; c < NG; c++) allpop &= g.pop[c];
#pragma unroll
                    for (int c = 0; c < NA; c++) allpop &= a.pop[c];
                    plain_tile = __builtin_amdgcn_ballot_w64(allpop != 0xFu) == 0;  // (wave-uniform)
                }
                if (plain_tile && !outliers) {
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++)
                        packed_row<NF, NG, NA, MODE, TIME, false, FRESH>(P, f, g, a, t, k, (uint32_t)k < left, lds, L, matched, overflow);
                } else if (plain_tile) {
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++)
                        packed_row<NF, NG, NA, MODE, TIME, false, FRESH, true>(P, f, g, a, t, k, (uint32_t)k < left, lds, L, matched, overflow);
                } else if constexpr (!NUL) {  // (the plain body the plan allows: wave-uniform, once per tile)
                    if (NF == 0) matched += left < (uint32_t)kPackedRows ? left : (uint32_t)kPackedRows;  // no filter: every row of the tile
                    packed_plain_tile<NF, NG, NA, MODE, TIME, FRESH, NF == 0, LEANV>(P, f, g, a, t, [&](int k) { return (uint32_t)k < left; }, lds, L,
                                                                              kMax32 && !P.ext_general, matched, overflow);
                } else {
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++)
                        packed_row<NF, NG, NA, MODE, TIME, NUL, FRESH>(P, f, g, a, t, k, (uint32_t)k < left, lds, L, matched, overflow, xpop);
                }
                if (more) packed_decode_all<NF, NG, NA, TIME, G1, NUL, FRESH>(P, rf, rg, ra, rt, f, g, a, t, (uint32_t)(first + rn) & 31u);
                xpop = xpop_n;
            }
        }
    }
    const uint64_t clock_out = P.wg_clock ? wall_clock64() : 0;
    // (!NUL: no row body counted overflow -- fast_finish derives it)
    fast_finish(P, lds, L, matched, overflow, kMax32 && !P.ext_general, lean_layout ? (uint32_t)NA : 0u, !NUL);
    if (P.wg_clock && tid == 0) {
        P.wg_clock[2 * blockIdx.x] = clock_in;
        P.wg_clock[2 * blockIdx.x + 1] = clock_out;
    }
}

// k_emit over compact storage (strategy 5, see k_emit in scan_fast.h): the same records, staged and
// flushed the same way; rows are loaded and filtered in the offset domain like k_scan_packed.
// One column's four rows for this lane with a descriptor that ends at row n -- or holds nothing at all (`wanted` false,
// wave-uniform): the range check then returns zeros without touching memory.  What the late paths below issue.
__device__ __forceinline__ void packed_issue_clamped(const uint8_t *col, int width, uint32_t r, uint32_t n, bool wanted, pu32x4 &raw) {
    const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
    const uint32_t lane_row = r - r0;
    const uint32_t rows = wanted && r0 < n ? (n - r0 < 64u * kPackedRows ? (n - r0 + kPackedRows - 1) & ~(uint32_t)(kPackedRows - 1) : 64u * kPackedRows) : 0u;
    const uint32_t w = (uint32_t)width;  // (products of the width: packed_issue_w)
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)(col + (size_t)((rows ? r0 : 0u) * w)), 0, (int)(rows * w), (int)kBufferRsrcWord3);
    raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(__umul24(lane_row, w)), 0, 2);
}

// LATE (round 6, a kernel of its own -- two loops in one body wreck the other's register allocation): the filter
// columns run a tile ahead; the key and value columns of a tile are only requested when some row of the wave passed.  Chosen
// by the planner's selectivity estimate (FastPlan::late): at 0.1 % most waves never touch them.
template <int NF, int NG, int NA, bool LATE = false>
__global__ __launch_bounds__(kWgThreads, 4) void k_emit_packed(const EmitPlan E) {
    extern __shared__ uint32_t elds[];
    const FastPlan &P = E.fp;
    const uint32_t tid = threadIdx.x;
    const EmitLds S = emit_begin(E, elds);

    uint32_t matched = 0, overflow = 0;
    constexpr uint32_t kTile = kPackedTileRows;
    const int s0 = P.wg_seg_begin[blockIdx.x], s1 = P.wg_seg_begin[blockIdx.x + 1];
    for (int si = s0; si < s1; si++) {
        const Segment seg = P.segs[si];
        for (int64_t c0 = 0; c0 < seg.n; c0 += kPackedChunkRows) {
            const int64_t first = seg.start + c0;
            const uint32_t n = (uint32_t)(seg.n - c0 < kPackedChunkRows ? seg.n - c0 : kPackedChunkRows);
            PackedBases<NF, NG, NA> B;
#pragma unroll
            for (int c = 0; c < NF; c++) B.f[c] = (const uint8_t *)P.fcol[c] + first * P.fwid[c];
#pragma unroll
            for (int c = 0; c < NG; c++) B.g[c] = (const uint8_t *)P.gcol[c] + first * P.gwid[c];
#pragma unroll
            for (int c = 0; c < NA; c++) B.a[c] = (const uint8_t *)P.acol[c] + first * P.awid[c];
            B.t = nullptr;
            if constexpr (LATE) {
                const uint32_t n_tiles = (n + kTile - 1) / kTile;
                const uint32_t r_first = tid * kPackedRows;
                PackedRaw<NF> rfn;
                PackedRaw<NG> rgl;
                PackedRaw<NA> ral;
#pragma unroll
                for (int c = 0; c < NF; c++) packed_issue_clamped(B.f[c], P.fwid[c], r_first, n, true, rfn.v[c]);
                for (uint32_t it = 0; it < n_tiles; it++) {
                    const uint32_t r = r_first + it * kTile;
                    uint32_t fu[NF > 0 ? NF : 1][kPackedRows];
#pragma unroll
                    for (int c = 0; c < NF; c++) packed_decode(P.fwid[c], rfn.v[c], fu[c]);
#pragma unroll
                    for (int c = 0; c < NF; c++) packed_issue_clamped(B.f[c], P.fwid[c], r + kTile, n, true, rfn.v[c]);
                    const uint32_t left = r < n ? n - r : 0u;
                    bool pass[kPackedRows], any = false;
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        pass[k] = (uint32_t)k < left;
#pragma unroll
                        for (int c = 0; c < NF; c++) pass[k] = pass[k] & (fu[c][k] >= P.plo[c]) & (fu[c][k] <= P.phi[c]);
                        any = any | pass[k];
                        matched += pass[k] ? 1u : 0u;
                    }
                    if (!__builtin_amdgcn_ballot_w64(any)) continue;  // (wave-uniform: no row of these 256 passed)
#pragma unroll
                    for (int c = 0; c < NG; c++) packed_issue_clamped(B.g[c], P.gwid[c], r, n, true, rgl.v[c]);
#pragma unroll
                    for (int c = 0; c < NA; c++) packed_issue_clamped(B.a[c], P.awid[c], r, n, true, ral.v[c]);
                    uint32_t gu[NG > 0 ? NG : 1][kPackedRows], au[NA > 0 ? NA : 1][kPackedRows];
#pragma unroll
                    for (int c = 0; c < NG; c++) packed_decode(P.gwid[c], rgl.v[c], gu[c]);
#pragma unroll
                    for (int c = 0; c < NA; c++) packed_decode(P.awid[c], ral.v[c], au[c]);
                    uint32_t bin[kPackedRows * NA], rec[kPackedRows * NA];
                    bool act[kPackedRows * NA];
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        uint32_t cell = 0;
                        bool inb = true;
#pragma unroll
                        for (int c = 0; c < NG; c++) {
                            const uint32_t d = gu[c][k] + P.gdoff[c];
                            inb = inb & (d < P.gcard[c]);
                            cell += __umul24(d, (uint32_t)P.gstride[c]);
                        }
                        overflow += (pass[k] & !inb) ? 1u : 0u;
#pragma unroll
                        for (int c = 0; c < NA; c++) {
                            const uint32_t n32 = au[c][k] + P.adoff[c];  // value - h.Min
                            const uint32_t pair = cell * (uint32_t)NA + (uint32_t)c;
                            const int at = k * NA + c;
                            bin[at] = emit_bin(S, pair);
                            rec[at] = emit_record(pair, n32);
                            act[at] = pass[k] & inb;
                        }
                    }
                    emit_push_all<kPackedRows * NA, kEmitQueue>(E, S, bin, rec, act);
                }
                continue;
            }
            // D tiles of loads in flight per lane (narrow queries move few bytes per tile)
            constexpr int D = emit_depth(NF + NG + NA);
            // With one aggregation a tile is only four records per lane, and a push is a chain of ~7 dependent LDS round
            // trips (slot, wr, write + publish, queue, chunk, copy) that four waves per SIMD do not hide: two tiles are
            // pushed together (eight records per round trip; the drain then has four store instructions).
            constexpr int T = (NA == 1 && D % 2 == 0) ? 2 : 1;
            constexpr uint32_t Q = T == 2 ? kEmitQueueMax : kEmitQueue;
            PackedRaw<NF> rf[D];
            PackedRaw<NG> rg[D];
            PackedRaw<NA> ra[D];
            PackedRaw<1> rt;
            PackedTile<NF> f;
            PackedTile<NG> g;
            PackedTile<NA> a;
            PackedTile<1> t;
            const uint32_t n_tiles = (n + kTile - 1) / kTile;
            const uint32_t r_first = tid * kPackedRows;
#pragma unroll
            for (int d = 0; d < D; d++) {
                packed_issue_always<NF, NG, NA>(P, B, r_first + (uint32_t)d * kTile, n, rf[d], rg[d], ra[d]);
                if (d % T == T - 1) emit_pad_stores<Q>(S);  // (the ring as the steady state has it: see emit_pad_stores)
                __builtin_amdgcn_sched_barrier(0);  // oldest tile first: the ring is consumed in this order
            }
            for (uint32_t it0 = 0; it0 < n_tiles; it0 += D) {
#pragma unroll
              for (int d0 = 0; d0 < D; d0 += T) {
                // (no early exit inside a round: a tile past the end loads nothing -- the descriptor's range check -- and
                // pushes nothing; a conditional exit here is one more path the compiler's load / store counting must
                // take the minimum over)
                uint32_t bin[kPackedRows * NA * T], rec[kPackedRows * NA * T];
                bool act[kPackedRows * NA * T];
#pragma unroll
                for (int dd = 0; dd < T; dd++) {
                    const int d = d0 + dd;
                    const uint32_t r = r_first + (it0 + d) * kTile;   // (< 2^28 + 2^12: no wrap)
                    packed_decode_all<NF, NG, NA, false, false, false>(P, rf[d], rg[d], ra[d], rt, f, g, a, t, 0u);
                    packed_issue_always<NF, NG, NA>(P, B, r + (uint32_t)D * kTile, n, rf[d], rg[d], ra[d]);
                    const uint32_t left = r < n ? n - r : 0u;
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        bool pass = (uint32_t)k < left;
#pragma unroll
                        for (int c = 0; c < NF; c++) {
                            const uint32_t u = f.u[c][k];
                            pass = pass & (u >= P.plo[c]) & (u <= P.phi[c]);
                        }
                        uint32_t cell = 0;
                        bool inb = true;
#pragma unroll
                        for (int c = 0; c < NG; c++) {
                            const uint32_t d = g.u[c][k] + P.gdoff[c];
                            inb = inb & (d < P.gcard[c]);
                            cell += __umul24(d, (uint32_t)P.gstride[c]);
                        }
                        matched += pass ? 1u : 0u;
                        overflow += (pass & !inb) ? 1u : 0u;
#pragma unroll
                        for (int c = 0; c < NA; c++) {
                            const uint32_t n32 = a.u[c][k] + P.adoff[c];  // value - h.Min
                            const uint32_t pair = cell * (uint32_t)NA + (uint32_t)c;
                            const int at = (dd * kPackedRows + k) * NA + c;
                            bin[at] = emit_bin(S, pair);
                            rec[at] = emit_record(pair, n32);
                            act[at] = pass & inb;
                        }
                    }
                }
                emit_push_all<kPackedRows * NA * T, Q>(E, S, bin, rec, act);
              }
            }
        }
    }
    emit_finish(E, S, matched, overflow);
}

// k_count over compact storage: the counting pass of k_emit_packed (see k_count in scan_fast.h).
template <int NF, int NG, bool LATE = false>
__global__ __launch_bounds__(kWgThreads, 4) void k_count_packed(const EmitPlan E) {
    extern __shared__ uint32_t elds[];
    const FastPlan &P = E.fp;
    const uint32_t tid = threadIdx.x;
    uint32_t *mine = count_begin(E, elds);
    const uint32_t na = (uint32_t)E.n_aggs, ss = (uint32_t)E.sub_shift;
    const int s0 = P.wg_seg_begin[blockIdx.x], s1 = P.wg_seg_begin[blockIdx.x + 1];
    for (int si = s0; si < s1; si++) {
        const Segment seg = P.segs[si];
        for (int64_t c0 = 0; c0 < seg.n; c0 += kPackedChunkRows) {
            const int64_t first = seg.start + c0;
            const uint32_t n = (uint32_t)(seg.n - c0 < kPackedChunkRows ? seg.n - c0 : kPackedChunkRows);
            PackedBases<NF, NG, 0> B;
#pragma unroll
            for (int c = 0; c < NF; c++) B.f[c] = (const uint8_t *)P.fcol[c] + first * P.fwid[c];
#pragma unroll
            for (int c = 0; c < NG; c++) B.g[c] = (const uint8_t *)P.gcol[c] + first * P.gwid[c];
            B.a[0] = nullptr;
            B.t = nullptr;
            if constexpr (LATE) {
                // (see k_emit_packed<.., LATE>: the same rows pass, so the regions it fills are the ones counted here)
                const uint32_t n_tiles = (n + kPackedTileRows - 1) / kPackedTileRows;
                const uint32_t r_first = tid * kPackedRows;
                PackedRaw<NF> rfn;
                PackedRaw<NG> rgl;
#pragma unroll
                for (int c = 0; c < NF; c++) packed_issue_clamped(B.f[c], P.fwid[c], r_first, n, true, rfn.v[c]);
                for (uint32_t it = 0; it < n_tiles; it++) {
                    const uint32_t r = r_first + it * kPackedTileRows;
                    uint32_t fu[NF > 0 ? NF : 1][kPackedRows];
#pragma unroll
                    for (int c = 0; c < NF; c++) packed_decode(P.fwid[c], rfn.v[c], fu[c]);
#pragma unroll
                    for (int c = 0; c < NF; c++) packed_issue_clamped(B.f[c], P.fwid[c], r + kPackedTileRows, n, true, rfn.v[c]);
                    const uint32_t left = r < n ? n - r : 0u;
                    bool pass[kPackedRows], any = false;
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        pass[k] = (uint32_t)k < left;
#pragma unroll
                        for (int c = 0; c < NF; c++) pass[k] = pass[k] & (fu[c][k] >= P.plo[c]) & (fu[c][k] <= P.phi[c]);
                        any = any | pass[k];
                    }
                    if (!__builtin_amdgcn_ballot_w64(any)) continue;
#pragma unroll
                    for (int c = 0; c < NG; c++) packed_issue_clamped(B.g[c], P.gwid[c], r, n, true, rgl.v[c]);
                    uint32_t gu[NG > 0 ? NG : 1][kPackedRows];
#pragma unroll
                    for (int c = 0; c < NG; c++) packed_decode(P.gwid[c], rgl.v[c], gu[c]);
#pragma unroll
                    for (int k = 0; k < kPackedRows; k++) {
                        uint32_t cell = 0;
                        bool ok = pass[k];
#pragma unroll
                        for (int c = 0; c < NG; c++) {
                            const uint32_t d = gu[c][k] + P.gdoff[c];
                            ok = ok & (d < P.gcard[c]);
                            cell += __umul24(d, (uint32_t)P.gstride[c]);
                        }
                        if (ok) __hip_atomic_fetch_add(mine + (((cell * na) >> kPartCellBits) << ss), na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                continue;
            }
            constexpr int D = count_depth(NF + NG);
            PackedRaw<NF> rf[D];
            PackedRaw<NG> rg[D];
            PackedRaw<0> ra;
            PackedRaw<1> rt;
            PackedTile<NF> f;
            PackedTile<NG> g;
            PackedTile<0> a;
            PackedTile<1> t;
            const uint32_t n_tiles = (n + kPackedTileRows - 1) / kPackedTileRows;
            const uint32_t r_first = tid * kPackedRows;
#pragma unroll
            for (int d = 0; d < D; d++) {
                packed_issue_always<NF, NG, 0>(P, B, r_first + (uint32_t)d * kPackedTileRows, n, rf[d], rg[d], ra);
                __builtin_amdgcn_sched_barrier(0);  // oldest tile first: the ring is consumed in this order
            }
            for (uint32_t it0 = 0; it0 < n_tiles; it0 += D) {
#pragma unroll
              for (int d = 0; d < D; d++) {
                if (it0 + d >= n_tiles) break;
                const uint32_t r = r_first + (it0 + d) * kPackedTileRows;
                packed_decode_all<NF, NG, 0, false, false, false>(P, rf[d], rg[d], ra, rt, f, g, a, t, 0u);
                packed_issue_always<NF, NG, 0>(P, B, r + (uint32_t)D * kPackedTileRows, n, rf[d], rg[d], ra);
                const uint32_t left = r < n ? n - r : 0u;
#pragma unroll
                for (int k = 0; k < kPackedRows; k++) {
                    bool pass = (uint32_t)k < left;
#pragma unroll
                    for (int c = 0; c < NF; c++) {
                        const uint32_t u = f.u[c][k];
                        pass = pass & (u >= P.plo[c]) & (u <= P.phi[c]);
                    }
                    uint32_t cell = 0;
#pragma unroll
                    for (int c = 0; c < NG; c++) {
                        const uint32_t d = g.u[c][k] + P.gdoff[c];
                        pass = pass & (d < P.gcard[c]);
                        cell += __umul24(d, (uint32_t)P.gstride[c]);
                    }
                    if (pass) __hip_atomic_fetch_add(mine + (((cell * na) >> kPartCellBits) << ss), na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
              }
            }
        }
    }
    count_finish(E, elds);
}

// k_count_key: the counting pass for its commonest shape -- ONE key column, no filter, one bin per partition (sub_shift 0:
// config 4) -- with every lane's 16-byte load FULL of keys (eight 2-byte keys, sixteen 1-byte, four 4-byte) instead of the
// four rows k_count_packed shares with k_emit_packed's row -> lane mapping (a 2-byte key column then brings 8 useful
// bytes per 16-byte instruction: half the load instructions and half the tile overhead for the same 2 GB).  With one bin
// per partition the count of a (workgroup, bin) does not depend on WHICH lane saw a row, only on the workgroup's row range,
// which is the plan's: k_emit_packed's regions come out the same.  (SYBL_NO_COUNT16=1: k_count_packed.)
template <int W>
__global__ __launch_bounds__(kWgThreads, 4) void k_count_key(const EmitPlan E) {
    extern __shared__ uint32_t elds[];
    const FastPlan &P = E.fp;
    const uint32_t tid = threadIdx.x;
    uint32_t *bins = count_begin(E, elds);  // (sub_shift 0: the counters themselves)
    const uint32_t na = (uint32_t)E.n_aggs;
    constexpr uint32_t R = 16u / (uint32_t)W;       // keys per lane and tile
    constexpr uint32_t kTile = kWgThreads * R;       // rows per workgroup and tile
    constexpr int D = 4;                             // tiles of loads in flight
    const uint32_t gdoff = P.gdoff[0], gcard = P.gcard[0], gstride = (uint32_t)P.gstride[0];
    const int s0 = P.wg_seg_begin[blockIdx.x], s1 = P.wg_seg_begin[blockIdx.x + 1];
    for (int si = s0; si < s1; si++) {
        const Segment seg = P.segs[si];
        for (int64_t c0 = 0; c0 < seg.n; c0 += kPackedChunkRows) {
            const int64_t first = seg.start + c0;
            const uint32_t n = (uint32_t)(seg.n - c0 < kPackedChunkRows ? seg.n - c0 : kPackedChunkRows);
            const uint8_t *col = (const uint8_t *)P.gcol[0] + first * W;
            // one descriptor for the chunk: a lane (or a dword of it) past row n reads zeros without touching memory; the
            // rows it would stand for are masked by `left` below
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)col, 0, (int)(((n * (uint32_t)W) + 3u) & ~3u), (int)kBufferRsrcWord3);
            pu32x4 raw[D];
            const uint32_t r_first = tid * R;
            const uint32_t n_tiles = (n + kTile - 1) / kTile;
#pragma unroll
            for (int d = 0; d < D; d++) raw[d] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((r_first + (uint32_t)d * kTile) * (uint32_t)W), 0, 2);
            for (uint32_t it0 = 0; it0 < n_tiles; it0 += D) {
#pragma unroll
                for (int d = 0; d < D; d++) {
                    const uint32_t r = r_first + (it0 + d) * kTile;  // (< 2^28 + 2^16: no wrap)
                    const pu32x4 v = raw[d];
                    raw[d] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((r + (uint32_t)D * kTile) * (uint32_t)W), 0, 2);
                    const uint32_t left = r < n ? n - r : 0u;
                    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (uint32_t k = 0; k < R; k++) {
                        uint32_t u;
                        if (W == 4) u = w4[k];
                        else if (W == 2) u = (w4[k >> 1] >> ((k & 1u) * 16u)) & 0xFFFFu;
                        else u = (w4[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
                        const uint32_t dgt = u + gdoff;
                        if (k < left && dgt < gcard)
                            __hip_atomic_fetch_add(bins + ((__umul24(dgt, gstride) * na) >> kPartCellBits), na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
    }
    count_finish(E, elds);
}

template <int NF>
static hipError_t count_packed_launch_nf(const EmitPlan &E, int ng, int n_wg, hipStream_t st) {
    const size_t lds = count_lds_bytes(E);
    if (count_takes_key_kernel(E, NF, ng)) {
        switch (E.fp.gwid[0]) {
        case 1: hipLaunchKernelGGL((k_count_key<1>), dim3(n_wg), dim3(kWgThreads), lds, st, E); return hipGetLastError();
        case 2: hipLaunchKernelGGL((k_count_key<2>), dim3(n_wg), dim3(kWgThreads), lds, st, E); return hipGetLastError();
        case 4: hipLaunchKernelGGL((k_count_key<4>), dim3(n_wg), dim3(kWgThreads), lds, st, E); return hipGetLastError();
        default: break;
        }
    }
    if constexpr (NF > 0) {
        if (E.fp.late) {  // (the planner's estimate: few rows pass -- filters first, keys for the waves with a match)
            switch (ng) {
            case 0: hipLaunchKernelGGL((k_count_packed<NF, 0, true>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
            case 1: hipLaunchKernelGGL((k_count_packed<NF, 1, true>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
            case 2: hipLaunchKernelGGL((k_count_packed<NF, 2, true>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
            default: return hipErrorInvalidValue;
            }
            return hipGetLastError();
        }
    }
    switch (ng) {
    case 0: hipLaunchKernelGGL((k_count_packed<NF, 0>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
    case 1: hipLaunchKernelGGL((k_count_packed<NF, 1>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
    case 2: hipLaunchKernelGGL((k_count_packed<NF, 2>), dim3(n_wg), dim3(kWgThreads), lds, st, E); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int NF>
static hipError_t emit_packed_launch_nf(const EmitPlan &E, int ng, int na, int n_wg, hipStream_t st) {
    const size_t lds = emit_lds_bytes(E);
#define SYBL_EMITP_CASE(G, A)                                                                              \
    case (G)*3 + (A): {                                                                                    \
        auto k = k_emit_packed<NF, G, A>;                                                                  \
        hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                     \
        hipLaunchKernelGGL(k, dim3(n_wg), dim3(kWgThreads), lds, st, E);                                   \
        return hipGetLastError();                                                                          \
    }
#define SYBL_EMITL_CASE(G, A)                                                                              \
    case (G)*3 + (A): {                                                                                    \
        auto k = k_emit_packed<NF, G, A, true>;                                                            \
        hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                     \
        hipLaunchKernelGGL(k, dim3(n_wg), dim3(kWgThreads), lds, st, E);                                   \
        return hipGetLastError();                                                                          \
    }
    if constexpr (NF > 0) {
        if (E.fp.late) {
            switch (ng * 3 + na) {
                SYBL_EMITL_CASE(0, 1)
                SYBL_EMITL_CASE(0, 2)
                SYBL_EMITL_CASE(1, 1)
                SYBL_EMITL_CASE(1, 2)
                SYBL_EMITL_CASE(2, 1)
                SYBL_EMITL_CASE(2, 2)
            default: return hipErrorInvalidValue;
            }
        }
    }
#undef SYBL_EMITL_CASE
    switch (ng * 3 + na) {
        SYBL_EMITP_CASE(0, 1)
        SYBL_EMITP_CASE(0, 2)
        SYBL_EMITP_CASE(1, 1)
        SYBL_EMITP_CASE(1, 2)
        SYBL_EMITP_CASE(2, 1)
        SYBL_EMITP_CASE(2, 2)
    default: return hipErrorInvalidValue;
    }
#undef SYBL_EMITP_CASE
}

// the dynamic kernels (FastPlan::dyn) of one shape: the instantiation for the plan's lean bits, reading the filter columns or,
// FW, a filter word; KW, the keys and aggregation 0 from a key word
template <int NF, int NG, int NA, int MODE, bool TIME, bool G1, bool FW, bool KW, class LAUNCH>
static hipError_t packed_launch_dyn(const FastPlan &P, LAUNCH &&launch_lean) {
    if constexpr (NA >= 1 && MODE == kFastMoments) {
        switch (P.lean) {
        case 0: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, 0, true, FW, KW>);
        case kLeanMoments: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, kLeanMoments, true, FW, KW>);
        case kLeanProved: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, kLeanProved, true, FW, KW>);
        case kLeanMoments | kLeanProved: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, kLeanMoments | kLeanProved, true, FW, KW>);
        default: return hipErrorInvalidValue;
        }
    } else if constexpr (NA >= 1 && MODE == kFastHist) {
        if (P.lean == kLeanProved) return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, kLeanProved, true, FW, KW>);
        if (P.lean) return hipErrorInvalidValue;
        return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, 0, true, FW, KW>);
    } else {
        if (P.lean) return hipErrorInvalidValue;
        return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, false, 0, 0, true, FW, KW>);
    }
}

template <int NF, int NG, int NA, int MODE, bool TIME, bool G1, bool NUL>
static hipError_t packed_launch_k1(const FastPlan &P, int n_wg, size_t lds_bytes, hipStream_t st) {
    // SYBL_PACKED_RING=1..3 (tuning): the BASELINE shapes with an explicit ring depth, for same-box A/B runs
    constexpr bool kAb = !NUL && ((NF == 3 && NG == 2 && NA == 2 && MODE == kFastMoments && !TIME && G1) ||
                                  (NF == 0 && NG == 1 && NA == 2 && MODE == kFastAvgMax && !TIME && G1) ||
                                  (NF == 0 && NG == 1 && NA == 1 && MODE == kFastAvg && TIME && !G1));
    auto launch_lean = [&](auto kern) {
        hipError_t e2 = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(kern, dim3(n_wg), dim3(kWgThreads), lds_bytes, st, P);
        return hipGetLastError();
    };
    // FastPlan::dyn: the kernels with the dynamic loops (the planner takes it for plans without NUL only, and not beside
    // SYBL_PACKED_RING); a missing kernel is an error
    if (P.dyn) {
        if constexpr (!NUL) {
            if (!P.pieces || !P.piece_queue || P.n_pieces < 1 || P.piece_cap < 1) return hipErrorInvalidValue;
            // FastPlan::fword: the FW kernels (the planner takes a word for NF >= 2 only; the fields must lie inside the word)
            if (P.fword) {
                if constexpr (NF >= kFwordMinFields) {
                    for (int c = 0; c < NF; c++)
                        if (P.fbits[c] < 1 || P.fshift[c] < 0 || P.fshift[c] + P.fbits[c] > kFwordBits) return hipErrorInvalidValue;
                } else {
                    return hipErrorInvalidValue;
                }
            }
            // FastPlan::kword: the KW kernels -- the late loop without a time column, with a filter word iff NF >= 2 (what the
            // planner takes a key word for, plan_kword); the fields must lie inside the word
            if (P.kword) {
                if constexpr (kPackedLate && !TIME && NF >= 1 && NG >= 1 && NA >= 1) {
                    if ((P.fword != nullptr) != (NF >= kFwordMinFields)) return hipErrorInvalidValue;
                    for (int c = 0; c < NG; c++)
                        if (P.gbits[c] < 1 || P.gshift[c] < 0 || P.gshift[c] + P.gbits[c] > kFwordBits) return hipErrorInvalidValue;
                    if (P.kabits < 1 || P.kashift < 0 || P.kashift + P.kabits > kFwordBits) return hipErrorInvalidValue;
                    return packed_launch_dyn<NF, NG, NA, MODE, TIME, false, (NF >= kFwordMinFields), true>(P, launch_lean);
                } else {
                    return hipErrorInvalidValue;
                }
            }
            if constexpr (NF >= kFwordMinFields) {
                if (P.fword) return packed_launch_dyn<NF, NG, NA, MODE, TIME, G1, true, false>(P, launch_lean);
            }
            return packed_launch_dyn<NF, NG, NA, MODE, TIME, G1, false, false>(P, launch_lean);
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (P.fword || P.kword) return hipErrorInvalidValue;  // (a filter word or a key word is read by the dynamic loops alone)
    // FastPlan::lean: the kernel must be the one the planner sized the table for.  (The lean kernels have no ring variants:
    // SYBL_PACKED_RING acts on a plan without lean -- set SYBL_NO_LEAN=1 beside it.)
    if (P.lean) {
        if constexpr (!NUL && NA >= 1 && MODE == kFastMoments) {
            switch (P.lean) {
            case kLeanMoments: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, 0, kLeanMoments>);
            case kLeanProved: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, 0, kLeanProved>);
            case kLeanMoments | kLeanProved: return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, 0, kLeanMoments | kLeanProved>);
            default: return hipErrorInvalidValue;
            }
        } else if constexpr (!NUL && NA >= 1 && MODE == kFastHist) {
            if (P.lean != kLeanProved) return hipErrorInvalidValue;
            return launch_lean(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, 0, kLeanProved>);
        } else {
            return hipErrorInvalidValue;  // (the planner sets it for those kernels only)
        }
    }
    if (kAb) {
        if (const char *e = env("SYBL_PACKED_RING")) {
            const int d = atoi(e);
            auto launch = [&](auto kern) {
                hipError_t e2 = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
                if (e2 != hipSuccess) return e2;
                hipLaunchKernelGGL(kern, dim3(n_wg), dim3(kWgThreads), lds_bytes, st, P);
                return hipGetLastError();
            };
            if (d == 1) return launch(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, kAb ? 1 : 0>);
            if (d == 2) return launch(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, kAb ? 2 : 0>);
            if (d == 3) return launch(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, kAb ? 3 : 0>);
            if (d == 4) return launch(k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL, kAb ? 4 : 0>);
        }
    }
    auto k = k_scan_packed<NF, NG, NA, MODE, TIME, G1, NUL>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n_wg), dim3(kWgThreads), lds_bytes, st, P);
    return hipGetLastError();
}

template <int NF, int NG, int NA, int MODE, bool TIME>
static hipError_t packed_launch_k(const FastPlan &P, int n_wg, size_t lds_bytes, hipStream_t st) {
    bool g1 = NG > 0;  // every group column is stored in one byte
    for (int c = 0; c < NG; c++) g1 = g1 && P.gwid[c] == 1;
    // NUL: missing rows / str ids / the reject gate (validity bitmaps are loaded next to the columns)
    if (P.nul) return packed_launch_k1<NF, NG, NA, MODE, TIME, false, true>(P, n_wg, lds_bytes, st);
    if (NG > 0 && g1) return packed_launch_k1<NF, NG, NA, MODE, TIME, (NG > 0), false>(P, n_wg, lds_bytes, st);
    return packed_launch_k1<NF, NG, NA, MODE, TIME, false, false>(P, n_wg, lds_bytes, st);
}

template <int NF, int NG, int NA>
static hipError_t packed_launch_mode(const FastPlan &P, int mode, bool time, int n_wg, size_t lds, hipStream_t st) {
#define SYBL_PACKED_MODE(M) \
    return time ? packed_launch_k<NF, NG, NA, M, true>(P, n_wg, lds, st) : packed_launch_k<NF, NG, NA, M, false>(P, n_wg, lds, st)
    if (NA == 0) SYBL_PACKED_MODE(kFastAvg);
    switch (mode) {
    case kFastAvg: SYBL_PACKED_MODE(kFastAvg);
    case kFastAvgMax: SYBL_PACKED_MODE(kFastAvgMax);
    case kFastMoments: SYBL_PACKED_MODE(kFastMoments);
    case kFastHist: SYBL_PACKED_MODE(kFastHist);
    default: return hipErrorInvalidValue;
    }
#undef SYBL_PACKED_MODE
}

template <int NF>
static hipError_t packed_launch_nf(const FastPlan &P, int ng, int na, int mode, bool time, int n_wg, size_t lds, hipStream_t st) {
    switch (ng * 3 + na) {
    case 0: return packed_launch_mode<NF, 0, 0>(P, mode, time, n_wg, lds, st);
    case 1: return packed_launch_mode<NF, 0, 1>(P, mode, time, n_wg, lds, st);
    case 2: return packed_launch_mode<NF, 0, 2>(P, mode, time, n_wg, lds, st);
    case 3: return packed_launch_mode<NF, 1, 0>(P, mode, time, n_wg, lds, st);
    case 4: return packed_launch_mode<NF, 1, 1>(P, mode, time, n_wg, lds, st);
    case 5: return packed_launch_mode<NF, 1, 2>(P, mode, time, n_wg, lds, st);
    case 6: return packed_launch_mode<NF, 2, 0>(P, mode, time, n_wg, lds, st);
    case 7: return packed_launch_mode<NF, 2, 1>(P, mode, time, n_wg, lds, st);
    case 8: return packed_launch_mode<NF, 2, 2>(P, mode, time, n_wg, lds, st);
    default: return hipErrorInvalidValue;
    }
}

#endif  // __HIPCC__

}  // namespace sybl
