// concat.hip -- resident tables joined end to end as a NEW resident table: the call of the samples / digest / select family
// that takes more than one table.  The semantics are restated in include/sybilgpu.h ("concat") and DESIGN.md 3.10; this file
// is the device work and the host code that drives it.
//
// Blocks are KEPT: the output's blocks are the sources' live non-empty blocks, each at the next multiple of 32 physical rows.
// So a maximal run of consecutive live blocks of a source is contiguous in the source AND in the output, and per (source,
// output column) the work is a short list of runs (source start, output start, rows), every number a multiple of 32.
//
//   same stored form   (width, base) equal and no id table needed: hipMemcpyAsync device to device, run by run.
//   k_cc_transcode     anything else: <WS, WD, LUT> reads the stored bits at WS bytes, value = sbase + zext(bits), with LUT
//                      the value goes through the (source, column) id -> id table, and value - dbase is written at WD
//                      bytes.  The NARROWER side moves 16 bytes per lane, the wider side WW / WN 16-byte accesses of one
//                      contiguous span, lane after lane: no sub-dword access, no LDS, no atomics.  One launch per (source,
//                      column) over its run list; a wave finds the run of its first row by bisection (block_of, derived.h).
//   k_cc_valid         validity words: copied where the source column has a bitmap, ones for the logical rows where it has
//                      none but the output does; the padding bits of a block's last word are zero either way.  A source
//                      that lacks the column leaves the zeroed words alone.
//   statistics         the sources' own per-block min / max / populated counts; for a str column whose ids were remapped one
//                      k_block_minmax launch over the output's blocks, and one readback for the table.
//
// Set columns: validity as above; the CSR (Column::h_set_off / h_set_vals) is concatenated on the host, member ids through
// the same id table -- a host pass per set column.
//
// The storage rule is fit_storage (colstats.h), as for appended blocks; the call wrapper and the statistics of the remapped
// columns (derived_block_stats) are derived.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "derived.h"

namespace sybl {

constexpr int kCcThreads = 256;

struct CcRun {
    int64_t src, dst;  // first physical row in the source / in the output
    int64_t rows;      // physical rows, the padding of every block included
    int64_t lbase;     // rows of the runs before this one
};

struct CcBlk {
    int64_t src, dst;  // first physical row of a live block in the source / in the output
    int64_t n;         // its logical rows
    int64_t wbase;     // validity words of the blocks before this one
};

// Why every 16-byte access below is aligned and inside its arrays.  hipMalloc bases are 256-byte aligned.  A run starts at
// a multiple of 32 rows in the source and in the output and is a multiple of 32 rows long (blocks start on multiples of 32
// and the run counts its last block's padding), so it starts at a multiple of 32 * W >= 32 bytes on either side.  A lane
// takes R = 16 / min(WS, WD) consecutive rows -- 2, 4, 8 or 16: R divides 32 -- at R * k rows into its run: R * WS and R * WD
// are multiples of 16, so both spans are 16-byte aligned, and a span never crosses its run's padded end.  The padded end of a
// table's LAST block may lie up to 31 rows behind Table::phys_rows: table_reserve keeps kTileRows (2048) rows of slack
// behind phys_rows in every column, on the source side and in the output.
template <int WS, int WD, bool LUT>
__global__ __launch_bounds__(kCcThreads) void k_cc_transcode(const void *__restrict__ src, int64_t sbase, void *__restrict__ dst, int64_t dbase,
                                                             const CcRun *__restrict__ runs, int nr, int64_t T,
                                                             const int32_t *__restrict__ lut, int32_t n_lut) {
    constexpr int WN = WS < WD ? WS : WD;
    constexpr int R = 16 / WN;          // rows per lane
    constexpr int NS = R * WS / 16;     // 16-byte loads per lane
    constexpr int ND = R * WD / 16;     // 16-byte stores per lane
    const int64_t i = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) * R;
    if (i >= T) return;
    const int a = block_of(runs, nr, i - (int64_t)(threadIdx.x & 63) * R, i, &CcRun::lbase);
    const int64_t off = i - runs[a].lbase;
    const uint4 *sp = (const uint4 *)((const char *)src + (size_t)(runs[a].src + off) * WS);
    uint4 *dp = (uint4 *)((char *)dst + (size_t)(runs[a].dst + off) * WD);
    uint32_t in[NS * 4], out[ND * 4];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const uint4 q = sp[j];
        in[4 * j] = q.x;
        in[4 * j + 1] = q.y;
        in[4 * j + 2] = q.z;
        in[4 * j + 3] = q.w;
    }
#pragma unroll
    for (int j = 0; j < ND * 4; j++) out[j] = 0;
#pragma unroll
    for (int k = 0; k < R; k++) {
        uint64_t u;
        if (WS == 8) u = (uint64_t)in[2 * k] | ((uint64_t)in[2 * k + 1] << 32);
        else if (WS == 4) u = in[k];
        else if (WS == 2) u = (in[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        else u = (in[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        uint64_t v = (uint64_t)sbase + u;
        if (LUT) {
            // the stored bits of an unpopulated row are arbitrary: an id outside the table reads entry 0
            const int64_t id = (int64_t)v;
            v = (uint64_t)(int64_t)lut[(id >= 0 && id < (int64_t)n_lut) ? id : 0];
        }
        const uint64_t o = v - (uint64_t)dbase;  // (truncated to WD bytes: what an unpopulated row leaves is never looked at)
        if (WD == 8) {
            out[2 * k] = (uint32_t)o;
            out[2 * k + 1] = (uint32_t)(o >> 32);
        } else if (WD == 4) {
            out[k] = (uint32_t)o;
        } else if (WD == 2) {
            out[k >> 1] |= ((uint32_t)o & 0xFFFFu) << (16 * (k & 1));
        } else {
            out[k >> 2] |= ((uint32_t)o & 0xFFu) << (8 * (k & 3));
        }
    }
#pragma unroll
    for (int j = 0; j < ND; j++) dp[j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
}

// ---- validity words of one source's blocks in the output: n_words of them, a lane each.  valid == nullptr: the source
// column is fully populated -- ones.  The bits behind a block's last row are zero.
__global__ __launch_bounds__(kCcThreads) void k_cc_valid(const uint32_t *__restrict__ valid, const CcBlk *__restrict__ blk, int nb, int64_t n_words,
                                                         uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (i >= n_words) return;
    const CcBlk B = blk[block_of(blk, nb, i - (threadIdx.x & 63), i, &CcBlk::wbase)];
    const int64_t w = i - B.wbase;
    uint32_t bits = valid ? valid[(B.src >> 5) + w] : 0xFFFFFFFFu;
    const int64_t left = B.n - w * 32;  // >= 1: the block has ceil(n / 32) words
    if (left < 32) bits &= (1u << left) - 1u;
    out[(B.dst >> 5) + w] = bits;
}

namespace {

struct CcPiece {
    const void *src;
    int64_t sbase;
    void *dst;
    int64_t dbase;
    const CcRun *runs;
    int nr;
    int64_t T;
    const int32_t *lut;
    int32_t n_lut;
};

template <int WS, int WD, bool LUT>
void launch_tc(const CcPiece &p, hipStream_t st) {
    constexpr int R = 16 / (WS < WD ? WS : WD);
    hipLaunchKernelGGL((k_cc_transcode<WS, WD, LUT>), dim3(grid_for(p.T / R, kCcThreads)), dim3(kCcThreads), 0, st, p.src, p.sbase, p.dst, p.dbase,
                       p.runs, p.nr, p.T, p.lut, p.n_lut);
}

// the (WS, WD) pairs the storage rule can produce: widening and equal widths, every pair of {1, 2, 4} (str ids can narrow:
// a column sybl_table_set_dict returned to int32 ids in a compact table), 8 -> 8.  Anything else is a bug, not a fallback.
bool launch_transcode(int ws, int wd, const CcPiece &p, hipStream_t st) {
#define CC_PAIR(S, D)                                 \
    case S * 16 + D:                                  \
        if (p.lut) launch_tc<S, D, true>(p, st);      \
        else launch_tc<S, D, false>(p, st);           \
        return true;
#define CC_PAIR_PLAIN(S, D)                           \
    case S * 16 + D:                                  \
        if (p.lut) return false;                      \
        launch_tc<S, D, false>(p, st);                \
        return true;
    switch (ws * 16 + wd) {
        CC_PAIR(1, 1) CC_PAIR(1, 2) CC_PAIR(1, 4)
        CC_PAIR(2, 1) CC_PAIR(2, 2) CC_PAIR(2, 4)
        CC_PAIR(4, 1) CC_PAIR(4, 2) CC_PAIR(4, 4)
        CC_PAIR_PLAIN(1, 8) CC_PAIR_PLAIN(2, 8) CC_PAIR_PLAIN(4, 8) CC_PAIR_PLAIN(8, 8)
    default: return false;
    }
#undef CC_PAIR
#undef CC_PAIR_PLAIN
}

struct Source {
    Table *t = nullptr;
    std::vector<CcRun> runs;
    std::vector<CcBlk> blks;
    std::vector<int64_t> blk_ix;  // index of each live block in t->blocks
    int64_t rows = 0, padded = 0;
    int64_t first_out = 0;        // index of its first block among the output's
    CcRun *d_runs = nullptr;
    CcBlk *d_blks = nullptr;
};

int run(const sybl_concat_desc *d, Table *o, sybl_concat_stats *S) {
    Table *t0 = d->tables[0];
    Ctx *ctx = t0->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    const int ns = d->n_tables;
    if (d->n_columns < 0) return fail(SYBL_E_INVAL, "sybl_table_concat: bad column list");
    if ((rc = load_sync_all(ctx))) return rc;
    for (int s = 0; s < ns; s++)
        if ((rc = table_ensure_stats(d->tables[s]))) return rc;  // (the tracked extrema and block statistics; no version moves)

    // ---- the output's columns: the named ones in the order named, each once; else the union in first-seen order
    std::vector<std::string> names;
    if (d->columns && d->n_columns > 0) {
        for (int i = 0; i < d->n_columns; i++) {
            const char *nm = d->columns[i];
            bool held = false;
            for (int s = 0; s < ns && nm; s++) held = held || d->tables[s]->find(nm);
            if (!held) return fail(SYBL_E_INVAL, "sybl_table_concat: unknown column '%s'", nm ? nm : "(null)");
            if (std::find(names.begin(), names.end(), nm) == names.end()) names.push_back(nm);
        }
    } else {
        for (int s = 0; s < ns; s++)
            for (auto &cp : d->tables[s]->cols)
                if (std::find(names.begin(), names.end(), cp->name) == names.end()) names.push_back(cp->name);
    }
    const size_t nc = names.size();
    std::vector<std::vector<const Column *>> sc(nc, std::vector<const Column *>((size_t)ns, nullptr));  // [column][source]
    bool compact = true;
    for (int s = 0; s < ns; s++) compact = compact && d->tables[s]->compact_mode;
    o->compact_mode = compact;

    // ---- the output's blocks: the sources' live non-empty blocks in order, each at the next multiple of 32 rows
    std::vector<Source> src((size_t)ns);
    std::vector<Segment> osegs;
    int64_t N = 0, cur = 0, n_runs = 0;
    for (int s = 0; s < ns; s++) {
        Source &Z = src[(size_t)s];
        Z.t = d->tables[s];
        Z.first_out = (int64_t)osegs.size();
        int64_t words = 0;
        for (size_t b = 0; b < Z.t->blocks.size(); b++) {
            const Segment &blk = Z.t->blocks[b];
            if (blk.n <= 0) continue;  // (a dead block, sybl_table_refresh)
            const int64_t pad = round_up(blk.n, 32);
            Z.blks.push_back(CcBlk{blk.start, cur, blk.n, words});
            Z.blk_ix.push_back((int64_t)b);
            if (!Z.runs.empty() && Z.runs.back().src + Z.runs.back().rows == blk.start) Z.runs.back().rows += pad;
            else Z.runs.push_back(CcRun{blk.start, cur, pad, Z.padded});
            osegs.push_back(Segment{cur, blk.n});
            words += pad / 32;
            Z.padded += pad;
            Z.rows += blk.n;
            cur += pad;
        }
        N += Z.rows;
        n_runs += (int64_t)Z.runs.size();
    }
    const int64_t nb_out = (int64_t)osegs.size();
    const int64_t phys_out = nb_out ? osegs.back().start + osegs.back().n : 0;

    // ---- columns: type, IntInfo, has_missing, the merged dictionary and the id tables
    std::vector<std::vector<std::vector<int32_t>>> luts(nc, std::vector<std::vector<int32_t>>((size_t)ns));  // empty: ids unchanged
    for (size_t k = 0; k < nc; k++) {
        auto n = std::make_unique<Column>();
        n->name = names[k];
        int first = -1;
        bool all_given = true, lacking = false;
        int64_t imin = INT64_MAX, imax = INT64_MIN;
        for (int s = 0; s < ns; s++) {
            const Column *c = src[(size_t)s].t->find(names[k].c_str());
            sc[k][(size_t)s] = c;
            if (!c) {
                lacking = lacking || src[(size_t)s].rows > 0;
                continue;
            }
            if (first < 0) {
                first = s;
                n->type = c->type;
            } else if (c->type != n->type) {
                return fail(SYBL_E_INVAL, "sybl_table_concat: column '%s' is a %s column in table %d ('%s') and a %s column in table %d ('%s')",
                            names[k].c_str(), type_name(n->type), first, src[(size_t)first].t->name.c_str(), type_name(c->type), s,
                            src[(size_t)s].t->name.c_str());
            }
            all_given = all_given && c->info_given;
            imin = std::min(imin, c->info_min);
            imax = std::max(imax, c->info_max);
            n->has_missing = n->has_missing || c->has_missing;
            if (c->type == SYBL_INT_VAL) continue;
            // the first holder's dictionary id for id, then each later one's strings in its id order where they are new
            std::vector<int32_t> &lut = luts[k][(size_t)s];
            bool same = true;
            lut.resize(c->dict.size());
            for (size_t i = 0; i < c->dict.size(); i++) {
                lut[i] = dict_intern(n.get(), c->dict[i]);
                same = same && lut[i] == (int32_t)i;
            }
            if (same) lut.clear();
        }
        n->has_missing = n->has_missing || lacking;
        n->info_given = n->type == SYBL_INT_VAL && all_given;
        if (n->info_given) {
            n->info_min = imin;
            n->info_max = imax;
        } else {
            n->info_min = 1;  // (info_min > info_max: the exact extrema are in force)
            n->info_max = 0;
        }
        n->elem = n->canon();
        o->col_ix[n->name] = (int)o->cols.size();
        o->cols.push_back(std::move(n));
    }

    // ---- storage: compact iff every source is, each column at the narrowest width that holds the sources' tracked extrema
    // (a remapped str source: the extrema of its id table over the ids it tracks)
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        if (n->type == SYBL_SET_VAL) continue;
        bool any = false;
        int64_t lo = INT64_MAX, hi = INT64_MIN, pop = 0;
        for (int s = 0; s < ns; s++) {
            const Column *c = sc[k][(size_t)s];
            if (!c || c->n_pop <= 0) continue;
            int64_t a = c->exact_min, b = c->exact_max;
            const std::vector<int32_t> &lut = luts[k][(size_t)s];
            if (!lut.empty()) {
                const int64_t i0 = std::max<int64_t>(a, 0), i1 = std::min<int64_t>(b, (int64_t)lut.size() - 1);
                a = INT64_MAX;
                b = INT64_MIN;
                for (int64_t i = i0; i <= i1; i++) {
                    a = std::min<int64_t>(a, lut[(size_t)i]);
                    b = std::max<int64_t>(b, lut[(size_t)i]);
                }
                if (a > b) continue;
            }
            any = true;
            lo = std::min(lo, a);
            hi = std::max(hi, b);
            pop += c->n_pop;
        }
        if (compact) fit_storage(n->canon(), any, lo, hi, &n->elem, &n->vbase);
        n->exact_min = lo;
        n->exact_max = hi;
        n->n_pop = pop;
    }

    S->rows = N;
    S->blocks = nb_out;
    S->tables = ns;
    S->columns = (int32_t)nc;
    S->runs = (int32_t)std::min<int64_t>(n_runs, INT32_MAX);
    if (N == 0) {  // (the columns and no blocks; no kernel runs)
        for (auto &cp : o->cols) {
            cp->exact_min = INT64_MAX;
            cp->exact_max = INT64_MIN;
            cp->n_pop = 0;
        }
        return SYBL_OK;
    }
    if (nb_out > INT32_MAX) return fail(SYBL_E_INVAL, "sybl_table_concat: %lld blocks are more than a launch counts", (long long)nb_out);

    // ---- device copies of the run and block lists, the id tables
    GatherPool pool;
    hipEvent_t ev[3];
    for (Source &Z : src) {
        if (Z.rows == 0) continue;
        if ((rc = pool.alloc(&Z.d_runs, Z.runs.size(), "concat runs"))) return rc;
        if ((rc = pool.alloc(&Z.d_blks, Z.blks.size(), "concat blocks"))) return rc;
        if ((rc = host_to_device(ctx, Z.d_runs, Z.runs.data(), Z.runs.size() * sizeof(CcRun), "concat runs"))) return rc;
        if ((rc = host_to_device(ctx, Z.d_blks, Z.blks.data(), Z.blks.size() * sizeof(CcBlk), "concat blocks"))) return rc;
    }
    std::vector<std::vector<int32_t *>> d_luts(nc, std::vector<int32_t *>((size_t)ns, nullptr));
    for (size_t k = 0; k < nc; k++) {
        if (o->cols[k]->type != SYBL_STR_VAL) continue;
        for (int s = 0; s < ns; s++) {
            const std::vector<int32_t> &lut = luts[k][(size_t)s];
            if (lut.empty() || src[(size_t)s].rows == 0) continue;
            if ((rc = pool.alloc(&d_luts[k][(size_t)s], lut.size(), "concat id table"))) return rc;
            if ((rc = host_to_device(ctx, d_luts[k][(size_t)s], lut.data(), lut.size() * 4, "concat id table"))) return rc;
        }
    }

    // ---- the output's arrays, once, at their final size
    std::vector<char> recompute(nc, 0);
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        bool bitmap = false;
        for (int s = 0; s < ns; s++) {
            const Column *c = sc[k][(size_t)s];
            if (c ? c->d_valid != nullptr : src[(size_t)s].rows > 0) bitmap = true;
            if (c && n->type != SYBL_SET_VAL && !c->d_data && src[(size_t)s].rows > 0) bitmap = true;  // (rows never written: unpopulated)
        }
        if (n->type != SYBL_SET_VAL && (rc = table_reserve(o, n, phys_out))) return rc;
        if (bitmap && (rc = valid_reserve(o, n, phys_out))) return rc;  // (zeroed)
    }

    // ---- copies and transcodes, source by source
    if ((rc = pool.event(&ev[0], st))) return rc;
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        for (int s = 0; s < ns; s++) {
            const Source &Z = src[(size_t)s];
            if (Z.rows == 0) continue;
            const Column *c = sc[k][(size_t)s];
            const bool holds = c && (n->type == SYBL_SET_VAL || c->d_data);
            if (n->d_valid && holds) {
                const int64_t words = Z.padded / 32;
                hipLaunchKernelGGL(k_cc_valid, dim3(grid_for(words, kCcThreads)), dim3(kCcThreads), 0, st, (const uint32_t *)c->d_valid,
                                   (const CcBlk *)Z.d_blks, (int)Z.blks.size(), words, n->d_valid);
                SYBL_HIP(hipGetLastError());
                S->copy_bytes += words * 4 * (c->d_valid ? 2 : 1);
            }
            if (n->type == SYBL_SET_VAL) continue;
            if (!holds) {  // unpopulated rows for its blocks
                for (const CcRun &r : Z.runs)
                    SYBL_HIP(hipMemsetAsync((char *)n->d_data + (size_t)r.dst * (size_t)n->elem, 0, (size_t)r.rows * (size_t)n->elem, st));
                S->copy_bytes += Z.padded * (int64_t)n->elem;
                continue;
            }
            const int32_t *lut = d_luts[k][(size_t)s];
            if (!lut && c->elem == n->elem && c->vbase == n->vbase) {
                for (const CcRun &r : Z.runs)
                    SYBL_HIP(hipMemcpyAsync((char *)n->d_data + (size_t)r.dst * (size_t)n->elem, (const char *)c->d_data + (size_t)r.src * (size_t)c->elem,
                                            (size_t)r.rows * (size_t)n->elem, hipMemcpyDeviceToDevice, st));
                S->copies++;
            } else {
                const CcPiece p{c->d_data, c->vbase, n->d_data, n->vbase, Z.d_runs, (int)Z.runs.size(), Z.padded, lut, (int32_t)luts[k][(size_t)s].size()};
                if (!launch_transcode(c->elem, n->elem, p, st))
                    return fail(SYBL_E_STATE, "sybl_table_concat: no transcode from %d to %d bytes%s for column '%s' (internal error)", c->elem, n->elem,
                                lut ? " through an id table" : "", n->name.c_str());
                SYBL_HIP(hipGetLastError());
                if (lut) {
                    S->lut_transcodes++;
                    S->copy_bytes += (int64_t)luts[k][(size_t)s].size() * 4;
                    recompute[k] = 1;
                } else {
                    S->transcodes++;
                }
            }
            S->copy_bytes += Z.padded * (int64_t)(c->elem + n->elem);
        }
    }
    if ((rc = pool.event(&ev[1], st))) return rc;

    // ---- block statistics: recomputed where ids were remapped (the extrema with them); else the sources' own
    std::vector<Column *> remapped;
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        if (!recompute[k]) continue;
        n->exact_min = INT64_MAX;
        n->exact_max = INT64_MIN;
        n->n_pop = 0;
        remapped.push_back(n);
    }
    Segment *d_osegs = nullptr;
    if (!remapped.empty()) {
        if ((rc = pool.alloc(&d_osegs, (size_t)nb_out, "concat blocks"))) return rc;
        if ((rc = host_to_device(ctx, d_osegs, osegs.data(), osegs.size() * sizeof(Segment), "concat blocks"))) return rc;
    }
    if ((rc = derived_block_stats(o, remapped, d_osegs, nb_out, pool, "concat statistics", &ev[2]))) return rc;  // the ONE wait of the call

    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        if (n->type == SYBL_SET_VAL || recompute[k]) continue;
        n->blk_min.assign((size_t)nb_out, INT64_MAX);
        n->blk_max.assign((size_t)nb_out, INT64_MIN);
        n->blk_pop.assign((size_t)nb_out, 0);
        for (int s = 0; s < ns; s++) {
            const Source &Z = src[(size_t)s];
            const Column *c = sc[k][(size_t)s];
            if (!c || !c->d_data) continue;
            for (size_t b = 0; b < Z.blk_ix.size(); b++) {
                const size_t from = (size_t)Z.blk_ix[b], to = (size_t)Z.first_out + b;
                if (from >= c->blk_pop.size()) return fail(SYBL_E_STATE, "sybl_table_concat: column '%s' of table %d lacks its block statistics", n->name.c_str(), s);
                n->blk_min[to] = c->blk_min[from];
                n->blk_max[to] = c->blk_max[from];
                n->blk_pop[to] = c->blk_pop[from];
            }
        }
        n->stats_blocks = nb_out;
    }

    // ---- set columns: the host CSR over the output's physical rows, member ids through the id table
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        if (n->type != SYBL_SET_VAL) continue;
        n->h_set_off.assign(1, 0);
        n->h_set_off.reserve((size_t)phys_out + 1);
        for (int s = 0; s < ns; s++) {
            const Source &Z = src[(size_t)s];
            const Column *c = sc[k][(size_t)s];
            const std::vector<int32_t> &lut = luts[k][(size_t)s];
            for (const CcBlk &B : Z.blks) {
                while ((int64_t)n->h_set_off.size() < B.dst + 1) n->h_set_off.push_back(n->h_set_off.back());  // (padding rows: empty sets)
                for (int64_t r = 0; r < B.n; r++) {
                    const size_t row = (size_t)(B.src + r);
                    if (c && row + 1 < c->h_set_off.size()) {
                        for (int64_t m = c->h_set_off[row]; m < c->h_set_off[row + 1]; m++) {
                            const int32_t id = c->h_set_vals[(size_t)m];
                            n->h_set_vals.push_back(lut.empty() ? id : lut[(size_t)id]);
                        }
                    }
                    n->h_set_off.push_back((int64_t)n->h_set_vals.size());
                }
            }
        }
        n->set_dirty = true;
    }

    // ---- the table
    o->blocks = osegs;
    o->phys_rows = phys_out;
    o->logical_rows = N;
    o->version++;
    for (size_t k = 0; k < nc; k++)
        if (o->cols[k]->type == SYBL_SET_VAL && (rc = column_upload_set(o, o->cols[k].get()))) return rc;
    float f = 0;
    SYBL_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
    S->copy_ms = f;
    SYBL_HIP(hipEventElapsedTime(&f, ev[1], ev[2]));
    S->stats_ms = f;
    return SYBL_OK;
}

}  // namespace

int concat_run(const sybl_concat_desc *d, sybl_table **out) {
    Ctx *ctx = d->tables[0]->ctx;
    TableOwner O;
    int rc = derived_new_table(ctx, d->tables[0]->name, "sybl_table_concat", O);
    if (rc) return rc;
    return derived_call(ctx, "sybl_table_concat", O, out, [&] { return run(d, O.t, &O.t->concat_stats); });
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_concat(const sybl_concat_desc *d, sybl_table **out) {
    if (out) *out = nullptr;
    if (!d || !out) return fail(SYBL_E_INVAL, "sybl_table_concat: NULL argument");
    if (d->n_tables < 1 || !d->tables) return fail(SYBL_E_INVAL, "sybl_table_concat: no tables");
    for (int s = 0; s < d->n_tables; s++)
        if (!d->tables[s]) return fail(SYBL_E_INVAL, "sybl_table_concat: table %d is NULL", s);
    SYBL_API_GUARD(d->tables[0]);
    for (int s = 1; s < d->n_tables; s++)
        if (d->tables[s]->ctx != d->tables[0]->ctx)
            return fail(SYBL_E_INVAL, "sybl_table_concat: table %d belongs to another context than table 0", s);
    return concat_run(d, out);
}

int sybl_table_concat_stats(const sybl_table *t, sybl_concat_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_concat_stats: NULL argument");
    *out = t->concat_stats;
    return SYBL_OK;
}

}  // extern "C"
