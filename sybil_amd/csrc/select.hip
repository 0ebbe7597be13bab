// select.hip -- the rows of a resident table that pass a filter, as a NEW resident table: the third call of the samples /
// digest family.  The semantics are restated in include/sybilgpu.h ("select") and DESIGN.md 3.9; this file is the device
// work between the two halves that exist -- filters to a bit per row (samples.hip), a row list to a table (digest.hip) --
// and the host code that drives all of it.
//
//   filter        k_prefilter (kernels.hip) over the filter slots the planner lowered (plan_filter_slots), ONE pass over the
//                 whole table into a zeroed bitmap indexed by physical row.  No windows: nothing ends the visit early.
//                 Without filters there is no bitmap.
//   k_sel_count   per source block, the popcount of its bitmap words (smp_count_block, bitmap_rank.h); one readback of an
//                 int64 per block; the host takes the exclusive prefix and M, so everything behind is sized exactly.
//   k_sel_rows    a workgroup per source block walks the block's words 256 at a time, a word per lane.  The rank of a
//                 lane's first matching row = the block's exclusive prefix + the matches of the chunks before + an
//                 exclusive popcount scan (within the wave by shuffles, across the waves through LDS): the structure of
//                 k_smp_compact.  The matching rows' physical row numbers go to rows[rank], ascending: no atomics, every
//                 position is written exactly once.
//   gather        gather_rows (derived.h, digest.hip): the row list is a permutation for digest's machinery.
// The call wrapper and the column list are derived.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitmap_rank.h"
#include "derived.h"

namespace sybl {

constexpr int kSelMaxFilterCols = 8;  // k_prefilter is instantiated for 1..8 slots

// ---- m_b: the matching rows of source block b
__global__ __launch_bounds__(kSmpThreads) void k_sel_count(const uint32_t *bits, const SmpBlock *blk, int64_t *cnt) {
    smp_count_block(bits, 0, blk, cnt);
}

// ---- the ascending row list.  excl[b] = matching rows before block b; M = all of them: rows[] has M places (a rank beyond
// them would mean the bitmap changed since the count: nothing is stored there).
__global__ __launch_bounds__(kSmpThreads) void k_sel_rows(const uint32_t *bits, const SmpBlock *blk, const int64_t *excl, int64_t M,
                                                          uint32_t *__restrict__ rows) {
    __shared__ int32_t wave_tot[kSmpThreads / 64];
    const SmpBlock B = blk[blockIdx.x];
    const int64_t words = (B.n + 31) >> 5, w0 = B.start >> 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = excl[blockIdx.x];
    for (int64_t base = 0; base < words; base += kSmpThreads) {
        const int64_t i = base + tid;
        uint32_t w = i < words ? smp_word(bits, w0, i, B.n) : 0u;
        const int32_t pc = __popc(w);
        const int32_t incl = wave_scan_incl(pc);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int32_t before = 0, all = 0;
        for (int k = 0; k < kSmpThreads / 64; k++) {
            const int32_t t = wave_tot[k];
            if (k < wave) before += t;
            all += t;
        }
        int64_t rank = carry + before + (incl - pc);
        const uint32_t row0 = (uint32_t)(B.start + i * 32);
        while (w) {
            const int bit = __ffs(w) - 1;
            w &= w - 1;
            if (rank < M) rows[rank] = row0 + (uint32_t)bit;
            rank++;
        }
        carry += all;
        __syncthreads();  // (wave_tot is written again)
    }
}

namespace {

// the bytes one pass over a filter column reads, from the shapes
int64_t filter_col_bytes(const Column *c, int64_t N) {
    int64_t b = c->d_valid ? (N + 7) / 8 : 0;
    if (c->type == SYBL_SET_VAL) b += N * 8 + (int64_t)c->h_set_vals.size() * 4;  // (CSR offsets, members)
    else if (c->d_data) b += N * (int64_t)c->elem;
    return b;
}

int run(Table *t, const sybl_select_desc *d, int64_t block_rows, Table *o, sybl_select_stats *S) {
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    if (d->n_filters < 0 || (d->n_filters > 0 && !d->filters)) return fail(SYBL_E_INVAL, "select: bad filter list");
    if (d->n_columns < 0) return fail(SYBL_E_INVAL, "select: bad column list");
    if ((rc = load_sync_all(ctx))) return rc;

    // ---- the output's columns (NULL / 0: every column), each once, in the order named
    std::vector<Column *> src;
    if ((rc = resolve_columns(t, d->columns, d->n_columns, "select", "", nullptr, &src))) return rc;

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
    if (n_slots > kSelMaxFilterCols)
        return fail(SYBL_E_INVAL, "select: filters on %d distinct columns; the limit is %d", n_slots, kSelMaxFilterCols);
    const bool filtered = n_slots > 0;

    gather_make_columns(t, src, o);

    // ---- the source rows: every block (a dead one has no rows and matches nothing), the live ones as runs for the filter
    const int64_t B = (int64_t)t->blocks.size();
    std::vector<SmpBlock> hb((size_t)B);
    std::vector<int64_t> hcnt((size_t)B), hexcl((size_t)B);
    std::vector<Segment> runs;
    int64_t N = 0, row_hi = 0, live = 0;
    for (int64_t b = 0; b < B; b++) {
        const Segment &blk = t->blocks[(size_t)b];
        const int64_t n = std::max<int64_t>(blk.n, 0);
        hb[(size_t)b] = SmpBlock{blk.start, n, N};
        hcnt[(size_t)b] = n;
        N += n;
        if (n == 0) continue;
        live++;
        row_hi = std::max(row_hi, blk.start + n);
        if (!runs.empty() && runs.back().start + runs.back().n == blk.start) runs.back().n += n;
        else runs.push_back(Segment{blk.start, n});
    }
    if (t->phys_rows > (int64_t)UINT32_MAX)
        return fail(SYBL_E_INVAL, "select: %lld physical rows (dead blocks included) are more than a 32-bit row number holds", (long long)t->phys_rows);
    S->rows_in = N;
    S->blocks_in = live;
    if (N == 0 || fp->q.never_matches) return SYBL_OK;  // (the columns and no blocks; no kernel runs)

    GatherPool pool;
    hipEvent_t ev[6];
    const int64_t n_words = (row_hi + 31) >> 5;
    SmpBlock *d_blk = nullptr;
    int64_t *d_cnt = nullptr, *d_excl = nullptr;
    uint32_t *bits = nullptr;
    if ((rc = pool.alloc(&d_blk, (size_t)B, "select blocks"))) return rc;
    if ((rc = pool.alloc(&d_excl, (size_t)B, "select ranks"))) return rc;
    if ((rc = host_to_device(ctx, d_blk, hb.data(), (size_t)B * sizeof(SmpBlock), "select blocks"))) return rc;

    // ---- filter + count
    if (filtered) {
        const int n_wg = ctx->n_cus > 0 ? ctx->n_cus : 256;
        ScanPlan *d_plan = nullptr;
        Segment *d_segs = nullptr;
        int32_t *d_wgb = nullptr;
        std::vector<Segment> segs;
        std::vector<int32_t> wg_seg_begin;
        deal_tiles(runs, n_wg, segs, wg_seg_begin);
        if ((rc = pool.alloc(&bits, (size_t)n_words, "select bitmap"))) return rc;
        if ((rc = pool.alloc(&d_cnt, (size_t)B, "select counts"))) return rc;
        if ((rc = pool.alloc(&d_plan, 1, "select plan"))) return rc;
        if ((rc = pool.alloc(&d_segs, segs.size(), "select segments"))) return rc;
        if ((rc = pool.alloc(&d_wgb, wg_seg_begin.size(), "select segments"))) return rc;
        if ((rc = host_to_device(ctx, d_segs, segs.data(), segs.size() * sizeof(Segment), "select segments"))) return rc;
        if ((rc = host_to_device(ctx, d_wgb, wg_seg_begin.data(), wg_seg_begin.size() * sizeof(int32_t), "select segments"))) return rc;
        plan.segs = d_segs;
        plan.wg_seg_begin = d_wgb;
        static_assert(sizeof(ScanPlan) % 4 == 0, "host_to_device copies whole words");
        if ((rc = host_to_device(ctx, d_plan, &plan, sizeof(ScanPlan), "select plan"))) return rc;
        if ((rc = pool.event(&ev[0], st))) return rc;
        // (zeroed: the padding to 32 rows and dead blocks read 0)
        SYBL_HIP(hipMemsetAsync(bits, 0, (size_t)n_words * 4, st));
        hipError_t e = launch_prefilter(d_plan, n_slots, bits, n_wg, st);
        if (e != hipSuccess) return hip_fail(e, "k_prefilter");
        if ((rc = pool.event(&ev[1], st))) return rc;
        hipLaunchKernelGGL(k_sel_count, dim3((unsigned)B), dim3(kSmpThreads), 0, st, (const uint32_t *)bits, (const SmpBlock *)d_blk, d_cnt);
        SYBL_HIP(hipGetLastError());
        if ((rc = pool.event(&ev[2], st))) return rc;
        SYBL_HIP(hipMemcpyAsync(hcnt.data(), d_cnt, (size_t)B * 8, hipMemcpyDeviceToHost, st));  // one int64 per block, one copy
        SYBL_HIP(hipStreamSynchronize(st));
        std::vector<const Column *> fcols;  // (a slot per distinct filter column)
        for (int i = 0; i < d->n_filters; i++) {
            const Column *c = d->filters[i].col ? t->find(d->filters[i].col) : nullptr;
            if (c && std::find(fcols.begin(), fcols.end(), c) == fcols.end()) fcols.push_back(c);
        }
        for (const Column *c : fcols) S->filter_bytes += filter_col_bytes(c, N);
        S->filter_bytes += 2 * n_words * 4;  // (the bitmap: zeroed, written)
        S->rows_bytes += n_words * 4 + B * ((int64_t)sizeof(SmpBlock) + 8);
        float f = 0;
        SYBL_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
        S->filter_ms = f;
        SYBL_HIP(hipEventElapsedTime(&f, ev[1], ev[2]));
        S->rows_ms = f;
    }
    // (without filters m_b is the block's row count)
    int64_t M = 0;
    for (int64_t b = 0; b < B; b++) {
        hexcl[(size_t)b] = M;
        M += hcnt[(size_t)b];
    }
    if (M == 0) return SYBL_OK;

    // ---- rows
    uint32_t *rows = nullptr;
    if ((rc = pool.alloc(&rows, (size_t)M, "select rows"))) return rc;
    if ((rc = host_to_device(ctx, d_excl, hexcl.data(), (size_t)B * 8, "select ranks"))) return rc;
    if ((rc = pool.event(&ev[3], st))) return rc;
    hipLaunchKernelGGL(k_sel_rows, dim3((unsigned)B), dim3(kSmpThreads), 0, st, (const uint32_t *)bits, (const SmpBlock *)d_blk,
                       (const int64_t *)d_excl, M, rows);
    SYBL_HIP(hipGetLastError());
    if ((rc = pool.event(&ev[4], st))) return rc;
    S->rows_bytes += (filtered ? n_words * 4 : 0) + B * ((int64_t)sizeof(SmpBlock) + 8) + M * 4;

    // ---- gather, statistics, set columns, the block writer
    if ((rc = gather_rows(t, src, rows, M, block_rows, o, pool, "select", &ev[5], &S->gather_bytes, &S->blocks_out))) return rc;
    S->rows_out = M;
    float f = 0;
    SYBL_HIP(hipEventElapsedTime(&f, ev[3], ev[4]));
    S->rows_ms += f;
    SYBL_HIP(hipEventElapsedTime(&f, ev[4], ev[5]));
    S->gather_ms = f;
    return SYBL_OK;
}

}  // namespace

int select_run(Table *t, const sybl_select_desc *d, sybl_table **out) {
    if (d->block_rows < 0 || d->block_rows > SYBL_BLOCK_ROWS)
        return fail(SYBL_E_INVAL, "select: block_rows %d is outside 0 .. %d", d->block_rows, SYBL_BLOCK_ROWS);
    const int64_t br = d->block_rows ? d->block_rows : SYBL_BLOCK_ROWS;
    TableOwner O;
    int rc = derived_new_table(t->ctx, t->name, "select", O);
    if (rc) return rc;
    return derived_call(t->ctx, "select", O, out, [&] { return run(t, d, br, O.t, &O.t->select_stats); });
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_select(sybl_table *t, const sybl_select_desc *d, sybl_table **out) {
    SYBL_API_GUARD(t);
    if (!t || !d || !out) return fail(SYBL_E_INVAL, "sybl_table_select: NULL argument");
    *out = nullptr;
    return select_run(t, d, out);
}

int sybl_table_select_stats(const sybl_table *t, sybl_select_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_select_stats: NULL argument");
    *out = t->select_stats;
    return SYBL_OK;
}

}  // extern "C"
