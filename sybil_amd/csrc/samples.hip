// samples.hip -- `sybil query -samples` on the resident table: the rows behind a filter, newest first or ordered by an int
// column (cmd_query.go:330-343, table_query.go:96-228, printer.go:388-476).  The semantics are restated in
// include/sybilgpu.h ("samples") and DESIGN.md; this file is the device work behind them and the host code that drives it.
//
//   filter        k_prefilter (kernels.hip) over the query's filter slots -- lowered by the planner itself
//                 (planner.cpp: plan_filter_slots) -- writes one bit per physical row.  A query without filters has no bitmap.
//   k_smp_count   per block, the popcount of its bitmap words: m_b.
//   k_smp_prefix  one workgroup: exclusive scan of m_b, continuing from the windows before; finds the visited prefix P and
//                 the matched count M -- the first block at which the running count is STRICTLY greater than the limit.
//   k_smp_compact ordered compaction: every matching row of blocks 0..P-1 whose rank lies in [W0, M) is written at
//                 position M-1-rank, i.e. in descending row order; for a sorted query also its order key.
//   sort          (sorted queries) a stable ascending radix sort of (key, position) on the order-REVERSING image of the
//                 value, then a stable 1-bit pass that moves the rows without the column to the front.  The input is in
//                 descending row order, so stability yields the tie rule (equal values: descending row).
//   k_smp_gather  one lane per (output row, column): value / dictionary id / set length and the validity bit;
//                 k_smp_gather_set copies the members of set columns behind a prefix over the L lengths (host).
//
// The reference stops at the first block prefix that exceeds the limit, so the work must follow the visited prefix and not
// the table: filter + count + prefix run over WINDOWS of consecutive blocks, the first of kSmpFirstWindow blocks, each next
// one kSmpWindowGrowth times larger; after each window the host reads back whether the limit was exceeded, and where.
// Every allocation is sized by a window or by M.  Ranks and counts are int64.
//
// Out of scope: -str-replace on samples, -encode-results of samples, the text form, multi-rank merging (the calls are
// rank-local; a host concatenates and truncates as node_aggregator.go:59-79 does).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>

#include "bitmap_rank.h"
#include "engine.h"

namespace sybl {

// The first window of blocks a samples query filters.  16 is a choice, not a measurement: one launch over 16 reference
// blocks (~1e6 rows) costs about what a launch costs at all, and most -samples queries (limit 100 or so, a filter that is
// not needle-in-haystack) are answered inside it.
constexpr int kSmpFirstWindow = 16;
constexpr int kSmpWindowGrowth = 4;
constexpr int kSmpPrefixThreads = 1024;
constexpr int kSmpMaxFilterCols = 8;       // k_prefilter is instantiated for 1..8 slots

// device state of one query: int64 words
enum { kSmpTotal = 0, kSmpDone = 1, kSmpP = 2, kSmpM = 3, kSmpStateWords = 4 };

// a column as the compaction (order key) and gather kernels read it
struct SmpCol {
    const void *base;        // INT / STR: stored values, `width` bytes per row; nullptr: no row has the column
    const uint32_t *valid;   // bit per physical row; nullptr = every row populated
    const int64_t *set_off;  // SET: CSR offsets per physical row
    int64_t vbase;
    int32_t width;
    int32_t is_set;
};

// value = vbase + zero-extended stored bits (8-byte columns hold the value itself: their base is 0)
__device__ __forceinline__ int64_t smp_load(const void *base, int width, int64_t vbase, int64_t row) {
    switch (width) {
    case 8: return ((const int64_t *)base)[row];
    case 4: return vbase + (int64_t)((const uint32_t *)base)[row];
    case 2: return vbase + (int64_t)((const uint16_t *)base)[row];
    default: return vbase + (int64_t)((const uint8_t *)base)[row];
    }
}

__device__ __forceinline__ bool smp_valid(const uint32_t *valid, int64_t row) {
    return valid == nullptr || ((valid[row >> 5] >> (row & 31)) & 1u);
}

// ---- m_b (bitmap_rank.h: the block descriptor, smp_word, wave_scan_incl and the count are shared with select.hip)
__global__ __launch_bounds__(kSmpThreads) void k_smp_count(const uint32_t *bits, int64_t word0, const SmpBlock *blk, int64_t *cnt) {
    smp_count_block(bits, word0, blk, cnt);
}

// ---- exclusive scan of the window's m_b (excl[b] = matching rows before block b, table-wide), continuing from the windows
// before; the first block at which the running count exceeds the limit closes the visit: P = its number + 1, M = the count
// there.  The counts never decrease, so exactly one block has  excl <= limit < excl + m_b : one lane writes, no atomics.
__global__ __launch_bounds__(kSmpPrefixThreads) void k_smp_prefix(const int64_t *cnt, int64_t *excl, int nb, int64_t block0, int64_t limit,
                                                                  int64_t *state) {
    __shared__ int64_t wave_tot[kSmpPrefixThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = state[kSmpTotal];
    const bool done = state[kSmpDone] != 0;
    __syncthreads();  // (every lane has read the state before a lane writes it)
    for (int base = 0; base < nb; base += kSmpPrefixThreads) {
        const int i = base + tid;
        const int64_t v = i < nb ? cnt[i] : 0;
        int64_t incl = wave_scan_incl(v);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int64_t before = 0, all = 0;
        for (int w = 0; w < kSmpPrefixThreads / 64; w++) {
            const int64_t t = wave_tot[w];
            if (w < wave) before += t;
            all += t;
        }
        incl += carry + before;
        if (i < nb) {
            excl[i] = incl - v;
            if (!done && incl > limit && incl - v <= limit) {
                state[kSmpP] = block0 + i + 1;
                state[kSmpM] = incl;
                state[kSmpDone] = 1;
            }
        }
        carry += all;
        __syncthreads();  // (wave_tot is written again)
    }
    if (tid == 0) state[kSmpTotal] = carry;
}

// ---- ordered compaction.  A workgroup per block of the window walks the block's words 256 at a time: the rank of a
// lane's first matching row is  excl[b] + (matches in the chunks before) + (exclusive popcount scan: within the wave by
// shuffles, across the waves through LDS).  A row of rank r in [W0, M) lands at position M-1-r.
__global__ __launch_bounds__(kSmpThreads) void k_smp_compact(const uint32_t *bits, int64_t word0, const SmpBlock *blk, const int64_t *cnt,
                                                             const int64_t *excl, int64_t block0, int64_t P, int64_t M, int64_t W0,
                                                             int64_t *out_phys, int64_t *out_lrow, SmpCol order, int has_order, uint64_t *out_key,
                                                             uint32_t *out_present) {
    __shared__ int32_t wave_tot[kSmpThreads / 64];
    const int64_t b = blockIdx.x;
    if (block0 + b >= P) return;
    const int64_t r0 = excl[b], r1 = r0 + cnt[b];
    if (r1 <= W0 || r0 >= M) return;  // (uniform over the workgroup)
    const SmpBlock B = blk[b];
    const int64_t words = (B.n + 31) >> 5, w0 = (B.start >> 5) - word0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = r0;
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
        while (w) {
            const int bit = __ffs(w) - 1;
            w &= w - 1;
            if (rank >= W0 && rank < M) {
                const int64_t pos = M - 1 - rank;
                const int64_t in_block = i * 32 + bit, phys = B.start + in_block;
                out_phys[pos] = phys;
                out_lrow[pos] = B.lbase + in_block;
                if (has_order) {
                    const bool pop = order.base != nullptr && smp_valid(order.valid, phys);
                    // descending value = ascending key: the complement of the order-preserving unsigned image
                    out_key[pos] = pop ? ~((uint64_t)smp_load(order.base, order.width, order.vbase, phys) ^ 0x8000000000000000ull) : 0ull;
                    out_present[pos] = pop ? 1u : 0u;
                }
            }
            rank++;
        }
        carry += all;
        __syncthreads();  // (wave_tot is written again)
    }
}

__global__ void k_smp_iota(uint32_t *p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (uint32_t)i;
}

// the 1-bit keys of the second sort pass, in the order the first pass left the candidates in
__global__ void k_smp_flags(const uint32_t *present, const uint32_t *perm, int64_t n, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = present[perm[i]];
}

// the first L of the sorted candidates, or the last L reversed (order_asc: the reference reverses, then truncates)
__global__ void k_smp_pick(const uint32_t *perm, int64_t M, int64_t L, int asc, const int64_t *cand_phys, const int64_t *cand_lrow,
                           int64_t *out_phys, int64_t *out_lrow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const uint32_t j = perm[asc ? M - 1 - i : i];
    out_phys[i] = cand_phys[j];
    out_lrow[i] = cand_lrow[j];
}

// one lane per (output row, column): vals[c][i] = the value / dictionary id / set length, pop[c][i] = the validity bit
__global__ void k_smp_gather(const SmpCol *cols, int n_cols, const int64_t *phys, int64_t L, int64_t *vals, uint8_t *pop) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= L * n_cols) return;
    const int64_t c = idx / L, i = idx - c * L;
    const SmpCol C = cols[c];
    const int64_t row = phys[i];
    int64_t v = 0;
    bool p;
    if (C.is_set) {
        p = C.set_off != nullptr && smp_valid(C.valid, row);
        if (p) v = C.set_off[row + 1] - C.set_off[row];
    } else {
        p = C.base != nullptr && smp_valid(C.valid, row);
        if (p) v = smp_load(C.base, C.width, C.vbase, row);
    }
    vals[idx] = v;
    pop[idx] = p ? 1 : 0;
}

// the members of one set column: row i's extent of the table's CSR -> its extent of the output CSR
__global__ void k_smp_gather_set(const int64_t *set_off, const int32_t *set_vals, const int64_t *phys, int64_t L, const int64_t *out_off,
                                 int32_t *out_ids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int64_t o0 = out_off[i], n = out_off[i + 1] - o0;
    if (n <= 0) return;
    const int64_t s0 = set_off[phys[i]];
    for (int64_t k = 0; k < n; k++) out_ids[o0 + k] = set_vals[s0 + k];
}

// ------------------------------------------------------------------ the result

struct SamplesCol {
    std::string name;
    int type = SYBL_INT_VAL;
    std::vector<uint8_t> populated;
    std::vector<int64_t> ints;
    std::vector<int32_t> str_ids;
    std::vector<const char *> strings;
    std::vector<int64_t> set_off;
    std::vector<const char *> set_strings;
    std::unordered_map<int32_t, std::string> pool;  // the dictionary strings of exactly the ids that occur (node-based: stable)
};

struct Samples {
    std::shared_ptr<std::recursive_mutex> api_m;  // the ctx's lock, kept alive by the result
    sybl_samples_info info{};
    std::vector<SamplesCol> cols;
    std::vector<int64_t> row_ids;
    std::string rendered;
};

}  // namespace sybl

struct sybl_samples : sybl::Samples {};

namespace sybl {

inline std::shared_ptr<std::recursive_mutex> api_mutex_of(const sybl_samples *s) { return s ? s->api_m : nullptr; }

namespace {

// everything a run allocates on the device, freed on every exit
struct DevPool {
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> events;
    ~DevPool() {
        for (void *p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    template <typename T>
    int alloc(T **out, size_t n, const char *what) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) return hip_fail(e, what);  // (out of memory: SYBL_E_NOMEM)
        ptrs.push_back(p);
        *out = (T *)p;
        return SYBL_OK;
    }
};

// hipEvent time of the regions of one kind, summed after the stream has drained
struct Stopwatch {
    DevPool &pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    explicit Stopwatch(DevPool &p) : pool(p) {}
    int start(hipStream_t st) {
        hipEvent_t a = nullptr, b = nullptr;
        SYBL_HIP(hipEventCreate(&a));
        pool.events.push_back(a);
        SYBL_HIP(hipEventCreate(&b));
        pool.events.push_back(b);
        spans.emplace_back(a, b);
        SYBL_HIP(hipEventRecord(a, st));
        return SYBL_OK;
    }
    int stop(hipStream_t st) {
        SYBL_HIP(hipEventRecord(spans.back().second, st));
        return SYBL_OK;
    }
    int total(double *ms) {
        *ms = 0;
        for (auto &s : spans) {
            float f = 0;
            SYBL_HIP(hipEventElapsedTime(&f, s.first, s.second));
            *ms += f;
        }
        return SYBL_OK;
    }
};

template <typename T>
int upload(T *dst, const T *src, size_t n, hipStream_t st) {
    if (!n) return SYBL_OK;
    SYBL_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    SYBL_HIP(hipStreamSynchronize(st));  // (src is ordinary host memory the caller reuses)
    return SYBL_OK;
}
template <typename T>
int download(T *dst, const T *src, size_t n, hipStream_t st) {
    if (!n) return SYBL_OK;
    SYBL_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st));
    SYBL_HIP(hipStreamSynchronize(st));
    return SYBL_OK;
}

// one window of consecutive blocks [b0, b1) and what the visit left of it on the device
struct Window {
    int64_t b0 = 0, b1 = 0;
    int64_t word0 = 0;          // bitmap word of bits[0]
    uint32_t *bits = nullptr;   // nullptr: no filters
    SmpBlock *blk = nullptr;
    int64_t *cnt = nullptr, *excl = nullptr;
};

inline unsigned grid_for(int64_t n, int threads) { return (unsigned)std::max<int64_t>(1, (n + threads - 1) / threads); }

SmpCol col_desc(const Column *c) {
    SmpCol d{};
    d.valid = c->d_valid;
    d.vbase = c->vbase;
    d.width = c->elem;
    d.is_set = c->type == SYBL_SET_VAL;
    if (d.is_set) d.set_off = c->d_set_off;  // (nullptr: the column never held a row)
    else d.base = c->d_data;
    return d;
}

int run(Table *t, const sybl_samples_desc *d, Samples *R) {
    Ctx *ctx = t->ctx;
    int rc;
    if (d->limit < 0) return fail(SYBL_E_INVAL, "samples: limit %d is negative", d->limit);
    if (d->n_filters < 0 || (d->n_filters > 0 && !d->filters)) return fail(SYBL_E_INVAL, "samples: bad filter list");
    if (d->n_columns < 0) return fail(SYBL_E_INVAL, "samples: bad column list");

    // ---- the columns to return (NULL / 0: every column, LoadAllColumns), each once
    std::vector<Column *> out_cols;
    if (d->columns && d->n_columns > 0) {
        for (int i = 0; i < d->n_columns; i++) {
            Column *c = t->find(d->columns[i]);
            if (!c) return fail(SYBL_E_INVAL, "samples: unknown column '%s'", d->columns[i] ? d->columns[i] : "(null)");
            if (std::find(out_cols.begin(), out_cols.end(), c) == out_cols.end()) out_cols.push_back(c);
        }
    } else {
        for (auto &cp : t->cols) out_cols.push_back(cp.get());
    }
    // ---- the order
    Column *order = nullptr;
    const bool asc = d->order_asc != 0;
    if (d->order_by && d->order_by[0] && strcmp(d->order_by, "$COUNT") != 0) {
        order = t->find(d->order_by);
        if (!order) return fail(SYBL_E_INVAL, "samples: unknown order_by column '%s'", d->order_by);
        if (order->type != SYBL_INT_VAL)
            return fail(SYBL_E_INVAL, "samples: order_by '%s' is a %s column; only int columns order samples (dictionary ids mean nothing as an order)",
                        d->order_by, order->type == SYBL_STR_VAL ? "str" : "set");
    }

    SYBL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t B = (int64_t)t->blocks.size(), limit = d->limit;
    R->info.blocks_total = B;
    R->info.n_columns = (int32_t)out_cols.size();
    R->cols.resize(out_cols.size());
    for (size_t c = 0; c < out_cols.size(); c++) {
        R->cols[c].name = out_cols[c]->name;
        R->cols[c].type = out_cols[c]->type;
        if (out_cols[c]->type == SYBL_SET_VAL) {
            R->cols[c].set_off.assign(1, 0);
            if ((rc = column_upload_set(t, out_cols[c]))) return rc;
        }
    }

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
    if (n_slots > kSmpMaxFilterCols)
        return fail(SYBL_E_INVAL, "samples: filters on %d distinct columns; the limit is %d", n_slots, kSmpMaxFilterCols);
    const bool filtered = n_slots > 0;

    DevPool pool;
    Stopwatch t_filter(pool), t_select(pool);
    int64_t P = B, M = 0, blocks_filtered = 0;
    std::vector<Window> wins;
    std::vector<int64_t> lbase((size_t)B + 1, 0);
    for (int64_t b = 0; b < B; b++) lbase[(size_t)b + 1] = lbase[(size_t)b] + t->blocks[(size_t)b].n;

    if (!fp->q.never_matches && B > 0) {
        const int n_wg = ctx->n_cus > 0 ? ctx->n_cus : 256;
        int64_t *d_state = nullptr;
        ScanPlan *d_plan = nullptr;
        if ((rc = pool.alloc(&d_state, kSmpStateWords, "samples state"))) return rc;
        SYBL_HIP(hipMemsetAsync(d_state, 0, kSmpStateWords * 8, st));
        if (filtered && (rc = pool.alloc(&d_plan, 1, "samples plan"))) return rc;
        int64_t state[kSmpStateWords] = {0, 0, 0, 0};
        int64_t b0 = 0, span = kSmpFirstWindow;
        while (b0 < B && !state[kSmpDone]) {
            Window W;
            W.b0 = b0;
            W.b1 = std::min(B, b0 + span);
            const int64_t nb = W.b1 - W.b0;
            std::vector<SmpBlock> hb((size_t)nb);
            std::vector<int64_t> hcnt((size_t)nb);
            std::vector<Segment> runs;
            int64_t row_lo = INT64_MAX, row_hi = 0;
            for (int64_t k = 0; k < nb; k++) {
                const Segment &blk = t->blocks[(size_t)(W.b0 + k)];
                hb[(size_t)k] = SmpBlock{blk.start, blk.n, lbase[(size_t)(W.b0 + k)]};
                hcnt[(size_t)k] = blk.n;
                if (blk.n == 0) continue;  // (a dead block)
                row_lo = std::min(row_lo, blk.start);
                row_hi = std::max(row_hi, blk.start + blk.n);
                if (!runs.empty() && runs.back().start + runs.back().n == blk.start) runs.back().n += blk.n;
                else runs.push_back(blk);
            }
            if ((rc = pool.alloc(&W.blk, (size_t)nb, "samples blocks"))) return rc;
            if ((rc = pool.alloc(&W.cnt, (size_t)nb, "samples counts"))) return rc;
            if ((rc = pool.alloc(&W.excl, (size_t)nb, "samples ranks"))) return rc;
            if ((rc = upload(W.blk, hb.data(), (size_t)nb, st))) return rc;
            if (filtered && !runs.empty()) {
                // the window's bitmap, zeroed: padding rows (blocks are padded to 32 physical rows) and dead blocks read 0
                W.word0 = row_lo >> 5;
                const int64_t n_words = ((row_hi + 31) >> 5) - W.word0;
                if ((rc = pool.alloc(&W.bits, (size_t)n_words, "samples bitmap"))) return rc;
                std::vector<Segment> segs;
                std::vector<int32_t> wg_seg_begin;
                deal_tiles(runs, n_wg, segs, wg_seg_begin);
                Segment *d_segs = nullptr;
                int32_t *d_wgb = nullptr;
                if ((rc = pool.alloc(&d_segs, segs.size(), "samples segments"))) return rc;
                if ((rc = pool.alloc(&d_wgb, wg_seg_begin.size(), "samples segments"))) return rc;
                if ((rc = upload(d_segs, segs.data(), segs.size(), st))) return rc;
                if ((rc = upload(d_wgb, wg_seg_begin.data(), wg_seg_begin.size(), st))) return rc;
                plan.segs = d_segs;
                plan.wg_seg_begin = d_wgb;
                if ((rc = upload(d_plan, &plan, 1, st))) return rc;
                if ((rc = t_filter.start(st))) return rc;
                SYBL_HIP(hipMemsetAsync(W.bits, 0, (size_t)n_words * 4, st));
                // (k_prefilter indexes the bitmap by physical row: the window's first word is word0)
                hipError_t e = launch_prefilter(d_plan, n_slots, W.bits - W.word0, n_wg, st);
                if (e != hipSuccess) return hip_fail(e, "k_prefilter");
                if ((rc = t_filter.stop(st))) return rc;
                blocks_filtered += nb;
                if ((rc = t_select.start(st))) return rc;
                hipLaunchKernelGGL(k_smp_count, dim3((unsigned)nb), dim3(kSmpThreads), 0, st, (const uint32_t *)W.bits, W.word0,
                                   (const SmpBlock *)W.blk, W.cnt);
            } else {
                // without filters m_b is the block's row count (and a window of dead blocks matches nothing)
                if ((rc = upload(W.cnt, hcnt.data(), (size_t)nb, st))) return rc;
                if ((rc = t_select.start(st))) return rc;
            }
            hipLaunchKernelGGL(k_smp_prefix, dim3(1), dim3(kSmpPrefixThreads), 0, st, (const int64_t *)W.cnt, W.excl, (int)nb, W.b0, limit,
                               d_state);
            SYBL_HIP(hipGetLastError());
            if ((rc = t_select.stop(st))) return rc;
            if ((rc = download(state, (const int64_t *)d_state, (size_t)kSmpStateWords, st))) return rc;
            wins.push_back(W);
            b0 = W.b1;
            span *= kSmpWindowGrowth;
        }
        if (state[kSmpDone]) {
            P = state[kSmpP];
            M = state[kSmpM];
        } else {
            P = B;
            M = state[kSmpTotal];
        }
    }
    const int64_t L = std::min<int64_t>(limit, M);
    R->info.matched = M;
    R->info.blocks_visited = P;
    R->info.blocks_filtered = blocks_filtered;
    R->info.n_rows = L;
    R->row_ids.assign((size_t)L, 0);

    if (L > 0) {
        // ---- the rank window [W0, M) that is materialised: the last L for the default order, everything for a sorted query
        const int64_t W0 = order ? 0 : M - L, n_cand = M - W0;
        if (order && M >= ((int64_t)1 << 31)) return fail(SYBL_E_INVAL, "samples: %lld candidate rows are more than a sorted query orders", (long long)M);
        int64_t *cand_phys = nullptr, *cand_lrow = nullptr;
        uint64_t *key = nullptr;
        uint32_t *present = nullptr;
        if ((rc = pool.alloc(&cand_phys, (size_t)n_cand, "samples candidates"))) return rc;
        if ((rc = pool.alloc(&cand_lrow, (size_t)n_cand, "samples candidates"))) return rc;
        SmpCol oc{};
        if (order) {
            oc = col_desc(order);
            if ((rc = pool.alloc(&key, (size_t)n_cand, "samples keys"))) return rc;
            if ((rc = pool.alloc(&present, (size_t)n_cand, "samples keys"))) return rc;
        }
        if ((rc = t_select.start(st))) return rc;
        for (const Window &W : wins) {
            if (W.b0 >= P) break;
            hipLaunchKernelGGL(k_smp_compact, dim3((unsigned)(W.b1 - W.b0)), dim3(kSmpThreads), 0, st, (const uint32_t *)W.bits, W.word0,
                               (const SmpBlock *)W.blk, (const int64_t *)W.cnt, (const int64_t *)W.excl, W.b0, P, M, W0, cand_phys, cand_lrow, oc,
                               order ? 1 : 0, key, present);
        }
        SYBL_HIP(hipGetLastError());
        int64_t *out_phys = cand_phys, *out_lrow = cand_lrow;
        if (order) {
            uint64_t *key2 = nullptr;
            uint32_t *perm0 = nullptr, *perm1 = nullptr;
            if ((rc = pool.alloc(&key2, (size_t)n_cand, "samples sort"))) return rc;
            if ((rc = pool.alloc(&perm0, (size_t)n_cand, "samples sort"))) return rc;
            if ((rc = pool.alloc(&perm1, (size_t)n_cand, "samples sort"))) return rc;
            hipLaunchKernelGGL(k_smp_iota, dim3(grid_for(n_cand, 256)), dim3(256), 0, st, perm0, n_cand);
            size_t need = 0, need2 = 0;
            SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key, key2, perm0, perm1, (int)n_cand, 0, 64, st));
            const bool has_missing = order->d_valid != nullptr || order->d_data == nullptr;
            uint32_t *flag0 = nullptr, *flag1 = nullptr;
            if (has_missing) {
                if ((rc = pool.alloc(&flag0, (size_t)n_cand, "samples sort"))) return rc;
                if ((rc = pool.alloc(&flag1, (size_t)n_cand, "samples sort"))) return rc;
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need2, flag0, flag1, perm1, perm0, (int)n_cand, 0, 1, st));
            }
            char *tmp = nullptr;
            if ((rc = pool.alloc(&tmp, std::max(need, need2), "samples sort"))) return rc;
            // stable, ascending on the order-reversing key: value descending, equal values in input (= descending row) order
            SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, need, key, key2, perm0, perm1, (int)n_cand, 0, 64, st));
            uint32_t *perm = perm1;
            if (has_missing) {
                // the stable 1-bit pass: rows without the column (0) in front of those with it (1)
                hipLaunchKernelGGL(k_smp_flags, dim3(grid_for(n_cand, 256)), dim3(256), 0, st, (const uint32_t *)present, (const uint32_t *)perm1,
                                   n_cand, flag0);
                SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, need2, flag0, flag1, perm1, perm0, (int)n_cand, 0, 1, st));
                perm = perm0;
            }
            if ((rc = pool.alloc(&out_phys, (size_t)L, "samples rows"))) return rc;
            if ((rc = pool.alloc(&out_lrow, (size_t)L, "samples rows"))) return rc;
            hipLaunchKernelGGL(k_smp_pick, dim3(grid_for(L, 256)), dim3(256), 0, st, (const uint32_t *)perm, M, L, asc ? 1 : 0,
                               (const int64_t *)cand_phys, (const int64_t *)cand_lrow, out_phys, out_lrow);
            SYBL_HIP(hipGetLastError());
        }

        // ---- values
        const size_t nc = out_cols.size();
        std::vector<int64_t> vals(nc * (size_t)L);
        std::vector<uint8_t> pop(nc * (size_t)L);
        int64_t *d_vals = nullptr;
        uint8_t *d_pop = nullptr;
        if (nc) {
            std::vector<SmpCol> hc(nc);
            for (size_t c = 0; c < nc; c++) hc[c] = col_desc(out_cols[c]);
            SmpCol *d_cols = nullptr;
            if ((rc = pool.alloc(&d_cols, nc, "samples columns"))) return rc;
            if ((rc = pool.alloc(&d_vals, vals.size(), "samples values"))) return rc;
            if ((rc = pool.alloc(&d_pop, pop.size(), "samples values"))) return rc;
            if ((rc = upload(d_cols, hc.data(), nc, st))) return rc;
            hipLaunchKernelGGL(k_smp_gather, dim3(grid_for(L * (int64_t)nc, 256)), dim3(256), 0, st, (const SmpCol *)d_cols, (int)nc,
                               (const int64_t *)out_phys, L, d_vals, d_pop);
            SYBL_HIP(hipGetLastError());
        }
        if ((rc = t_select.stop(st))) return rc;
        if ((rc = download(R->row_ids.data(), (const int64_t *)out_lrow, (size_t)L, st))) return rc;
        if ((rc = download(vals.data(), (const int64_t *)d_vals, vals.size(), st))) return rc;
        if ((rc = download(pop.data(), (const uint8_t *)d_pop, pop.size(), st))) return rc;

        for (size_t c = 0; c < nc; c++) {
            SamplesCol &S = R->cols[c];
            Column *col = out_cols[c];
            const int64_t *v = vals.data() + c * (size_t)L;
            S.populated.assign(pop.begin() + (ptrdiff_t)(c * (size_t)L), pop.begin() + (ptrdiff_t)((c + 1) * (size_t)L));
            auto intern = [&](int32_t id) -> const char * {
                auto it = S.pool.find(id);
                if (it == S.pool.end())
                    it = S.pool.emplace(id, id >= 0 && (size_t)id < col->dict.size() ? col->dict[(size_t)id] : std::string()).first;
                return it->second.c_str();
            };
            if (col->type == SYBL_INT_VAL) {
                S.ints.assign(v, v + L);
            } else if (col->type == SYBL_STR_VAL) {
                S.str_ids.resize((size_t)L);
                S.strings.resize((size_t)L);
                for (int64_t i = 0; i < L; i++) {
                    S.str_ids[(size_t)i] = S.populated[(size_t)i] ? (int32_t)v[i] : -1;
                    S.strings[(size_t)i] = S.populated[(size_t)i] ? intern((int32_t)v[i]) : nullptr;
                }
            } else {
                // the output CSR: a prefix over the L lengths here, the members copied on the device
                S.set_off.assign((size_t)L + 1, 0);
                for (int64_t i = 0; i < L; i++) S.set_off[(size_t)i + 1] = S.set_off[(size_t)i] + std::max<int64_t>(v[i], 0);
                const int64_t n_ids = S.set_off[(size_t)L];
                std::vector<int32_t> ids((size_t)n_ids);
                if (n_ids > 0) {
                    int64_t *d_off = nullptr;
                    int32_t *d_ids = nullptr;
                    if ((rc = pool.alloc(&d_off, (size_t)L + 1, "samples set members"))) return rc;
                    if ((rc = pool.alloc(&d_ids, (size_t)n_ids, "samples set members"))) return rc;
                    if ((rc = upload(d_off, S.set_off.data(), (size_t)L + 1, st))) return rc;
                    if ((rc = t_select.start(st))) return rc;
                    hipLaunchKernelGGL(k_smp_gather_set, dim3(grid_for(L, 256)), dim3(256), 0, st, (const int64_t *)col->d_set_off,
                                       (const int32_t *)col->d_set_vals, (const int64_t *)out_phys, L, (const int64_t *)d_off, d_ids);
                    SYBL_HIP(hipGetLastError());
                    if ((rc = t_select.stop(st))) return rc;
                    if ((rc = download(ids.data(), (const int32_t *)d_ids, (size_t)n_ids, st))) return rc;
                }
                S.set_strings.resize((size_t)n_ids);
                for (int64_t k = 0; k < n_ids; k++) S.set_strings[(size_t)k] = intern(ids[(size_t)k]);
            }
        }
    } else {
        for (SamplesCol &S : R->cols)
            if (S.type == SYBL_SET_VAL) S.set_off.assign(1, 0);
    }
    SYBL_HIP(hipStreamSynchronize(st));
    if ((rc = t_filter.total(&R->info.filter_ms))) return rc;
    if ((rc = t_select.total(&R->info.select_ms))) return rc;
    return SYBL_OK;
}

}  // namespace

int samples_run(Table *t, const sybl_samples_desc *d, sybl_samples **out) {
    std::unique_ptr<sybl_samples> R(new (std::nothrow) sybl_samples());
    if (!R) return fail(SYBL_E_NOMEM, "samples: out of host memory");
    R->api_m = t->ctx->api_m;
    try {
        int rc = run(t, d, R.get());
        if (rc) {
            (void)hipStreamSynchronize(t->ctx->stream);  // (nothing of this call is in flight when its buffers go)
            return rc;
        }
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(t->ctx->stream);
        return fail(SYBL_E_NOMEM, "samples: out of host memory");
    } catch (const std::exception &e) {
        (void)hipStreamSynchronize(t->ctx->stream);
        return fail(SYBL_E_INVAL, "samples: %s", e.what());
    }
    *out = R.release();
    return SYBL_OK;
}

// printJson([]*Sample): encoding/json of a slice of maps -- keys sorted bytewise, unpopulated columns absent
static void render_samples(Samples *S) {
    std::string &o = S->rendered;
    o.clear();
    std::vector<size_t> by_name(S->cols.size());
    for (size_t c = 0; c < by_name.size(); c++) by_name[c] = c;
    std::sort(by_name.begin(), by_name.end(), [&](size_t a, size_t b) { return S->cols[a].name < S->cols[b].name; });
    o += '[';
    for (int64_t i = 0; i < S->info.n_rows; i++) {
        if (i) o += ',';
        o += '{';
        bool first = true;
        for (size_t c : by_name) {
            const SamplesCol &C = S->cols[c];
            if (!C.populated[(size_t)i]) continue;
            if (!first) o += ',';
            first = false;
            json_escape(C.name, o);
            o += ':';
            if (C.type == SYBL_INT_VAL) {
                o += std::to_string((long long)C.ints[(size_t)i]);
            } else if (C.type == SYBL_STR_VAL) {
                json_escape(C.strings[(size_t)i] ? C.strings[(size_t)i] : "", o);
            } else {
                o += '[';
                for (int64_t k = C.set_off[(size_t)i]; k < C.set_off[(size_t)i + 1]; k++) {
                    if (k > C.set_off[(size_t)i]) o += ',';
                    json_escape(C.set_strings[(size_t)k], o);
                }
                o += ']';
            }
        }
        o += '}';
    }
    o += ']';
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_samples(sybl_table *t, const sybl_samples_desc *d, sybl_samples **out) {
    SYBL_API_GUARD(t);
    if (!t || !d || !out) return fail(SYBL_E_INVAL, "sybl_table_samples: NULL argument");
    *out = nullptr;
    return samples_run(t, d, out);
}

void sybl_samples_free(sybl_samples *s) {
    SYBL_API_GUARD(s);
    delete s;
}

int sybl_samples_get_info(const sybl_samples *s, sybl_samples_info *out) {
    SYBL_API_GUARD(s);
    if (!s || !out) return fail(SYBL_E_INVAL, "sybl_samples_get_info: NULL argument");
    *out = s->info;
    return SYBL_OK;
}

int sybl_samples_column(const sybl_samples *s, int32_t i, sybl_samples_col *out) {
    SYBL_API_GUARD(s);
    if (!s || !out) return fail(SYBL_E_INVAL, "sybl_samples_column: NULL argument");
    if (i < 0 || (size_t)i >= s->cols.size()) return fail(SYBL_E_INVAL, "sybl_samples_column: column %d of %zu", i, s->cols.size());
    const SamplesCol &C = s->cols[(size_t)i];
    memset(out, 0, sizeof(*out));
    out->name = C.name.c_str();
    out->type = C.type;
    out->populated = C.populated.data();
    if (C.type == SYBL_INT_VAL) {
        out->ints = C.ints.data();
    } else if (C.type == SYBL_STR_VAL) {
        out->str_ids = C.str_ids.data();
        out->strings = C.strings.data();
    } else {
        out->set_off = C.set_off.data();
        out->set_strings = C.set_strings.data();
    }
    return SYBL_OK;
}

int sybl_samples_row_ids(const sybl_samples *s, const int64_t **logical_rows) {
    SYBL_API_GUARD(s);
    if (!s || !logical_rows) return fail(SYBL_E_INVAL, "sybl_samples_row_ids: NULL argument");
    *logical_rows = s->row_ids.data();
    return SYBL_OK;
}

const char *sybl_samples_render(sybl_samples *s) {
    SYBL_API_GUARD(s);
    if (!s) {
        set_error("sybl_samples_render: NULL argument");
        return nullptr;
    }
    try {
        render_samples(s);
    } catch (const std::exception &) {
        set_error("sybl_samples_render: out of host memory");
        return nullptr;
    }
    return s->rendered.c_str();
}

}  // extern "C"
