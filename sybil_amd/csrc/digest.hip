// digest.hip -- the reference's digest step on the resident table (table_io.go:119-130, SaveRecordsToColumns): the rows in
// time order, cut into blocks, as a NEW resident table.  The semantics are restated in include/sybilgpu.h ("digest") and
// DESIGN.md; this file is the device work behind them and the host code that drives it.
//
//   k_dg_keys      one pass over the time column at its stored width: (sortable key, source physical row) for the N live
//                  rows in source order.  The key is the offset from min(0, exact_min) -- from exact_min when every row has the
//                  column -- as 32 bits when the range fits them, else the sign-flipped 64-bit value; a row without the
//                  column has the value 0.
//   sort           hipcub::DeviceRadixSort::SortPairs over the bits the range needs: LSD, stable -- equal keys keep source
//                  order.  What it leaves is the permutation: perm[i] = the source physical row of sorted row i.
//   k_dg_gather<W> the bulk of the bytes, in GATHER form: a lane produces consecutive OUTPUT physical rows (4 / 2 of them for
//                  1- / 2-byte columns, so that every store is a whole dword) and reads its source rows wherever they are.
//                  The stored bits are copied as they are: every output value is a source value, so the source column's
//                  (width, base) holds the output.  Instantiated per stored width, not switched inside one body.
//   k_dg_valid     validity: a lane fetches the source bit of its output row, a wave ballot makes the two 32-bit words, one
//                  lane each stores them.  Padding rows (blocks are padded to 32 physical rows) read 0.
//   statistics     k_block_minmax (kernels.hip) over the gathered column, all output blocks in ONE launch per column and one
//                  readback for the table; the block writer then records them block by block without waiting for the GPU.
//
// Set columns: validity as above; the CSR (Column::h_set_off / h_set_vals, the host mirror every upload starts from) is
// gathered on the host from the permutation.
//
// Everything behind the sort -- layout, gather, validity, statistics, set columns, the block writer -- is gather_rows
// (derived.h): select.hip runs it over its ascending row list and a column subset.  The call wrapper, the block search and the
// small helpers are derived.h too; the set-column gather is colstats.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "derived.h"

namespace sybl {

constexpr int kDgThreads = 256;

// where output physical row p comes from: block j = p / stride holds sorted rows [j * block_rows, ...); rows of the padding
// behind a block, and behind the last row, have no source
__device__ __forceinline__ bool dg_sorted_index(int64_t p, int64_t stride, int64_t block_rows, int64_t N, int64_t *i) {
    const int64_t j = p / stride, r = p - j * stride;
    *i = j * block_rows + r;
    return r < block_rows && *i < N;
}

// ---- keys.  A lane per live row; blk: the live source blocks, base = the index of a block's first row among the live rows
// (block_of, derived.h).
template <int W, bool K64>
__global__ __launch_bounds__(kDgThreads) void k_dg_keys(const void *__restrict__ col, int64_t vbase, const uint32_t *__restrict__ valid,
                                                        const RowBlk *__restrict__ blk, int nb, int64_t N, int64_t lo,
                                                        void *__restrict__ keys, uint32_t *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * kDgThreads + threadIdx.x;
    if (i >= N) return;
    const int a = block_of(blk, nb, i - (threadIdx.x & 63), i, &RowBlk::base);
    const int64_t row = blk[a].start + (i - blk[a].base);
    int64_t v = 0;
    if (col != nullptr && (valid == nullptr || valid_bit(valid, row))) {
        if (W == 8) v = ((const int64_t *)col)[row];
        else if (W == 4) v = vbase + (int64_t)((const uint32_t *)col)[row];
        else if (W == 2) v = vbase + (int64_t)((const uint16_t *)col)[row];
        else v = vbase + (int64_t)((const uint8_t *)col)[row];
    }
    if (K64) ((uint64_t *)keys)[i] = (uint64_t)v ^ 0x8000000000000000ull;
    else ((uint32_t *)keys)[i] = (uint32_t)((uint64_t)v - (uint64_t)lo);
    rows[i] = (uint32_t)row;
}

// ---- values.  n_out = the output's physical rows rounded up to 32: the padding is written too (zero).
template <int W>
__global__ __launch_bounds__(kDgThreads) void k_dg_gather(const void *__restrict__ src, const uint32_t *__restrict__ perm, int64_t N,
                                                          int64_t block_rows, int64_t stride, int64_t n_out, void *__restrict__ dst) {
    constexpr int K = W == 1 ? 4 : W == 2 ? 2 : 1;  // rows per lane: one dword (W = 8: two)
    const int64_t p0 = ((int64_t)blockIdx.x * kDgThreads + threadIdx.x) * K;
    if (p0 >= n_out) return;  // (n_out and p0 are multiples of K)
    if (W == 8) {
        int64_t i;
        ((uint64_t *)dst)[p0] = dg_sorted_index(p0, stride, block_rows, N, &i) ? ((const uint64_t *)src)[perm[i]] : 0ull;
    } else {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            int64_t i;
            if (!dg_sorted_index(p0 + k, stride, block_rows, N, &i)) continue;
            const uint32_t s = perm[i];
            if (W == 4) word = ((const uint32_t *)src)[s];
            else if (W == 2) word |= (uint32_t)((const uint16_t *)src)[s] << (16 * k);
            else word |= (uint32_t)((const uint8_t *)src)[s] << (8 * k);
        }
        ((uint32_t *)dst)[p0 / K] = word;
    }
}

// ---- validity words of the output: n_words of them, a wave per two
__global__ __launch_bounds__(kDgThreads) void k_dg_valid(const uint32_t *__restrict__ valid, const uint32_t *__restrict__ perm, int64_t N,
                                                         int64_t block_rows, int64_t stride, int64_t n_words, uint32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kDgThreads + threadIdx.x;
    int64_t i;
    bool bit = false;
    if (dg_sorted_index(p, stride, block_rows, N, &i)) {
        const uint32_t s = perm[i];
        bit = valid_bit(valid, s);
    }
    const unsigned long long m = __ballot(bit);
    const int lane = threadIdx.x & 63;
    const int64_t w = p >> 5;
    if ((lane == 0 || lane == 32) && w < n_words) out[w] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
}

namespace {

template <int W>
void launch_keys(bool k64, const Column *c, const RowBlk *blk, int nb, int64_t N, int64_t lo, void *keys, uint32_t *rows, hipStream_t st) {
    if (k64)
        hipLaunchKernelGGL((k_dg_keys<W, true>), dim3(grid_for(N, kDgThreads)), dim3(kDgThreads), 0, st, (const void *)c->d_data, c->vbase,
                           (const uint32_t *)c->d_valid, blk, nb, N, lo, keys, rows);
    else
        hipLaunchKernelGGL((k_dg_keys<W, false>), dim3(grid_for(N, kDgThreads)), dim3(kDgThreads), 0, st, (const void *)c->d_data, c->vbase,
                           (const uint32_t *)c->d_valid, blk, nb, N, lo, keys, rows);
}

template <int W>
void launch_gather(const void *src, const uint32_t *perm, int64_t N, int64_t block_rows, int64_t stride, int64_t n_out, void *dst,
                   hipStream_t st) {
    constexpr int K = W == 1 ? 4 : W == 2 ? 2 : 1;
    hipLaunchKernelGGL((k_dg_gather<W>), dim3(grid_for(n_out / K, kDgThreads)), dim3(kDgThreads), 0, st, src, perm, N, block_rows, stride, n_out,
                       dst);
}

}  // namespace

// (derived.h) name, type, IntInfo, dictionaries, declared bounds, storage
void gather_make_columns(const Table *t, const std::vector<Column *> &src, Table *o) {
    o->compact_mode = t->compact_mode;
    for (const Column *c : src) {
        auto n = std::make_unique<Column>();
        n->name = c->name;
        n->type = c->type;
        n->elem = c->elem;
        n->vbase = c->vbase;
        n->info_given = c->info_given;
        n->info_min = c->info_min;
        n->info_max = c->info_max;
        n->has_missing = c->has_missing;
        n->bounds_set = c->bounds_set;
        n->bound_lo = c->bound_lo;
        n->bound_hi = c->bound_hi;
        n->dict = c->dict;        // id for id
        n->dict_ix = c->dict_ix;
        o->col_ix[n->name] = (int)o->cols.size();
        o->cols.push_back(std::move(n));
    }
}

// (derived.h) the back half of a digest, shared with select.hip: there the row list is ascending, here it is the sort's
// permutation -- the name it keeps below
int gather_rows(Table *t, const std::vector<Column *> &src, const uint32_t *perm, int64_t N, int64_t block_rows, Table *o, GatherPool &pool,
                const char *who, hipEvent_t *gathered, int64_t *bytes, int64_t *blocks) {
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;

    // ---- the output's layout: block j at physical row j * stride, as the block writer will place it
    const int64_t stride = round_up(block_rows, 32);
    const int64_t nb_out = (N + block_rows - 1) / block_rows;
    const int64_t last_n = N - (nb_out - 1) * block_rows;
    const int64_t phys_out = (nb_out - 1) * stride + last_n;
    const int64_t n_out = round_up(phys_out, 32), n_words = n_out / 32;
    std::vector<Segment> osegs((size_t)nb_out);
    for (int64_t j = 0; j < nb_out; j++) osegs[(size_t)j] = Segment{j * stride, j + 1 < nb_out ? block_rows : last_n};

    // ---- gather: every column whole, into its final place; validity words into scratch (the writer sets a block's words
    // when the block is begun: the gathered words are copied over them at the end)
    const size_t nc = src.size();
    std::vector<uint32_t *> vbits(nc, nullptr);
    const bool want_stats = o->compact_mode;  // (canonical storage: table_ensure_stats computes them on first use, as for appended blocks)
    Segment *d_osegs = nullptr;
    int64_t *d_stats = nullptr;
    if (want_stats) {
        if ((rc = pool.alloc(&d_osegs, (size_t)nb_out, "gather blocks"))) return rc;
        if ((rc = pool.alloc(&d_stats, nc * 3 * (size_t)nb_out, "gather statistics"))) return rc;
        if ((rc = host_to_device(ctx, d_osegs, osegs.data(), osegs.size() * sizeof(Segment), "gather blocks"))) return rc;
    }
    for (size_t k = 0; k < nc; k++) {
        const Column *c = src[k];
        Column *n = o->cols[k].get();
        if (c->d_valid) {
            if ((rc = pool.alloc(&vbits[k], (size_t)n_words, "gather validity"))) return rc;
            if ((rc = valid_reserve(o, n, phys_out))) return rc;
            hipLaunchKernelGGL(k_dg_valid, dim3(grid_for(n_out, kDgThreads)), dim3(kDgThreads), 0, st, (const uint32_t *)c->d_valid,
                               (const uint32_t *)perm, N, block_rows, stride, n_words, vbits[k]);
            *bytes += N * 4 + N * 4 + n_words * 4;  // (a 32-byte sector per source bit is what the memory sees: counted as a word)
        }
        if (c->type == SYBL_SET_VAL) continue;
        if ((rc = table_reserve(o, n, phys_out))) return rc;
        if (!c->d_data) {
            SYBL_HIP(hipMemsetAsync(n->d_data, 0, (size_t)n_out * (size_t)n->elem, st));
        } else {
            by_width(c->elem, [&](auto W) { launch_gather<decltype(W)::value>(c->d_data, perm, N, block_rows, stride, n_out, n->d_data, st); });
            *bytes += N * 4 + 2 * N * (int64_t)c->elem;
        }
        SYBL_HIP(hipGetLastError());
        if (want_stats) {
            int64_t *out = d_stats + k * 3 * (size_t)nb_out;
            hipError_t e = launch_block_minmax(n->d_data, n->elem, n->vbase, vbits[k], d_osegs, (int)nb_out, out, out + nb_out, out + 2 * nb_out, st);
            if (e != hipSuccess) return hip_fail(e, "k_block_minmax");
        }
    }
    if ((rc = pool.event(gathered, st))) return rc;
    std::vector<int64_t> stats;
    if (want_stats) {
        stats.resize(nc * 3 * (size_t)nb_out);
        SYBL_HIP(hipMemcpyAsync(stats.data(), d_stats, stats.size() * 8, hipMemcpyDeviceToHost, st));
    }
    SYBL_HIP(hipStreamSynchronize(st));  // the ONE wait for the statistics of every block of every column

    // ---- set columns: the host CSR over the output's physical rows, gathered from the permutation
    bool any_set = false;
    for (const Column *c : src) any_set = any_set || c->type == SYBL_SET_VAL;
    if (any_set) {
        std::vector<uint32_t> hperm((size_t)N);
        SYBL_HIP(hipMemcpy(hperm.data(), perm, (size_t)N * 4, hipMemcpyDeviceToHost));
        // the source row of every output physical row (padding rows: none; the table ends with its last row)
        std::vector<uint32_t> map((size_t)phys_out, kSetNoRow);
        for (int64_t i = 0; i < N; i++) map[(size_t)(i / block_rows * stride + i % block_rows)] = hperm[(size_t)i];
        for (size_t k = 0; k < nc; k++) {
            const Column *c = src[k];
            Column *n = o->cols[k].get();
            if (c->type != SYBL_SET_VAL) continue;
            n->h_set_off.assign(1, 0);
            set_gather(c->h_set_off, c->h_set_vals, map.data(), phys_out, n->h_set_off, n->h_set_vals);
            n->set_dirty = true;
        }
    }

    // ---- the block writer: segments, block statistics, versions.  Nothing here waits for the GPU.
    for (int64_t j = 0; j < nb_out; j++) {
        const Segment &sg = osegs[(size_t)j];
        BlockWriter w;
        if ((rc = block_begin(o, sg.n, &w))) return rc;
        if (w.start != sg.start) return fail(SYBL_E_STATE, "%s: block %lld begins at row %lld, not %lld", who, (long long)j, (long long)w.start, (long long)sg.start);
        for (size_t k = 0; k < nc; k++) {
            Column *n = o->cols[k].get();
            void *col = nullptr;
            uint32_t *valid = nullptr;
            // all_populated: the writer leaves the rows alone (they are in place) and sets the block's validity words, if the
            // column has any, to ones -- the gathered words replace them below
            bool direct = false;
            if (want_stats && n->type != SYBL_SET_VAL) {
                const int64_t *h = stats.data() + k * 3 * (size_t)nb_out;
                const int64_t mn = h[j], mx = h[nb_out + j], pop = h[2 * nb_out + j];
                if ((rc = block_col_direct(w, n, true, mn, mx, pop, &col, &valid, &direct))) return rc;
                if (!direct) {
                    // (SYBL_NO_DIRECT_DECODE: through the staging block -- the rows in place, decoded, and packed back at commit)
                    if ((rc = block_col_device(w, n, true, &col, &valid))) return rc;
                    hipError_t e = launch_repack((const char *)n->d_data + (size_t)sg.start * (size_t)n->elem, n->elem, n->vbase, col, n->canon(), 0, sg.n, st);
                    if (e != hipSuccess) return hip_fail(e, "k_repack");
                    block_col_stats(w, n, mn, mx, pop);
                    continue;
                }
            } else if ((rc = block_col_device(w, n, true, &col, &valid))) {
                return rc;
            }
            if (n->type != SYBL_SET_VAL && col != (char *)n->d_data + (size_t)sg.start * (size_t)n->elem)
                return fail(SYBL_E_STATE, "%s: column '%s' moved under the writer", who, n->name.c_str());
        }
        if ((rc = block_commit(w))) return rc;
    }
    for (size_t k = 0; k < nc; k++) {
        Column *n = o->cols[k].get();
        if (!vbits[k]) continue;
        SYBL_HIP(hipMemcpyAsync(n->d_valid, vbits[k], (size_t)n_words * 4, hipMemcpyDeviceToDevice, st));
        n->has_missing = n->has_missing || src[k]->has_missing;
    }
    SYBL_HIP(hipStreamSynchronize(st));
    *blocks = nb_out;
    return SYBL_OK;
}

namespace {

int run(Table *t, Column *tc, int64_t block_rows, Table *o, sybl_digest_stats *S) {
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = load_sync_all(ctx))) return rc;
    if ((rc = table_ensure_stats(t))) return rc;  // (the key column's extrema; the table's version does not move)

    // ---- the output's columns: every column of the source, in its order
    std::vector<Column *> src;
    for (auto &cp : t->cols) src.push_back(cp.get());
    gather_make_columns(t, src, o);

    // ---- the source rows: the live blocks in resident order
    std::vector<RowBlk> live;
    int64_t N = 0;
    for (const Segment &b : t->blocks) {
        if (b.n <= 0) continue;  // (a dead block, sybl_table_refresh)
        live.push_back(RowBlk{b.start, b.n, N});
        N += b.n;
    }
    if (N >= ((int64_t)1 << 31)) return fail(SYBL_E_INVAL, "digest: %lld rows are more than the sort orders (2^31 - 1)", (long long)N);
    if (t->phys_rows > (int64_t)UINT32_MAX)
        return fail(SYBL_E_INVAL, "digest: %lld physical rows (dead blocks included) are more than a 32-bit row number holds", (long long)t->phys_rows);
    S->rows = N;
    if (N == 0) return SYBL_OK;
    const int nb_src = (int)live.size();

    GatherPool pool;
    hipEvent_t ev[4];

    // ---- keys
    // (the key 0 of a row without the column takes part in the range -- unless the column has no bitmap: every row has a value)
    const bool any = tc->n_pop > 0, dense = tc->d_valid == nullptr && tc->d_data != nullptr;
    const int64_t lo = !any ? 0 : dense ? tc->exact_min : std::min<int64_t>(0, tc->exact_min);
    const int64_t hi = !any ? 0 : dense ? tc->exact_max : std::max<int64_t>(0, tc->exact_max);
    const unsigned __int128 range = (unsigned __int128)((__int128)hi - (__int128)lo);
    const bool k64 = range >= ((unsigned __int128)1 << 32);
    int bits = 64;
    if (!k64) {
        bits = 1;  // (a range of one value: one pass that moves nothing)
        while (bits < 32 && (range >> bits) != 0) bits++;
    }
    S->key_bits = bits;
    const size_t ksz = k64 ? 8 : 4;
    RowBlk *d_blk = nullptr;
    char *key0 = nullptr, *key1 = nullptr;
    uint32_t *row0 = nullptr, *perm = nullptr;
    if ((rc = pool.alloc(&d_blk, (size_t)nb_src, "digest blocks"))) return rc;
    if ((rc = pool.alloc(&key0, (size_t)N * ksz, "digest keys"))) return rc;
    if ((rc = pool.alloc(&key1, (size_t)N * ksz, "digest keys"))) return rc;
    if ((rc = pool.alloc(&row0, (size_t)N, "digest rows"))) return rc;
    if ((rc = pool.alloc(&perm, (size_t)N, "digest rows"))) return rc;
    size_t tmp_bytes = 0;
    if (k64) SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint64_t *)key0, (uint64_t *)key1, row0, perm, (int)N, 0, bits, st));
    else SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint32_t *)key0, (uint32_t *)key1, row0, perm, (int)N, 0, bits, st));
    char *tmp = nullptr;
    if ((rc = pool.alloc(&tmp, tmp_bytes, "digest sort"))) return rc;
    if ((rc = host_to_device(ctx, d_blk, live.data(), live.size() * sizeof(RowBlk), "digest blocks"))) return rc;
    if ((rc = pool.event(&ev[0], st))) return rc;
    by_width(tc->d_data ? tc->elem : 8, [&](auto W) { launch_keys<decltype(W)::value>(k64, tc, d_blk, nb_src, N, lo, key0, row0, st); });
    SYBL_HIP(hipGetLastError());
    if ((rc = pool.event(&ev[1], st))) return rc;

    // ---- sort: stable, ascending, over the bits the range needs
    if (k64) SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (uint64_t *)key0, (uint64_t *)key1, row0, perm, (int)N, 0, bits, st));
    else SYBL_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (uint32_t *)key0, (uint32_t *)key1, row0, perm, (int)N, 0, bits, st));
    if ((rc = pool.event(&ev[2], st))) return rc;

    // ---- gather, statistics, set columns, the block writer (gather_rows below)
    if ((rc = gather_rows(t, src, perm, N, block_rows, o, pool, "digest", &ev[3], &S->gather_bytes, &S->blocks))) return rc;
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) SYBL_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    S->keys_ms = ms[0];
    S->sort_ms = ms[1];
    S->gather_ms = ms[2];
    S->keys_bytes = N * ((int64_t)tc->elem + (int64_t)ksz + 4);
    // (an LSD pass per 8 bits reads and writes every pair; the histogram pass reads the keys once more)
    S->sort_bytes = (int64_t)((bits + 7) / 8) * 2 * N * ((int64_t)ksz + 4) + N * (int64_t)ksz;
    return SYBL_OK;
}

}  // namespace

int digest_run(Table *t, const char *time_col, int32_t block_rows, sybl_table **out) {
    const char *name = time_col && time_col[0] ? time_col : "time";
    Column *tc = t->find(name);
    if (!tc) return fail(SYBL_E_INVAL, "digest: unknown time column '%s'", name);
    if (tc->type != SYBL_INT_VAL)
        return fail(SYBL_E_INVAL, "digest: time column '%s' is a %s column; rows are ordered by an int column", name, tc->type == SYBL_STR_VAL ? "str" : "set");
    if (block_rows < 0 || block_rows > SYBL_BLOCK_ROWS) return fail(SYBL_E_INVAL, "digest: block_rows %d is outside 0 .. %d", block_rows, SYBL_BLOCK_ROWS);
    const int64_t br = block_rows ? block_rows : SYBL_BLOCK_ROWS;
    TableOwner O;
    int rc = derived_new_table(t->ctx, t->name, "digest", O);
    if (rc) return rc;
    return derived_call(t->ctx, "digest", O, out, [&] { return run(t, tc, br, O.t, &O.t->digest_stats); });
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_digest(sybl_table *t, const char *time_col, int32_t block_rows, sybl_table **out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_digest: NULL argument");
    *out = nullptr;
    return digest_run(t, time_col, block_rows, out);
}

int sybl_table_digest_stats(const sybl_table *t, sybl_digest_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_digest_stats: NULL argument");
    *out = t->digest_stats;
    return SYBL_OK;
}

}  // extern "C"
