// lookup.hip -- columns of a second resident table attached by key, as a NEW resident table: a left join with first match, in
// broadcast form (every rank holds all of `dim`).  The semantics are restated in include/sybilgpu.h ("lookup") and DESIGN.md
// 3.11; this file is the device work and the host code that drives it.
//
// The `t` half of the output IS sybl_table_concat of t alone (derived_copy, derived.h): rows, blocks, columns, storage, statistics.  The
// attached columns are added to that table: output physical row p of a live block is the row the key column of the OUTPUT
// holds at p, so the probe reads the output's own key column and no row of t has to be located again.
//
//   k_lk_build   a lane per live dim row (the wave bisects the block list for its first row: block_of, derived.h): the key at its
//                stored width and base, the validity bit, the key's cell, an agent-scope atomicMin of the physical row number
//                into first_row[cell] (all-ones = nobody yet).  The lowest row wins whatever the order of arrival.
//                  direct  cell = v - lo over the key's tracked range
//                  hash    open addressing, linear probing, splitmix64(key) >> 32 & mask as hash_table.h; the key word is
//                          claimed by a 64-bit compare-and-swap against kHashEmpty (all ones).  All ones as an int64 is the
//                          key -1: that key never enters the table -- its row number lives in the side cell first_row[slots].
//                  str     cell = the dim dictionary id: direct over the dictionary
//                The lane whose atomicMin saw all-ones is the cell's first occupant: occupied cells and populated rows are
//                counted by ballot / popcount per wave, summed through LDS, and leave as ONE 64-bit atomic per workgroup
//                (populated in the high half, occupied in the low half: each is below 2^32).
//   k_lk_probe   a lane per physical row of the output (padding rows included: they match nothing): the key, for str through
//                the host-made id table (t's dictionary id -> dim's, or -1), the cell found read-only -- the hash walk stops at a
//                free slot and is bounded by the slot count --, match[p] = first_row[cell] or all-ones.  `matched` by ballot /
//                popcount and one atomic per workgroup.
//   k_lk_gather  <WS, WD> per attached int / str column: out[p] = encode(decode(src[match[p]])), 0 where there is no match or
//                the dim value is unpopulated.  Whole dwords per lane (4 rows at width 1, 2 at width 2), as k_dg_gather.
//   k_lk_valid   validity words by ballot, as k_dg_valid: matched && (dim has no bitmap || dim bit).
//   statistics   k_block_minmax (kernels.hip) over every attached column, one readback for all of them.
//
// Set columns: validity as above; the CSR is built on the host from the match list that was read back (set_gather, colstats.h).
// The call wrapper, the column list, the width dispatch and the statistics (BlockStats) are derived.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "derived.h"
#include "scan_generic.h"

namespace sybl {

constexpr int kLkThreads = 256;
constexpr uint32_t kLkNone = kSetNoRow;  // all ones: no match
enum { kLkDirect = 1, kLkHash = 2, kLkStr = 3 };

struct LkTable {
    uint32_t *first_row;  // [cells] (+ the side cell of the key -1 on the hash path)
    uint64_t *keys;       // hash: [slots]
    int64_t lo;           // direct / str: cell = v - lo
    uint64_t span;        // direct / str: hi - lo
    uint32_t slots;       // hash
};

template <int W>
__device__ __forceinline__ uint64_t lk_bits(const void *col, size_t row) {
    if (W == 8) return ((const uint64_t *)col)[row];
    if (W == 4) return ((const uint32_t *)col)[row];
    if (W == 2) return ((const uint16_t *)col)[row];
    return ((const uint8_t *)col)[row];
}

// sums `bit` over the workgroup; the total is in thread 0 (every thread of the workgroup calls this)
__device__ __forceinline__ uint32_t lk_wg_count(bool bit, uint32_t *lds) {
    const unsigned long long m = __ballot(bit);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t n = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kLkThreads / 64; k++) n += lds[k];
    __syncthreads();
    return n;
}

// ---- build.  counters[0]: populated << 32 | occupied, counters[1]: keys that found no slot (hash)
template <int W, int MODE>
__global__ __launch_bounds__(kLkThreads) void k_lk_build(const void *__restrict__ col, int64_t vbase, const uint32_t *__restrict__ valid,
                                                         const RowBlk *__restrict__ blk, int nb, int64_t R, LkTable T,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ uint32_t lds[kLkThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    bool populated = false, first_here = false;
    if (i < R) {
        const int a = block_of(blk, nb, i - (threadIdx.x & 63), i, &RowBlk::base);
        const int64_t row = blk[a].start + (i - blk[a].base);
        if (valid == nullptr || valid_bit(valid, (size_t)row)) {
            populated = true;
            const uint64_t v = (uint64_t)vbase + lk_bits<W>(col, (size_t)row);
            int64_t cell = -1;
            if (MODE == kLkHash) {
                if (v == kHashEmpty) {
                    cell = (int64_t)T.slots;  // the side cell of the key -1
                } else {
                    const uint32_t mask = T.slots - 1u;
                    uint32_t h = (uint32_t)(splitmix64(v) >> 32) & mask;
                    for (uint32_t probe = 0; probe < T.slots; probe++) {  // bounded by the slot count: a full table ends the walk
                        uint64_t k = __hip_atomic_load(T.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (k == kHashEmpty) {
                            unsigned long long expect = kHashEmpty;
                            if (__hip_atomic_compare_exchange_strong((unsigned long long *)T.keys + h, &expect, (unsigned long long)v,
                                                                     __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                k = v;
                            else
                                k = expect;
                        }
                        if (k == v) {
                            cell = (int64_t)h;
                            break;
                        }
                        h = (h + 1) & mask;
                    }
                    if (cell < 0) __hip_atomic_fetch_add(counters + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the call fails)
                }
            } else {
                const uint64_t off = v - (uint64_t)T.lo;
                if (off <= T.span) cell = (int64_t)off;  // (the tracked range bounds every value: anything else is left out)
            }
            if (cell >= 0)
                first_here = __hip_atomic_fetch_min(T.first_row + cell, (uint32_t)row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kLkNone;
        }
    }
    const uint32_t n_pop = lk_wg_count(populated, lds);
    const uint32_t n_occ = lk_wg_count(first_here, lds);
    if (threadIdx.x == 0 && n_pop)
        __hip_atomic_fetch_add(counters, ((unsigned long long)n_pop << 32) | n_occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- probe.  col: the OUTPUT's key column; blk: the output's blocks (start ascending, blk[0].start = 0); n_out: the
// output's physical rows rounded up to 32.  counters[2]: matched.
template <int W, int MODE>
__global__ __launch_bounds__(kLkThreads) void k_lk_probe(const void *__restrict__ col, int64_t vbase, const uint32_t *__restrict__ valid,
                                                         const RowBlk *__restrict__ blk, int nb, int64_t n_out, LkTable T,
                                                         const int32_t *__restrict__ lut, int64_t n_lut, uint32_t *__restrict__ match,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ uint32_t lds[kLkThreads / 64];
    const int64_t p = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    uint32_t m = kLkNone;
    if (p < n_out) {
        const int a = block_of(blk, nb, p - (threadIdx.x & 63), p, &RowBlk::start);
        const bool live = p < blk[a].start + blk[a].n;  // (else a padding row)
        if (live && col != nullptr && (valid == nullptr || valid_bit(valid, (size_t)p))) {
            const uint64_t v = (uint64_t)vbase + lk_bits<W>(col, (size_t)p);
            if (MODE == kLkHash) {
                if (v == kHashEmpty) {
                    m = T.first_row[T.slots];
                } else {
                    const uint32_t mask = T.slots - 1u;
                    uint32_t h = (uint32_t)(splitmix64(v) >> 32) & mask;
                    for (uint32_t probe = 0; probe < T.slots; probe++) {
                        const uint64_t k = T.keys[h];
                        if (k == kHashEmpty) break;
                        if (k == v) {
                            m = T.first_row[h];
                            break;
                        }
                        h = (h + 1) & mask;
                    }
                }
            } else if (MODE == kLkStr) {
                const int64_t id = (int64_t)v;
                const int64_t did = id >= 0 && id < n_lut ? (int64_t)lut[id] : -1;
                if (did >= 0 && (uint64_t)did <= T.span) m = T.first_row[did];
            } else {
                // unsigned: holds at the int64 edges, where v - lo as a signed number wraps
                const uint64_t off = v - (uint64_t)T.lo;
                if (off <= T.span) m = T.first_row[off];
            }
        }
        match[p] = m;
    }
    const uint32_t n = lk_wg_count(m != kLkNone, lds);
    if (threadIdx.x == 0 && n) __hip_atomic_fetch_add(counters + 2, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- values.  n_out: a multiple of 32, so of the rows a lane writes; the padding is written too (zero).
template <int WS, int WD>
__global__ __launch_bounds__(kLkThreads) void k_lk_gather(const void *__restrict__ src, int64_t sbase, const uint32_t *__restrict__ svalid,
                                                          const uint32_t *__restrict__ match, int64_t n_out, void *__restrict__ dst,
                                                          int64_t dbase) {
    constexpr int K = WD == 1 ? 4 : WD == 2 ? 2 : 1;  // rows per lane: one dword (WD = 8: two)
    const int64_t p0 = ((int64_t)blockIdx.x * kLkThreads + threadIdx.x) * K;
    if (p0 >= n_out) return;
    uint32_t word = 0;
    uint64_t wide = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t m = match[p0 + k];
        if (m == kLkNone || (svalid != nullptr && !valid_bit(svalid, (size_t)m))) continue;
        const uint64_t o = (uint64_t)sbase + lk_bits<WS>(src, (size_t)m) - (uint64_t)dbase;
        if (WD == 8) wide = o;
        else if (WD == 4) word = (uint32_t)o;
        else if (WD == 2) word |= ((uint32_t)o & 0xFFFFu) << (16 * k);
        else word |= ((uint32_t)o & 0xFFu) << (8 * k);
    }
    if (WD == 8) ((uint64_t *)dst)[p0] = wide;
    else ((uint32_t *)dst)[p0 / K] = word;
}

// ---- validity words of an attached column: n_out / 32 of them, a wave per two
__global__ __launch_bounds__(kLkThreads) void k_lk_valid(const uint32_t *__restrict__ svalid, const uint32_t *__restrict__ match, int64_t n_out,
                                                         uint32_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    bool bit = false;
    if (p < n_out) {
        const uint32_t m = match[p];
        bit = m != kLkNone && (svalid == nullptr || valid_bit(svalid, (size_t)m));
    }
    const unsigned long long b = __ballot(bit);
    const int lane = threadIdx.x & 63;
    if ((lane == 0 || lane == 32) && p < n_out) out[p >> 5] = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
}

namespace {

struct KeySide {
    const void *col;
    int64_t vbase;
    const uint32_t *valid;
    const RowBlk *blk;
    int nb;
    int64_t rows;  // build: live rows; probe: n_out
};

template <int W>
void launch_build(int mode, const KeySide &k, const LkTable &T, unsigned long long *counters, hipStream_t st) {
    const dim3 g(grid_for(k.rows, kLkThreads)), b(kLkThreads);
    if (mode == kLkHash) hipLaunchKernelGGL((k_lk_build<W, kLkHash>), g, b, 0, st, k.col, k.vbase, k.valid, k.blk, k.nb, k.rows, T, counters);
    else hipLaunchKernelGGL((k_lk_build<W, kLkDirect>), g, b, 0, st, k.col, k.vbase, k.valid, k.blk, k.nb, k.rows, T, counters);
}

template <int W>
void launch_probe(int mode, const KeySide &k, const LkTable &T, const int32_t *lut, int64_t n_lut, uint32_t *match, unsigned long long *counters,
                  hipStream_t st) {
    const dim3 g(grid_for(k.rows, kLkThreads)), b(kLkThreads);
    if (mode == kLkHash)
        hipLaunchKernelGGL((k_lk_probe<W, kLkHash>), g, b, 0, st, k.col, k.vbase, k.valid, k.blk, k.nb, k.rows, T, lut, n_lut, match, counters);
    else if (mode == kLkStr)
        hipLaunchKernelGGL((k_lk_probe<W, kLkStr>), g, b, 0, st, k.col, k.vbase, k.valid, k.blk, k.nb, k.rows, T, lut, n_lut, match, counters);
    else
        hipLaunchKernelGGL((k_lk_probe<W, kLkDirect>), g, b, 0, st, k.col, k.vbase, k.valid, k.blk, k.nb, k.rows, T, lut, n_lut, match, counters);
}

template <int WS, int WD>
void launch_gather(const Column *c, const uint32_t *match, int64_t n_out, Column *n, hipStream_t st) {
    constexpr int K = WD == 1 ? 4 : WD == 2 ? 2 : 1;
    hipLaunchKernelGGL((k_lk_gather<WS, WD>), dim3(grid_for(n_out / K, kLkThreads)), dim3(kLkThreads), 0, st, (const void *)c->d_data, c->vbase,
                       (const uint32_t *)c->d_valid, match, n_out, n->d_data, n->vbase);
}

// SYBL_LOOKUP_SLOTS: a power of two in 2 .. kHashMaxSlots
bool slots_ok(long long n) { return n >= 2 && n <= kHashMaxSlots && (n & (n - 1)) == 0; }

int run(Table *t, const sybl_lookup_desc *d, TableOwner &O) {
    Table *dim = d->dim;
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;

    // ---- the arguments: everything that can be refused is refused before anything is made
    if (d->n_columns < 0) return fail(SYBL_E_INVAL, "sybl_table_lookup: bad column list");
    const char *kname = d->key;
    const char *dkname = d->dim_key && d->dim_key[0] ? d->dim_key : d->key;
    Column *tk = t->find(kname), *dk = dim->find(dkname);
    if (!tk) return fail(SYBL_E_INVAL, "sybl_table_lookup: unknown key column '%s'", kname ? kname : "(null)");
    if (!dk) return fail(SYBL_E_INVAL, "sybl_table_lookup: unknown key column '%s' of the dim table", dkname ? dkname : "(null)");
    if (tk->type == SYBL_SET_VAL) return fail(SYBL_E_INVAL, "sybl_table_lookup: key column '%s' is a set column; a key is an int or a str column", kname);
    if (dk->type == SYBL_SET_VAL)
        return fail(SYBL_E_INVAL, "sybl_table_lookup: key column '%s' of the dim table is a set column; a key is an int or a str column", dkname);
    if (tk->type != dk->type)
        return fail(SYBL_E_INVAL, "sybl_table_lookup: key column '%s' is a %s column and '%s' of the dim table a %s column", kname, type_name(tk->type),
                    dkname, type_name(dk->type));
    std::vector<Column *> src;
    if ((rc = resolve_columns(dim, d->columns, d->n_columns, "sybl_table_lookup", " of the dim table", dk, &src))) return rc;
    const std::string prefix = d->prefix ? d->prefix : "";
    std::vector<std::string> names;
    for (const Column *c : src) {
        const std::string nm = prefix + c->name;
        if (t->find(nm.c_str()) || std::find(names.begin(), names.end(), nm) != names.end())
            return fail(SYBL_E_INVAL, "sybl_table_lookup: the output already holds a column '%s'", nm.c_str());
        names.push_back(nm);
    }
    if (dim->phys_rows > (int64_t)UINT32_MAX - 1)
        return fail(SYBL_E_INVAL, "sybl_table_lookup: %lld physical rows in the dim table are more than a 32-bit row number holds (2^32 - 2)",
                    (long long)dim->phys_rows);
    if ((rc = load_sync_all(ctx))) return rc;
    if ((rc = table_ensure_stats(dim))) return rc;  // (the tracked extrema; no version moves)

    // ---- dim's live rows
    std::vector<RowBlk> dblk;
    int64_t R = 0;
    for (const Segment &b : dim->blocks) {
        if (b.n <= 0) continue;  // (a dead block, sybl_table_refresh)
        dblk.push_back(RowBlk{b.start, b.n, R});
        R += b.n;
    }
    const bool any_keys = R > 0 && dk->n_pop > 0 && dk->d_data != nullptr;

    // ---- the path and its table
    int path = 0;
    int64_t cells = 0, slots = 0;
    LkTable T{};
    if (any_keys && tk->type == SYBL_STR_VAL) {
        path = kLkStr;
        cells = (int64_t)dk->dict.size();
        T.lo = 0;
        T.span = (uint64_t)(cells - 1);
        if (cells <= 0) path = 0;
    } else if (any_keys) {
        const unsigned __int128 range = (unsigned __int128)((__int128)dk->exact_max - (__int128)dk->exact_min) + 1;
        const unsigned __int128 direct_max = (unsigned __int128)kHashMaxSlots;  // 2^27 cells
        path = range <= (unsigned __int128)std::max<int64_t>((int64_t)1 << 16, 4 * R) && range <= direct_max ? kLkDirect : kLkHash;
        if (const char *e = env("SYBL_LOOKUP_PATH")) {
            if (!strcmp(e, "direct")) {
                if (range > direct_max)
                    return fail(SYBL_E_INVAL, "sybl_table_lookup: SYBL_LOOKUP_PATH=direct: the range of key column '%s' needs more than 2^27 cells", dkname);
                path = kLkDirect;
            } else if (!strcmp(e, "hash")) {
                path = kLkHash;
            } else if (e[0]) {
                return fail(SYBL_E_INVAL, "sybl_table_lookup: SYBL_LOOKUP_PATH='%s' is neither direct nor hash", e);
            }
        }
        if (path == kLkDirect) {
            cells = (int64_t)range;
            T.lo = dk->exact_min;
            T.span = (uint64_t)dk->exact_max - (uint64_t)dk->exact_min;
        } else {
            slots = 64;
            while (slots < 2 * R && slots <= kHashMaxSlots) slots <<= 1;
            if (const char *e = env("SYBL_LOOKUP_SLOTS")) {
                const long long want = atoll(e);
                if (!slots_ok(want))
                    return fail(SYBL_E_INVAL, "sybl_table_lookup: SYBL_LOOKUP_SLOTS=%s is not a power of two between 2 and %lld", e, (long long)kHashMaxSlots);
                slots = want;
            }
            if (slots > kHashMaxSlots)
                return fail(SYBL_E_INVAL, "sybl_table_lookup: %lld live rows in the dim table need %lld hash slots; the limit is kHashMaxSlots = %lld",
                            (long long)R, (long long)slots, (long long)kHashMaxSlots);
            cells = slots + 1;  // (+ the side cell of the key -1)
            T.slots = (uint32_t)slots;
        }
    }

    // ---- the t half: concat of t alone
    if ((rc = derived_copy(t, O))) return rc;
    Table *o = O.t;
    sybl_lookup_stats *S = &o->lookup_stats;
    const int64_t N = o->logical_rows, nb_out = (int64_t)o->blocks.size(), phys_out = o->phys_rows;
    const int64_t n_out = round_up(phys_out, 32);
    S->rows = N;
    S->blocks = nb_out;
    S->dim_rows = R;
    S->columns = (int32_t)src.size();

    // ---- the attached columns: type, IntInfo, dictionary id for id; storage by the storage rule over dim's tracked extrema
    const size_t nc = src.size();
    std::vector<Column *> att(nc);
    for (size_t k = 0; k < nc; k++) {
        const Column *c = src[k];
        auto n = std::make_unique<Column>();
        n->name = names[k];
        n->type = c->type;
        n->info_given = c->info_given;
        n->info_min = c->info_min;
        n->info_max = c->info_max;
        n->has_missing = c->has_missing;
        n->dict = c->dict;
        n->dict_ix = c->dict_ix;
        n->elem = n->canon();
        if (o->compact_mode && c->type != SYBL_SET_VAL) fit_storage(n->canon(), c->n_pop > 0 && c->d_data, c->exact_min, c->exact_max, &n->elem, &n->vbase);
        att[k] = n.get();
        o->col_ix[n->name] = (int)o->cols.size();
        o->cols.push_back(std::move(n));
    }
    if (N == 0) return SYBL_OK;  // (the columns and no blocks; no kernel runs)
    if (nb_out > INT32_MAX || (int64_t)dblk.size() > INT32_MAX)
        return fail(SYBL_E_INVAL, "sybl_table_lookup: more blocks than a launch counts");

    GatherPool pool;
    hipEvent_t ev[5];
    unsigned long long *counters = nullptr, h_counters[3] = {0, 0, 0};
    uint32_t *match = nullptr;
    RowBlk *d_dblk = nullptr, *d_oblk = nullptr;
    int32_t *d_lut = nullptr;
    std::vector<int32_t> lut;
    if ((rc = pool.alloc(&counters, 3, "lookup counters"))) return rc;
    if ((rc = pool.alloc(&match, (size_t)n_out, "lookup matches"))) return rc;
    SYBL_HIP(hipMemsetAsync(counters, 0, 3 * sizeof(unsigned long long), st));
    Column *ok = o->find(kname);  // t's key column as the output holds it
    if (path) {
        std::vector<RowBlk> oblk;
        for (const Segment &b : o->blocks) oblk.push_back(RowBlk{b.start, b.n, 0});
        if ((rc = pool.alloc(&d_dblk, dblk.size(), "lookup blocks"))) return rc;
        if ((rc = pool.alloc(&d_oblk, oblk.size(), "lookup blocks"))) return rc;
        if ((rc = pool.alloc(&T.first_row, (size_t)cells, "lookup cells"))) return rc;
        if (path == kLkHash && (rc = pool.alloc(&T.keys, (size_t)slots, "lookup hash keys"))) return rc;
        if ((rc = host_to_device(ctx, d_dblk, dblk.data(), dblk.size() * sizeof(RowBlk), "lookup blocks"))) return rc;
        if ((rc = host_to_device(ctx, d_oblk, oblk.data(), oblk.size() * sizeof(RowBlk), "lookup blocks"))) return rc;
        if (path == kLkStr) {  // t's dictionary id -> dim's, or -1 (the output holds t's dictionary id for id)
            lut.resize(std::max<size_t>(ok->dict.size(), 1), -1);
            for (size_t i = 0; i < ok->dict.size(); i++) {
                auto it = dk->dict_ix.find(ok->dict[i]);
                if (it != dk->dict_ix.end()) lut[i] = it->second;
            }
            if ((rc = pool.alloc(&d_lut, lut.size(), "lookup id table"))) return rc;
            if ((rc = host_to_device(ctx, d_lut, lut.data(), lut.size() * 4, "lookup id table"))) return rc;
        }

        // ---- build
        if ((rc = pool.event(&ev[0], st))) return rc;
        SYBL_HIP(hipMemsetAsync(T.first_row, 0xFF, (size_t)cells * 4, st));
        if (path == kLkHash) SYBL_HIP(hipMemsetAsync(T.keys, 0xFF, (size_t)slots * 8, st));
        const KeySide bs{dk->d_data, dk->vbase, dk->d_valid, d_dblk, (int)dblk.size(), R};
        by_width(dk->elem, [&](auto W) { launch_build<decltype(W)::value>(path, bs, T, counters, st); });
        SYBL_HIP(hipGetLastError());
        if ((rc = pool.event(&ev[1], st))) return rc;

        // ---- probe
        const KeySide ps{ok->d_data, ok->vbase, ok->d_valid, d_oblk, (int)oblk.size(), n_out};
        by_width(ok->elem, [&](auto W) { launch_probe<decltype(W)::value>(path, ps, T, d_lut, (int64_t)ok->dict.size(), match, counters, st); });
        SYBL_HIP(hipGetLastError());
        if ((rc = pool.event(&ev[2], st))) return rc;
        uint32_t side = kLkNone;  // (hash: the side cell of the key -1)
        SYBL_HIP(hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));  // read back once
        if (path == kLkHash) SYBL_HIP(hipMemcpyAsync(&side, T.first_row + slots, 4, hipMemcpyDeviceToHost, st));
        SYBL_HIP(hipStreamSynchronize(st));
        const int64_t populated = (int64_t)(h_counters[0] >> 32), occupied = (int64_t)(h_counters[0] & 0xFFFFFFFFull);
        // a key that found no slot, or no free slot left: the table needs its keys + 1 slots
        if (path == kLkHash && (h_counters[1] != 0 || occupied - (side != kLkNone ? 1 : 0) >= slots))
            return fail(SYBL_E_NOMEM, "sybl_table_lookup: the hash table of %lld slots is full (%lld rows of the dim table found no slot)",
                        (long long)slots, (long long)h_counters[1]);
        S->dim_keys = occupied;
        S->dim_duplicates = populated - occupied;
        S->matched = (int64_t)h_counters[2];
        S->slots = slots;
        S->path = path;
        const int64_t dvalid = dk->d_valid ? (R + 7) / 8 : 0, ovalid = ok->d_valid ? (N + 7) / 8 : 0;
        S->build_bytes = cells * 4 + slots * 8 + R * ((int64_t)dk->elem + 4 + (path == kLkHash ? 8 : 0)) + dvalid;
        S->probe_bytes = n_out * 4 + N * ((int64_t)ok->elem + 4 + (path == kLkHash ? 8 : path == kLkStr ? 4 : 0)) + ovalid;
    } else {
        // no populated key in dim: nothing matches, no table is built
        SYBL_HIP(hipMemsetAsync(match, 0xFF, (size_t)n_out * 4, st));
    }
    const bool missed = S->matched < N;

    // ---- gather: every attached column whole, into its final place
    if ((rc = table_upload_blocks(o))) return rc;
    if ((rc = pool.event(&ev[3], st))) return rc;
    size_t n_stat = 0;
    for (size_t k = 0; k < nc; k++) n_stat += att[k]->type != SYBL_SET_VAL;
    BlockStats stats;
    if ((rc = stats.begin(n_stat, o->d_blocks, nb_out, pool, "lookup statistics"))) return rc;
    for (size_t k = 0; k < nc; k++) {
        const Column *c = src[k];
        Column *n = att[k];
        const bool holds = c->type == SYBL_SET_VAL || c->d_data != nullptr;  // (else no row of the column was ever written)
        n->has_missing = n->has_missing || missed || !holds;
        if (c->d_valid || missed || !holds) {
            if ((rc = valid_reserve(o, n, phys_out))) return rc;  // (the words behind the output's rows: zero)
            if (holds && S->matched > 0) {
                hipLaunchKernelGGL(k_lk_valid, dim3(grid_for(n_out, kLkThreads)), dim3(kLkThreads), 0, st, (const uint32_t *)c->d_valid,
                                   (const uint32_t *)match, n_out, n->d_valid);
                SYBL_HIP(hipGetLastError());
            } else {
                SYBL_HIP(hipMemsetAsync(n->d_valid, 0, (size_t)(n_out / 32) * 4, st));
            }
            S->gather_bytes += n_out * 4 + n_out / 8 + (c->d_valid ? S->matched * 4 : 0);
        }
        if (n->type == SYBL_SET_VAL) continue;
        if ((rc = table_reserve(o, n, phys_out))) return rc;
        if (!holds || S->matched == 0) {
            SYBL_HIP(hipMemsetAsync(n->d_data, 0, (size_t)n_out * (size_t)n->elem, st));
            S->gather_bytes += n_out * (int64_t)n->elem;
        } else {
            by_width(c->elem, [&](auto WS) {
                by_width(n->elem, [&](auto WD) { launch_gather<decltype(WS)::value, decltype(WD)::value>(c, match, n_out, n, st); });
            });
            SYBL_HIP(hipGetLastError());
            S->gather_bytes += n_out * (4 + (int64_t)n->elem) + S->matched * (int64_t)c->elem + (c->d_valid ? S->matched * 4 : 0);
        }
        if ((rc = stats.launch(n, st))) return rc;  // (behind its gather: the column is read back from the cache)
    }
    if ((rc = stats.finish(st, pool, &ev[4]))) return rc;  // the ONE wait for the statistics of every block of every attached column

    // ---- set columns: the host CSR over the output's physical rows, from the match list
    bool any_set = false;
    for (const Column *c : src) any_set = any_set || c->type == SYBL_SET_VAL;
    if (any_set) {
        std::vector<uint32_t> hm((size_t)n_out);
        SYBL_HIP(hipMemcpy(hm.data(), match, (size_t)n_out * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nc; k++) {
            const Column *c = src[k];
            Column *n = att[k];
            if (c->type != SYBL_SET_VAL) continue;
            n->h_set_off.assign(1, 0);
            set_gather(c->h_set_off, c->h_set_vals, hm.data(), phys_out, n->h_set_off, n->h_set_vals);  // (padding rows match nothing: empty sets)
            n->set_dirty = true;
            if ((rc = column_upload_set(o, n))) return rc;
        }
    }
    o->version++;
    float f = 0;
    if (path) {
        SYBL_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
        S->build_ms = f;
        SYBL_HIP(hipEventElapsedTime(&f, ev[1], ev[2]));
        S->probe_ms = f;
    }
    SYBL_HIP(hipEventElapsedTime(&f, ev[3], ev[4]));
    S->gather_ms = f;
    return SYBL_OK;
}

}  // namespace

int lookup_run(Table *t, const sybl_lookup_desc *d, sybl_table **out) {
    TableOwner O;  // (run makes the table: the copy of t)
    return derived_call(t->ctx, "sybl_table_lookup", O, out, [&] { return run(t, d, O); });
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_lookup(sybl_table *t, const sybl_lookup_desc *d, sybl_table **out) {
    SYBL_API_GUARD(t);
    if (out) *out = nullptr;
    if (!t || !d || !out || !d->dim) return fail(SYBL_E_INVAL, "sybl_table_lookup: NULL argument");
    if (d->dim->ctx != t->ctx) return fail(SYBL_E_INVAL, "sybl_table_lookup: the dim table belongs to another context");
    return lookup_run(t, d, out);
}

int sybl_table_lookup_stats(const sybl_table *t, sybl_lookup_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_lookup_stats: NULL argument");
    *out = t->lookup_stats;
    return SYBL_OK;
}

}  // extern "C"
