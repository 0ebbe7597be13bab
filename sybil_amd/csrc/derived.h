// derived.h -- what the calls that make a NEW resident table from resident ones share on the HIP side: digest.hip, select.hip,
// concat.hip, lookup.hip, compute.hip.  The host rules (storage, statistics fold, set-column gather) are colstats.h; the
// function bodies that launch no kernel are derived.cpp; gather_make_columns / gather_rows are in digest.hip, beside their
// kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <type_traits>
#include <vector>

#include "colstats.h"
#include "engine.h"

namespace sybl {

// ------------------------------------------------------------------ device

// a live block among the rows a kernel walks
struct RowBlk {
    int64_t start;  // its first physical row
    int64_t n;      // its logical rows
    int64_t base;   // what lies before it, in the unit the kernel counts: live rows (digest keys, lookup build), tiles (compute)
};

// Which block holds index i: the last of blk[0 .. nb) whose `key` member is <= i, by bisection.
template <class B>
__device__ __forceinline__ int block_of(const B *__restrict__ blk, int nb, int64_t i, int64_t B::*key) {
    int a = 0, b = nb - 1;
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (blk[m].*key <= i) a = m;
        else b = m - 1;
    }
    return a;
}

// ... for a lane per index: the bisection runs on `first` <= i, the wave's first index -- the same addresses in every lane,
// broadcast loads -- and every lane walks on from there.
template <class B>
__device__ __forceinline__ int block_of(const B *__restrict__ blk, int nb, int64_t first, int64_t i, int64_t B::*key) {
    int a = block_of(blk, nb, first, key);
    while (a + 1 < nb && blk[a + 1].*key <= i) a++;
    return a;
}

template <class I>
__device__ __forceinline__ bool valid_bit(const uint32_t *valid, I row) {
    return (valid[row >> 5] >> (row & 31)) & 1u;
}

// ------------------------------------------------------------------ host

inline unsigned grid_for(int64_t n, int threads) { return (unsigned)std::max<int64_t>(1, (n + threads - 1) / threads); }
inline const char *type_name(int ty) { return ty == SYBL_INT_VAL ? "int" : ty == SYBL_STR_VAL ? "str" : "set"; }

// f(std::integral_constant<int, W>) for the stored width W = 8 / 4 / 2 / 1
template <class F>
inline void by_width(int width, F &&f) {
    switch (width) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
    }
}

inline ColStats col_stats(Column *c, bool missing = false) {
    return ColStats{c->blk_min, c->blk_max, c->blk_pop, c->exact_min, c->exact_max, c->n_pop, c->stats_blocks, missing ? &c->has_missing : nullptr};
}

// everything a run allocates on the device, freed on every exit
struct GatherPool {
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> events;
    ~GatherPool() {
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
    int event(hipEvent_t *out, hipStream_t st) {
        hipEvent_t e = nullptr;
        SYBL_HIP(hipEventCreate(&e));
        events.push_back(e);
        SYBL_HIP(hipEventRecord(e, st));
        *out = e;
        return SYBL_OK;
    }
};

// the output table, freed on every exit unless it is handed to the caller
struct TableOwner {
    sybl_table *t = nullptr;
    ~TableOwner() {
        if (t) sybl_table_free(t);
    }
};

// an empty output table of ctx in O.  `who` opens the messages of errors, here and below.
int derived_new_table(Ctx *ctx, const std::string &name, const char *who, TableOwner &O);

// The call around a run: the device, `body`, its exceptions as error codes.  On failure the stream is drained, so nothing of
// the call is in flight when O frees the table; on success O.t is handed to *out.
int derived_call(Ctx *ctx, const char *who, TableOwner &O, sybl_table **out, const std::function<int()> &body);

// O.t = sybl_table_concat of t alone -- rows, blocks, columns, storage, statistics --, its concat_stats zero: the table belongs
// to the call that adds columns to it.
int derived_copy(Table *t, TableOwner &O);

// the named columns of t, each once, in the order named; names == nullptr or n <= 0: every column but `except`.  An unknown
// name: "<who>: unknown column '<name>'<where>".
int resolve_columns(Table *t, const char *const *names, int n, const char *who, const char *where, const Column *except, std::vector<Column *> *out);

// Block statistics of freshly written non-set columns over the nb blocks of the device list `segs`: begin (scratch for
// n_cols columns; `what` names it in an allocation error), one k_block_minmax launch per column -- each as soon as the column
// is written, while it is in the cache --, then finish: *launched (if given) recorded behind the launches, one readback, the
// ONE wait, stats_fold into each column.  With no column finish still records and waits.
struct BlockStats {
    const Segment *segs = nullptr;
    int64_t nb = 0;
    int64_t *d_out = nullptr;
    std::vector<Column *> cols;
    int begin(size_t n_cols, const Segment *segs_, int64_t nb_, GatherPool &pool, const char *what);
    int launch(Column *c, hipStream_t st);
    int finish(hipStream_t st, GatherPool &pool, hipEvent_t *launched);
};

// begin, a launch per column, finish
int derived_block_stats(Table *o, const std::vector<Column *> &cols, const Segment *segs, int64_t nb, GatherPool &pool, const char *what,
                        hipEvent_t *launched);

// the output's columns -- src[k] of t becomes column k of o --: name, type, IntInfo, dictionaries (id for id), declared
// bounds, has_missing, storage (width, base)
void gather_make_columns(const Table *t, const std::vector<Column *> &src, Table *o);

// Output block j of o = rows[j * block_rows, min(N, (j+1) * block_rows)) of t, for the columns gather_make_columns made:
// the output layout, k_dg_gather<W> per column, k_dg_valid, the block statistics, the host CSR gather for set columns, the
// block writer and the validity copy.  rows: N physical source rows, on the device.  N > 0.  *gathered is recorded on the
// ctx stream behind the last gather launch (the pool owns it); *bytes grows by the bytes the gather moves, computed from
// the shapes; *blocks = the output's blocks.  Complete on return.
int gather_rows(Table *t, const std::vector<Column *> &src, const uint32_t *rows, int64_t N, int64_t block_rows, Table *o, GatherPool &pool,
                const char *who, hipEvent_t *gathered, int64_t *bytes, int64_t *blocks);

}  // namespace sybl
