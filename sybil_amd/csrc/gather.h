// gather.h -- a NEW resident table from a row list of a resident one: what digest.hip (the list is the sort's permutation)
// and select.hip (the list is the matching rows, ascending) share.  The kernels and the function bodies are in digest.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine.h"

namespace sybl {

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

// the output's columns -- src[k] of t becomes column k of o --: name, type, IntInfo, dictionaries (id for id), declared
// bounds, has_missing, storage (width, base)
void gather_make_columns(const Table *t, const std::vector<Column *> &src, Table *o);

// Output block j of o = rows[j * block_rows, min(N, (j+1) * block_rows)) of t, for the columns gather_make_columns made:
// the output layout, k_dg_gather<W> per column, k_dg_valid, the block statistics, the host CSR gather for set columns, the
// block writer and the validity copy.  rows: N physical source rows, on the device.  N > 0.  *gathered is recorded on the
// ctx stream behind the last gather launch (the pool owns it); *bytes grows by the bytes the gather moves, computed from
// the shapes; *blocks = the output's blocks.  `who` opens the messages of errors.  Complete on return.
int gather_rows(Table *t, const std::vector<Column *> &src, const uint32_t *rows, int64_t N, int64_t block_rows, Table *o, GatherPool &pool,
                const char *who, hipEvent_t *gathered, int64_t *bytes, int64_t *blocks);

// concat.hip: the (width, base) of a compact column whose tracked extrema are [lo, hi] (any = false: no populated row -- width 1,
// base 0): the narrowest of 1 / 2 / 4 / 8 bytes that holds hi - lo, offsets from lo; the canonical width has base 0.  Shared with
// lookup.hip.
void concat_fit(const Column *c, bool any, int64_t lo, int64_t hi, int *width, int64_t *base);

}  // namespace sybl
