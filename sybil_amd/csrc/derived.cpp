// derived.cpp -- the host scaffold of the calls that make a new resident table (derived.h): nothing here launches a kernel of
// its own.
#include <new>

#include "derived.h"

namespace sybl {

int derived_new_table(Ctx *ctx, const std::string &name, const char *who, TableOwner &O) {
    O.t = new (std::nothrow) sybl_table();
    if (!O.t) return fail(SYBL_E_NOMEM, "%s: out of host memory", who);
    O.t->ctx = ctx;
    O.t->name = name;
    return SYBL_OK;
}

int derived_call(Ctx *ctx, const char *who, TableOwner &O, sybl_table **out, const std::function<int()> &body) {
    SYBL_HIP(hipSetDevice(ctx->device));
    int rc;
    try {
        rc = body();
    } catch (const std::bad_alloc &) {
        rc = fail(SYBL_E_NOMEM, "%s: out of host memory", who);
    } catch (const std::exception &e) {
        rc = fail(SYBL_E_INVAL, "%s: %s", who, e.what());
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call is in flight when its buffers go)
        return rc;
    }
    *out = O.t;
    O.t = nullptr;
    return SYBL_OK;
}

int derived_copy(Table *t, TableOwner &O) {
    sybl_table *tt = static_cast<sybl_table *>(t);
    sybl_concat_desc cd{};
    cd.n_tables = 1;
    cd.tables = &tt;
    int rc = concat_run(&cd, &O.t);
    if (rc) return rc;
    O.t->concat_stats = sybl_concat_stats{};  // (this table was made by the caller)
    return SYBL_OK;
}

int resolve_columns(Table *t, const char *const *names, int n, const char *who, const char *where, const Column *except, std::vector<Column *> *out) {
    if (names && n > 0) {
        for (int i = 0; i < n; i++) {
            Column *c = t->find(names[i]);
            if (!c) return fail(SYBL_E_INVAL, "%s: unknown column '%s'%s", who, names[i] ? names[i] : "(null)", where);
            if (std::find(out->begin(), out->end(), c) == out->end()) out->push_back(c);
        }
    } else {
        for (auto &cp : t->cols)
            if (cp.get() != except) out->push_back(cp.get());
    }
    return SYBL_OK;
}

int BlockStats::begin(size_t n_cols, const Segment *segs_, int64_t nb_, GatherPool &pool, const char *what) {
    segs = segs_;
    nb = nb_;
    cols.reserve(n_cols);
    return n_cols ? pool.alloc(&d_out, n_cols * 3 * (size_t)nb, what) : SYBL_OK;
}

int BlockStats::launch(Column *c, hipStream_t st) {
    int64_t *out = d_out + cols.size() * 3 * (size_t)nb;
    hipError_t e = launch_block_minmax(c->d_data, c->elem, c->vbase, c->d_valid, segs, (int)nb, out, out + nb, out + 2 * nb, st);
    if (e != hipSuccess) return hip_fail(e, "k_block_minmax");
    cols.push_back(c);
    return SYBL_OK;
}

int BlockStats::finish(hipStream_t st, GatherPool &pool, hipEvent_t *launched) {
    int rc;
    if (launched && (rc = pool.event(launched, st))) return rc;
    const size_t per = 3 * (size_t)nb;
    std::vector<int64_t> stats(cols.size() * per);
    if (!cols.empty()) SYBL_HIP(hipMemcpyAsync(stats.data(), d_out, stats.size() * 8, hipMemcpyDeviceToHost, st));
    SYBL_HIP(hipStreamSynchronize(st));  // the ONE wait for the statistics of every block of every column
    for (size_t k = 0; k < cols.size(); k++) stats_fold(col_stats(cols[k]), stats.data() + k * per, nb, 0, nb);
    return SYBL_OK;
}

int derived_block_stats(Table *o, const std::vector<Column *> &cols, const Segment *segs, int64_t nb, GatherPool &pool, const char *what,
                        hipEvent_t *launched) {
    hipStream_t st = o->ctx->stream;
    BlockStats bs;
    int rc = bs.begin(cols.size(), segs, nb, pool, what);
    for (size_t k = 0; k < cols.size() && !rc; k++) rc = bs.launch(cols[k], st);
    return rc ? rc : bs.finish(st, pool, launched);
}

}  // namespace sybl
