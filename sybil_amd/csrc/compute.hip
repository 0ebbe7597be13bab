// compute.hip -- int columns computed from expressions over a resident table's columns, as a NEW resident table.  The semantics
// are restated in include/sybilgpu.h ("compute") and DESIGN.md 3.12; the expression language, its parser and the host evaluator
// are compute_expr.h, the arithmetic of every op is compute_ops.h (shared with the kernel).  This file is the device work and the
// host code that drives it.
//
// The `t` half of the output IS sybl_table_concat of t alone (derived_copy, derived.h; the call wrapper, the block search and
// the statistics -- derived_block_stats -- are there too).  Expression k is evaluated on the OUTPUT's own columns
// at each physical row -- no row of t has to be located again, and expression k may name computed columns 0 .. k-1.
//
//   k_cx_eval<false, 0>  the range pass: every live row evaluated; per lane the running min / max of the populated results and
//                        their count, reduced over the wave (shuffles), then through LDS, and ONE signed 64-bit atomic min, one
//                        max and one add per workgroup.  The host reads the three words back, fits (width, base) with the storage
//                        rule (colstats.h), decides has_missing and the bitmap and reserves the column.
//   k_cx_eval<true, W>   the store pass: evaluates again and writes (v - base) at width W, 0 where unpopulated and in padding; a
//                        lane writes whole dwords.  Where the column has a bitmap its words are OR-ed together from the 8 lanes
//                        that hold a word's 32 rows.
//   statistics           k_block_minmax (kernels.hip) over every computed column, one readback for all of them.
//
// The interpreter: a lane owns FOUR consecutive physical rows and runs the program once for all four -- the dispatch is paid per
// four rows and a column is read as one dword (width 1), two (2), four (4) or eight (8) per lane, when its push op executes.  The
// program, the constants and the column table arrive as a kernel argument and stay scalar; the ops are dispatched by a
// wave-uniform switch.  The top of the operand stack is four registers; everything below it lives in LDS as [depth][row][thread]
// (8-byte words, consecutive lanes consecutive words: no bank conflict), sized for the program's own depth by the launch; the
// populated bits are one 32-bit mask per lane, four bits per depth.  No scratch.
// A block starts on a multiple of 32 physical rows; a tile is 1024 rows of ONE block, the host makes the prefix of tiles per
// block and a workgroup finds the block of a tile by a scalar bisection.  Workgroups take tiles grid-stride.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "compute_expr.h"
#include "derived.h"

namespace sybl {

constexpr int kCxThreads = 256;
constexpr int kCxRows = 4;                          // per lane
constexpr int kCxTileRows = kCxThreads * kCxRows;   // 1024
constexpr int kCxWgPerCu = 8;

struct CxCol {
    const void *data;       // nullptr: a set column, or no row was ever written
    const uint32_t *valid;  // nullptr: every row populated
    int64_t base;
    int32_t width;
    int32_t holds;  // 0: every row unpopulated
};

struct CxArgs {
    uint32_t ops[kCxMaxOps];  // op | arg << 8
    int64_t consts[kCxMaxOps];
    CxCol cols[kCxMaxCols];
    const RowBlk *blk;  // base: the tiles before a block
    int64_t n_tiles;
    int32_t n_ops, nb;
    void *out;             // store pass
    uint32_t *out_valid;   // ... nullptr: the column has no bitmap
    int64_t out_base;
    long long *acc;        // range pass: min, max, populated count
};

// the four rows p0 .. p0 + 3 of a column (p0 a multiple of 4, inside a block's padded rows): values and populated bits
__device__ __forceinline__ void cx_load(const CxCol &c, int64_t p0, uint32_t live, bool want_values, int64_t v[kCxRows], uint32_t *pop) {
    *pop = 0;
#pragma unroll
    for (int k = 0; k < kCxRows; k++) v[k] = 0;
    if (!c.holds || live == 0) return;
    uint32_t bits = 0xFu;
    if (c.valid != nullptr) bits = (c.valid[p0 >> 5] >> (p0 & 31)) & 0xFu;
    bits &= live;
    *pop = bits;
    if (!want_values || c.data == nullptr) return;
    uint64_t raw[kCxRows];
    switch (c.width) {
    case 8: {
        const ulonglong2 a = ((const ulonglong2 *)c.data)[p0 >> 1], b = ((const ulonglong2 *)c.data)[(p0 >> 1) + 1];
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
    for (int k = 0; k < kCxRows; k++) v[k] = (bits >> k) & 1u ? (int64_t)((uint64_t)c.base + raw[k]) : 0;
}

// the program over the lane's four rows.  stk: the lane's column of the LDS stack (stride kCxThreads words).
__device__ __forceinline__ void cx_run(const CxArgs &A, int64_t p0, uint32_t live, int64_t *stk, int64_t top[kCxRows], uint32_t *top_pop) {
    uint32_t pb = 0;  // populated bits: 4 per stack position
    int sp = 0;       // operands on the stack; position sp - 1 is `top`, the ones below are in LDS
#pragma unroll
    for (int k = 0; k < kCxRows; k++) top[k] = 0;
    for (int pc = 0; pc < A.n_ops; pc++) {
        const uint32_t w = A.ops[pc];
        const int op = (int)(w & 0xFFu), arg = (int)(w >> 8);
        if (op <= kCxHas) {
            if (sp > 0) {
#pragma unroll
                for (int k = 0; k < kCxRows; k++) stk[((sp - 1) * kCxRows + k) * kCxThreads] = top[k];
            }
            uint32_t np = 0xFu;
            if (op == kCxPushConst) {
                const int64_t c = A.consts[arg];
#pragma unroll
                for (int k = 0; k < kCxRows; k++) top[k] = c;
            } else if (op == kCxPushCol) {
                cx_load(A.cols[arg], p0, live, true, top, &np);
            } else {
                cx_load(A.cols[arg], p0, live, false, top, &np);
#pragma unroll
                for (int k = 0; k < kCxRows; k++) top[k] = cx_has((np >> k) & 1u).v;
                np = 0xFu;
            }
            pb = (pb & ~(0xFu << (4 * sp))) | (np << (4 * sp));
            sp++;
            continue;
        }
        const uint32_t pt = (pb >> (4 * (sp - 1))) & 0xFu;
        uint32_t np = 0;
        if (op <= kCxAbs) {
#define CX_UN(f)                                                       \
    _Pragma("unroll") for (int k = 0; k < kCxRows; k++) {              \
        const CxVal r = f(CxVal{top[k], (bool)((pt >> k) & 1u)});      \
        top[k] = r.v;                                                  \
        np |= (uint32_t)r.p << k;                                      \
    }                                                                  \
    break;
            switch (op) {
            case kCxNeg: CX_UN(cx_neg)
            case kCxNot: CX_UN(cx_not)
            default: CX_UN(cx_abs)
            }
#undef CX_UN
            pb = (pb & ~(0xFu << (4 * (sp - 1)))) | (np << (4 * (sp - 1)));
            continue;
        }
        int64_t a[kCxRows];
        const uint32_t pa = (pb >> (4 * (sp - 2))) & 0xFu;
#pragma unroll
        for (int k = 0; k < kCxRows; k++) a[k] = stk[((sp - 2) * kCxRows + k) * kCxThreads];
        if (op == kCxIf) {
            const uint32_t pc_ = (pb >> (4 * (sp - 3))) & 0xFu;
#pragma unroll
            for (int k = 0; k < kCxRows; k++) {
                const int64_t c = stk[((sp - 3) * kCxRows + k) * kCxThreads];
                const CxVal r = cx_if(CxVal{c, (bool)((pc_ >> k) & 1u)}, CxVal{a[k], (bool)((pa >> k) & 1u)}, CxVal{top[k], (bool)((pt >> k) & 1u)});
                top[k] = r.v;
                np |= (uint32_t)r.p << k;
            }
            sp -= 2;
        } else {
#define CX_BIN(f)                                                                                    \
    _Pragma("unroll") for (int k = 0; k < kCxRows; k++) {                                            \
        const CxVal r = f(CxVal{a[k], (bool)((pa >> k) & 1u)}, CxVal{top[k], (bool)((pt >> k) & 1u)}); \
        top[k] = r.v;                                                                                \
        np |= (uint32_t)r.p << k;                                                                    \
    }                                                                                                \
    break;
            switch (op) {
            case kCxMul: CX_BIN(cx_mul)
            case kCxDiv: CX_BIN(cx_div)
            case kCxMod: CX_BIN(cx_mod)
            case kCxAdd: CX_BIN(cx_add)
            case kCxSub: CX_BIN(cx_sub)
            case kCxLt: CX_BIN(cx_lt)
            case kCxLe: CX_BIN(cx_le)
            case kCxGt: CX_BIN(cx_gt)
            case kCxGe: CX_BIN(cx_ge)
            case kCxEq: CX_BIN(cx_eq)
            case kCxNe: CX_BIN(cx_ne)
            case kCxAnd: CX_BIN(cx_and)
            case kCxOr: CX_BIN(cx_or)
            case kCxMin: CX_BIN(cx_min)
            case kCxMax: CX_BIN(cx_max)
            default: CX_BIN(cx_coalesce)
            }
#undef CX_BIN
            sp -= 1;
        }
        pb = (pb & ~(0xFu << (4 * (sp - 1)))) | (np << (4 * (sp - 1)));
    }
    *top_pop = pb & 0xFu;  // (a compiled program leaves exactly one operand)
}

template <bool STORE, int W>
__global__ __launch_bounds__(kCxThreads) void k_cx_eval(const CxArgs A) {
    extern __shared__ int64_t cx_stack[];  // [depth - 1][kCxRows][kCxThreads]
    __shared__ long long red[3 * (kCxThreads / 64)];
    const int tid = (int)threadIdx.x;
    long long mn = INT64_MAX, mx = INT64_MIN, cnt = 0;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const RowBlk B = A.blk[block_of(A.blk, A.nb, tile, &RowBlk::base)];  // (uniform, scalar)
        const int64_t p0 = B.start + (tile - B.base) * kCxTileRows + (int64_t)tid * kCxRows;
        const int64_t pad_end = B.start + ((B.n + 31) & ~(int64_t)31);
        const bool active = p0 < pad_end;  // (8 lanes = one 32-row word: all of them active or none)
        const int64_t left = B.start + B.n - p0;
        const uint32_t live = !active || left <= 0 ? 0u : left >= kCxRows ? 0xFu : (1u << (int)left) - 1u;
        int64_t v[kCxRows];
        uint32_t pop = 0;
        cx_run(A, p0, live, cx_stack + tid, v, &pop);
        pop &= live;
        if (STORE) {
            if (active) {
                uint64_t e[kCxRows];
#pragma unroll
                for (int k = 0; k < kCxRows; k++) e[k] = (pop >> k) & 1u ? (uint64_t)v[k] - (uint64_t)A.out_base : 0;
                if (W == 8) {
                    ((ulonglong2 *)A.out)[p0 >> 1] = make_ulonglong2(e[0], e[1]);
                    ((ulonglong2 *)A.out)[(p0 >> 1) + 1] = make_ulonglong2(e[2], e[3]);
                } else if (W == 4) {
                    ((uint4 *)A.out)[p0 >> 2] = make_uint4((uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]);
                } else if (W == 2) {
                    ((uint2 *)A.out)[p0 >> 2] = make_uint2(((uint32_t)e[0] & 0xFFFFu) | ((uint32_t)e[1] << 16), ((uint32_t)e[2] & 0xFFFFu) | ((uint32_t)e[3] << 16));
                } else {
                    ((uint32_t *)A.out)[p0 >> 2] =
                        ((uint32_t)e[0] & 0xFFu) | (((uint32_t)e[1] & 0xFFu) << 8) | (((uint32_t)e[2] & 0xFFu) << 16) | ((uint32_t)e[3] << 24);
                }
            }
            if (A.out_valid != nullptr) {  // (uniform; every lane takes part in the shuffles)
                uint32_t word = pop << (4 * (tid & 7));
                word |= (uint32_t)__shfl_xor((int)word, 1);
                word |= (uint32_t)__shfl_xor((int)word, 2);
                word |= (uint32_t)__shfl_xor((int)word, 4);
                if (active && (tid & 7) == 0) A.out_valid[p0 >> 5] = word;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kCxRows; k++)
                if ((pop >> k) & 1u) {
                    mn = v[k] < mn ? v[k] : mn;
                    mx = v[k] > mx ? v[k] : mx;
                    cnt++;
                }
        }
    }
    if (!STORE) {
        for (int d = 32; d > 0; d >>= 1) {
            const long long omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d), oc = __shfl_xor(cnt, d);
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
            for (int k = 1; k < kCxThreads / 64; k++) {
                mn = red[3 * k] < mn ? red[3 * k] : mn;
                mx = red[3 * k + 1] > mx ? red[3 * k + 1] : mx;
                cnt += red[3 * k + 2];
            }
            if (cnt > 0) {  // one set of atomics per workgroup
                __hip_atomic_fetch_min(A.acc, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(A.acc + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(A.acc + 2, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

namespace {

void launch_eval(bool store, int width, const CxArgs &A, unsigned grid, size_t lds, hipStream_t st) {
    const dim3 g(grid), b(kCxThreads);
    if (!store) hipLaunchKernelGGL((k_cx_eval<false, 0>), g, b, lds, st, A);
    else by_width(width, [&](auto W) { hipLaunchKernelGGL((k_cx_eval<true, decltype(W)::value>), g, b, lds, st, A); });
}

// compiles `expr` against a column list; on a refusal the message is "column '<name>': <why>"
bool compile_for(const char *name, const char *expr, const std::vector<const char *> &names, const std::vector<int32_t> &types, CxProgram *P,
                 std::string *err) {
    CxParser parser(expr, strlen(expr), (int32_t)names.size(), names.data(), types.data(), P);
    if (parser.compile()) return true;
    *err = std::string("column '") + name + "': " + parser.error();
    return false;
}

int run(Table *t, const sybl_compute_desc *d, TableOwner &O) {
    Ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    int rc;

    // ---- the arguments: everything that can be refused is refused before anything is made
    if (d->n_exprs < 1) return fail(SYBL_E_INVAL, "sybl_table_compute: n_exprs = %d: at least one expression is needed", (int)d->n_exprs);
    const size_t ne = (size_t)d->n_exprs;
    std::vector<const char *> names;
    std::vector<int32_t> types;
    for (auto &cp : t->cols) {
        names.push_back(cp->name.c_str());
        types.push_back(cp->type);
    }
    const size_t nt = names.size();
    std::vector<CxProgram> progs(ne);
    for (size_t k = 0; k < ne; k++) {
        const char *nm = d->exprs[k].name, *ex = d->exprs[k].expr;
        if (!nm) return fail(SYBL_E_INVAL, "sybl_table_compute: NULL name of expression %d", (int)k);
        if (!ex) return fail(SYBL_E_INVAL, "sybl_table_compute: NULL expr of column '%s'", nm);
        if (!nm[0]) return fail(SYBL_E_INVAL, "sybl_table_compute: column '': expression %d has an empty name", (int)k);
        for (size_t j = 0; j < names.size(); j++)
            if (!strcmp(names[j], nm)) return fail(SYBL_E_INVAL, "sybl_table_compute: column '%s': the output already holds a column of that name", nm);
        std::string err;
        if (!compile_for(nm, ex, names, types, &progs[k], &err)) return fail(SYBL_E_INVAL, "sybl_table_compute: %s", err.c_str());
        names.push_back(nm);
        types.push_back(SYBL_INT_VAL);
    }
    if ((rc = load_sync_all(ctx))) return rc;

    // ---- the t half: concat of t alone
    if ((rc = derived_copy(t, O))) return rc;
    Table *o = O.t;
    if (o->cols.size() != nt) return fail(SYBL_E_STATE, "sybl_table_compute: the copy of the table holds %d columns, not %d", (int)o->cols.size(), (int)nt);
    sybl_compute_stats *S = &o->compute_stats;
    const int64_t N = o->logical_rows, nb_out = (int64_t)o->blocks.size(), phys_out = o->phys_rows;
    S->rows = N;
    S->blocks = nb_out;
    S->exprs = (int32_t)ne;
    for (const CxProgram &P : progs) S->ops += P.n_ops;

    // ---- the computed columns: INT, no IntInfo, no dictionary, no declared bounds; canonical until the range is known
    std::vector<Column *> att(ne);
    for (size_t k = 0; k < ne; k++) {
        auto n = std::make_unique<Column>();
        n->name = d->exprs[k].name;
        n->type = SYBL_INT_VAL;
        n->elem = n->canon();
        if (o->compact_mode) fit_storage(n->canon(), false, 0, 0, &n->elem, &n->vbase);
        att[k] = n.get();
        o->col_ix[n->name] = (int)o->cols.size();
        o->cols.push_back(std::move(n));
    }
    if (N == 0) return SYBL_OK;  // (the columns and no blocks; no kernel runs)
    if (nb_out > INT32_MAX) return fail(SYBL_E_INVAL, "sybl_table_compute: more blocks than a launch counts");

    // ---- tiles per block
    std::vector<RowBlk> blk;
    int64_t n_tiles = 0;
    for (const Segment &b : o->blocks) {
        if (b.n <= 0) continue;
        blk.push_back(RowBlk{b.start, b.n, n_tiles});
        n_tiles += (round_up(b.n, 32) + kCxTileRows - 1) / kCxTileRows;
    }
    const int64_t n_out = round_up(phys_out, 32);
    GatherPool pool;
    RowBlk *d_blk = nullptr;
    long long *d_acc = nullptr;
    if ((rc = pool.alloc(&d_blk, blk.size(), "compute blocks"))) return rc;
    if ((rc = pool.alloc(&d_acc, 3 * ne + 1, "compute extrema"))) return rc;
    if ((rc = host_to_device(ctx, d_blk, blk.data(), blk.size() * sizeof(RowBlk), "compute blocks"))) return rc;
    std::vector<long long> h_acc(3 * ne + 1, 0);
    for (size_t k = 0; k < ne; k++) h_acc[3 * k] = INT64_MAX, h_acc[3 * k + 1] = INT64_MIN;
    if ((rc = host_to_device(ctx, d_acc, h_acc.data(), h_acc.size() * sizeof(long long), "compute extrema"))) return rc;
    if ((rc = table_upload_blocks(o))) return rc;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)std::max(ctx->n_cus, 1) * kCxWgPerCu));

    std::vector<hipEvent_t> ev(4 * ne + 2);
    for (size_t k = 0; k < ne; k++) {
        const CxProgram &P = progs[k];
        Column *n = att[k];
        CxArgs A{};
        for (int i = 0; i < P.n_ops; i++) A.ops[i] = (uint32_t)P.op[i] | ((uint32_t)P.arg[i] << 8);
        for (int i = 0; i < P.n_consts; i++) A.consts[i] = P.consts[i];
        int64_t src_bytes = 0;
        for (int i = 0; i < P.n_cols; i++) {
            const Column *c = o->cols[(size_t)P.cols[i]].get();
            const bool holds = c->type == SYBL_SET_VAL || c->d_data != nullptr;
            A.cols[i] = CxCol{c->type == SYBL_SET_VAL ? nullptr : c->d_data, c->d_valid, c->vbase, c->type == SYBL_SET_VAL ? 0 : c->elem, holds ? 1 : 0};
            src_bytes += N * (int64_t)A.cols[i].width + (c->d_valid ? (N + 7) / 8 : 0);
        }
        A.blk = d_blk;
        A.nb = (int32_t)blk.size();
        A.n_tiles = n_tiles;
        A.n_ops = P.n_ops;
        A.acc = d_acc + 3 * k;
        const size_t lds = (size_t)std::max(P.depth - 1, 1) * kCxRows * kCxThreads * sizeof(int64_t);

        // ---- range
        if ((rc = pool.event(&ev[4 * k], st))) return rc;
        launch_eval(false, 0, A, grid, lds, st);
        SYBL_HIP(hipGetLastError());
        if ((rc = pool.event(&ev[4 * k + 1], st))) return rc;
        long long got[3] = {0, 0, 0};
        SYBL_HIP(hipMemcpyAsync(got, d_acc + 3 * k, sizeof(got), hipMemcpyDeviceToHost, st));  // read back once
        SYBL_HIP(hipStreamSynchronize(st));
        const int64_t populated = got[2];
        const bool missing = populated < N;
        S->unpopulated += N - populated;
        S->range_bytes += src_bytes;
        if (o->compact_mode) fit_storage(n->canon(), populated > 0, populated > 0 ? got[0] : 0, populated > 0 ? got[1] : 0, &n->elem, &n->vbase);
        n->has_missing = missing;
        if ((rc = table_reserve(o, n, phys_out))) return rc;
        if (missing && (rc = valid_reserve(o, n, phys_out))) return rc;

        // ---- store
        A.out = n->d_data;
        A.out_valid = missing ? n->d_valid : nullptr;
        A.out_base = n->vbase;
        if ((rc = pool.event(&ev[4 * k + 2], st))) return rc;
        launch_eval(true, n->elem, A, grid, lds, st);
        SYBL_HIP(hipGetLastError());
        if ((rc = pool.event(&ev[4 * k + 3], st))) return rc;
        S->store_bytes += src_bytes + n_out * (int64_t)n->elem + (missing ? n_out / 8 : 0);
    }

    // ---- statistics
    if ((rc = pool.event(&ev[4 * ne], st))) return rc;
    // (the ONE wait for the statistics of every block of every computed column)
    if ((rc = derived_block_stats(o, att, o->d_blocks, nb_out, pool, "compute statistics", &ev[4 * ne + 1]))) return rc;
    o->version++;
    float f = 0;
    for (size_t k = 0; k < ne; k++) {
        SYBL_HIP(hipEventElapsedTime(&f, ev[4 * k], ev[4 * k + 1]));
        S->range_ms += f;
        SYBL_HIP(hipEventElapsedTime(&f, ev[4 * k + 2], ev[4 * k + 3]));
        S->store_ms += f;
    }
    SYBL_HIP(hipEventElapsedTime(&f, ev[4 * ne], ev[4 * ne + 1]));
    S->stats_ms = f;
    return SYBL_OK;
}

}  // namespace

int compute_run(Table *t, const sybl_compute_desc *d, sybl_table **out) {
    TableOwner O;  // (run makes the table: the copy of t)
    return derived_call(t->ctx, "sybl_table_compute", O, out, [&] { return run(t, d, O); });
}

}  // namespace sybl

using namespace sybl;

extern "C" {

int sybl_table_compute(sybl_table *t, const sybl_compute_desc *d, sybl_table **out) {
    SYBL_API_GUARD(t);
    if (out) *out = nullptr;
    if (!t || !d || !out || !d->exprs) return fail(SYBL_E_INVAL, "sybl_table_compute: NULL argument");
    return compute_run(t, d, out);
}

int sybl_table_compute_stats(const sybl_table *t, sybl_compute_stats *out) {
    SYBL_API_GUARD(t);
    if (!t || !out) return fail(SYBL_E_INVAL, "sybl_table_compute_stats: NULL argument");
    *out = t->compute_stats;
    return SYBL_OK;
}

const char *sybl_debug_compute_program(const char *expr, int32_t n_cols, const char *const *names, const int32_t *types) {
    static thread_local std::string text;
    if (!expr || n_cols < 0 || (n_cols > 0 && (!names || !types))) {
        set_error("sybl_debug_compute_program: NULL argument");
        return nullptr;
    }
    CxProgram P;
    CxParser parser(expr, strlen(expr), n_cols, names, types, &P);
    if (!parser.compile()) {
        set_error("sybl_debug_compute_program: %s", parser.error().c_str());
        return nullptr;
    }
    text = cx_program_text(P);
    return text.c_str();
}

int sybl_debug_compute_eval(const char *expr, int32_t n_cols, const char *const *names, const int32_t *types, const int64_t *values,
                            const uint8_t *populated, int64_t n_rows, int64_t *out, uint8_t *out_populated) {
    if (!expr || n_cols < 0 || n_rows < 0 || (n_cols > 0 && (!names || !types)) || (n_rows > 0 && (!out || !out_populated)) ||
        (n_cols > 0 && n_rows > 0 && (!values || !populated)))
        return fail(SYBL_E_INVAL, "sybl_debug_compute_eval: NULL argument");
    CxProgram P;
    CxParser parser(expr, strlen(expr), n_cols, names, types, &P);
    if (!parser.compile()) return fail(SYBL_E_INVAL, "sybl_debug_compute_eval: %s", parser.error().c_str());
    for (int64_t r = 0; r < n_rows; r++) {
        const CxVal v = cx_eval_row(P, [&](int slot) {
            const int64_t at = (int64_t)P.cols[slot] * n_rows + r;
            return CxVal{values[at], populated[at] != 0};
        });
        out[r] = v.v;
        out_populated[r] = v.p ? 1 : 0;
    }
    return SYBL_OK;
}

}  // extern "C"
