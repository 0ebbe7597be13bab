// compute_ops.h -- the ops of a compute expression (include/sybilgpu.h, "compute"): the op codes and ONE function per op that
// defines its arithmetic and its populated-bit rule.  Shared by the kernel (compute.hip: k_cx_eval) and the host evaluator
// (compute_expr.h), as hll.h is shared by the sketch kernel and its test hook.  Plain C++17 when compiled without HIP.
//
// Every value is a signed 64-bit integer with Go's semantics: + - * unary - and abs wrap mod 2^64, / truncates toward zero, % takes
// the dividend's sign, INT64_MIN / -1 == INT64_MIN and INT64_MIN % -1 == 0 (guarded: plain C++ is undefined there).  A value is
// populated or not; an unpopulated value is carried as 0, so host and device agree on every bit of a result.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CX_HD __host__ __device__ __forceinline__
#else
#define CX_HD inline
#endif

namespace sybl {

enum CxOpCode : uint8_t {
    kCxPushCol = 0,  // arg: column slot
    kCxPushConst,    // arg: index into the constant pool
    kCxHas,          // arg: column slot; pushes 1 / 0, always populated
    kCxNeg,          // unary
    kCxNot,
    kCxAbs,
    kCxMul,          // binary: a below b on the stack
    kCxDiv,
    kCxMod,
    kCxAdd,
    kCxSub,
    kCxLt,
    kCxLe,
    kCxGt,
    kCxGe,
    kCxEq,
    kCxNe,
    kCxAnd,
    kCxOr,
    kCxMin,
    kCxMax,
    kCxCoalesce,
    kCxIf,           // ternary: c, a, b
    kCxOpCount
};

constexpr int kCxMaxOps = 64;    // postfix ops per expression
constexpr int kCxMaxCols = 8;    // distinct columns per expression (the filters' limit)
constexpr int kCxMaxStack = 8;   // operand stack
constexpr int kCxMaxNest = 64;   // parentheses / calls

struct CxVal {
    int64_t v;
    bool p;  // populated
};

CX_HD CxVal cx_make(int64_t v, bool p) { return CxVal{p ? v : 0, p}; }
CX_HD int64_t cx_wrap_neg(int64_t a) { return (int64_t)(0 - (uint64_t)a); }

CX_HD CxVal cx_neg(CxVal a) { return cx_make(cx_wrap_neg(a.v), a.p); }
CX_HD CxVal cx_not(CxVal a) { return cx_make(a.v == 0, a.p); }
CX_HD CxVal cx_abs(CxVal a) { return cx_make(a.v < 0 ? cx_wrap_neg(a.v) : a.v, a.p); }
CX_HD CxVal cx_mul(CxVal a, CxVal b) { return cx_make((int64_t)((uint64_t)a.v * (uint64_t)b.v), a.p && b.p); }
CX_HD CxVal cx_add(CxVal a, CxVal b) { return cx_make((int64_t)((uint64_t)a.v + (uint64_t)b.v), a.p && b.p); }
CX_HD CxVal cx_sub(CxVal a, CxVal b) { return cx_make((int64_t)((uint64_t)a.v - (uint64_t)b.v), a.p && b.p); }
// a populated zero divisor: unpopulated (Go would panic); -1 is the one divisor C++ leaves undefined at INT64_MIN
CX_HD CxVal cx_div(CxVal a, CxVal b) {
    const bool p = a.p && b.p && b.v != 0;
    if (!p) return CxVal{0, false};
    return CxVal{b.v == -1 ? cx_wrap_neg(a.v) : a.v / b.v, true};
}
CX_HD CxVal cx_mod(CxVal a, CxVal b) {
    const bool p = a.p && b.p && b.v != 0;
    if (!p) return CxVal{0, false};
    return CxVal{b.v == -1 ? 0 : a.v % b.v, true};
}
CX_HD CxVal cx_lt(CxVal a, CxVal b) { return cx_make(a.v < b.v, a.p && b.p); }
CX_HD CxVal cx_le(CxVal a, CxVal b) { return cx_make(a.v <= b.v, a.p && b.p); }
CX_HD CxVal cx_gt(CxVal a, CxVal b) { return cx_make(a.v > b.v, a.p && b.p); }
CX_HD CxVal cx_ge(CxVal a, CxVal b) { return cx_make(a.v >= b.v, a.p && b.p); }
CX_HD CxVal cx_eq(CxVal a, CxVal b) { return cx_make(a.v == b.v, a.p && b.p); }
CX_HD CxVal cx_ne(CxVal a, CxVal b) { return cx_make(a.v != b.v, a.p && b.p); }
// both sides are always evaluated: nothing short-circuits
CX_HD CxVal cx_and(CxVal a, CxVal b) { return cx_make(a.v != 0 && b.v != 0, a.p && b.p); }
CX_HD CxVal cx_or(CxVal a, CxVal b) { return cx_make(a.v != 0 || b.v != 0, a.p && b.p); }
CX_HD CxVal cx_min(CxVal a, CxVal b) { return cx_make(a.v < b.v ? a.v : b.v, a.p && b.p); }
CX_HD CxVal cx_max(CxVal a, CxVal b) { return cx_make(a.v > b.v ? a.v : b.v, a.p && b.p); }
CX_HD CxVal cx_coalesce(CxVal a, CxVal b) { return a.p ? a : cx_make(b.v, b.p); }
// unpopulated where c is; elsewhere the value AND the populatedness of the chosen branch only
CX_HD CxVal cx_if(CxVal c, CxVal a, CxVal b) {
    if (!c.p) return CxVal{0, false};
    return c.v != 0 ? cx_make(a.v, a.p) : cx_make(b.v, b.p);
}
CX_HD CxVal cx_has(bool populated) { return CxVal{populated ? 1 : 0, true}; }

CX_HD int cx_arity(int op) { return op <= kCxHas ? 0 : op <= kCxAbs ? 1 : op == kCxIf ? 3 : 2; }

CX_HD CxVal cx_unary(int op, CxVal a) {
    switch (op) {
    case kCxNeg: return cx_neg(a);
    case kCxNot: return cx_not(a);
    default: return cx_abs(a);
    }
}

CX_HD CxVal cx_binary(int op, CxVal a, CxVal b) {
    switch (op) {
    case kCxMul: return cx_mul(a, b);
    case kCxDiv: return cx_div(a, b);
    case kCxMod: return cx_mod(a, b);
    case kCxAdd: return cx_add(a, b);
    case kCxSub: return cx_sub(a, b);
    case kCxLt: return cx_lt(a, b);
    case kCxLe: return cx_le(a, b);
    case kCxGt: return cx_gt(a, b);
    case kCxGe: return cx_ge(a, b);
    case kCxEq: return cx_eq(a, b);
    case kCxNe: return cx_ne(a, b);
    case kCxAnd: return cx_and(a, b);
    case kCxOr: return cx_or(a, b);
    case kCxMin: return cx_min(a, b);
    case kCxMax: return cx_max(a, b);
    default: return cx_coalesce(a, b);
    }
}

}  // namespace sybl
