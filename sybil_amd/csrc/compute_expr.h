// compute_expr.h -- a compute expression (include/sybilgpu.h, "compute") from text to a postfix program, and the row-wise host
// evaluator over the ops of compute_ops.h.  Plain C++17: it compiles with g++ alone (tests/compute_host_main.cpp holds it under
// the sanitizers), and nothing here touches the GPU.
//
//   program   <= kCxMaxOps ops {op, arg}, a constant pool, <= kCxMaxCols column slots (indices into the column list the expression
//             was compiled against).  The stack depth is checked while the ops are emitted: a compiled program never needs more
//             than kCxMaxStack operands, so the evaluators do not check it again.
//   parser    precedence climbing over the characters; unary operators are collected in a loop, parentheses and calls count
//             their nesting: hostile input hits kCxMaxNest or kCxMaxOps, never the C stack.
//   grammar   C precedence, binary operators left-associative:  ||  &&  == !=  < <= > >=  + -  * / %  unary - !
//             primary: literal | column | `any name` | ( expr ) | min(a,b) max(a,b) abs(a) if(c,a,b) coalesce(a,b) has(column)
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "compute_ops.h"

namespace sybl {

enum { kCxTypeInt = 1, kCxTypeStr = 2, kCxTypeSet = 3 };  // SYBL_INT_VAL, SYBL_STR_VAL, SYBL_SET_VAL

struct CxProgram {
    int n_ops = 0;
    uint8_t op[kCxMaxOps] = {};
    uint8_t arg[kCxMaxOps] = {};
    int n_consts = 0;
    int64_t consts[kCxMaxOps] = {};
    int n_cols = 0;
    int32_t cols[kCxMaxCols] = {};  // slot -> index into the column list
    int depth = 0;                  // the deepest the operand stack gets
};

inline const char *cx_op_name(int op) {
    static const char *const names[kCxOpCount] = {"col", "const", "has", "neg", "not", "abs", "mul", "div", "mod", "add", "sub", "lt",
                                                  "le",  "gt",    "ge",  "eq",  "ne",  "and", "or",  "min", "max", "coalesce", "if"};
    return op >= 0 && op < kCxOpCount ? names[op] : "?";
}

// "c0 c1 sub 1000 div": c<slot>, has(c<slot>), constants by value, ops by name
inline std::string cx_program_text(const CxProgram &P) {
    std::string o;
    for (int i = 0; i < P.n_ops; i++) {
        if (i) o += ' ';
        if (P.op[i] == kCxPushCol) o += "c" + std::to_string((int)P.arg[i]);
        else if (P.op[i] == kCxHas) o += "has(c" + std::to_string((int)P.arg[i]) + ")";
        else if (P.op[i] == kCxPushConst) o += std::to_string((long long)P.consts[P.arg[i]]);
        else o += cx_op_name(P.op[i]);
    }
    return o;
}

class CxParser {
public:
    CxParser(const char *text, size_t len, int32_t n_cols, const char *const *names, const int32_t *types, CxProgram *out)
        : s_(text), n_(len), n_cols_(n_cols), names_(names), types_(types), P_(out) {}

    // false: error() says why (with the byte offset where the text is at fault)
    bool compile() {
        *P_ = CxProgram{};
        if (!expr(1)) return false;
        ws();
        if (i_ < n_) return fail(i_, "unexpected character");
        return true;
    }
    const std::string &error() const { return err_; }

private:
    const char *s_;
    size_t n_, i_ = 0;
    int32_t n_cols_;
    const char *const *names_;
    const int32_t *types_;
    CxProgram *P_;
    std::string err_;
    int nest_ = 0, sp_ = 0;

    bool fail(size_t at, const std::string &what) {
        if (err_.empty()) err_ = what + " at byte " + std::to_string(at);
        return false;
    }
    void ws() {
        while (i_ < n_ && (s_[i_] == ' ' || s_[i_] == '\t' || s_[i_] == '\n' || s_[i_] == '\r')) i_++;
    }
    static bool ident_start(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_'; }
    static bool digit(char c) { return c >= '0' && c <= '9'; }

    bool emit(int op, int arg, size_t at) {
        if (P_->n_ops >= kCxMaxOps) return fail(at, "more than 64 ops");
        sp_ += 1 - cx_arity(op);
        if (sp_ > kCxMaxStack) return fail(at, "operand stack deeper than 8");
        if (sp_ > P_->depth) P_->depth = sp_;
        P_->op[P_->n_ops] = (uint8_t)op;
        P_->arg[P_->n_ops] = (uint8_t)arg;
        P_->n_ops++;
        return true;
    }
    bool enter(size_t at) {
        if (++nest_ > kCxMaxNest) return fail(at, "nested deeper than 64");
        return true;
    }

    // the binary operator at i_: its op, precedence and length (0: none)
    int binop(int *op, int *prec) const {
        const char c = i_ < n_ ? s_[i_] : 0, d = i_ + 1 < n_ ? s_[i_ + 1] : 0;
        switch (c) {
        case '|': if (d == '|') { *op = kCxOr; *prec = 1; return 2; } return 0;
        case '&': if (d == '&') { *op = kCxAnd; *prec = 2; return 2; } return 0;
        case '=': if (d == '=') { *op = kCxEq; *prec = 3; return 2; } return 0;
        case '!': if (d == '=') { *op = kCxNe; *prec = 3; return 2; } return 0;
        case '<': *prec = 4; if (d == '=') { *op = kCxLe; return 2; } *op = kCxLt; return 1;
        case '>': *prec = 4; if (d == '=') { *op = kCxGe; return 2; } *op = kCxGt; return 1;
        case '+': *op = kCxAdd; *prec = 5; return 1;
        case '-': *op = kCxSub; *prec = 5; return 1;
        case '*': *op = kCxMul; *prec = 6; return 1;
        case '/': *op = kCxDiv; *prec = 6; return 1;
        case '%': *op = kCxMod; *prec = 6; return 1;
        default: return 0;
        }
    }

    bool expr(int min_prec) {
        if (!unary()) return false;
        for (;;) {
            ws();
            int op = 0, prec = 0;
            const int len = binop(&op, &prec);
            if (!len || prec < min_prec) return true;
            const size_t at = i_;
            i_ += (size_t)len;
            if (!expr(prec + 1)) return false;
            if (!emit(op, 0, at)) return false;
        }
    }

    bool unary() {
        uint8_t pre[kCxMaxOps];
        size_t at[kCxMaxOps];
        int n = 0;
        for (;;) {
            ws();
            if (i_ < n_ && (s_[i_] == '-' || (s_[i_] == '!' && !(i_ + 1 < n_ && s_[i_ + 1] == '=')))) {
                if (n >= kCxMaxOps) return fail(i_, "more than 64 ops");
                pre[n] = s_[i_] == '-' ? kCxNeg : kCxNot;
                at[n++] = i_++;
            } else {
                break;
            }
        }
        if (!primary()) return false;
        while (n > 0) {
            n--;
            if (!emit(pre[n], 0, at[n])) return false;
        }
        return true;
    }

    // a column name at i_ (plain or between backticks) -> [*b, *e); false and an error otherwise
    bool name_at(size_t *b, size_t *e) {
        if (i_ < n_ && s_[i_] == '`') {
            const size_t open = i_++;
            *b = i_;
            while (i_ < n_ && s_[i_] != '`') i_++;
            if (i_ >= n_) return fail(open, "unterminated backtick");
            *e = i_++;
            if (*e == *b) return fail(open, "empty column name");
            return true;
        }
        if (i_ < n_ && ident_start(s_[i_])) {
            *b = i_;
            while (i_ < n_ && (ident_start(s_[i_]) || digit(s_[i_]))) i_++;
            *e = i_;
            return true;
        }
        return fail(i_, "a column name is expected");
    }

    // the slot of column [b, e); value: it is read as a value (INT only)
    bool column(size_t b, size_t e, bool value, int *slot) {
        const std::string nm(s_ + b, e - b);
        int ix = -1;
        for (int32_t k = 0; k < n_cols_; k++)
            if (names_[k] && nm == names_[k]) {
                ix = k;
                break;
            }
        if (ix < 0) return fail(b, "unknown column '" + nm + "'");
        if (value && types_[ix] != kCxTypeInt)
            return fail(b, "column '" + nm + "' is a " + (types_[ix] == kCxTypeStr ? "str" : "set") + " column: only has() takes one");
        for (int k = 0; k < P_->n_cols; k++)
            if (P_->cols[k] == ix) {
                *slot = k;
                return true;
            }
        if (P_->n_cols >= kCxMaxCols) return fail(b, "more than 8 distinct columns");
        P_->cols[P_->n_cols] = ix;
        *slot = P_->n_cols++;
        return true;
    }

    bool primary() {
        ws();
        if (i_ >= n_) return fail(i_, "unexpected end of the expression");
        const size_t at = i_;
        const char c = s_[i_];
        if (digit(c)) {
            uint64_t v = 0;
            while (i_ < n_ && digit(s_[i_])) {
                const uint64_t d = (uint64_t)(s_[i_] - '0');
                if (v > 922337203685477580ull || v * 10 + d > ((uint64_t)1 << 63)) return fail(at, "literal above 2^63");
                v = v * 10 + d;
                i_++;
            }
            if (i_ < n_ && ident_start(s_[i_])) return fail(i_, "unexpected character");
            if (P_->n_consts >= kCxMaxOps) return fail(at, "more than 64 ops");
            P_->consts[P_->n_consts] = (int64_t)v;  // 2^63 wraps to INT64_MIN: -9223372036854775808 can be written
            return emit(kCxPushConst, P_->n_consts++, at);
        }
        if (c == '(') {
            if (!enter(at)) return false;
            i_++;
            if (!expr(1)) return false;
            ws();
            if (i_ >= n_ || s_[i_] != ')') return fail(i_, "')' is expected");
            i_++;
            nest_--;
            return true;
        }
        if (c == '`') {
            size_t b, e;
            int slot;
            if (!name_at(&b, &e) || !column(b, e, true, &slot)) return false;
            return emit(kCxPushCol, slot, at);
        }
        if (ident_start(c)) {
            size_t b, e;
            if (!name_at(&b, &e)) return false;
            const size_t after = i_;
            ws();
            if (i_ < n_ && s_[i_] == '(') return call(b, e);
            i_ = after;
            int slot;
            if (!column(b, e, true, &slot)) return false;
            return emit(kCxPushCol, slot, at);
        }
        return fail(at, "unexpected character");
    }

    // a call: i_ is at its '('
    bool call(size_t b, size_t e) {
        const std::string fn(s_ + b, e - b);
        if (!enter(b)) return false;
        i_++;
        if (fn == "has") {
            ws();
            if (i_ < n_ && s_[i_] == ')') return fail(i_, "wrong argument count: has() takes 1");
            size_t cb, ce;
            int slot;
            if (!name_at(&cb, &ce) || !column(cb, ce, false, &slot)) return false;
            ws();
            if (i_ >= n_ || s_[i_] != ')') return fail(i_, "has() takes one column name");
            i_++;
            nest_--;
            return emit(kCxHas, slot, b);
        }
        int op, want;
        if (fn == "min") op = kCxMin, want = 2;
        else if (fn == "max") op = kCxMax, want = 2;
        else if (fn == "abs") op = kCxAbs, want = 1;
        else if (fn == "if") op = kCxIf, want = 3;
        else if (fn == "coalesce") op = kCxCoalesce, want = 2;
        else return fail(b, "unknown function '" + fn + "'");
        int got = 0;
        ws();
        if (!(i_ < n_ && s_[i_] == ')')) {
            for (;;) {
                if (got == want) return fail(i_, "wrong argument count: " + fn + "() takes " + std::to_string(want));
                if (!expr(1)) return false;
                got++;
                ws();
                if (i_ < n_ && s_[i_] == ',') {
                    i_++;
                    continue;
                }
                break;
            }
        }
        if (i_ >= n_ || s_[i_] != ')') return fail(i_, "')' is expected");
        if (got != want) return fail(i_, "wrong argument count: " + fn + "() takes " + std::to_string(want));
        i_++;
        nest_--;
        return emit(op, 0, b);
    }
};

// One row: get(slot) is the column's value at the row (CxVal; only .p is read by has()).
template <class Get>
inline CxVal cx_eval_row(const CxProgram &P, Get get) {
    CxVal st[kCxMaxStack + 1];
    int sp = 0;
    for (int i = 0; i < P.n_ops; i++) {
        const int op = P.op[i];
        switch (cx_arity(op)) {
        case 0:
            if (op == kCxPushCol) {
                const CxVal c = get((int)P.arg[i]);
                st[sp++] = cx_make(c.v, c.p);
            } else if (op == kCxHas) {
                st[sp++] = cx_has(get((int)P.arg[i]).p);
            } else {
                st[sp++] = CxVal{P.consts[P.arg[i]], true};
            }
            break;
        case 1: st[sp - 1] = cx_unary(op, st[sp - 1]); break;
        case 2:
            st[sp - 2] = cx_binary(op, st[sp - 2], st[sp - 1]);
            sp--;
            break;
        default:
            st[sp - 3] = cx_if(st[sp - 3], st[sp - 2], st[sp - 1]);
            sp -= 2;
            break;
        }
    }
    return sp == 1 ? st[0] : CxVal{0, false};
}

}  // namespace sybl
