// compute_host_main.cpp -- the parser and the host evaluator of compute expressions (sybil_amd/csrc/compute_expr.h,
// compute_ops.h) as a program of their own, for tests/test_compute_host.py to build with AddressSanitizer and
// UndefinedBehaviorSanitizer and run as a child process.  Everything here must be refused or evaluated without a report:
//   the known answers of the contract; every prefix and every one-byte deletion of a set of valid expressions; 1e5 seeded random
//   strings over the grammar's alphabet; 10 000 nested parentheses, minus signs and min( calls.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "compute_expr.h"

using namespace sybl;

static const char *const kNames[] = {"a", "b", "min", "a.b", "s", "tags", "c", "d", "e", "f", "g", "h", "x"};
static const int32_t kTypes[] = {1, 1, 1, 1, 2, 3, 1, 1, 1, 1, 1, 1, 1};
static const int kCols = 13;
static const int64_t kVals[] = {0, 1, -1, 2, -2, INT64_MIN, INT64_MAX, 7, -1000, 86400};
static const int kNVals = 10;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// compiles; when it compiles, evaluates it over rows that put every edge value into every column.  Returns whether it compiled.
static bool exercise(const std::string &text, uint64_t *sink) {
    CxProgram P;
    CxParser parser(text.data(), text.size(), kCols, kNames, kTypes, &P);
    if (!parser.compile()) {
        if (parser.error().empty()) {
            printf("refused without a message: %s\n", text.c_str());
            exit(1);
        }
        return false;
    }
    if (P.n_ops < 1 || P.n_ops > kCxMaxOps || P.depth < 1 || P.depth > kCxMaxStack || P.n_cols > kCxMaxCols) {
        printf("a program outside the limits: %s\n", text.c_str());
        exit(1);
    }
    for (int r = 0; r < kNVals * 3; r++) {
        const CxVal v = cx_eval_row(P, [&](int slot) { return CxVal{kVals[(r + 3 * slot) % kNVals], (r + slot) % 5 != 0}; });
        *sink += (uint64_t)v.v + (v.p ? 1 : 0);
        if (!v.p && v.v != 0) {
            printf("an unpopulated result that is not 0: %s\n", text.c_str());
            exit(1);
        }
    }
    return true;
}

struct Known {
    const char *expr;
    int64_t want;
    bool populated;
};

int main() {
    uint64_t sink = 0;
    const Known known[] = {
        {"7 / -2", -3, true}, {"-7 / 2", -3, true}, {"-7 % 2", -1, true}, {"7 % -2", 1, true}, {"2 - 3 - 4", -5, true},
        {"100 / 10 / 5", 2, true}, {"1 + 2 * 3 == 7 && !0", 1, true}, {"1 < 2 == 1", 1, true}, {"- - 3", 3, true},
        {"9223372036854775807 + 1", INT64_MIN, true}, {"-9223372036854775808 / -1", INT64_MIN, true},
        {"-9223372036854775808 % -1", 0, true}, {"abs(-9223372036854775808)", INT64_MIN, true},
        {"3037000500 * 3037000500", -9223372036709301616ll, true}, {"1 / 0", 0, false}, {"if(0, 1/0, 5)", 5, true},
        {"if(1/0, 1, 2)", 0, false}, {"coalesce(1/0, 9)", 9, true}, {"0 && 1/0", 0, false}, {"1 % 0", 0, false},
        {"-9223372036854775807 - 2", INT64_MAX, true}, {"9223372036854775807 * 9223372036854775807", 1, true},
        {"-(-9223372036854775808)", INT64_MIN, true}, {"min(3, -4) + max(3, -4)", -1, true},
    };
    for (const Known &k : known) {
        CxProgram P;
        CxParser parser(k.expr, strlen(k.expr), 0, nullptr, nullptr, &P);
        if (!parser.compile()) {
            printf("refused: %s: %s\n", k.expr, parser.error().c_str());
            return 1;
        }
        const CxVal v = cx_eval_row(P, [](int) { return CxVal{0, false}; });
        if (v.p != k.populated || v.v != k.want) {
            printf("%s = %lld (populated %d), expected %lld (%d)\n", k.expr, (long long)v.v, (int)v.p, (long long)k.want, (int)k.populated);
            return 1;
        }
    }
    printf("known answers ok\n");

    const char *const valid[] = {
        "a - b", "(a - b) / 1000", "x % 86400 / 3600", "if(a >= 500, 1, 0)", "coalesce(`a.b`, 0)", "min + min(min, 1)", "has(s) + has(tags)",
        "a+b+c+d+e+f+g+h", "-a * !b || a && b == c != d < e <= f > g >= h", "abs(max(a, -9223372036854775808)) % -1",
        "if(has(`a.b`), a / b, a % b) + 9223372036854775807", " a\t+\n( b ) ",
    };
    long compiled = 0;
    for (const char *v : valid) {
        const std::string s(v);
        if (!exercise(s, &sink)) {
            printf("a valid expression was refused: %s\n", v);
            return 1;
        }
        for (size_t n = 0; n <= s.size(); n++) compiled += exercise(s.substr(0, n), &sink);
        for (size_t n = 0; n < s.size(); n++) compiled += exercise(s.substr(0, n) + s.substr(n + 1), &sink);
    }
    printf("prefixes and deletions ok\n");

    const char *const atoms[] = {"a", "b", "min", "max", "abs", "if", "coalesce", "has", "`a.b`", "s", "tags", "x", "0", "1", "7", "86400",
                                 "9223372036854775807", "9223372036854775808", "9223372036854775809", "(", ")", ",", "-", "!", "*", "/",
                                 "%", "+", "<", "<=", ">", ">=", "==", "!=", "&&", "||", " ", "`", "=", "&", "|", "q", "(", ")", "(", ")"};
    const int n_atoms = (int)(sizeof(atoms) / sizeof(atoms[0]));
    for (int i = 0; i < 100000; i++) {
        std::string s;
        const int len = 1 + (int)(rnd() % 24);
        for (int k = 0; k < len; k++) s += atoms[rnd() % (uint64_t)n_atoms];
        compiled += exercise(s, &sink);
    }
    printf("random strings ok\n");

    const char *const units[] = {"(", "-", "min(", "!", "abs(", "if(", "`", "((a)+"};
    for (const char *u : units) {
        std::string s;
        for (int i = 0; i < 10000; i++) s += u;
        if (exercise(s + "1", &sink) || exercise(s, &sink)) {
            printf("10000 x '%s' was accepted\n", u);
            return 1;
        }
    }
    std::string closed(10000, '(');
    closed += "1";
    closed += std::string(10000, ')');
    if (exercise(closed, &sink)) {
        printf("10000 closed parentheses were accepted\n");
        return 1;
    }
    printf("deep nesting ok\n");
    printf("%ld compiled, checksum %llu\n", compiled, (unsigned long long)sink);
    return 0;
}
