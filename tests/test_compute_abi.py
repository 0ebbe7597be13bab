"""CPU-side checks of the compute part of the C ABI (include/sybilgpu.h, "compute"): the symbols, the mirrors, the example, and
the parser and host evaluator behind the two debug hooks against the restatement in tests/compute_ref.py.  Table.compute itself
needs a GPU: tests/test_gpu_compute.py."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from tests import compute_ref as R
from tests.test_compute_ref import KNOWN, UNPOP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = R.I64_MIN, R.I64_MAX
TYPE_ID = {"int": 1, "str": 2, "set": 3}


def _cols(types):
    from sybil_amd import _native as N
    names = [n.encode() for n in types]
    narr = (ctypes.c_char_p * max(len(names), 1))(*names)
    tarr = (ctypes.c_int32 * max(len(names), 1))(*[TYPE_ID[t] for t in types.values()])
    return N.lib(), len(names), narr, tarr


def program(expr, types):
    """The library's postfix text, or None and the error message."""
    lib, n, narr, tarr = _cols(types)
    got = lib.sybl_debug_compute_program(expr.encode(), n, narr, tarr)
    return (got.decode(), None) if got is not None else (None, lib.sybl_last_error().decode())


def evaluate(expr, types, values, populated):
    """values / populated: [n_cols][n_rows] in the order of `types`.  Returns (rc, values, populated)."""
    lib, n, narr, tarr = _cols(types)
    v = np.ascontiguousarray(values, dtype=np.int64).reshape(n, -1) if n else np.zeros((0, 1), dtype=np.int64)
    p = np.ascontiguousarray(populated, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 1), dtype=np.uint8)
    rows = v.shape[1]
    out, outp = np.full(rows, 99, dtype=np.int64), np.full(rows, 99, dtype=np.uint8)
    rc = lib.sybl_debug_compute_eval(expr.encode(), n, narr, tarr, v.ctypes.data, p.ctypes.data, rows, out.ctypes.data, outp.ctypes.data)
    return rc, out.tolist(), [bool(x) for x in outp.tolist()]


def test_compute_entry_points_are_exported_and_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_compute", "sybl_table_compute_stats", "sybl_debug_compute_program", "sybl_debug_compute_eval"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move
    import sybil_amd.engine as E
    assert callable(E.Table.compute) and callable(E.Table.compute_stats)


def test_header_compiles_as_c99_and_the_mirrors_have_their_layout(tmp_path):
    from sybil_amd import _native as N
    mirrors = [("sybl_compute_col", N.ComputeCol), ("sybl_compute_desc", N.ComputeDesc), ("sybl_compute_stats", N.ComputeStats)]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){
  int (*f)(sybl_table *, const sybl_compute_desc *, sybl_table **) = sybl_table_compute; (void)f;
  int (*g)(const sybl_table *, sybl_compute_stats *) = sybl_table_compute_stats; (void)g;
  const char *(*h)(const char *, int32_t, const char *const *, const int32_t *) = sybl_debug_compute_program; (void)h;
''' + "".join('  printf("%%zu ", sizeof(%s));\n' % c for c, _ in mirrors) \
        + "".join('  printf("%%zu ", offsetof(%s, %s));\n' % (c, f) for c, m in mirrors for f, _ in m._fields_) + '  printf("\\n");\n  return 0; }\n'
    (tmp_path / "s.c").write_text(prog)
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert [len(m._fields_) for _, m in mirrors] == [2, 2, 10]
    assert out == [ctypes.sizeof(m) for _, m in mirrors] + [getattr(m, f).offset for _, m in mirrors for f, _ in m._fields_]


def test_null_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p(1234)
    d = N.ComputeDesc()
    assert lib.sybl_table_compute(None, ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL
    assert lib.sybl_last_error().startswith(b"sybl_table_compute: NULL")
    assert h.value is None                                   # *out is NULL after a failure
    assert lib.sybl_table_compute(None, None, None) == N.E_INVAL
    assert lib.sybl_table_compute(None, None, ctypes.byref(h)) == N.E_INVAL
    assert lib.sybl_table_compute_stats(None, None) == N.E_INVAL
    assert lib.sybl_last_error().startswith(b"sybl_table_compute_stats: NULL")
    st = N.ComputeStats()
    assert lib.sybl_table_compute_stats(None, ctypes.byref(st)) == N.E_INVAL
    assert lib.sybl_debug_compute_program(None, 0, None, None) is None
    assert lib.sybl_debug_compute_eval(None, 0, None, None, None, None, 0, None, None) == N.E_INVAL


def test_c_compute_example_links_against_the_library(tmp_path):
    """tools/example_compute.c: a table -> compute -> stats -> a query grouped by a computed column -> free from C99, linked
    against the in-tree library."""
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_compute.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_compute")])


TYPES = {"a": "int", "b": "int", "min": "int", "a.b": "int", "s": "str", "tags": "set", "c": "int", "d": "int", "e": "int", "f": "int",
         "g": "int", "h": "int"}


@pytest.mark.parametrize("expr", [
    "a - b / 1000", "(a - b) / 1000", "a - b - c", "a / b / c", "a % b * c", "1 + 2 * 3 == 7 && !0", "1 < 2 == 1", "- - 3", "-a * !b",
    "a < b == b >= a && a || has(b)", "a || b && c", "(a || b) && c", "a == b != c", "a <= b > c", "a + b < c - d", "!a == b",
    "if(a, min(a, b), coalesce(b, 1))", "min + min(min, 1)", "`a.b` + 1", "has(s) + has(tags) + has(`a.b`)", "abs(-a)", "max (a, b)",
    "-9223372036854775808", " a\t+\n b ", "a+b+c+d+e+f+g+h",
])
def test_the_program_is_the_restatements(expr):
    got, err = program(expr, TYPES)
    assert err is None and got == R.text(R.compile_expr(expr, TYPES)[0])


def test_program_text_of_the_precedence_cases():
    assert program("end - start", {"start": "int", "end": "int"})[0] == "c0 c1 sub"
    assert program("(a - b) / 1000", TYPES)[0] == "c0 c1 sub 1000 div"
    assert program("2 - 3 - 4", {})[0] == "2 3 sub 4 sub"
    assert program("1 + 2 * 3 == 7 && !0", {})[0] == "1 2 3 mul add 7 eq 0 not and"
    assert program("x % 86400 / 3600", {"x": "int"})[0] == "c0 86400 mod 3600 div"


@pytest.mark.parametrize("expr,want", KNOWN)
def test_known_answers_on_the_host_evaluator(expr, want):
    rc, v, p = evaluate(expr, {}, [], [])
    assert rc == 0 and (v[0] if p[0] else UNPOP) == want
    if not p[0]:
        assert v[0] == 0                                     # an unpopulated result is carried as 0


def test_has_and_names_on_the_host_evaluator():
    types = {"x": "int", "a.b": "int", "min": "int", "s": "str", "tags": "set"}
    vals, pops = [[77], [41], [10], [0], [0]], [[0], [1], [1], [1], [0]]
    for expr, want in (("has(x)", 0), ("x + 1", UNPOP), ("`a.b` + 1", 42), ("min + min(min, 1)", 11), ("has(s) + has(tags) * 2 + has(`a.b`) * 4", 5),
                       ("coalesce(x, 0 - 1)", -1)):
        rc, v, p = evaluate(expr, types, vals, pops)
        assert rc == 0 and (v[0] if p[0] else UNPOP) == want, expr


def _gen(rng, cols, depth):
    k = rng.random()
    if depth <= 0 or k < 0.25:
        if rng.random() < 0.5:
            return str(rng.choice([0, 1, 2, 3, 7, 1000, 86400, 9223372036854775807, 9223372036854775808, rng.randrange(1 << 40)]))
        c = rng.choice(cols)
        return "`%s`" % c if "." in c or rng.random() < 0.1 else c
    if k < 0.35:
        return rng.choice(["-", "!", "- ", "!!"]) + _gen(rng, cols, depth - 1)
    if k < 0.75:
        op = rng.choice(["*", "/", "%", "+", "-", "<", "<=", ">", ">=", "==", "!=", "&&", "||"])
        return "%s %s %s" % (_gen(rng, cols, depth - 1), op, _gen(rng, cols, depth - 1))
    if k < 0.83:
        return "(" + _gen(rng, cols, depth - 1) + ")"
    if k < 0.87:
        return "has(%s)" % rng.choice(cols + ["s", "tags"])
    fn = rng.choice(["min", "max", "abs", "if", "coalesce"])
    return "%s(%s)" % (fn, ", ".join(_gen(rng, cols, depth - 1) for _ in range(R.FUNCS[fn])))


def test_200_random_expressions_agree_with_the_restatement():
    rng = random.Random(20240607)
    types = {"a": "int", "b": "int", "a.b": "int", "min": "int", "e": "int", "s": "str", "tags": "set"}
    ints = [c for c, t in types.items() if t == "int"]
    rows = 24
    done = 0
    while done < 200:
        expr = _gen(rng, ints, rng.randrange(1, 6))
        try:
            R.compile_expr(expr, types)
        except R.ComputeError:
            continue                                         # (outside the limits: a deeper stack, more ops)
        pool = [0, 1, -1, 2, -2, I64_MIN, I64_MAX] + [rng.randrange(-1000, 1000) for _ in range(4)]
        vals = [[rng.choice(pool) for _ in range(rows)] for _ in types]
        pops = [[rng.random() < 0.8 for _ in range(rows)] for _ in types]
        want_v, want_p = R.evaluate(expr, types, {c: (vals[i], pops[i]) for i, c in enumerate(types)}, rows)
        rc, v, p = evaluate(expr, types, vals, pops)
        assert rc == 0 and p == want_p and v == want_v, expr
        assert program(expr, types)[0] == R.text(R.compile_expr(expr, types)[0]), expr
        done += 1


@pytest.mark.parametrize("expr,why", [
    ("nope + 1", "unknown column 'nope'"), ("s + 1", "str column"), ("tags", "set column"), ("1 +", "at byte 3"), ("(1", "at byte"),
    ("1)", "at byte 1"), ("", "at byte 0"), ("1 2", "at byte 2"), ("1 & 2", "at byte 2"), ("1 = 2", "at byte"), ("`a", "backtick"),
    ("``", "empty"), ("2x", "at byte 1"), ("1 << 2", "at byte"), ("~1", "at byte 0"), ("1.5", "at byte 1"), ("has(1)", "column name"),
    ("has()", "argument count"), ("has(a, b)", "has()"), ("min(1)", "argument count"), ("min(1, 2, 3)", "argument count"),
    ("abs()", "argument count"), ("if(1, 2)", "argument count"), ("foo(1)", "unknown function 'foo'"),
    ("9223372036854775809", "literal above 2^63"), ("99999999999999999999999999", "literal above 2^63"),
    ("a+b+c+d+e+f+g+h+min", "8 distinct columns"), ("+".join(["1"] * 33), "64 ops"), ("-" * 10000 + "1", "64 ops"),
    ("1+(1+(1+(1+(1+(1+(1+(1+(1" + ")" * 8, "stack deeper than 8"), ("(" * 65 + "1" + ")" * 65, "nested deeper than 64"),
    ("(" * 10000 + "1", "nested deeper than 64"), ("min(" * 10000, "nested deeper than 64"),
])
def test_refusals_through_the_debug_hooks(expr, why):
    from sybil_amd import _native as N
    got, err = program(expr, TYPES)
    assert got is None and err.startswith("sybl_debug_compute_program: ") and why in err, err
    rc, _, _ = evaluate(expr, TYPES, np.zeros((len(TYPES), 1)), np.ones((len(TYPES), 1)))
    assert rc == N.E_INVAL
    with pytest.raises(R.ComputeError):
        R.compile_expr(expr, TYPES)


def test_the_limits_themselves_are_accepted():
    for expr in ("+".join(["1"] * 32), "-(" + "+".join(["1"] * 32) + ")", "1+(1+(1+(1+(1+(1+(1+(1" + ")" * 7, "(" * 64 + "1" + ")" * 64,
                 "a+b+c+d+e+f+g+h"):
        got, err = program(expr, TYPES)
        assert err is None and got == R.text(R.compile_expr(expr, TYPES)[0])
