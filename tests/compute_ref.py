"""Python restatement of table compute (Table.compute / sybl_table_compute), written from the definition in include/sybilgpu.h
("compute") and not from the library: the checker of tests/test_gpu_compute.py and tests/test_compute_abi.py, itself checked by
tests/test_compute_ref.py.  It has its own parser; values are Python integers wrapped to int64.

A table is a list of blocks in the form tests/digest_ref.py uses.  compile_expr gives the postfix program as a list of
(op, arg) -- ("col", slot), ("has", slot), ("const", value), (name, None) -- and text() writes it the way
sybl_debug_compute_program does ("c0 c1 sub 1000 div")."""
import re

import numpy as np

from tests import digest_ref as D

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_OPS, MAX_COLS, MAX_STACK, MAX_NEST = 64, 8, 8, 64
FUNCS = {"min": 2, "max": 2, "abs": 1, "if": 3, "coalesce": 2, "has": 1}
BINARY = [("||", "or", 1), ("&&", "and", 2), ("==", "eq", 3), ("!=", "ne", 3), ("<=", "le", 4), (">=", "ge", 4), ("<", "lt", 4),
          (">", "gt", 4), ("+", "add", 5), ("-", "sub", 5), ("*", "mul", 6), ("/", "div", 6), ("%", "mod", 6)]
ARITY = {"col": 0, "has": 0, "const": 0, "neg": 1, "not": 1, "abs": 1, "if": 3}
_TOKEN = re.compile(r"[ \t\r\n]*(?:(\d+)|([A-Za-z_][A-Za-z0-9_]*)|`([^`]*)`|(\|\||&&|==|!=|<=|>=|[-+*/%<>!(),]))")


class ComputeError(ValueError):
    pass


def wrap(x):
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def _tokens(expr):
    out, i = [], 0
    while True:
        m = _TOKEN.match(expr, i)
        if not m:
            if expr[i:].strip(" \t\r\n") == "":
                return out
            raise ComputeError("syntax error at byte %d" % (len(expr) - len(expr[i:].lstrip(" \t\r\n"))))
        at = m.end() - len(m.group(m.lastindex))
        if m.group(1) is not None:
            if m.end() < len(expr) and re.match(r"[A-Za-z_]", expr[m.end()]):
                raise ComputeError("syntax error at byte %d" % m.end())
            out.append(("num", int(m.group(1)), at))
        elif m.group(2) is not None:
            out.append(("name", m.group(2), at))
        elif m.group(3) is not None:
            if m.group(3) == "":
                raise ComputeError("empty column name at byte %d" % (at - 1))
            out.append(("quoted", m.group(3), at - 1))
        else:
            out.append(("op", m.group(4), at))
        i = m.end()


class _Parser:
    def __init__(self, expr, types):
        self.toks, self.i, self.types = _tokens(expr), 0, types
        self.prog, self.cols, self.sp, self.depth, self.nest = [], [], 0, 0, 0

    def peek(self, kind=None, val=None):
        if self.i >= len(self.toks):
            return False
        k, v, _ = self.toks[self.i]
        return (kind is None or k == kind) and (val is None or v == val)

    def emit(self, op, arg=None):
        if len(self.prog) >= MAX_OPS:
            raise ComputeError("more than 64 ops")
        self.sp += 1 - ARITY.get(op, 2)
        if self.sp > MAX_STACK:
            raise ComputeError("operand stack deeper than 8")
        self.depth = max(self.depth, self.sp)
        self.prog.append((op, arg))

    def enter(self):
        self.nest += 1
        if self.nest > MAX_NEST:
            raise ComputeError("nested deeper than 64")

    def slot(self, name, value):
        if name not in self.types:
            raise ComputeError("unknown column '%s'" % name)
        if value and self.types[name] != "int":
            raise ComputeError("column '%s' is a %s column" % (name, self.types[name]))
        if name not in self.cols:
            if len(self.cols) >= MAX_COLS:
                raise ComputeError("more than 8 distinct columns")
            self.cols.append(name)
        return self.cols.index(name)

    def expect(self, val):
        if not self.peek("op", val):
            raise ComputeError("'%s' is expected" % val)
        self.i += 1

    def expr(self, min_prec=1):
        self.unary()
        while self.peek("op"):
            sym = self.toks[self.i][1]
            hit = [(name, prec) for s, name, prec in BINARY if s == sym]
            if not hit or hit[0][1] < min_prec:
                return
            self.i += 1
            self.expr(hit[0][1] + 1)
            self.emit(hit[0][0])

    def unary(self):
        pre = []
        while self.peek("op", "-") or self.peek("op", "!"):
            if len(pre) >= MAX_OPS:
                raise ComputeError("more than 64 ops")
            pre.append("neg" if self.toks[self.i][1] == "-" else "not")
            self.i += 1
        self.primary()
        for op in reversed(pre):
            self.emit(op)

    def primary(self):
        if self.i >= len(self.toks):
            raise ComputeError("unexpected end of the expression")
        kind, val, _ = self.toks[self.i]
        if kind == "num":
            if val > 1 << 63:
                raise ComputeError("literal above 2^63")
            self.i += 1
            self.emit("const", wrap(val))
        elif kind == "quoted":
            self.i += 1
            self.emit("col", self.slot(val, True))
        elif kind == "name":
            self.i += 1
            if self.peek("op", "("):
                self.call(val)
            else:
                self.emit("col", self.slot(val, True))
        elif kind == "op" and val == "(":
            self.enter()
            self.i += 1
            self.expr()
            self.expect(")")
            self.nest -= 1
        else:
            raise ComputeError("syntax error")

    def call(self, fn):
        if fn not in FUNCS:
            raise ComputeError("unknown function '%s'" % fn)
        self.enter()
        self.i += 1
        if fn == "has":
            if self.peek("op", ")"):
                raise ComputeError("wrong argument count")
            if not (self.peek("name") or self.peek("quoted")):
                raise ComputeError("has() takes a column name")
            name = self.toks[self.i][1]
            self.i += 1
            s = self.slot(name, False)
            if not self.peek("op", ")"):
                raise ComputeError("has() takes one column name")
            self.i += 1
            self.nest -= 1
            self.emit("has", s)
            return
        got = 0
        if not self.peek("op", ")"):
            while True:
                if got == FUNCS[fn]:
                    raise ComputeError("wrong argument count")
                self.expr()
                got += 1
                if self.peek("op", ","):
                    self.i += 1
                    continue
                break
        if not self.peek("op", ")"):
            raise ComputeError("')' is expected")
        if got != FUNCS[fn]:
            raise ComputeError("wrong argument count")
        self.i += 1
        self.nest -= 1
        self.emit(fn)


def compile_expr(expr, types):
    """types: {column: "int" | "str" | "set"}.  Returns (program, columns by slot, stack depth); ComputeError on a refusal."""
    p = _Parser(expr, types)
    p.expr()
    if p.i < len(p.toks):
        raise ComputeError("syntax error at byte %d" % p.toks[p.i][2])
    return p.prog, p.cols, p.depth


def text(prog):
    return " ".join("c%d" % a if op == "col" else "has(c%d)" % a if op == "has" else str(a) if op == "const" else op for op, a in prog)


def _div(a, b):
    q = abs(a) // abs(b)
    return wrap(q if (a < 0) == (b < 0) else -q)


def _binary(op, a, b):
    (av, ap), (bv, bp) = a, b
    if op == "coalesce":
        return a if ap else b
    p = ap and bp
    if op in ("div", "mod"):
        if not p or bv == 0:
            return (0, False)
        q = _div(av, bv)
        return (q, True) if op == "div" else (wrap(av - q * bv) if bv != -1 else 0, True)
    v = {"mul": lambda: wrap(av * bv), "add": lambda: wrap(av + bv), "sub": lambda: wrap(av - bv), "lt": lambda: int(av < bv),
         "le": lambda: int(av <= bv), "gt": lambda: int(av > bv), "ge": lambda: int(av >= bv), "eq": lambda: int(av == bv),
         "ne": lambda: int(av != bv), "and": lambda: int(av != 0 and bv != 0), "or": lambda: int(av != 0 or bv != 0),
         "min": lambda: min(av, bv), "max": lambda: max(av, bv)}[op]()
    return (v, True) if p else (0, False)


def eval_row(prog, get):
    """get(slot) -> (value, populated).  Returns (value, populated); the value of an unpopulated result is 0."""
    st = []
    for op, a in prog:
        if op == "col":
            v, p = get(a)
            st.append((wrap(v), True) if p else (0, False))
        elif op == "has":
            st.append((1 if get(a)[1] else 0, True))
        elif op == "const":
            st.append((a, True))
        elif op in ("neg", "not", "abs"):
            v, p = st.pop()
            st.append(((wrap(-v) if op == "neg" else int(v == 0) if op == "not" else wrap(abs(v))), True) if p else (0, False))
        elif op == "if":
            b, a_, c = st.pop(), st.pop(), st.pop()
            r = (0, False) if not c[1] else (a_ if c[0] != 0 else b)
            st.append(r if r[1] else (0, False))
        else:
            b, a_ = st.pop(), st.pop()
            r = _binary(op, a_, b)
            st.append(r if r[1] else (0, False))
    assert len(st) == 1
    return st[0]


def evaluate(expr, types, columns, n):
    """columns: {name: (values, populated)} of n rows each (for str / set columns only populated is read).  Returns two lists."""
    prog, cols, _ = compile_expr(expr, types)
    vals, pops = [], []
    for r in range(n):
        v, p = eval_row(prog, lambda s: (int(columns[cols[s]][0][r]) if types[cols[s]] == "int" else 0, bool(columns[cols[s]][1][r])))
        vals.append(v)
        pops.append(p)
    return vals, pops


def storage_of(lo, hi, any_populated, compact):
    """(width, base) of a computed column whose populated results span [lo, hi]: concat's rule."""
    if not compact:
        return (8, 0)
    if not any_populated:
        return (1, 0)
    span = hi - lo
    w = 1 if span < 1 << 8 else 2 if span < 1 << 16 else 4 if span < 1 << 32 else 8
    return (w, lo if w < 8 else 0)


def compute_ref(blocks, exprs, compact=False):
    """exprs: [(name, expr)].  Returns {"blocks": the output's block list (the live blocks of `blocks`, the computed columns
    appended as int columns), "computed": [names], "storage": {name: (width, base)}, "has_missing": {name: bool} (= it has a
    bitmap), "extrema": {name: (lo, hi)} ((I64_MAX, I64_MIN) with no populated row), "stats": rows, blocks, exprs, ops,
    unpopulated}.  ComputeError on a refusal."""
    if len(exprs) < 1:
        raise ComputeError("n_exprs < 1")
    types = dict(D.column_types(blocks))
    progs = []
    for name, expr in exprs:
        if name == "":
            raise ComputeError("empty name")
        if name in types:
            raise ComputeError("the output already holds '%s'" % name)
        progs.append(compile_expr(expr, types))
        types[name] = "int"
    live = [(n, dict(cols)) for n, cols in blocks if n > 0]
    out = {"computed": [n for n, _ in exprs], "storage": {}, "has_missing": {}, "extrema": {},
           "stats": {"rows": sum(b[0] for b in live), "blocks": len(live), "exprs": len(exprs), "ops": sum(len(p[0]) for p in progs), "unpopulated": 0}}
    for (name, _), (prog, cols, _) in zip(exprs, progs):
        lo, hi, any_pop, missing = I64_MAX, I64_MIN, False, False
        for n, bc in live:
            got = {}
            for c in cols:
                spec = bc.get(c)
                if spec is None:
                    got[c] = ([0] * n, [False] * n)
                elif spec[0] == "int":
                    p = [True] * n if len(spec) < 3 or spec[2] is None else [bool(x) for x in np.asarray(spec[2]).tolist()]
                    got[c] = ([int(x) for x in np.asarray(spec[1]).tolist()], p)
                else:
                    got[c] = ([0] * n, [x is not None for x in spec[1]])
            vals, pops = [], []
            for r in range(n):
                v, p = eval_row(prog, lambda s: (got[cols[s]][0][r], got[cols[s]][1][r]))
                vals.append(v)
                pops.append(p)
                if p:
                    lo, hi, any_pop = min(lo, v), max(hi, v), True
                else:
                    missing = True
                    out["stats"]["unpopulated"] += 1
            bc[name] = ("int", np.array(vals, dtype=np.int64).reshape(n), np.array(pops, dtype=bool).reshape(n))
        out["storage"][name] = storage_of(lo, hi, any_pop, compact)
        out["has_missing"][name] = missing
        out["extrema"][name] = (lo, hi)
    out["blocks"] = live
    return out
