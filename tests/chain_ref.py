"""Chains of the calls that make a resident table from resident tables -- digest, select, concat, lookup, compute, rollup and
rollup with percentiles --, on the restatements (run_ref) and on the GPU (run_gpu): the checker of
tests/test_gpu_derived_chains.py, itself checked by tests/test_chain_ref.py.

It composes and writes no semantics of its own: every stage is restated by the module that restates the call (digest_ref,
select_ref, concat_ref, lookup_ref, compute_ref, rollup_ref, rollup_pct_ref), fed the block list the stage before it gave.  What
a block list cannot say about a derived table travels beside it, in Blocks:
  dicts  the str / set dictionaries, which a derived table inherits id for id (concat_ref.table_dict hands them out; a rollup
         orders its str keys by them);
  bitmap which columns have a validity bitmap: a derived column can have one without an unpopulated row (a select that keeps
         only populated rows of a column with a bitmap), and a rollup's key has the MISSING digit where there is a bitmap;
  a block of zero rows that declares the columns, where the table has no rows ("the columns and no blocks").

A stage is (op, kwargs).  kwargs are the call's own, and
  src     the table the call is made on (lookup_dim: the table used as dim): the name of a source, the index of an earlier
          stage, or absent = the stage before (the first source for stage 0);
  srcs    concat: the tables joined, in order (absent = [src]);
  dim     lookup: the table looked up in;          t   lookup_dim: the table the columns are attached to;
  force, slots, pct_force   rollup / rollup_pct: the diagnostic switches (SYBL_ROLLUP_PATH, _SLOTS, _PCT), which the
          restatement takes as arguments and the library reads from the environment at call time.
"""
import contextlib
import os

import numpy as np

from tests import compute_ref as X
from tests import concat_ref as C
from tests import digest_ref as D
from tests import lookup_ref as L
from tests import rollup_pct_ref as P
from tests import rollup_ref as U
from tests import select_ref as S

OPS = ("digest", "select", "concat", "lookup", "lookup_dim", "compute", "rollup", "rollup_pct")
SWITCHES = (("force", "SYBL_ROLLUP_PATH"), ("slots", "SYBL_ROLLUP_SLOTS"), ("pct_force", "SYBL_ROLLUP_PCT"))
_PLUMBING = ("src", "srcs", "dim", "t")


class Blocks(list):
    """The block list of a derived table, with the dictionaries it carries ({str / set column: [strings by id]}) and which of
    its columns have a validity bitmap ({column: bool})."""

    def __init__(self, blocks=(), dicts=None, bitmap=None):
        super().__init__(blocks)
        self.dicts = dict(dicts or {})
        self.bitmap = dict(bitmap or {})


def dicts_of(blocks):
    """{str / set column: the table's dictionary}."""
    return {name: C.table_dict(blocks, name) for name, ty in D.column_types(blocks).items() if ty != "int"}


def live(blocks):
    return [b for b in blocks if b[0] > 0]


def has_unpopulated(blocks, name):
    if not live(blocks):
        return False
    return not bool(D.concat(live(blocks))[name][2].all())


def bitmap_of(blocks, name):
    """Whether the table's column has a validity bitmap: what a derived table carries, else -- a table built block by block --
    whether some row is unpopulated."""
    carried = getattr(blocks, "bitmap", {})
    return carried[name] if name in carried else has_unpopulated(blocks, name)


def declared(columns):
    """The block of zero rows that declares [(name, type)]."""
    return (0, {name: (("int", np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)) if ty == "int" else (ty, [])) for name, ty in columns})


def normalise(blocks, columns, dicts, bitmap):
    """The output of a stage as Blocks: its non-empty blocks -- or, without rows, the declaring block --, the dictionaries
    of its str / set columns and which columns have a bitmap."""
    got = live(blocks)
    return Blocks(got if got else [declared(columns)], {n: dicts[n] for n, ty in columns if ty != "int"}, {n: bool(bitmap[n]) for n, _ in columns})


def _pick(sources, results, ref):
    if isinstance(ref, str):
        return sources[ref]
    got = results[ref]
    return got["blocks"] if isinstance(got, dict) else got


def _inputs(sources, results, kw, k):
    """(the table the call is made on, the other tables by role) of stage k."""
    first = next(iter(sources))
    src = kw.get("src", (k - 1) if k else first)
    return _pick(sources, results, src), {r: kw[r] for r in ("srcs", "dim", "t") if r in kw}


def _own(kw, ref_side):
    """The call's own arguments; the switches only for the restatement."""
    drop = _PLUMBING if ref_side else _PLUMBING + tuple(s for s, _ in SWITCHES)
    return {k: v for k, v in kw.items() if k not in drop}


def ref_stage(op, src, others, kw, compact, out=None):
    """One stage on block lists.  Returns the restatement's result as a dict with "blocks" (Blocks) and "columns"
    [(name, type)]; what the restatement returned beside its blocks is kept.  out: the result of lookup_ref, compute_ref,
    rollup_ref or rollup_pct_ref for this very call, where the caller has it already (it is completed in place)."""
    assert op in OPS, op
    types = D.column_types(src)
    if op == "digest":
        out = dict(blocks=D.digest_ref(src, **kw))
        cols, dicts = list(types.items()), dicts_of(src)
        bitmap = {n: bitmap_of(src, n) for n, _ in cols}              # digest, select: iff the source column has one
    elif op == "select":
        out = dict(blocks=S.select_ref(src, **kw))
        cols, dicts = [(n, types[n]) for n in S.output_columns(src, kw.get("columns"))], dicts_of(src)
        bitmap = {n: bitmap_of(src, n) for n, _ in cols}
    elif op == "concat":
        lists = others["srcs"]
        out = dict(blocks=C.concat_ref(lists, **kw))
        cols = C.output_columns(lists, kw.get("columns"))
        dicts = {n: C.merged_dict([C.table_dict(b, n) for b in lists if n in D.column_types(b)]) for n, ty in cols if ty != "int"}
        # iff some source column has one, or some source with rows lacks the column
        bitmap = {n: any((bitmap_of(b, n) if n in D.column_types(b) else bool(live(b))) for b in lists) for n, _ in cols}
    elif op in ("lookup", "lookup_dim"):
        t, dim = (src, others["dim"]) if op == "lookup" else (others["t"], src)
        out = out if out is not None else L.lookup_ref(t, dim, compact=compact, **kw)
        cols = list(D.column_types(t).items()) + out["attached"]
        dicts = dict(dicts_of(t), **out["dicts"])
        bitmap = dict({n: bitmap_of(t, n) for n in D.column_types(t)}, **out["bitmap"])      # t's columns as concat of t alone gives them
    elif op == "compute":
        out = out if out is not None else X.compute_ref(src, compact=compact, **kw)
        cols, dicts = list(types.items()) + [(n, "int") for n in out["computed"]], dicts_of(src)
        bitmap = dict({n: bitmap_of(src, n) for n in types}, **out["has_missing"])
    else:
        out = out if out is not None else (U.rollup_ref if op == "rollup" else P.rollup_pct_ref)(src, compact=compact, **kw)
        cols, dicts, bitmap = out["columns"], out["dicts"], out["bitmap"]          # a key: iff the MISSING group occurs
    out["op"], out["columns"] = op, cols
    out["blocks"] = normalise(out["blocks"], cols, dicts, bitmap)
    return out


def run_ref(sources, stages, compact=False):
    """sources: {name: block list}.  Returns the result of every stage, in order (ref_stage's dicts)."""
    results = []
    for k, (op, kw) in enumerate(stages):
        src, roles = _inputs(sources, results, kw, k)
        others = {r: ([_pick(sources, results, x) for x in v] if r == "srcs" else _pick(sources, results, v)) for r, v in roles.items()}
        if op == "concat":
            others.setdefault("srcs", [src])
        results.append(ref_stage(op, src, others, _own(kw, True), compact))
    return results


@contextlib.contextmanager
def switches(kw):
    """The rollup's diagnostic switches of a stage in the environment, for the duration of the call."""
    before = {env: os.environ.get(env) for _, env in SWITCHES}
    try:
        for key, env in SWITCHES:
            if kw.get(key):
                os.environ[env] = str(kw[key])
            else:
                os.environ.pop(env, None)
        yield
    finally:
        for env, v in before.items():
            if v is None:
                os.environ.pop(env, None)
            else:
                os.environ[env] = v


def gpu_stage(op, src, others, kw):
    """One stage on Tables: the same call with the same arguments.  Returns the new Table."""
    assert op in OPS, op
    if op == "digest":
        return src.digest(**kw)
    if op == "select":
        return src.select(**kw)
    if op == "concat":
        return others["srcs"][0].ctx.concat(others["srcs"], **kw)
    if op == "lookup":
        return src.lookup(others["dim"], **kw)
    if op == "lookup_dim":
        return others["t"].lookup(src, **kw)
    if op == "compute":
        return src.compute(**kw)
    return src.rollup(**kw)


def gpu_one(tables, made, k, stage):
    """Stage k on Tables, with its switches set: the new Table, which is the caller's to free.  made: the Tables of the
    stages before it."""
    op, kw = stage
    src, roles = _inputs(tables, made, kw, k)
    others = {r: ([_pick(tables, made, x) for x in v] if r == "srcs" else _pick(tables, made, v)) for r, v in roles.items()}
    if op == "concat":
        others.setdefault("srcs", [src])
    with switches(kw):
        return gpu_stage(op, src, others, _own(kw, False))


@contextlib.contextmanager
def run_gpu(tables, stages):
    """tables: {name: Table}, the sources (they stay the caller's).  Yields the Table of every stage, in order; every one of
    them is freed when the block is left, by an exception too -- also those made before a stage that failed."""
    made = []
    try:
        for k, stage in enumerate(stages):
            made.append(gpu_one(tables, made, k, stage))
        yield made
    finally:
        for tb in reversed(made):
            tb.free()


# ------------------------------------------------------------------ what two tables are compared by

def exact_extrema(blocks, name):
    """(min, max) of a column's populated values (dictionary ids for str): what a table tracks where its statistics are exact;
    (INT64_MAX, INT64_MIN) without a populated row."""
    ty, v, p = D.concat(live(blocks))[name] if live(blocks) else (D.column_types(blocks)[name], [], np.zeros(0, dtype=bool))
    if ty == "int":
        return (int(v[p].min()), int(v[p].max())) if p.any() else (C.INT64_MAX, C.INT64_MIN)
    d = C.table_dict(blocks, name)
    ids = [d.index(s) for s in set(x for x in v if x is not None)] if ty == "str" else []
    return (min(ids), max(ids)) if ids else (C.INT64_MAX, C.INT64_MIN)


def fitted_storage(blocks, name, compact):
    """concat's rule over a column's extrema: what concat, lookup and compute store a column of their source at."""
    ty = D.column_types(blocks)[name]
    if not compact:
        return (8, 0) if ty == "int" else (4, 0)
    lo, hi = exact_extrema(blocks, name)
    return C.storage_of(lo, hi, ty)


def renamed_rows(blocks, names):
    """The rows of a block list with its columns renamed by {old: new}; columns not named are dropped."""
    return [{names[k]: v for k, v in row.items() if k in names} for row in D.rows_of(live(blocks))]


# ------------------------------------------------------------------ the three routes the documents name, as stages

ALL = "n,sum,min,max"
RANKS = ((0, 4), (4, 5), (5, None))
RANK_PATHS = ("direct", "global", "hash")
NOTHING = [("f", "gt", 5), ("f", "lt", 3)]
RANK_ROLLUP = dict(groups=["k2", "s"], aggs=[("v8", ALL), ("nb", ALL)], time_col="time", time_bucket=3600)
MERGE_AGGS = [("count", "sum"), ("v8_n", "sum"), ("v8_sum", "sum"), ("v8_min", "min"), ("v8_max", "max"), ("nb_n", "sum"), ("nb_min", "min"),
              ("nb_max", "max")]
# merged column -> the column of one rollup of all the rows it has to equal
MERGED = {"time": "time", "k2": "k2", "s": "s", "count_sum": "count", "v8_n_sum": "v8_n", "v8_sum_sum": "v8_sum", "v8_min_min": "v8_min",
          "v8_max_max": "v8_max", "nb_n_sum": "nb_n", "nb_min_min": "nb_min", "nb_max_max": "nb_max"}


def merge_route(blocks):
    """"sybl_table_concat of the ranks' rollups, then a rollup of the sums".  Three ranks hold blocks[0:4],
    [4:5] and [5:] and roll up on three different paths; a fourth holds every block and its filter matches nothing.  Returns
    (sources, stages); stage 4 is the concat, stage 5 the merged rollup, stage 6 one rollup of all the rows."""
    sources = {"all": blocks}
    stages = []
    for r, ((a, b), path) in enumerate(zip(RANKS, RANK_PATHS)):
        sources["rank%d" % r] = blocks[a:b]
        stages.append(("rollup", dict(RANK_ROLLUP, src="rank%d" % r, force=path)))
    stages.append(("rollup", dict(RANK_ROLLUP, src="all", filters=NOTHING)))
    stages.append(("concat", dict(srcs=[0, 1, 2, 3])))
    stages.append(("rollup", dict(src=4, groups=["k2", "s"], aggs=MERGE_AGGS, time_col="time", time_bucket=1)))
    stages.append(("rollup", dict(RANK_ROLLUP, src="all")))
    return sources, stages


AVERAGES = [("nb_avg", "nb_sum / nb_n"), ("v8_avg", "v8_sum / v8_n")]


def average_route(blocks):
    """"divide _sum by _n with compute", then a rollup of the computed column.  Stage 0 the rollup, 1 the
    compute, 2 the rollup of nb_avg by s."""
    return {"all": blocks}, [("rollup", dict(RANK_ROLLUP)), ("compute", dict(exprs=AVERAGES)),
                             ("rollup_pct", dict(groups=["s"], aggs=[("nb_avg", "min,max,p50")]))]


# Ten rows pass.  By k2 and by s alike the small side then has the MISSING group, groups without a populated nb (nb_min unpopulated
# there) and groups with one; by s one string of the big side is not in it at all.
SMALL_SIDE = [("v2", "gt", 315), ("v2", "lt", 385)]
ATTACHED = ["count", "v1_sum", "nb_min", "v4_p50"]


def lookup_route(blocks, key):
    """The rollup commit: "a materialised group-by as the small side of a lookup".  Stage 0 the rollup by `key`, stage 1 the
    lookup of every row's group."""
    return {"all": blocks}, [("rollup_pct", dict(groups=[key], aggs=[("v1", "sum"), ("nb", "n,min"), ("v4", "p50")], filters=SMALL_SIDE)),
                             ("lookup_dim", dict(t="all", key=key, columns=ATTACHED, prefix="g_"))]
