"""GPU: derived tables as each other's inputs, and tables with dead blocks as the input of select, compute and rollup.

The seven calls that make a resident table from resident tables -- digest, select, concat, lookup, compute, rollup, rollup with
percentiles -- each have an exact test file that feeds them tables made by append_block and reads the output back.  What only
the NEXT call reads of a derived table -- n_pop and the tracked extrema, the per-block minima and maxima, whether a bitmap or
a data array exists, the stored bytes of unpopulated and padding rows, the dictionaries carried id for id, the (width, base) a
column keeps while its values shrink -- is pinned here: every producer's output is the input of every consumer, and the result
is compared, exactly, with the restatement of the restatement (tests/chain_ref.py, checked on the CPU by
tests/test_chain_ref.py), through the consumer's own _check where it has one.

Shapes: MAIN of tests/test_gpu_rollup.py (3 161 rows in blocks of 1, 70, 33, 2049, 31, 64, 777, 32, 1, 70, 33), compact and
canonical; the producers cut their output into blocks of 7 and 33 rows.  The loaded table has 1 860 rows in five blocks."""
import os
import shutil

import numpy as np
import pytest

from tests import chain_ref as CH
from tests import concat_ref as C
from tests import digest_ref as D
from tests import rollup_pct_ref as P
from tests import rollup_ref as U
from tests import sybil_fixture as F
from tests import test_gpu_compute as TC
from tests import test_gpu_lookup as TL
from tests import test_gpu_rollup as TR
from tests import test_gpu_rollup_pct as TP
from tests.test_gpu_concat import _against_oracle, _check_concat, _check_storage, _cut, _expected_storage, _rows
from tests.test_gpu_digest import _check_digest
from tests.test_gpu_rollup import MAIN, N_T
from tests.test_gpu_samples import build
from tests.test_gpu_samples import check as check_samples
from tests.test_gpu_select import _check_select

pytestmark = pytest.mark.gpu

E_INVAL = -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL = CH.ALL
COUNTS, PCT_COUNTS = TR.COUNTS, TP.PCT_COUNTS
TYPE_ID = {"int": 1, "str": 2, "set": 3}

# the small second table: the dim of the lookups made ON a derived table, and the second source of the producer concat.  Its key
# 1000 is there twice (the first row wins), 7 matches nothing, 31000 sits in a row whose key is unpopulated
DIM = _cut({"id": (np.array([1000, 61000, 7, 1000, 31000], dtype=np.int64), np.array([1, 1, 1, 1, 0], dtype=bool)),
            "w": (np.array([10, -20, 30, 40, 50], dtype=np.int64), np.array([1, 0, 1, 1, 1], dtype=bool))},
           {"label": ["x", "y", None, "z", "x"]}, {}, (5,))
SOURCES = {"main": MAIN, "dim": DIM}
MAIN_COLUMNS = list(D.column_types(MAIN))
NOTHING = CH.NOTHING                                       # the kernels find no row
PROVEN = [("f", "gt", I64_MAX)]                            # the planner proves it

ROLLUP_KW = dict(groups=["k2", "s", "f"], aggs=[("v1", ALL), ("v8", ALL), ("nb", ALL), ("none", "n,sum")], time_col="time", time_bucket=3600,
                 block_rows=33)
PCT_KW = dict(groups=["k2", "s", "f"], aggs=[("v1", "sum,p50"), ("v8", "min,p1,p99"), ("nb", "n,min,p50"), ("none", "sum,p50")], time_col="time",
              time_bucket=3600, block_rows=7)
# one fixed call per producer, made on MAIN
PRODUCERS = {
    "digest": ("digest", dict(src="main", time_col="time", block_rows=33)),
    "select": ("select", dict(src="main", filters=[("v2", "gt", 700), ("f", "neq", 3)], block_rows=7)),
    "concat": ("concat", dict(srcs=["main", "dim"], columns=MAIN_COLUMNS)),       # dim lacks every column: three rows of nothing
    "lookup": ("lookup", dict(src="main", dim="main", key="v1", columns=["nb", "none", "v8", "s"], prefix="d_")),
    "compute": ("compute", dict(src="main", exprs=[("c_sum", "v1 + nb"), ("c_none", "none * 2"), ("c_big", "v8 - 1"), ("c_has", "has(s) + has(tags)")])),
    "rollup": ("rollup", dict(ROLLUP_KW, src="main")),
    "rollup_pct": ("rollup_pct", dict(PCT_KW, src="main")),
    # the intermediates without rows
    "none_select": ("select", dict(src="main", filters=NOTHING)),
    "none_proven": ("rollup", dict(ROLLUP_KW, src="main", filters=PROVEN)),
    "none_found": ("rollup", dict(ROLLUP_KW, src="main", filters=NOTHING)),
}
SEVEN = ["digest", "select", "concat", "lookup", "compute", "rollup", "rollup_pct"]
EMPTY = ["none_select", "none_proven", "none_found"]
ROLLED = ("rollup", "rollup_pct", "none_proven", "none_found")
# per producer: a column it made (a carried one where it makes none) whose rows are partly unpopulated, one wholly unpopulated
# (storage (1, 0) when compact, extrema (INT64_MAX, INT64_MIN)), an 8-byte one, and the column the block-statistics filters are on
NAMES = {"digest": dict(part="nb", none="none", big="v8", stat="v2"), "select": dict(part="nb", none="none", big="v8", stat="v2"),
         "concat": dict(part="nb", none="none", big="v8", stat="v2"), "lookup": dict(part="d_nb", none="d_none", big="d_v8", stat="v2"),
         "compute": dict(part="c_sum", none="c_none", big="c_big", stat="v2"),
         "rollup": dict(part="nb_min", none="none_sum", big="v8_min", stat="v1_sum"),
         "rollup_pct": dict(part="nb_p50", none="none_p50", big="v8_p99", stat="v1_sum")}
NAMES.update(none_select=NAMES["select"], none_proven=NAMES["rollup"], none_found=NAMES["rollup"])
CONSUMERS = ["digest", "select", "concat", "lookup", "lookup_dim", "compute", "rollup", "rollup_pct", "samples", "save_open"]


def consumer_call(producer, consumer):
    """The one fixed call of a consumer on a producer's output.  Between its keys, filters, aggregated columns and operands it
    uses the carried int column with a bitmap (k2), the str column (s), and the producer's partly unpopulated, wholly unpopulated
    and 8-byte columns; a rollup takes 4 group and 8 aggregated columns at most."""
    n = NAMES[producer]
    part, none, big = n["part"], n["none"], n["big"]
    return {
        "digest": dict(time_col=part, block_rows=33),                 # a row without the key sorts as 0
        "select": dict(filters=[("k2", "lt", 40000), (part, "gt", -300), ("s", "neq", "host03"), (big, "lt", 1 << 62)],
                       columns=["s", "k2", part, none, big, "f"], block_rows=33),
        "concat": dict(),                                              # the table twice
        "lookup": dict(key="k2", dim_key="id", columns=["label", "w"]),
        "lookup_dim": dict(key="s", columns=["k2", part, none, big], prefix="x_"),     # the first row of each string wins
        "compute": dict(exprs=[("e_sum", "%s + k2" % part), ("e_none", "%s + 1" % none), ("e_big", "%s / 3 + has(s)" % big),
                               ("e_if", "if(has(%s), %s, f)" % (part, part))]),
        "rollup": dict(groups=["k2", "s"], aggs=[(part, ALL), (none, "n,sum"), (big, "min,max"), ("f", "sum")], filters=[("f", "neq", 4)], block_rows=7),
        "rollup_pct": dict(groups=["s"], aggs=[(part, "min,p50"), (none, "p50"), (big, "p1,p99"), ("k2", "n,p50")], block_rows=7),
    }.get(consumer)


@pytest.fixture(scope="module")
def ctx():
    import sybil_amd
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc
    return orc


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("SYBL_ROLLUP_PATH", "SYBL_ROLLUP_SLOTS", "SYBL_ROLLUP_MERGE", "SYBL_ROLLUP_PCT", "SYBL_LOOKUP_PATH", "SYBL_LOOKUP_SLOTS"):
        monkeypatch.delenv(name, raising=False)


class World:
    """The sources and every producer's output, made on first use and kept for the module (nothing here changes a table)."""

    def __init__(self, ctx):
        self.ctx, self.tables, self.made, self.refs = ctx, {}, {}, {}

    def table(self, name, compact):
        if (name, compact) not in self.tables:
            self.tables[(name, compact)] = build(self.ctx, SOURCES[name], compact=compact, name=name)
        return self.tables[(name, compact)]

    def ref(self, producer, compact):
        if (producer, compact) not in self.refs:
            self.refs[(producer, compact)] = CH.run_ref(SOURCES, [PRODUCERS[producer]], compact=compact)[0]
        return self.refs[(producer, compact)]

    def inter(self, producer, compact):
        """(the producer's output, the restatement's result)."""
        if (producer, compact) not in self.made:
            tables = {name: self.table(name, compact) for name in SOURCES}
            self.made[(producer, compact)] = CH.gpu_one(tables, [], 0, PRODUCERS[producer])
        return self.made[(producer, compact)], self.ref(producer, compact)

    def free(self):
        for tb in list(self.made.values()) + list(self.tables.values()):
            tb.free()


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.free()


def _storages(tb, names):
    return {n: tb.column_storage(n) for n in names}


def _check_table(tb, rb, storage=None, loaded=False, rows=True):
    """A table against a block list: rows, blocks, columns, every row, the dictionaries, the tracked extrema -- exact in every
    chain here: each source's are, digest / select / rollup / compute and the attached columns fold theirs from the new blocks,
    concat unites its sources' --, the populated values as stored, and the (width, base) of the columns `storage` names.
    loaded: the table was read back from a directory -- the loader orders columns and dictionaries its own way and keeps the
    IntInfo of the files: rows, blocks, every row and the stored values only.  rows=False: the caller's _check has compared
    every row already."""
    lv = CH.live(rb)
    n = sum(b[0] for b in lv)
    types = D.column_types(rb)
    assert (tb.rows, tb.blocks) == (n, len(lv))
    assert tb.samples(limit=1).columns == list(types) or (loaded and sorted(tb.samples(limit=1).columns) == sorted(types))
    assert not rows or _rows(tb) == D.rows_of(lv)
    cols = D.concat(lv) if lv else {}
    for name, ty in types.items():
        info = tb.column_info(name)
        assert info["type"] == TYPE_ID[ty], (name, info)
        if ty != "int" and not loaded:
            assert tb.column_dict(name) == C.table_dict(rb, name), name
        if ty != "set" and not loaded:
            assert (info["exact_min"], info["exact_max"]) == CH.exact_extrema(rb, name), (name, info)
        if storage and name in storage:
            assert tb.column_storage(name) == storage[name], (name, tb.column_storage(name), storage[name])
        if ty == "int" and n:
            _, v, p = cols[name]
            assert np.array_equal(tb.read_int(name, 0, n)[p], v[p]), name


def _fitted(rb, compact, names=None):
    """concat's rule over the columns of a table: what concat of it alone, lookup and compute store its columns at."""
    return {n: CH.fitted_storage(rb, n, compact) for n, ty in D.column_types(rb).items() if ty != "set" and (names is None or n in names)}


def _counts(st, names):
    return {k: st[k] for k in names}


# ------------------------------------------------------------------ 1. the intermediates are the first restatement

@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
@pytest.mark.parametrize("producer", SEVEN + EMPTY)
def test_the_intermediate_is_the_first_restatement(world, producer, compact):
    it, ref = world.inter(producer, compact)
    main = world.table("main", compact)
    rb, op = ref["blocks"], ref["op"]
    names = [n for n, ty in ref["columns"] if ty != "set"]
    if op in ("digest", "select"):
        storage = _storages(main, names)                               # every value is a source value: (width, base) kept
    elif op == "concat":
        storage = {n: _expected_storage([MAIN, DIM], compact, n, ty) for n, ty in ref["columns"] if ty != "set"}
    elif op in ("lookup", "compute"):
        storage = dict(_fitted(MAIN, compact), **ref["storage"])
    else:
        storage = dict(ref["storage"], **_storages(main, ["k2", "s", "f"]))
    _check_table(it, rb, storage)
    for name, _ in ref["columns"]:
        if name in ref.get("bitmap", {}) and op != "lookup":
            assert it.column_info(name)["has_missing"] == ref["bitmap"][name], name
    if op == "select":
        st = it.select_stats()
        assert (st["rows_in"], st["rows_out"], st["blocks_out"]) == (N_T, it.rows, it.blocks)
    elif op == "lookup":
        st = it.lookup_stats()
        assert (st["matched"], st["dim_keys"], st["dim_duplicates"], st["path"]) == (N_T, 200, N_T - 200, TL.DIRECT)
        assert (ref["matched"], ref["dim_keys"], ref["dim_duplicates"]) == (N_T, 200, N_T - 200)
    elif op == "compute":
        assert _counts(it.compute_stats(), ref["stats"]) == ref["stats"]
    elif op in ("rollup", "rollup_pct"):
        # (what the planner proves empty runs no kernel: no path, no cells -- the restatement does not plan filters)
        assert _counts(it.rollup_stats(), COUNTS) == (dict(ref["stats"], path=0, cells_or_slots=0) if producer == "none_proven" else ref["stats"])
        if op == "rollup_pct":
            assert _counts(it.rollup_pct_stats(), PCT_COUNTS) == ref["pct_stats"]
    if producer in SEVEN:
        n = NAMES[producer]
        c = D.concat(CH.live(rb))
        assert 0 < int(c[n["part"]][2].sum()) < it.rows and not c[n["none"]][2].any()
        assert it.column_info(n["none"])["exact_min"] == I64_MAX and it.column_info(n["none"])["exact_max"] == I64_MIN
        if compact:
            assert it.column_storage(n["none"]) == (1, 0) and it.column_storage(n["big"])[0] == 8
        assert len(rb) > 10                                            # many short blocks, padding behind most of them
    else:
        assert (it.rows, it.blocks) == (0, 0) and it.samples(limit=5).rows == []
        assert it.column_dict("s") == main.column_dict("s") and it.column_storage("s") == main.column_storage("s")
        if producer != "none_select":
            assert (it.rollup_stats()["path"] == 0) == (producer == "none_proven")
            if compact:
                assert [it.column_storage(c) for c in ("count", "time", "nb_min", "none_sum")] == [(1, 0)] * 4
    assert (main.rows, main.blocks) == (N_T, len(MAIN))


# ------------------------------------------------------------------ 2. every producer's output into every consumer

def _consume(world, producer, consumer, compact, tmp_path):
    it, ir = world.inter(producer, compact)
    ib = ir["blocks"]
    main, dim = world.table("main", compact), world.table("dim", compact)
    before = (it.rows, it.blocks, main.rows, main.blocks, dim.rows, dim.blocks)
    rolled = producer in ROLLED
    kw = consumer_call(producer, consumer)
    lv = CH.live(ib)
    out = None
    try:
        if consumer == "digest":
            ref = CH.ref_stage("digest", ib, {}, kw, compact)
            out = it.digest(**kw)
            _check_digest(it, out, ib, kw["block_rows"], kw["time_col"])
            _check_table(out, ref["blocks"], _storages(it, [n for n, ty in ref["columns"] if ty != "set"]), rows=False)
            assert out.digest_stats()["rows"] == it.rows
        elif consumer == "select":
            ref = CH.ref_stage("select", ib, {}, kw, compact)
            assert _check_select(it, ib, **kw) == sum(b[0] for b in CH.live(ref["blocks"]))
            out = it.select(**kw)
            _check_table(out, ref["blocks"], _storages(it, [n for n, ty in ref["columns"] if ty != "set"]), rows=False)
        elif consumer == "concat":
            ref = CH.ref_stage("concat", ib, {"srcs": [ib, ib]}, kw, compact)
            out = _check_concat(world.ctx, [it, it], [ib, ib])
            _check_storage(out, [ib, ib], compact)
            _check_table(out, ref["blocks"], _fitted(ib, compact), rows=False)
        elif consumer == "lookup":
            out, st, lref = TL._check(it, ib, dim, DIM, kw["key"], compact, **{k: v for k, v in kw.items() if k != "key"})
            ref = CH.ref_stage("lookup", ib, {"dim": DIM}, kw, compact, out=lref)
            assert (st["path"] == 0) == (not lv) and st["dim_duplicates"] == (1 if lv else st["dim_duplicates"])
            _check_table(out, ref["blocks"], dict(_fitted(ib, compact), **lref["storage"]), rows=False)
        elif consumer == "lookup_dim":
            out, st, lref = TL._check(main, MAIN, it, ib, kw["key"], compact, path=TL.STR if lv else 0, **{k: v for k, v in kw.items() if k != "key"})
            if not lv:                                                 # every row is unmatched
                assert st["matched"] == 0 and all(lref["bitmap"].values()) and not any("x_k2" in r for r in D.rows_of(lref["blocks"]))
            ref = CH.ref_stage("lookup_dim", ib, {"t": MAIN}, kw, compact, out=lref)
            _check_table(out, ref["blocks"], dict(_fitted(MAIN, compact), **lref["storage"]), rows=False)
        elif consumer == "compute":
            out, st, cref = TC._check(it, ib, kw["exprs"], compact)
            ref = CH.ref_stage("compute", ib, {}, kw, compact, out=cref)
            _check_table(out, ref["blocks"], dict(_fitted(ib, compact), **cref["storage"]), rows=False)
        elif consumer == "rollup":
            out, st, rref = TR._check(it, ib, compact, rolled=rolled, **kw)
            ref = CH.ref_stage("rollup", ib, {}, kw, compact, out=rref)
            _check_table(out, ref["blocks"], dict(rref["storage"], **_storages(it, ["k2", "s"])), rows=False)
        elif consumer == "rollup_pct":
            out, ps, rref = TP._check(it, ib, compact, rolled=rolled, **kw)
            ref = CH.ref_stage("rollup_pct", ib, {}, kw, compact, out=rref)
            _check_table(out, ref["blocks"], dict(rref["storage"], **_storages(it, ["s"])), rows=False)
            assert ps["columns"] == 4 and ps["percentiles"] == 5
        elif consumer == "samples":
            if lv:
                n = NAMES[producer]
                check_samples(it, lv, limit=it.rows)
                check_samples(it, lv, filters=[("k2", "lt", 40000), ("s", "neq", "host03")], order_by=n["part"], limit=50)
                check_samples(it, lv, filters=[(n["big"], "gt", 0)], columns=["s", n["none"], n["part"]], order_by=n["big"], order_asc=True, limit=40)
            else:
                assert it.samples(limit=5).rows == [] and it.samples(filters=[("k2", "lt", 40000)], limit=5).info["matched"] == 0
        else:
            root = str(tmp_path / "db")
            it.save(root)
            out = world.ctx.open_table(root, it.name, compact=compact)
            _check_table(out, ib, loaded=True)
            if lv:
                assert {s for s in out.column_dict("s")} <= set(it.column_dict("s"))
    finally:
        if out is not None:
            out.free()
    assert (it.rows, it.blocks, main.rows, main.blocks, dim.rows, dim.blocks) == before


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("producer", SEVEN)
def test_every_producer_into_every_consumer(world, producer, consumer, compact, tmp_path):
    _consume(world, producer, consumer, compact, tmp_path)


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("producer", EMPTY)
def test_a_table_without_rows_into_every_consumer(world, producer, consumer, compact, tmp_path):
    """A select that matches nothing, a rollup whose filter the planner proves empty and one the kernels find empty: the columns
    and no blocks.  Every consumer gives what the restatement gives of it: an empty table with the right columns, (1, 0) storage
    for what it makes, the source's dictionaries; as dim, every row is unmatched."""
    _consume(world, producer, consumer, compact, tmp_path)


# ------------------------------------------------------------------ 3. what the engine refuses of a derived table

@pytest.mark.parametrize("producer", SEVEN)
def test_documented_refusals(world, producer):
    """A rollup keyed on the 8-byte column: its tracked extrema span more than 2^62.  A set column as a lookup key, a str column
    as a value of an expression, a str column as digest's key."""
    import sybil_amd
    it, ref = world.inter(producer, True)
    n = NAMES[producer]
    lo, hi = CH.exact_extrema(ref["blocks"], n["big"])
    assert hi - lo > 1 << 62
    cases = [(lambda: it.rollup(groups=[n["big"]]), "sybl_table_rollup: ", "2^62"), (lambda: it.rollup(groups=["s", n["big"]], aggs=[(n["part"], "p50")]), "sybl_table_rollup: ", "2^62"),
             (lambda: it.compute([("x", "s + 1")]), "sybl_table_compute: ", "'s'"), (lambda: it.digest(time_col="s"), "digest: ", "'s'")]
    if "tags" in D.column_types(ref["blocks"]):
        cases.append((lambda: world.table("main", True).lookup(it, "tags"), "sybl_table_lookup: ", "tags"))
        cases.append((lambda: it.rollup(groups=["tags"]), "sybl_table_rollup: ", "tags"))
    for call, who, word in cases:
        with pytest.raises(sybil_amd.SyblError) as ei:
            call()
        assert ei.value.code == E_INVAL and who in str(ei.value) and word in str(ei.value), str(ei.value)
    assert (it.rows, it.blocks) == (sum(b[0] for b in ref["blocks"]), len(ref["blocks"]))


# ------------------------------------------------------------------ 4. block statistics through filters

def _populated(blk, col):
    """The populated values of a column in one block (none where the block lacks the column)."""
    _, v, p = D.concat([blk]).get(col, ("int", np.zeros(blk[0], dtype=np.int64), np.zeros(blk[0], dtype=bool)))
    return v[p]


def _stat_filters(rb, col, pair):
    """Filters whose constants sit on the per-block extrema of `col`, taken from the restatement's blocks: eq a value present in
    exactly one block; gt (max - 1) and lt (min + 1) of an inner block; `pair`, which no row passes."""
    per = [_populated(blk, col) for blk in CH.live(rb)]
    seen = {}
    for b, vals in enumerate(per):
        for x in set(vals.tolist()):
            seen.setdefault(x, []).append(b)
    inner = [b for b in range(1, len(per) - 1) if len(per[b])]
    b = inner[len(inner) // 2]
    once = [x for x in sorted(set(per[b].tolist())) if seen[x] == [b]] or [x for x, bs in sorted(seen.items()) if len(bs) == 1]
    return {"eq": [(col, "eq", int(once[0]))], "gt": [(col, "gt", int(per[b].max()) - 1)], "lt": [(col, "lt", int(per[b].min()) + 1)], "none": pair}


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
@pytest.mark.parametrize("producer", SEVEN)
def test_block_statistics_through_filters(world, producer, compact):
    """select and rollup skip the blocks whose minimum and maximum exclude a filter's constant, and prove `never matches` from
    them.  A block minimum or maximum that is too narrow drops rows here.  The last pair is passed by no row although the
    table's range, and that of every block that holds both a smaller and a larger value, admits it (a block of one row cannot
    admit a pair its row does not pass): the kernels run and find nothing."""
    it, ir = world.inter(producer, compact)
    ib = ir["blocks"]
    rolled = producer in ROLLED
    col = NAMES[producer]["stat"]
    pair = [("count", "gt", 1), ("count", "lt", 2)] if rolled else [("k1", "gt", 1), ("k1", "lt", 2)]
    admit = sum(bool(len(v) and v.max() > 1 and v.min() < 2) for v in (_populated(blk, pair[0][0]) for blk in CH.live(ib)))
    assert admit > len(CH.live(ib)) // 2
    for which, filters in _stat_filters(ib, col, pair).items():
        m = _check_select(it, ib, filters=filters, block_rows=33)
        out, st, ref = TR._check(it, ib, compact, rolled=rolled, groups=["s"], aggs=[(col, "n,sum"), ("k2", "n")], filters=filters)
        try:
            assert st["rows_matched"] == m and (m > 0) == (which != "none") and st["path"] != 0, (which, m, st)
        finally:
            out.free()


def test_a_bitmap_outlives_its_unpopulated_rows(world):
    """k2 has a bitmap; the select keeps rows whose k2 is populated only, and the output column keeps the bitmap (select's rule).
    A rollup gives a key column with a bitmap the MISSING digit, rows or not: 2 cells for the one value, and 2 x 5 with s, whose
    ids in these rows are 2 (host03) and 5 (host00) and which has a bitmap too."""
    main = world.table("main", True)
    stages = [("select", dict(src="main", filters=[("k2", "eq", 1000)], block_rows=33)), ("rollup", dict(groups=["k2"], aggs=[("v1", "sum")])),
              ("rollup", dict(src=0, groups=["k2", "s"], force="global")), ("lookup_dim", dict(src=1, t="main", key="k2", columns=["count"]))]
    refs = CH.run_ref(SOURCES, stages, compact=True)
    assert refs[1]["stats"]["cells_or_slots"] == 2 and refs[2]["stats"]["cells_or_slots"] == 10 and refs[1]["stats"]["groups"] == 1
    assert not CH.has_unpopulated(refs[0]["blocks"], "k2") and refs[0]["blocks"].bitmap["k2"] and not refs[1]["blocks"].bitmap["k2"]
    with CH.run_gpu({"main": main}, stages) as made:
        for tb, ref in zip(made, refs):
            _check_table(tb, ref["blocks"])
        assert _counts(made[1].rollup_stats(), COUNTS) == refs[1]["stats"] and _counts(made[2].rollup_stats(), COUNTS) == refs[2]["stats"]
        st = made[3].lookup_stats()
        assert (st["matched"], st["dim_keys"], st["path"]) == (refs[3]["matched"], 1, TL.DIRECT)


# ------------------------------------------------------------------ 5. the three documented routes

def _check_stage(tb, ref, compact):
    """A stage of a route against its restatement: the table, the storage of what the stage made, its counts."""
    op = ref["op"]
    _check_table(tb, ref["blocks"], ref.get("storage"))
    if op in ("rollup", "rollup_pct"):
        assert _counts(tb.rollup_stats(), COUNTS) == ref["stats"], (tb.rollup_stats(), ref["stats"])
        for name, has in ref["bitmap"].items():
            assert tb.column_info(name)["has_missing"] == has, name
    if op == "rollup_pct":
        assert _counts(tb.rollup_pct_stats(), PCT_COUNTS) == ref["pct_stats"]
    if op == "compute":
        assert _counts(tb.compute_stats(), ref["stats"]) == ref["stats"]
        for name in ref["computed"]:
            info = tb.column_info(name)
            assert (info["exact_min"], info["exact_max"], info["has_missing"]) == ref["extrema"][name] + (ref["has_missing"][name],)
    if op in ("lookup", "lookup_dim"):
        st = tb.lookup_stats()
        assert (st["matched"], st["dim_keys"], st["dim_duplicates"]) == (ref["matched"], ref["dim_keys"], ref["dim_duplicates"])


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
def test_merge_of_ranks_is_one_rollup_of_all_rows(ctx, world, compact):
    """concat of the ranks' rollups, then a rollup of the sums.  Three ranks roll up by hour x k2 (a MISSING
    group) x s with the switch at direct, global and hash; a fourth matches nothing and is a table without blocks inside the
    concat.  The merged rollup equals, column for renamed column and row for row, one rollup of all of MAIN: 88 groups, 5 with
    nb_n = 0 -- an unpopulated nb_min of one rank does not enter the merged minimum --, 36 with MISSING k2, the wrapped v8 sums
    equal mod 2^64."""
    sources, stages = CH.merge_route(MAIN)
    refs = CH.run_ref(sources, stages, compact=compact)
    ranks = {}
    try:
        for k in range(3):
            ranks["rank%d" % k] = build(ctx, sources["rank%d" % k], compact=compact, name="main")
        tables = dict(ranks, all=world.table("main", compact))
        with CH.run_gpu(tables, stages) as made:
            for tb, ref in zip(made, refs):
                _check_stage(tb, ref, compact)
            assert [tb.rollup_stats()["path"] for tb in made[:4]] == [U.GLOBAL, U.GLOBAL, U.HASH, U.HASH] and made[3].blocks == 0
            parts, merged, one = made[4], made[5], made[6]
            _check_storage(parts, [refs[k]["blocks"] for k in range(4)], compact)
            st = parts.concat_stats()
            assert (st["tables"], st["rows"], st["blocks"]) == (4, 144, 3) and merged.rows == one.rows == 88
            got = [{CH.MERGED[k]: v for k, v in row.items() if k in CH.MERGED} for row in _rows(merged)]
            want = [{k: v for k, v in row.items() if k in CH.MERGED.values()} for row in _rows(one)]
            assert got == want
            assert sum("nb_min" not in row for row in want) == 5 and sum("k2" not in row for row in want) == 36
            for name, same in CH.MERGED.items():
                assert merged.column_storage(name) == one.column_storage(same), name
                a, b = merged.column_info(name), one.column_info(same)
                assert (a["exact_min"], a["exact_max"], a["has_missing"]) == (b["exact_min"], b["exact_max"], b["has_missing"]), name
    finally:
        for tb in ranks.values():
            tb.free()


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
def test_average_by_compute_and_a_rollup_of_it(world, compact):
    """divide _sum by _n with compute.  Groups with n = 0 give an unpopulated average (unpopulated operand, zero
    divisor); negative sums truncate toward zero; then nb_avg: min, max, p50 by s."""
    sources, stages = CH.average_route(MAIN)
    refs = CH.run_ref(sources, stages, compact=compact)
    with CH.run_gpu({"all": world.table("main", compact)}, stages) as made:
        for tb, ref in zip(made, refs):
            _check_stage(tb, ref, compact)
        rows = _rows(made[1])
        assert sum("nb_avg" not in r for r in rows) == 5 == sum(r["nb_n"] == 0 for r in rows) and all("v8_avg" in r for r in rows)
        neg = [r for r in rows if r["nb_n"] and r["nb_sum"] < 0 and r["nb_sum"] % r["nb_n"]]
        assert neg and all(r["nb_avg"] == -(-r["nb_sum"] // r["nb_n"]) for r in neg)           # toward zero, not the floor
        assert made[2].rows == 7 and made[2].rollup_pct_stats()["items"] == 83


@pytest.mark.parametrize("key,force,path", [("k2", "direct", TL.DIRECT), ("k2", "hash", TL.HASH), ("s", None, TL.STR)])
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])
def test_rollup_as_the_small_side_of_a_lookup(world, oracle, monkeypatch, compact, key, force, path):
    """The rollup commit: a materialised group-by as the small side of a lookup.  The rollup's MISSING-key row matches no row of
    MAIN, rows of MAIN with an unpopulated key get nothing; attached: count, a _sum stored at 2 bytes, nb_min (partly unpopulated
    in the rollup) and a percentile.  Then a query grouped by k1 over the attached count, against the oracle."""
    sources, stages = CH.lookup_route(MAIN, key)
    refs = CH.run_ref(sources, stages, compact=compact)
    main = world.table("main", compact)
    if force:
        monkeypatch.setenv("SYBL_LOOKUP_PATH", force)
    with CH.run_gpu({"all": main}, stages[:1]) as made:
        small, sref = made[0], refs[0]
        _check_stage(small, sref, compact)
        kw = {k: v for k, v in stages[1][1].items() if k not in ("t", "key")}
        out, st, lref = TL._check(main, MAIN, small, sref["blocks"], key, compact, path=path, **kw)
        try:
            _check_table(out, refs[1]["blocks"], dict(_fitted(MAIN, compact), **lref["storage"]))
            assert st["matched"] == refs[1]["matched"] < N_T and st["dim_rows"] == small.rows == st["dim_keys"] + 1     # + the MISSING row
            if compact:
                assert small.column_storage("v1_sum")[0] == 2 == out.column_storage("g_v1_sum")[0]
            rows = _rows(out)
            assert not any("g_count" in r for r in rows if key not in r)                       # an unpopulated key gets nothing
            assert any("g_count" in r and "g_nb_min" not in r for r in rows) and any("g_nb_min" in r for r in rows)
            counts = D.concat(lref["blocks"])["g_count"]
            q = dict(groups=["k1"], aggs=["g_count"], op="avg")
            names = [("k1", "int"), ("g_count", "int")]
            assert _against_oracle(oracle, out, lref["blocks"], names, {}, q, {"g_count": (int(counts[1][counts[2]].min()), int(counts[1][counts[2]].max()))}) > 0
        finally:
            out.free()


# ------------------------------------------------------------------ 6. loaded tables with dead blocks

DEAD_SIZES = (300, 1000, 77, 450, 33)
DEAD = (1, 3)                                              # blocks 2 and 4 (directories count from 1)
LIVE_ROWS = 300 + 77 + 33


def _dead_blocks():
    """Five blocks; the two that die hold the table-wide minimum and maximum of the key k and of the aggregated v, the only
    populated rows of `only`, and the only rows with the string "ghost"."""
    blocks = []
    for b, n in enumerate(DEAD_SIZES):
        i = np.arange(n, dtype=np.int64)
        dead = b in DEAD
        k = 10 + (i * 3 + b) % 30
        v = (i * 7919 + b * 13) % 1000 - 500
        names = [None if x % 9 == 0 else "user%d" % (x % 50) for x in i.tolist()]
        if dead:
            k[1], v[1] = (0, -100000) if b == 1 else (99, 100000)
            if b == 1:
                names[5::100] = ["ghost"] * len(names[5::100])
        # (in name order: the order the loader gives a table's columns)
        blocks.append((n, {"dead": ("int", np.full(n, int(dead), dtype=np.int64), None), "k": ("int", k, i % 7 != 0), "name": ("str", names),
                           "only": ("int", i * 3, np.full(n, dead)), "row": ("int", i + 10000 * b, None), "v": ("int", v, None)}))
    return blocks


DEAD_BLOCKS = _dead_blocks()
DEAD_LIVE = [blk for b, blk in enumerate(DEAD_BLOCKS) if b not in DEAD]
IS_LIVE = [("dead", "eq", 0)]


def _from_a_live_block(rows, names=("row",)):
    return all(not (10000 <= r[n] < 20000 or 30000 <= r[n] < 40000) for r in rows for n in names if n in r)


@pytest.fixture(scope="module", params=[True, False], ids=["compact", "canonical"])
def loaded(ctx, request, tmp_path_factory):
    """(the table after refresh dropped blocks 2 and 4, compact?, the block list of ALL five blocks with the table's
    dictionary, that of the live three): three live runs that are not contiguous, statistics that still cover the dead rows."""
    root = str(tmp_path_factory.mktemp("dead") / "db")
    F.write_table(root, "events", [cols for _, cols in DEAD_BLOCKS])
    tb = ctx.open_table(root, "events", compact=request.param)
    try:
        assert tb.blocks == 5 and tb.rows == sum(DEAD_SIZES) == 1860
        for b in DEAD:
            shutil.rmtree(os.path.join(root, "events", "block%09d" % (b + 1)))
        assert tb.refresh()[1] == 2 and tb.rows == LIVE_ROWS
        names = tb.column_dict("name")
        assert sorted(names) == sorted(C.table_dict(DEAD_BLOCKS, "name")) and "ghost" in names      # the loader's id order is its own
        yield tb, request.param, CH.Blocks(DEAD_BLOCKS, {"name": names}), CH.Blocks(DEAD_LIVE, {"name": names})
    finally:
        tb.free()


def test_the_statistics_of_a_table_with_dead_blocks_still_cover_the_dead_rows(loaded):
    tb, compact, every, live = loaded
    for name, lo, hi in (("k", 0, 99), ("v", -100000, 100000)):
        info = tb.column_info(name)
        assert (info["exact_min"], info["exact_max"]) == (lo, hi) and CH.exact_extrema(live, name) != (lo, hi)
    assert CH.exact_extrema(live, "only") == (I64_MAX, I64_MIN) and "ghost" not in [r.get("name") for r in D.rows_of(live)]
    rows = _rows(tb)
    assert rows == D.rows_of(live) and _from_a_live_block(rows) and len(rows) == LIVE_ROWS
    assert tb.samples(filters=[("k", "eq", 0)], limit=10).rows == [] == tb.samples(filters=[("name", "eq", "ghost")], limit=10).rows


def _dead_ref(fn, every, compact, force=None, **kw):
    """The restatement of a rollup of the table with dead blocks.  The plan reads the TRACKED extrema, which cover the dead rows:
    so the restatement is given all five blocks and a filter that only the live rows pass -- its digits, product and value bits
    are then the table's, its rows the live ones.  What the header derives from the live row count N is put right: rows_in, and
    the slots of the hash table, max(64, pow2(2 x min(N, product)))."""
    ref = fn(every, compact=compact, force=force, filters=IS_LIVE + list(kw.pop("filters", [])), **kw)
    ref["stats"]["rows_in"] = LIVE_ROWS
    if ref["stats"]["path"] == U.HASH:
        ref["stats"]["cells_or_slots"] = U.slots_for(LIVE_ROWS, ref["product"])
    return ref


@pytest.mark.parametrize("groups,force,path", [(["k", "name"], None, U.GLOBAL), (["k", "name"], "direct", U.GLOBAL), (["k", "name"], "global", U.GLOBAL),
                                               (["k", "name"], "hash", U.HASH), (["name"], None, U.LDS), (["name"], "global", U.GLOBAL), ([], None, U.LDS)])
def test_rollup_of_a_table_with_dead_blocks(loaded, monkeypatch, groups, force, path):
    tb, compact, every, live = loaded
    if force:
        monkeypatch.setenv("SYBL_ROLLUP_PATH", force)
    kw = dict(groups=groups, aggs=[("v", ALL), ("only", "n,sum"), ("row", "min,max")])
    ref = _dead_ref(U.rollup_ref, every, compact, force=force, **kw)
    plain = U.rollup_ref(live, compact=compact, force=force, **kw)
    assert D.rows_of(ref["blocks"]) == D.rows_of(plain["blocks"]) and (ref["product"] > plain["product"] or not groups)     # looser digits, the same rows
    out, st, _ = TR._check(tb, live, compact, path=path, ref=ref, **kw)
    try:
        assert st["rows_in"] == LIVE_ROWS == st["rows_matched"]
        rows = _rows(out)
        assert _from_a_live_block(rows, ("row_min", "row_max")) and sum(r["count"] for r in rows) == LIVE_ROWS
        assert all(r["only_n"] == 0 and "only_sum" not in r for r in rows) and not any(r.get("name") == "ghost" for r in rows)
        if compact:
            assert out.column_storage("only_sum") == (1, 0)
    finally:
        out.free()


@pytest.mark.parametrize("pct", [None, "32", "64", "pairs"])
def test_rollup_percentiles_of_a_table_with_dead_blocks(loaded, monkeypatch, pct):
    """p1, p50, p99 in every variant that holds the bits (13 of the cells + 18 of v's tracked span, which the dead rows widen from
    10): the direct path, whose cells do not depend on the row count."""
    tb, compact, every, live = loaded
    if pct:
        monkeypatch.setenv("SYBL_ROLLUP_PCT", pct)
    kw = dict(groups=["k", "name"], aggs=[("v", "n,p1,p50,p99"), ("only", "p50"), ("row", "min,p50")])
    ref = _dead_ref(P.rollup_pct_ref, every, compact, pct_force=pct, **kw)
    assert P.plan(ref["stats"]["cells_or_slots"], -100000, 100000)[:2] == (13, 18) and ref["pct_stats"]["key_bits_max"] == 31
    assert ref["pct_stats"]["items"] == 2 * LIVE_ROWS                   # v and row; none of `only`
    out, ps, _ = TP._check(tb, live, compact, path=U.GLOBAL, pct=pct, ref=ref, **kw)
    try:
        rows = _rows(out)
        assert _from_a_live_block(rows, ("row_min", "row_p50")) and not any("only_p50" in r for r in rows)
        assert out.rollup_stats()["rows_in"] == LIVE_ROWS
    finally:
        out.free()


def test_select_compute_and_a_rollup_of_the_select_over_dead_blocks(loaded):
    tb, compact, every, live = loaded
    # filters on the extrema only dead rows hold: the table's range admits them, no live row passes
    for filters in ([("k", "eq", 0)], [("k", "gt", 98)], [("v", "gt", 99999)], [("v", "lt", -99999)], [("only", "gt", -1)], [("name", "eq", "ghost")]):
        assert _check_select(tb, live, filters=filters) == 0
    for filters, br in (([], 0), ([("k", "lt", 25)], 33), ([("v", "gt", 0), ("name", "neq", "user7")], 7)):
        assert _check_select(tb, live, filters=filters, block_rows=br) > 0
    sel = tb.select(filters=[("k", "lt", 25)], block_rows=33)
    out = None
    try:
        sref = CH.ref_stage("select", live, {}, dict(filters=[("k", "lt", 25)], block_rows=33), compact)
        _check_table(sel, sref["blocks"], _storages(tb, ["k", "v", "only", "name", "row", "dead"]))       # the extrema are exact again
        assert _from_a_live_block(_rows(sel)) and sel.select_stats()["rows_in"] == LIVE_ROWS
        out, st, ref = TR._check(sel, sref["blocks"], compact, groups=["k", "name"], aggs=[("v", ALL), ("only", "n,sum"), ("row", "min,max")])
        assert st["rows_in"] == sel.rows and _from_a_live_block(_rows(out), ("row_min", "row_max"))
    finally:
        for t in (out, sel):
            if t is not None:
                t.free()
    exprs = [("kv", "k * 1000 + v"), ("o", "only + 1"), ("h", "has(name) + has(only) * 2 + has(k) * 4"), ("r", "row % 10000")]
    out, st, ref = TC._check(tb, live, exprs, compact)
    try:
        assert st["rows"] == LIVE_ROWS and st["blocks"] == 3 and _from_a_live_block(_rows(out))
        assert out.column_info("o")["has_missing"] and (out.column_storage("o") == (1, 0) or not compact)
    finally:
        out.free()
    assert tb.rows == LIVE_ROWS
