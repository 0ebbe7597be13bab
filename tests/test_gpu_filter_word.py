"""GPU: filter words -- the stored offsets of a query's filter columns as bit fields of one 4-byte word per row, read by
k_scan_packed's dynamic loops in the columns' place (Table::fwords; fword.h, table.cpp: table_build_fword, kernels.hip:
k_pack_fword, planner.cpp: plan_fword, scan_packed.h: packed_scan_dyn<FW>) -- bit-exact against the oracle, and field for field
against the same query with SYBL_NO_FWORD=1.

A word is built for tables of at least SYBL_FWORD_MIN_ROWS physical rows (default 2^25); every case here sets it (and
SYBL_NARROW_MIN_ROWS) to 1 and takes the dynamic kernel (SYBL_DYN=1 SYBL_DYN_MIN_TILES=1 SYBL_DYN_PIECE_TILES=2); the plan trace
(SYBL_PLAN_TRACE=1: `narrow: f=word(10,10,10) a0=3 a1=3 bytes_per_row=12`, `filter word: cols=.. bits=.. rows=.. converted=..
bytes=..`, `filter word: cols=.. freed`) says what the plan reads.  Tables are sized as tests/test_gpu_narrow_twin.py sizes them:
4096 * (5 * n_wg + 3) + 1234 rows, the last tile partial and not a multiple of 4 rows.

  1. config 3's shape in the dynamic late loop, lean and not, twins on and off; without keys and aggregations (the plain dynamic
     loop); under SYBL_NO_DYN=1 and SYBL_PACKED_RING=2 the columns;
  2. field lanes: 0, 1, all ones and all ones - 1 in each field under neighbours of all ones / zeros, at each of a lane's four
     rows in lane 0 and lane 63, at a tile's first and last rows and in the partial tile, each under a key of its own, with
     bounds that a borrowed or a lost bit would cross;
  3. the bit budget: 11 + 11 + 10 bits get a word whose top field ends at bit 31, 33 bits and two 2-byte columns get none, over a
     positive and a negative value base; 4. filters in another order reuse the word, a one-sided filter and an empty range;
  5. no word for a column with a validity bitmap, a neq filter, a str filter, a single filter;
  6. neighbours: a hashed query, partitioned histograms, a select and a samples query keep the stored columns;
  7. life cycle: shared by prepared queries, extended by an appended block, freed by one beyond the fields, evicted least recently
     planned first while a prepared query keeps scanning its own share, counted in hbm_bytes;
  8. SYBL_NO_FWORD=1 and the default SYBL_FWORD_MIN_ROWS leave these tables on the column plan.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import parity
from tests import samples_ref

pytestmark = pytest.mark.gpu

NARROW = re.compile(r"^narrow:(.*) bytes_per_row=(\d+)$", re.M)
WORD = re.compile(r"^filter word: cols=([\w,]+) bits=([\d,]+) rows=(\d+) converted=(\d+) bytes=(\d+)$", re.M)
FREED = re.compile(r"^filter word: cols=([\w,]+) freed$", re.M)
NAMES = ["f1", "f2", "f3", "g1", "g2", "a1", "a2", "hk", "hj"]
INFO = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 63), "a1": (0, 999_999), "a2": (0, 999_996),
        "hk": (0, 65535), "hj": (0, 2999)}
_RANGE3 = [(c, op, v) for c in ("f1", "f2", "f3") for op, v in (("gt", 99), ("lt", 900))]
Q3 = dict(filters=_RANGE3, groups=["g1", "g2"], aggs=["a1", "a2"], op="hist", want_percentiles=False)
Q3_BARE = dict(filters=_RANGE3)
DYN = {"SYBL_DYN": "1", "SYBL_DYN_MIN_TILES": "1", "SYBL_DYN_PIECE_TILES": "2"}


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def small_tables_get_words(monkeypatch):
    monkeypatch.setenv("SYBL_FWORD_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_NARROW_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    for k, v in DYN.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def n_wg(ctx):
    tiny = ctx.create_table("probe")
    tiny.add_column("g", "int", 0, 3)
    tiny.add_column("v", "int", 0, 9)
    tiny.append_block(8, {"g": np.arange(8) % 4, "v": np.arange(8)})
    qy = tiny.query(groups=["g"], aggs=["v"])
    qy.run().free()
    n = qy.stats()["n_workgroups"]
    qy.free()
    tiny.free()
    assert 16 <= n <= 512, "n_workgroups = %d: this file is sized for one workgroup per CU of a 16..512-CU device" % n
    return n


def _columns(n, seed):
    rng = np.random.default_rng(seed)
    cols = {c: rng.integers(0, 1000, n) for c in ("f1", "f2", "f3")}
    cols["g1"] = rng.integers(0, 16, n)
    cols["g2"] = rng.integers(0, 64, n)
    cols["a1"] = rng.integers(0, 1_000_000, n)
    cols["a2"] = np.clip(rng.normal(500_000, 120_000, n).astype(np.int64), 0, 999_996)
    cols["hk"] = rng.integers(0, 65536, n)
    cols["hj"] = cols["hk"] % 3000                          # (hk, hj): a key space beyond direct mapping, 65536 distinct keys
    for c in NAMES:   # the declared extrema occur: the stored widths and bases are the same in every table
        cols[c][0], cols[c][n - 1] = INFO[c]
    return cols


def _table(ctx, name, cols, names=NAMES, info=INFO, block=65536):
    n = len(cols[names[0]])
    tb = ctx.create_table(name)
    for c in names:
        tb.add_column(c, "int", *info[c])
    for r0 in range(0, n, block):
        tb.append_block(min(block, n - r0), {c: cols[c][r0:r0 + block] for c in names})
    assert tb.rows == n
    for c in names:
        tb.set_bounds(c, *info[c])
    tb.compact()
    return tb


def _oracle(oracle, cols, names, info, q, threads=16):
    return oracle.run_query([{"type": "int", "data": cols[c]} for c in names], block_rows=65536, n_threads=threads,
                            **parity.oracle_query_kwargs(names, info, q))


class _T:
    pass


@pytest.fixture(scope="module")
def main_table(ctx, n_wg, oracle):
    T = _T()
    T.n = 4096 * (5 * n_wg + 3) + 1234
    assert T.n % 4 == 2
    T.cols = _columns(T.n, 51)
    T.tb = _table(ctx, "fword_main", T.cols)
    assert [T.tb.column_storage(c)[0] for c in NAMES[:7]] == [2, 2, 2, 1, 1, 4, 4]
    T.oracle = {}

    def answer(key, q):
        if key not in T.oracle:
            T.oracle[key] = _oracle(oracle, T.cols, NAMES, INFO, q)
        return T.oracle[key]
    T.answer = answer
    yield T
    T.tb.free()


def _fields(res):
    """Every field of every row and of Cumulative, in an order and a form that compares with ==."""
    def norm(v):
        if hasattr(v, "tolist"):
            return tuple(v.tolist())
        return repr(v) if isinstance(v, float) else v
    out = []
    for which in (0, 1, 2):
        for r in res.rows(which):
            out.append((which, r["key"], r["time_bucket"], r["count"], r["samples"],
                        tuple(tuple(sorted((k, norm(v)) for k, v in h.items())) for h in r["hists"])))
    return res.matched, sorted(out)


def _plans(err):
    """[(the word's field bits per filter or None, bytes per row)] of every `narrow:` line."""
    out = []
    for what, b in NARROW.findall(err):
        m = re.search(r"f=word\(([\d,]+)\)", what)
        out.append(([int(x) for x in m[1].split(",")] if m else None, int(b)))
    return out


def _run(tb, q, capfd):
    capfd.readouterr()
    qy = tb.query(**q)
    res = qy.run()
    st = qy.stats()
    qy.free()
    return res, st, capfd.readouterr().err


def _check(tb, q, ores, capfd, monkeypatch, want, strategy=2):
    """The query (trace: the plan in `want` = (field bits or None, bytes per row)) against the oracle, and against itself with
    SYBL_NO_FWORD=1: the same strategy, workgroups, replicas and algorithmic bytes, and every field equal."""
    n_aggs = len(q.get("aggs", ()))
    res, st, err = _run(tb, q, capfd)
    assert _plans(err) == [want], err[-2000:]
    assert (st["strategy"], st["packed_kernel"]) == (strategy, 1), st
    parity.compare(res, ores, op=q.get("op", "avg"), full=q.get("want_percentiles", True), n_aggs=n_aggs)
    got = _fields(res)
    res.free()
    monkeypatch.setenv("SYBL_NO_FWORD", "1")
    res, st0, err0 = _run(tb, q, capfd)
    monkeypatch.delenv("SYBL_NO_FWORD")
    assert [p[0] for p in _plans(err0)] == [None] and not WORD.findall(err0), err0[-2000:]
    assert (st0["strategy"], st0["n_workgroups"], st0["replicas"], st0["algorithmic_bytes"]) == \
           (st["strategy"], st["n_workgroups"], st["replicas"], st["algorithmic_bytes"])
    assert _fields(res) == got
    res.free()
    return st, err


# ---------------------------------------------------------------- 1. config 3's shape
SETTINGS = [("lean", {}, 12), ("not_lean", {"SYBL_NO_LEAN": "1"}, 12), ("lean_no_twins", {"SYBL_NO_NARROW": "1"}, 14),
            ("not_lean_no_twins", {"SYBL_NO_LEAN": "1", "SYBL_NO_NARROW": "1"}, 14)]


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_config3_shape_in_the_dynamic_late_loop(main_table, capfd, monkeypatch, setting):
    for k, v in setting[1].items():
        monkeypatch.setenv(k, v)
    st, err = _check(main_table.tb, Q3, main_table.answer("config3", Q3), capfd, monkeypatch, ([10, 10, 10], setting[2]))
    assert "dealing: dynamic=1" in err, err[-1000:]
    assert st["algorithmic_bytes"] == main_table.n * 16   # the table's stored bytes, as before


def test_config3_filters_alone_in_the_plain_dynamic_loop(main_table, capfd, monkeypatch):
    st, err = _check(main_table.tb, Q3_BARE, main_table.answer("bare", Q3_BARE), capfd, monkeypatch, ([10, 10, 10], 4))
    assert "dealing: dynamic=1" in err, err[-1000:]


@pytest.mark.parametrize("setting", [{"SYBL_NO_DYN": "1"}, {"SYBL_PACKED_RING": "2", "SYBL_NO_LEAN": "1"}], ids=["static", "ring_of_two"])
def test_static_and_ring_kernels_read_the_columns(main_table, ctx, capfd, monkeypatch, setting):
    """A table of its own: no word may be BUILT for a plan that cannot read one."""
    for k, v in setting.items():
        monkeypatch.setenv(k, v)
    T = main_table
    res, st, err = _run(T.tb, Q3, capfd)
    assert _plans(err) == [(None, 14)] and "dealing: dynamic=0" in err, err[-2000:]
    parity.compare(res, T.answer("config3", Q3), op="hist", full=False, n_aggs=2)
    res.free()
    n = 4096 * 3 + 5
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "fword_static", cols)
    hbm = tb.hbm_bytes
    res, st, err = _run(tb, dict(filters=_RANGE3, groups=["g1", "g2"]), capfd)   # (no aggregation: no twin either, hbm_bytes must not move)
    res.free()
    assert not WORD.findall(err) and "f=word" not in err and tb.hbm_bytes == hbm, err[-2000:]
    tb.free()


# ---------------------------------------------------------------- 2. field lanes
def test_field_lanes(ctx, n_wg, oracle, capfd, monkeypatch):
    n = 4096 * (5 * n_wg + 3) + 1234
    top = 1023
    rng = np.random.default_rng(52)
    # combination j of (field, kind) lives in tile j: kind 0: field = 0 under neighbours of all ones, 1: field = 1 under all ones,
    # 2: field = all ones under zeros, 3: field = all ones - 1 under zeros
    combos = [(c, k) for c in range(3) for k in range(4)]
    in_tile = [0, 1, 2, 3, 252, 253, 254, 255, 4092, 4093, 4094, 4095]   # lane 0 and lane 63 of the first wave; the last lane of the last
    special = [(4096 * j + r, combos[j]) for j in range(12) for r in in_tile]
    tail = [n - 1234, n - 1233, n - 1232, n - 1231, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1]   # the partial tile: its first lane, its ragged end
    special += [(r, combos[(5 * i) % 12]) for i, r in enumerate(tail)]
    assert len(special) < 256
    f = [rng.integers(1, top, n) for _ in range(3)]           # 1 .. all ones - 1: every other row passes every query below
    key = np.zeros(n, dtype=np.int64)
    val = rng.integers(0, 1000, n)
    for j, (r, (c, kind)) in enumerate(special):
        key[r] = j + 1
        for i in range(3):
            f[i][r] = (top if kind < 2 else 0) if i != c else (0, 1, top, top - 1)[kind]
    f[0][8], f[1][9], f[2][10] = 0, 0, 0   # (the declared minimum occurs outside the special rows too)
    f[0][12], f[1][13], f[2][14] = top, top, top
    names = ["f1", "f2", "f3", "key", "val"]
    info = {"f1": (0, top), "f2": (0, top), "f3": (0, top), "key": (0, 255), "val": (0, 999)}
    cols = {"f1": f[0], "f2": f[1], "f3": f[2], "key": key, "val": val}
    tb = _table(ctx, "fword_lanes", cols, names, info)
    assert [tb.column_storage(c)[0] for c in names] == [2, 2, 2, 1, 2]
    queries = [[(c, "gt", 0) for c in names[:3]],                                        # >= 1: a bit borrowed from a neighbour of all ones passes a 0
               [(c, "lt", top) for c in names[:3]],                                      # <= all ones - 1: a lost bit passes all ones
               [(c, op, v) for c in names[:3] for op, v in (("gt", 0), ("lt", top))]]
    for filters in queries:
        q = dict(filters=filters, groups=["key"], aggs=["val"], op="avg")
        ores = _oracle(oracle, cols, names, info, q)
        res, st, err = _run(tb, q, capfd)
        assert _plans(err) == [([10, 10, 10], 4 + 1 + 2)] and "dealing: dynamic=1" in err, err[-2000:]
        parity.compare(res, ores, op="avg", full=True, n_aggs=1)
        got = {r["key"][0]: (r["count"], r["hists"][0]["sum"]) for r in res.rows(0)}
        res.free()
        ok = np.ones(n, dtype=bool)
        for c, op, v in filters:
            ok &= (cols[c] > v) if op == "gt" else (cols[c] < v)
        want = {j + 1: (1, int(val[r])) for j, (r, _) in enumerate(special) if ok[r]}
        assert {k: v for k, v in got.items() if k != 0} == want
        if len(filters) == 3:
            assert 0 < len(want) < len(special)   # (some special rows pass and some fail under the one-sided bounds)
    tb.free()


# ---------------------------------------------------------------- 3. the bit budget, 4. filter order and one-sided / empty ranges
@pytest.mark.parametrize("vbase", [7777, -5000])
@pytest.mark.parametrize("tops", [(2047, 2047, 1023), (2047, 2047, 2047), (2047, 2047)], ids=["32_bits", "33_bits", "two_columns"])
def test_bit_budget_and_filter_order(ctx, oracle, capfd, monkeypatch, vbase, tops):
    n = 4096 * 3 + 5
    rng = np.random.default_rng(53)
    names = ["f%d" % (i + 1) for i in range(len(tops))] + ["g", "v"]
    cols, info = {}, {}
    for i, top in enumerate(tops):
        c = names[i]
        cols[c] = vbase + rng.integers(0, top + 1, n)
        cols[c][7 + i], cols[c][n - 2 - i] = vbase, vbase + top
        info[c] = (vbase, vbase + top)
    cols["g"], info["g"] = rng.integers(0, 16, n), (0, 15)
    cols["v"], info["v"] = rng.integers(0, 1000, n), (0, 999)
    cols["g"][0], cols["g"][1], cols["v"][0], cols["v"][1] = 0, 15, 0, 999
    # a row that passes with the last column at its largest value (bit 31 of the word when the budget is 32 bits)
    for i, top in enumerate(tops):
        cols[names[i]][100] = vbase + (top if i == len(tops) - 1 else 100)
    tb = _table(ctx, "fword_budget", cols, names, info)
    assert [tb.column_storage(c) for c in names[:len(tops)]] == [(2, vbase)] * len(tops)
    fcols = names[:len(tops)]
    bits = [11, 11, 10] if tops == (2047, 2047, 1023) else None
    filters = [(c, op, v) for c, top in zip(fcols, tops) for op, v in (("gt", vbase + 9), ("lt", vbase + top - 9))]
    filters[-1] = (fcols[-1], "lt", vbase + tops[-1] + 1)   # (the last column's largest value passes)
    q = dict(filters=filters, groups=["g"], aggs=["v"], op="avg")
    hbm0 = tb.hbm_bytes
    st, err = _check(tb, q, _oracle(oracle, cols, names, info, q, 2), capfd, monkeypatch, (bits, 4 + 1 + 2 if bits else 2 * len(tops) + 1 + 2))
    words = WORD.findall(err)
    if bits is None:
        assert not words and tb.hbm_bytes == hbm0
        tb.free()
        return
    assert len(words) == 1 and words[0][:2] == ("f1,f2,f3", "11,11,10") and int(words[0][2]) == int(words[0][3]) >= n, err[-2000:]
    assert tb.hbm_bytes - hbm0 == int(words[0][4]) >= 4 * int(words[0][2])
    # 4. the same filters in another order: the same word (nothing converted), this plan's fields in its own order
    q = dict(q, filters=[f for c in reversed(fcols) for f in filters if f[0] == c])
    st, err = _check(tb, q, _oracle(oracle, cols, names, info, q, 2), capfd, monkeypatch, ([10, 11, 11], 7))
    assert not WORD.findall(err), err[-2000:]
    # a one-sided filter, and a range nothing passes (plo > phi)
    for filters in ([("f1", "gt", vbase + 500), ("f3", "gt", vbase + 1000)],
                    [("f1", "gt", vbase + 900), ("f1", "lt", vbase + 100), ("f2", "gt", vbase + 5), ("f3", "lt", vbase + 1000)]):
        q = dict(q, filters=filters)
        ores = _oracle(oracle, cols, names, info, q, 2)
        res, st, err = _run(tb, q, capfd)
        parity.compare(res, ores, op="avg", full=True, n_aggs=1)
        got = _fields(res)
        res.free()
        monkeypatch.setenv("SYBL_NO_FWORD", "1")
        res, st0, err0 = _run(tb, q, capfd)
        monkeypatch.delenv("SYBL_NO_FWORD")
        assert _fields(res) == got and "f=word" not in err0
        res.free()
    assert tb.hbm_bytes - hbm0 <= 2 * int(words[0][4])   # (f1,f3 is a set of its own: at most one more word, never a third)
    tb.free()


# ---------------------------------------------------------------- 5. no word, and the result unchanged
def test_no_word_for_bitmaps_neq_str_and_single_filters(ctx, oracle, capfd, monkeypatch):
    n = 4096 * 3 + 5
    rng = np.random.default_rng(54)
    vocab = ["w%03d" % i for i in range(300)]
    ints = ["f1", "f2", "f3", "fm", "v"]
    d = {c: rng.integers(0, 1000, n) for c in ints}
    fs = rng.integers(0, 300, n).astype(np.int32)
    g = rng.integers(0, 16, n)
    pop = (rng.integers(0, 5, n) != 0).astype(np.uint8)
    for c in ints:
        d[c][0], d[c][1] = 0, 999
    pop[:2] = 1
    g[0], g[1], fs[0], fs[1] = 0, 15, 0, 299
    tb = ctx.create_table("fword_none")
    for c in ints:
        tb.add_column(c, "int", 0, 999)
    tb.add_column("fs", "str")
    tb.add_column("g", "int", 0, 15)
    block = {c: d[c] for c in ints}
    block.update(fm=(d["fm"], pop), fs={"ids": fs, "strings": vocab}, g=g)
    tb.append_block(n, block)
    for c in ints:
        tb.set_bounds(c, 0, 999, has_missing=(c == "fm"))
    tb.set_bounds("g", 0, 15)
    tb.compact()
    assert [tb.column_storage(c)[0] for c in ("f1", "f2", "f3", "fm", "fs")] == [2, 2, 2, 2, 2]
    order = ints + ["fs", "g"]   # the oracle's column indices
    ocols = [{"type": "int", "data": d[c]} for c in ints] + [{"type": "str", "data": fs}, {"type": "int", "data": g}]
    ocols[3]["populated"] = pop
    rng2 = [("gt", 99), ("lt", 900)]
    idt = np.array([bool(re.search("^w0[0-4]", s)) for s in vocab], dtype=np.uint8)
    two = [(c, op, x) for c in ("f1", "f2") for op, x in rng2]
    cases = [("bitmap", two + [("fm", op, x) for op, x in rng2], None),
             ("neq", two + [("f3", "neq", 5), ("f3", "lt", 990)], None),
             ("str", two + [("fs", "re", "^w0[0-4]")], two + [("fs", "re", 0, idt)]),
             ("single", [("f1", op, x) for op, x in rng2], None)]
    hbm = tb.hbm_bytes
    for name, filters, ofilters in cases:
        ofilters = [(order.index(f[0]),) + tuple(f[1:]) for f in (ofilters or filters)]
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=2, filters=ofilters, groups=[order.index("g")],
                                aggs=[(order.index("v"), 0, 999)], op="avg")
        res, st, err = _run(tb, dict(filters=filters, groups=["g"], aggs=["v"], op="avg"), capfd)
        assert "f=word" not in err and not WORD.findall(err), (name, err[-2000:])
        parity.compare(res, ores, op="avg", full=True, n_aggs=1)
        res.free()
    assert tb.hbm_bytes == hbm
    # ... while three plain ranges over the populated columns of this table do get one
    res, st, err = _run(tb, dict(filters=two + [("f3", op, x) for op, x in rng2], groups=["g"], aggs=["v"], op="avg"), capfd)
    res.free()
    assert _plans(err) == [([10, 10, 10], 4 + 1 + 2)] and len(WORD.findall(err)) == 1, err[-2000:]
    tb.free()


# ---------------------------------------------------------------- 6. neighbours
def test_neighbours_keep_the_stored_columns(main_table, ctx, oracle, capfd):
    """The word exists (the first query builds it); the hash path, the partitioned histograms, select and samples do not read it.  A
    table of its own, of the size at which tests/test_gpu_compact.py runs config 4: 65 536 groups are what these answers cost to check."""
    T = main_table
    n = 300_002
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "fword_neighbours", cols)
    res, st, err = _run(tb, Q3, capfd)
    res.free()
    assert _plans(err) == [([10, 10, 10], 12)] and [w[0] for w in WORD.findall(err)] == ["f1,f2,f3"], err[-2000:]
    for key, q, strategy in (("hashed", dict(filters=_RANGE3, groups=["hk", "hj"], aggs=["a1", "a2"], op="avg"), 7),
                             ("part_hist", dict(filters=_RANGE3, groups=["hk"], aggs=["a1"], op="hist", want_percentiles=True), 5)):
        ores = _oracle(oracle, cols, NAMES, INFO, q)
        res, st, err = _run(tb, q, capfd)
        assert st["strategy"] == strategy, (key, st)
        assert "f=word" not in err and "filter word" not in err, err[-2000:]   # no word read, built or freed
        parity.compare(res, ores, op=q["op"], full=q["op"] == "hist", n_aggs=len(q["aggs"]))
        res.free()
    hbm = tb.hbm_bytes   # (the hashed queries derive columns of their own -- dictionaries, ranks -- none of them a word: the trace)
    ok = np.ones(n, dtype=bool)
    for c, op, v in _RANGE3:
        ok &= (cols[c] > v) if op == "gt" else (cols[c] < v)
    capfd.readouterr()
    sel = tb.select(filters=_RANGE3, columns=["f2", "a1"])
    assert sel.rows == int(ok.sum())
    assert np.array_equal(sel.read_int("f2", 0, sel.rows), cols["f2"][ok]) and np.array_equal(sel.read_int("a1", 0, sel.rows), cols["a1"][ok])
    sel.free()
    blocks = [(min(65536, n - r0), {c: ("int", cols[c][r0:r0 + 65536], None) for c in ("f1", "f2", "f3", "a1")}) for r0 in range(0, n, 65536)]
    ref = samples_ref.samples_ref(blocks, filters=_RANGE3, columns=["f1", "f3", "a1"], limit=20)
    smp = tb.samples(filters=_RANGE3, columns=["f1", "f3", "a1"], limit=20)
    assert smp.rows == ref["rows"] and list(smp.row_ids) == ref["row_ids"]
    err = capfd.readouterr().err
    assert "f=word" not in err and "filter word" not in err and tb.hbm_bytes == hbm, err[-2000:]
    tb.free()


# ---------------------------------------------------------------- 7. life cycle
def test_life_cycle(ctx, oracle, capfd, monkeypatch):
    n0, n1, n2 = 4096 * 5 + 1234, 4096 + 70, 100
    n = n0 + n1 + n2
    rng = np.random.default_rng(55)
    names = ["f1", "f2", "f3", "f4", "g", "v"]
    info = {"f1": (0, 60000), "f2": (0, 60000), "f3": (0, 60000), "f4": (0, 60000), "g": (0, 15), "v": (0, 999)}
    cols = {c: rng.integers(0, 1000, n) for c in names[:4]}
    cols["g"], cols["v"] = rng.integers(0, 16, n), rng.integers(0, 1000, n)
    for c in names[:4]:
        cols[c][3], cols[c][n0 - 1] = 0, 1000       # 10 bits a field in the first block
    cols["f1"][n0 + 5] = 1023                       # the second block reaches the largest offset the field holds
    cols["f1"][n0 + n1 + 7] = 1024                  # the third goes one beyond it
    cols["g"][0], cols["g"][1], cols["v"][0], cols["v"][1] = 0, 15, 0, 999

    def build(name):
        tb = ctx.create_table(name)
        for c in names:
            tb.add_column(c, "int", *info[c])
        tb.append_block(n0, {c: cols[c][:n0] for c in names})
        for c in names:
            tb.set_bounds(c, *info[c])
        tb.compact()
        assert [tb.column_storage(c) for c in names[:4]] == [(2, 0)] * 4
        return tb

    def query(fcols):
        return dict(filters=[(c, op, x) for c in fcols for op, x in (("gt", 99), ("lt", 900))], groups=["g"], aggs=["v"], op="avg")

    def answer(q, rows):
        return _oracle(oracle, {c: cols[c][:rows] for c in names}, names, info, q, 2)
    A, B, C = ("f1", "f2", "f3"), ("f1", "f2", "f4"), ("f2", "f3", "f4")
    tb = build("fword_life")
    monkeypatch.setenv("SYBL_NO_FWORD", "1")
    plain = build("fword_life_plain")     # the same table without a word: what hbm_bytes is without one
    monkeypatch.delenv("SYBL_NO_FWORD")
    assert tb.hbm_bytes == plain.hbm_bytes

    # two prepared queries share one word: built once, 4 bytes per reserved row
    capfd.readouterr()
    qa, qb = tb.query(**query(A)), tb.query(**query(A))
    err = capfd.readouterr().err
    words = WORD.findall(err)
    assert len(words) == 1 and words[0][:2] == ("f1,f2,f3", "10,10,10") and int(words[0][2]) == int(words[0][3]) >= n0, err[-2000:]
    assert [p[0] for p in _plans(err)] == [[10, 10, 10]] * 2
    word_bytes = tb.hbm_bytes - plain.hbm_bytes
    assert word_bytes == int(words[0][4]) and word_bytes % 4 == 0 and word_bytes >= 4 * int(words[0][2])
    ans_a = answer(query(A), n0)
    for qy in (qa, qb, qa):
        res = qy.run()
        parity.compare(res, ans_a, op="avg", full=True, n_aggs=1)
        res.free()
    qb.free()

    # SYBL_FWORD_MAX=2: a third filter set evicts the least recently planned word -- qa's, which qa keeps scanning
    monkeypatch.setenv("SYBL_FWORD_MAX", "2")
    res, st, err = _run(tb, query(B), capfd)
    res.free()
    assert [w[0] for w in WORD.findall(err)] == ["f1,f2,f4"] and not FREED.findall(err), err[-2000:]
    assert tb.hbm_bytes - plain.hbm_bytes == 2 * word_bytes
    res, st, err = _run(tb, query(C), capfd)
    assert [w[0] for w in WORD.findall(err)] == ["f2,f3,f4"] and FREED.findall(err) == ["f1,f2,f3"], err[-2000:]
    parity.compare(res, answer(query(C), n0), op="avg", full=True, n_aggs=1)
    res.free()
    assert tb.hbm_bytes - plain.hbm_bytes == 2 * word_bytes
    res = qa.run()
    parity.compare(res, ans_a, op="avg", full=True, n_aggs=1)
    res.free()
    qa.free()
    # ... and planning A again builds it anew, evicting B's (C's was planned after it)
    res, st, err = _run(tb, query(A), capfd)
    res.free()
    assert [w[0] for w in WORD.findall(err)] == ["f1,f2,f3"] and FREED.findall(err) == ["f1,f2,f4"], err[-2000:]
    assert tb.hbm_bytes - plain.hbm_bytes == 2 * word_bytes

    # a block inside the fields: the word is extended by that block's rows alone
    for t in (tb, plain):
        t.append_block(n1, {c: cols[c][n0:n0 + n1] for c in names})
    res, st, err = _run(tb, query(A), capfd)
    words = WORD.findall(err)
    assert len(words) == 1 and words[0][:2] == ("f1,f2,f3", "10,10,10") and int(words[0][2]) >= n0 + n1 and n1 <= int(words[0][3]) < n1 + 32 + 4, err[-2000:]
    assert _plans(err) == [([10, 10, 10], 7)] and not FREED.findall(err)
    parity.compare(res, answer(query(A), n0 + n1), op="avg", full=True, n_aggs=1)
    res.free()

    # a block with an offset of 11 bits: the word is freed and this prepare plans on the columns
    for t in (tb, plain):
        t.append_block(n2, {c: cols[c][n0 + n1:] for c in names})
    held = tb.hbm_bytes - plain.hbm_bytes
    res, st, err = _run(tb, query(A), capfd)
    assert FREED.findall(err) == ["f1,f2,f3"] and not WORD.findall(err) and _plans(err) == [(None, 9)], err[-2000:]
    parity.compare(res, answer(query(A), n), op="avg", full=True, n_aggs=1)
    res.free()
    assert held - (tb.hbm_bytes - plain.hbm_bytes) >= 4 * (n0 + n1)   # its bytes are returned
    tb.free()
    plain.free()


# ---------------------------------------------------------------- 8. defaults
@pytest.mark.parametrize("how", ["SYBL_NO_FWORD", "default_min_rows"])
def test_small_tables_stay_on_the_column_plan(main_table, ctx, capfd, monkeypatch, how):
    T = main_table
    n = 4096 * 3 + 5
    if how == "SYBL_NO_FWORD":
        monkeypatch.setenv("SYBL_NO_FWORD", "1")
    else:
        monkeypatch.delenv("SYBL_FWORD_MIN_ROWS")
        assert n < 1 << 25
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "fword_off", cols)
    res, st, err = _run(tb, Q3, capfd)   # (the twins are built here, whatever the word does)
    res.free()
    hbm = tb.hbm_bytes
    for q in (Q3, Q3_BARE):
        res, st, err = _run(tb, q, capfd)
        assert [p[0] for p in _plans(err)] == [None] and "dealing: dynamic=1" in err and not WORD.findall(err), err[-2000:]
        res.free()
    assert tb.hbm_bytes == hbm
    tb.free()
