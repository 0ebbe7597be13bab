"""GPU: key words -- the stored offsets of a plan's group-key columns and of its aggregation 0 as bit fields of one 4-byte word
per row, read by k_scan_packed's dynamic late loop in the columns' place (Table::kwords; fword.h, table.cpp: table_build_kword,
kernels.hip: k_pack_fword, planner.cpp: plan_kword, scan_packed.h: packed_scan_dyn<KW>).  Every case is exact: bucket queries bit
for bit against the oracle, the others against a numpy group-by, and all of them field for field against the same query with
SYBL_NO_KWORD=1.

A key word is built for tables of at least SYBL_KWORD_MIN_ROWS physical rows (default 2^25); every case here sets it (and
SYBL_FWORD_MIN_ROWS, SYBL_NARROW_MIN_ROWS) to 1 and takes the dynamic kernel (SYBL_DYN=1 SYBL_DYN_MIN_TILES=1
SYBL_DYN_PIECE_TILES=2); the plan trace (SYBL_PLAN_TRACE=1: `narrow: f=word(10,10,10) k=word(4,6,20) a1=3 bytes_per_row=11`,
`key word: cols=.. bits=.. rows=.. converted=.. bytes=..`, `key word: cols=.. freed`) says what the plan reads.  Tables are sized
as tests/test_gpu_filter_word.py sizes them: 4096 * (5 * n_wg + 3) + 1234 rows, the last tile partial and not a multiple of 4.

  1. config 3's shape in the dynamic late loop, lean and not; one filter (no filter word: the filter's stored width + 4 + 3 bytes a
     row); under SYBL_NO_DYN=1, SYBL_PACKED_RING=2 and without a filter the columns, and no word is built;
  2. field lanes: 0, 1, all ones and all ones - 1 in each field under neighbours of all ones / zeros, at each of a lane's four rows
     in lane 0 and lane 63, at a tile's first and last rows and in the partial tile.  The keys ARE fields of the word, and a field's
     prescribed neighbours fix them, so a placed row cannot have a group cell of its own through them; it carries instead, in
     aggregation 1 (which is not in the word), a bit of its own among the rows of its cell, and no other row reaches these cells:
     a cell's exact sum of aggregation 1 says which placed rows arrived there, its exact sum of aggregation 0 what they carried --
     a borrowed or a lost bit changes a key (a row leaves its cell and enters another) or an exact sum;
  3. whole waves skipping a tile: tests/late_layout.py's `main` and `ragged` pass / skip sequences, failing rows with in-range keys,
     non-zero values and, in gx, a key outside its declared range (a leaked row is an overflow, which fails the query);
  4. the bit budget and the byte rule: 5 + 7 + 20 bits get a word whose top field ends at bit 31, 33 bits get none, aggregation 0
     too wide while aggregation 1 would fit gets none, one 1-byte key with a 2-byte aggregation gets none; over a positive and a
     negative value base;
  5. no word for a key or an aggregation 0 with a validity bitmap, an 8-byte aggregation, a weighted query, a time query, an
     aggregation 0 that carries outliers;
  6. neighbours: a hashed query, partitioned histograms, a select, a samples query and a pushed-down printer keep the columns;
  7. life cycle: shared by prepared queries, extended by an appended block, freed by one beyond the fields and laid out anew by the
     next prepare, evicted least recently planned first (SYBL_KWORD_MAX=1) while a prepared query keeps scanning its own share,
     counted in hbm_bytes as the word plus ONE twin, and apart from the filter words' list and cap;
  8. SYBL_NO_KWORD=1 and the default SYBL_KWORD_MIN_ROWS leave these tables on the column plan.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import late_layout as LL
from tests import parity
from tests import samples_ref

pytestmark = pytest.mark.gpu

NARROW = re.compile(r"^narrow:(.*) bytes_per_row=(\d+)$", re.M)
KWORD = re.compile(r"^key word: cols=([\w,]+) bits=([\d,]+) rows=(\d+) converted=(\d+) bytes=(\d+)$", re.M)
KFREED = re.compile(r"^key word: cols=([\w,]+) freed$", re.M)
TWIN = re.compile(r"^narrow twin: col=(\w+) rows=(\d+) converted=(\d+) bytes=(\d+)$", re.M)
NAMES = ["f1", "f2", "f3", "g1", "g2", "a1", "a2", "hk", "hj"]
INFO = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 63), "a1": (0, 999_999), "a2": (0, 999_996),
        "hk": (0, 65535), "hj": (0, 2999)}
_RANGE3 = [(c, op, v) for c in ("f1", "f2", "f3") for op, v in (("gt", 99), ("lt", 900))]
_RANGE1 = _RANGE3[:2]
Q3 = dict(filters=_RANGE3, groups=["g1", "g2"], aggs=["a1", "a2"], op="hist", want_percentiles=False)
Q1 = dict(Q3, filters=_RANGE1)
Q0 = dict(Q3, filters=[])
DYN = {"SYBL_DYN": "1", "SYBL_DYN_MIN_TILES": "1", "SYBL_DYN_PIECE_TILES": "2"}


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def small_tables_get_words(monkeypatch):
    monkeypatch.setenv("SYBL_KWORD_MIN_ROWS", "1")
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
    cols["hj"] = cols["hk"] % 3000
    for c in NAMES:   # the declared extrema occur: the stored widths and bases are the same in every table
        cols[c][0], cols[c][n - 1] = INFO[c]
    return cols


def _table(ctx, name, cols, names=NAMES, info=INFO, block=65536, bounds=None):
    n = len(cols[names[0]])
    tb = ctx.create_table(name)
    for c in names:
        tb.add_column(c, "int", *info[c])
    for r0 in range(0, n, block):
        tb.append_block(min(block, n - r0), {c: cols[c][r0:r0 + block] for c in names})
    assert tb.rows == n
    for c in names:
        tb.set_bounds(c, *(bounds or info)[c])
    tb.compact()
    return tb


def _oracle(oracle, cols, names, info, q, threads=16):
    return oracle.run_query([{"type": "int", "data": cols[c]} for c in names], block_rows=65536, n_threads=threads,
                            **parity.oracle_query_kwargs(names, info, q))


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _groupby(cols, q):
    """(matched, {key values: (count, (exact sum per aggregation))}) of the rows that pass q's range filters: a numpy int64 group-by."""
    keep = LL.keep(cols, q.get("filters", ()))
    idx = np.flatnonzero(keep)
    comp, digits = np.zeros(idx.size, dtype=np.int64), []
    for g in q["groups"]:
        v = cols[g][idx].astype(np.int64)
        lo, card = int(v.min()), int(v.max()) - int(v.min()) + 1
        comp = comp * card + (v - lo)
        digits.append((lo, card))
    order = np.argsort(comp, kind="stable")
    cs = comp[order]
    starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    counts = np.diff(np.r_[starts, cs.size])
    sums = [np.add.reduceat(cols[a][idx].astype(np.int64)[order], starts) for a in q["aggs"]]
    out = {}
    for j, s0 in enumerate(starts):
        rest, key = int(cs[s0]), []
        for lo, card in reversed(digits):
            rest, d = divmod(rest, card)
            key.append(d + lo)
        out[tuple(reversed(key))] = (int(counts[j]), tuple(int(sm[j]) for sm in sums))
    return int(keep.sum()), out


def _check_groupby(res, cols, q):
    matched, want = _groupby(cols, q)
    got = {tuple(_signed(v) for v in r["key_vals"]): (r["count"], tuple(h["sum"] for h in r["hists"][:len(q["aggs"])])) for r in res.rows(0)}
    assert res.matched == matched
    assert got == want, sorted(set(got.items()) ^ set(want.items()))[:6]
    return got


class _T:
    pass


@pytest.fixture(scope="module")
def main_table(ctx, n_wg, oracle):
    T = _T()
    T.n = 4096 * (5 * n_wg + 3) + 1234
    assert T.n % 4 == 2
    T.cols = _columns(T.n, 61)
    T.tb = _table(ctx, "kword_main", T.cols)
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
    """[(the filter word's field bits or None, the key word's field bits or None, bytes per row)] of every `narrow:` line."""
    out = []
    for what, b in NARROW.findall(err):
        f = re.search(r"f=word\(([\d,]+)\)", what)
        k = re.search(r"k=word\(([\d,]+)\)", what)
        assert not (k and " a0=" in what), what   # aggregation 0 is read from the word or at a width of its own, never both
        out.append(([int(x) for x in f[1].split(",")] if f else None, [int(x) for x in k[1].split(",")] if k else None, int(b)))
    return out


def _run(tb, q, capfd):
    capfd.readouterr()
    qy = tb.query(**q)
    res = qy.run()
    st = qy.stats()
    qy.free()
    return res, st, capfd.readouterr().err


def _check(tb, q, capfd, monkeypatch, want, ores=None, cols=None, strategy=2):
    """The query (trace: the plan in `want` = (filter word bits or None, key word bits or None, bytes per row)) bit for bit
    against the oracle (ores) or exact against a numpy group-by (cols), and against itself with SYBL_NO_KWORD=1: the same
    strategy, workgroups, replicas and algorithmic bytes, and every field equal."""
    n_aggs = len(q.get("aggs", ()))
    res, st, err = _run(tb, q, capfd)
    assert _plans(err) == [want], err[-2000:]
    assert "filter word" not in "\n".join(l for l in err.splitlines() if l.startswith("key word:"))
    assert (st["strategy"], st["packed_kernel"]) == (strategy, 1), st
    if ores is not None:
        parity.compare(res, ores, op=q.get("op", "avg"), full=q.get("want_percentiles", True), n_aggs=n_aggs)
    if cols is not None:
        _check_groupby(res, cols, q)
    got = _fields(res)
    res.free()
    monkeypatch.setenv("SYBL_NO_KWORD", "1")
    res, st0, err0 = _run(tb, q, capfd)
    monkeypatch.delenv("SYBL_NO_KWORD")
    assert [p[1] for p in _plans(err0)] == [None] and "key word:" not in err0, err0[-2000:]
    assert (st0["strategy"], st0["n_workgroups"], st0["replicas"], st0["algorithmic_bytes"]) == \
           (st["strategy"], st["n_workgroups"], st["replicas"], st["algorithmic_bytes"])
    assert _fields(res) == got
    res.free()
    return st, err


# ---------------------------------------------------------------- 1. config 3's shape
@pytest.mark.parametrize("setting", [{}, {"SYBL_NO_LEAN": "1"}], ids=["lean", "not_lean"])
def test_config3_shape_in_the_dynamic_late_loop(main_table, capfd, monkeypatch, setting):
    for k, v in setting.items():
        monkeypatch.setenv(k, v)
    st, err = _check(main_table.tb, Q3, capfd, monkeypatch, ([10, 10, 10], [4, 6, 20], 11), ores=main_table.answer("config3", Q3))
    assert "dealing: dynamic=1" in err and "k=word(4,6,20) a1=3 bytes_per_row=11" in err, err[-1000:]
    assert st["algorithmic_bytes"] == main_table.n * 16   # the table's stored bytes, as before


def test_one_filter_column_beside_a_key_word(main_table, capfd, monkeypatch):
    """NF == 1: no filter word, the filter at its stored width."""
    st, err = _check(main_table.tb, Q1, capfd, monkeypatch, (None, [4, 6, 20], 2 + 4 + 3), ores=main_table.answer("one_filter", Q1))
    assert "dealing: dynamic=1" in err, err[-1000:]


@pytest.mark.parametrize("setting", [({"SYBL_NO_DYN": "1"}, Q3, "dealing: dynamic=0"), ({"SYBL_PACKED_RING": "2", "SYBL_NO_LEAN": "1"}, Q3, "dealing: dynamic=0"),
                                     ({}, Q0, "dealing: dynamic=1")], ids=["static", "ring_of_two", "no_filter"])
def test_static_ring_and_filterless_kernels_read_the_columns(main_table, ctx, oracle, capfd, monkeypatch, setting):
    """A table of its own: no word may be BUILT for a plan that cannot read one."""
    env, q, dealing = setting
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 4096 * 3 + 5
    cols = {c: main_table.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "kword_static", cols)
    res, st, err = _run(tb, q, capfd)
    assert [p[1] for p in _plans(err)] == [None] and dealing in err and "key word:" not in err, err[-2000:]
    assert " a0=3 a1=3 " in err, err[-2000:]   # both twins: the plan of the parent
    parity.compare(res, _oracle(oracle, cols, NAMES, INFO, q, 2), op="hist", full=False, n_aggs=2)
    res.free()
    tb.free()


# ---------------------------------------------------------------- 2. field lanes
def test_field_lanes(ctx, n_wg, capfd, monkeypatch):
    n = 4096 * (5 * n_wg + 3) + 1234
    tops = (15, 63, (1 << 20) - 1)               # all ones of g1, g2 and v0: 4 + 6 + 20 bits
    rng = np.random.default_rng(62)
    combos = [(c, k) for c in range(3) for k in range(4)]   # (field, kind): kind 0: 0 under all ones, 1: 1 under all ones, 2: all ones under zeros, 3: all ones - 1 under zeros
    in_tile = [0, 1, 2, 3, 252, 253, 254, 255, 4092, 4093, 4094, 4095]   # lane 0 and lane 63 of the first wave; the last lane of the last
    special = [(4096 * j + r, combos[j]) for j in range(12) for r in in_tile]
    tail = [n - 1234, n - 1233, n - 1232, n - 1231, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1]   # the partial tile: its first lane, its ragged end
    special += [(r, combos[(5 * i) % 12]) for i, r in enumerate(tail)]
    # every other row: g1 in 2 .. 13 -- a special row's g1 is 0, 1, 14 or 15, so no other row reaches a special row's cell
    g1, g2 = rng.integers(2, 14, n), rng.integers(0, 64, n)
    v0, v1 = rng.integers(0, tops[2] + 1, n), rng.integers(0, 1000, n)
    f = rng.integers(0, 10, n)                    # the one filter: f > 0 (NF == 1)
    in_cell = {}
    for r, (c, kind) in special:
        vals = [(tops[i] if kind < 2 else 0) if i != c else (0, 1, tops[i], tops[i] - 1)[kind] for i in range(3)]
        g1[r], g2[r], v0[r], f[r] = vals[0], vals[1], vals[2], 5
        k = in_cell.setdefault((vals[0], vals[1]), [])
        v1[r] = 1 << len(k)                       # this row's own bit among the rows of its cell
        k.append(r)
    assert max(len(k) for k in in_cell.values()) <= 27 and all(g1[r] in (0, 1, 14, 15) for r, _ in special)
    g1[20], g1[21], f[20], f[21], v1[22] = 2, 13, 0, 9, 1 << 27
    names = ["f", "g1", "g2", "v0", "v1"]
    info = {"f": (0, 9), "g1": (0, 15), "g2": (0, 63), "v0": (0, tops[2]), "v1": (0, 1 << 27)}
    cols = {"f": f, "g1": g1, "g2": g2, "v0": v0, "v1": v1}
    tb = _table(ctx, "kword_lanes", cols, names, info)
    assert [tb.column_storage(c)[0] for c in names] == [1, 1, 1, 4, 4]
    q = dict(filters=[("f", "gt", 0)], groups=["g1", "g2"], aggs=["v0", "v1"], op="avg")
    st, err = _check(tb, q, capfd, monkeypatch, (None, [4, 6, 20], 1 + 4 + 4), cols=cols)   # (v1 reaches 2^27: no twin)
    assert "dealing: dynamic=1" in err, err[-1000:]
    res, st, err = _run(tb, q, capfd)
    got = {tuple(r["key_vals"]): (r["count"], r["hists"][0]["sum"], r["hists"][1]["sum"]) for r in res.rows(0)}
    res.free()
    for cell, rows in in_cell.items():            # (what _check_groupby has shown, spelled out for the placed rows)
        assert got[cell] == (len(rows), sum(int(v0[r]) for r in rows), (1 << len(rows)) - 1), (cell, got[cell])
    tb.free()


# ---------------------------------------------------------------- 3. whole waves skipping a tile
@pytest.fixture(scope="module")
def late_tables(ctx, n_wg):
    W = _T()
    W.layouts = {"main": LL.main(n_wg), "ragged": LL.ragged(n_wg)}
    W.tb = {}
    for name, layout in W.layouts.items():
        tb = ctx.create_table("kword_" + name)
        for c in LL.COLUMN_ORDER:
            tb.add_column(c, "int", *LL.INFO.get(c, (1, 0)))
        r0 = 0
        for b in layout.blocks:
            tb.append_block(b, {c: layout.cols[c][r0:r0 + b] for c in LL.COLUMN_ORDER})
            r0 += b
        for c in LL.COLUMN_ORDER:
            if c in LL.DECLARED:
                tb.set_bounds(c, *LL.DECLARED[c])
        tb.compact()
        W.tb[name] = tb
    W.refs = {}
    yield W
    for tb in W.tb.values():
        tb.free()


@pytest.mark.parametrize("filters", ["f1", "word3"])
@pytest.mark.parametrize("table", ["main", "ragged"])
def test_whole_waves_skip_a_tile(late_tables, oracle, capfd, monkeypatch, table, filters):
    """ga (2 bits), gx (8 bits: the failing rows' 200 is stored) and a4 (20 bits) in one word; a4 leads the aggregations, because a
    2-byte aggregation 0 beside two 1-byte keys costs 4 bytes today and gets no word."""
    W = late_tables
    flt, fbits = (LL.FILTERS["f1"], None) if filters == "f1" else (LL.WORD3, [8, 9, 12])
    q = dict(filters=flt, groups=["ga", "gx"], aggs=["a4", "a2b"], op="hist", want_percentiles=False, order_by=None)
    tb, cols = W.tb[table], W.layouts[table].cols
    names = ["f1", "gc", "gh", "ga", "gx", "a4", "a2b"]
    info = dict(LL.INFO, **{c: (1, 0) for c in names if c not in LL.INFO})
    ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in names], n_threads=16, **parity.oracle_query_kwargs(names, info, q))
    want = (fbits, [2, 8, 20], (1 if fbits is None else 4) + 4 + 2)     # (a2b is stored at 2 bytes: no twin)
    st, err = _check(tb, q, capfd, monkeypatch, want, ores=ores)
    ref = LL.reference(cols, q)
    assert ref["overflow"] == 0 and ref["matched"] == int(W.layouts[table].passing.sum()) >= 1
    res, st, err = _run(tb, q, capfd)
    got = {tuple(_signed(v) for v in r["key_vals"]): (r["count"], tuple(h["sum"] for h in r["hists"][:2])) for r in res.rows(0)}
    assert res.matched == ref["matched"]
    res.free()
    assert got == {k: (cnt, tuple(a[0] for a in aggs)) for k, (cnt, aggs) in ref["groups"].items()}


# ---------------------------------------------------------------- 4. the bit budget and the byte rule
BUDGET = {
    # case: (tops of key 1, key 2 (None: one key), aggregation 0, aggregation 1 (None: one aggregation); the word's bits or None)
    # (5 + 7 bits of keys are 4096 cells: with one aggregation their table fits the LDS, with two it does not)
    "32_bits": (31, 127, (1 << 20) - 1, None, [5, 7, 20]),
    "33_bits": (31, 127, (1 << 21) - 1, None, None),
    "agg0_too_wide": (15, 63, (1 << 23) - 1, (1 << 20) - 1, None),     # 4 + 6 + 23 = 33 bits; with aggregation 1 they would be 30
    "one_key_2byte_agg": (15, None, 60_000, 999, None),
}


@pytest.mark.parametrize("vbase", [7777, -5000])
@pytest.mark.parametrize("case", list(BUDGET))
def test_bit_budget_and_byte_rule(ctx, capfd, monkeypatch, vbase, case):
    k1, k2, a0, a1, bits = BUDGET[case]
    n = 4096 * 3 + 5
    rng = np.random.default_rng(63)
    keys = ["k1"] + (["k2"] if k2 is not None else [])
    aggs = ["v0"] + (["v1"] if a1 is not None else [])
    names = ["f"] + keys + aggs
    tops = {"k1": k1, "k2": k2, "v0": a0, "v1": a1}
    cols, info = {"f": rng.integers(0, 1000, n)}, {"f": (0, 999)}
    cols["f"][0], cols["f"][1] = 0, 999
    # (the base under the keys and aggregation 0, the word's columns.  Aggregation 1 starts at 0: with a negative Info.Max the
    # reference's Info.Min .. Info.Max * 10 gate rejects every value, which is not this file's subject)
    base = {c: (0 if c == "v1" else vbase) for c in names[1:]}
    for i, c in enumerate(names[1:]):
        cols[c] = base[c] + rng.integers(0, tops[c] + 1, n)
        cols[c][7 + i], cols[c][n - 2 - i] = base[c], base[c] + tops[c]
        info[c] = (base[c], base[c] + tops[c])
    cols["f"][100], cols["v0"][100] = 500, vbase + a0     # a row that passes with the last field all ones (bit 31 at 32 bits)
    for c in keys:
        cols[c][100] = vbase + 3
    tb = _table(ctx, "kword_budget", cols, names, info)
    assert [tb.column_storage(c)[1] for c in names[1:]] == [base[c] for c in names[1:]]
    q = dict(filters=[("f", "gt", 99), ("f", "lt", 900)], groups=keys, aggs=aggs, op="avg")
    widths = {c: tb.column_storage(c)[0] for c in names}
    read = lambda c: 3 if widths[c] == 4 and tops[c] < 1 << 24 else widths[c]       # (a 4-byte aggregation with a twin)
    if bits:
        want = (None, bits, 2 + 4 + sum(read(c) for c in aggs[1:]))
    else:
        want = (None, None, 2 + sum(widths[c] for c in keys) + sum(read(c) for c in aggs))
    st, err = _check(tb, q, capfd, monkeypatch, want, cols=cols)
    words = KWORD.findall(err)
    if bits is None:
        assert not words and "key word:" not in err, err[-2000:]
    else:
        assert len(words) == 1 and words[0][:2] == ("k1,k2,v0", "5,7,20") and int(words[0][2]) == int(words[0][3]) >= n, err[-2000:]
        twins = {m[0]: int(m[3]) for m in TWIN.findall(err)}
        assert set(twins) <= {"v1"}, err[-2000:]                # aggregation 0 gets no twin: nothing would read it
    tb.free()


# ---------------------------------------------------------------- 5. no word, and the result unchanged
def test_no_word_for_bitmaps_wide_weighted_time_and_outlier_queries(ctx, oracle, capfd, monkeypatch):
    n = 4096 * 3 + 5
    rng = np.random.default_rng(64)
    names = ["f", "g1", "g2", "gm", "v0", "vm", "v8", "vo", "v1", "w", "t"]
    info = {"f": (0, 999), "g1": (0, 15), "g2": (0, 63), "gm": (0, 63), "v0": (0, 999_999), "vm": (0, 999_999), "v8": (0, 1 << 40),
            "vo": (0, 500_000), "v1": (0, 999), "w": (1, 7), "t": (1, 0)}
    d = {"f": rng.integers(0, 1000, n), "g1": rng.integers(0, 16, n), "g2": rng.integers(0, 64, n), "gm": rng.integers(0, 64, n),
         "v0": rng.integers(0, 1_000_000, n), "vm": rng.integers(0, 1_000_000, n), "v8": rng.integers(0, (1 << 40) + 1, n),
         "vo": rng.integers(0, 1_000_000, n), "v1": rng.integers(0, 1000, n), "w": rng.integers(1, 8, n),
         "t": 1_700_000_000 + np.arange(n, dtype=np.int64) * 7200 // n}
    for c in names[:-1]:
        lo, hi = info[c]
        d[c][0], d[c][1] = lo, (999_999 if c == "vo" else hi)
    pop = {c: (rng.integers(0, 5, n) != 0).astype(np.uint8) for c in ("gm", "vm")}
    for p in pop.values():
        p[:2] = 1
    tb = ctx.create_table("kword_none")
    for c in names:
        tb.add_column(c, "int", *info[c])
    block = {c: d[c] for c in names}
    block.update(gm=(d["gm"], pop["gm"]), vm=(d["vm"], pop["vm"]))
    tb.append_block(n, block)
    for c in names[:-1]:
        tb.set_bounds(c, info[c][0], 999_999 if c == "vo" else info[c][1], has_missing=c in pop)
    tb.compact()
    ocols = [dict({"type": "int", "data": d[c]}, **({"populated": pop[c]} if c in pop else {})) for c in names]
    flt = [("f", "gt", 99), ("f", "lt", 900)]
    cases = [("key_bitmap", dict(filters=flt, groups=["g1", "gm"], aggs=["v0", "v1"], op="hist", want_percentiles=False)),
             ("agg0_bitmap", dict(filters=flt, groups=["g1", "g2"], aggs=["vm", "v1"], op="hist", want_percentiles=False)),
             ("agg0_8_bytes", dict(filters=flt, groups=["g1", "g2"], aggs=["v8", "v1"], op="avg")),
             ("weighted", dict(filters=flt, groups=["g1", "g2"], aggs=["v0", "v1"], op="avg", weight_col="w")),
             ("time", dict(filters=flt, groups=["g1", "g2"], aggs=["v0", "v1"], op="avg", time_col="t", time_bucket=3600)),
             ("agg0_outliers", dict(filters=flt, groups=["g1", "g2"], aggs=["vo", "v1"], op="hist", want_percentiles=False))]
    for name, q in cases:
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=2, **parity.oracle_query_kwargs(names, info, q))
        if name == "agg0_outliers":
            assert ores["cumulative"]["hists"][0]["n_outliers"] > 0
        res, st, err = _run(tb, q, capfd)
        assert "k=word" not in err and "key word:" not in err, (name, err[-2000:])
        parity.compare(res, ores, op=q["op"], full=False, n_aggs=2, time_mode=name == "time")
        res.free()
    # ... while the plain query over the populated columns of this table does get one
    res, st, err = _run(tb, dict(filters=flt, groups=["g1", "g2"], aggs=["v0", "v1"], op="avg"), capfd)
    res.free()
    assert [p[1] for p in _plans(err)] == [[4, 6, 20]] and [w[0] for w in KWORD.findall(err)] == ["g1,g2,v0"], err[-2000:]
    tb.free()


# ---------------------------------------------------------------- 6. neighbours
def test_neighbours_keep_the_stored_columns(main_table, ctx, oracle, capfd):
    """The word exists (the first query builds it); the hash path, the partitioned histograms, select, samples and a pushed-down
    printer do not read it.  A table of its own, of the size at which tests/test_gpu_filter_word.py runs them."""
    T = main_table
    n = 300_002
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "kword_neighbours", cols)
    res, st, err = _run(tb, Q3, capfd)
    res.free()
    assert _plans(err) == [([10, 10, 10], [4, 6, 20], 11)] and [w[0] for w in KWORD.findall(err)] == ["g1,g2,a1"], err[-2000:]
    for key, q, strategy in (("hashed", dict(filters=_RANGE3, groups=["hk", "hj"], aggs=["a1", "a2"], op="avg"), 7),
                             ("part_hist", dict(filters=_RANGE3, groups=["hk"], aggs=["a1"], op="hist", want_percentiles=True), 5)):
        ores = _oracle(oracle, cols, NAMES, INFO, q)
        res, st, err = _run(tb, q, capfd)
        assert st["strategy"] == strategy, (key, st)
        assert "k=word" not in err and "key word:" not in err, err[-2000:]   # no word read, built or freed
        parity.compare(res, ores, op=q["op"], full=q["op"] == "hist", n_aggs=len(q["aggs"]))
        res.free()
    # a printer whose rows beyond the limit need their Count only: the limit pushed into the scan where the plan allows it
    q = dict(groups=["hk"], aggs=["a1"], op="hist", want_percentiles=True, limit=10, printed_only=2)
    res, st, err = _run(tb, q, capfd)
    assert "k=word" not in err and "key word:" not in err, err[-2000:]
    res.free()
    hbm = tb.hbm_bytes   # (the hashed queries derive columns of their own -- dictionaries, ranks -- none of them a word: the trace)
    res, st, err = _run(tb, q, capfd)
    res.free()
    ok = LL.keep(cols, _RANGE3)
    capfd.readouterr()
    sel = tb.select(filters=_RANGE3, columns=["g1", "a1"])
    assert sel.rows == int(ok.sum())
    assert np.array_equal(sel.read_int("g1", 0, sel.rows), cols["g1"][ok]) and np.array_equal(sel.read_int("a1", 0, sel.rows), cols["a1"][ok])
    sel.free()
    blocks = [(min(65536, n - r0), {c: ("int", cols[c][r0:r0 + 65536], None) for c in ("f1", "f2", "f3", "g1", "a1")}) for r0 in range(0, n, 65536)]
    ref = samples_ref.samples_ref(blocks, filters=_RANGE3, columns=["g1", "a1"], limit=20)
    smp = tb.samples(filters=_RANGE3, columns=["g1", "a1"], limit=20)
    assert smp.rows == ref["rows"] and list(smp.row_ids) == ref["row_ids"]
    err = capfd.readouterr().err
    assert "k=word" not in err and "key word:" not in err and tb.hbm_bytes == hbm, err[-2000:]
    tb.free()


# ---------------------------------------------------------------- 7. life cycle
def test_life_cycle(ctx, capfd, monkeypatch):
    n0, n1, n2, n3 = 4096 * 5 + 1234, 4096 + 70, 100, 50
    n = n0 + n1 + n2 + n3
    rng = np.random.default_rng(65)
    names = ["f1", "f2", "f3", "g1", "g2", "g3", "v0", "v1"]
    info = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 63), "g3": (0, 63), "v0": (0, 999_999), "v1": (0, 999_996)}
    cols = {c: rng.integers(0, 1000, n) for c in names[:3]}
    cols["g1"], cols["g2"], cols["g3"] = rng.integers(0, 8, n), rng.integers(0, 64, n), rng.integers(0, 64, n)
    cols["v0"], cols["v1"] = rng.integers(0, 500_000, n), rng.integers(0, 999_997, n)
    for c in names:
        cols[c][3], cols[c][n0 - 1] = info[c][0], info[c][1]
    cols["g1"][n0 - 1] = 6                           # 3 bits in the first block ...
    cols["v0"][n0 - 1] = 500_000                     # ... and 19
    cols["g1"][n0 + 5], cols["v0"][n0 + 6] = 7, (1 << 19) - 1   # the second block reaches the largest offsets the fields hold
    cols["g1"][n0 + n1 + 7] = 8                      # the third goes one beyond g1's

    def build(name):
        tb = ctx.create_table(name)
        for c in names:
            tb.add_column(c, "int", *info[c])
        tb.append_block(n0, {c: cols[c][:n0] for c in names})
        for c in names:
            tb.set_bounds(c, *info[c])
        tb.compact()
        assert [tb.column_storage(c) for c in names] == [(2, 0)] * 3 + [(1, 0)] * 3 + [(4, 0)] * 2
        return tb

    def query(groups):
        return dict(filters=_RANGE3, groups=list(groups), aggs=["v0", "v1"], op="avg")

    def exact(res, q, rows):
        _check_groupby(res, {c: cols[c][:rows] for c in names}, q)
    A, B = ("g1", "g2"), ("g1", "g3")
    tb = build("kword_life")
    hbm0 = tb.hbm_bytes

    # two prepared queries share one word: built once, 4 bytes per reserved row, and ONE twin (aggregation 1's) beside it
    capfd.readouterr()
    qa, qb = tb.query(**query(A)), tb.query(**query(A))
    err = capfd.readouterr().err
    words, twins, fwords = KWORD.findall(err), TWIN.findall(err), re.findall(r"^filter word: cols=([\w,]+) bits", err, re.M)
    assert len(words) == 1 and words[0][:2] == ("g1,g2,v0", "3,6,19") and int(words[0][2]) == int(words[0][3]) >= n0, err[-2000:]
    assert [p[:2] for p in _plans(err)] == [([10, 10, 10], [3, 6, 19])] * 2 and fwords == ["f1,f2,f3"]
    assert [t[0] for t in twins] == ["v1"], err[-2000:]
    word_bytes, fword_bytes = int(words[0][4]), int(re.search(r"^filter word: .* bytes=(\d+)$", err, re.M)[1])
    assert word_bytes % 4 == 0 and word_bytes >= 4 * int(words[0][2])
    assert tb.hbm_bytes - hbm0 == word_bytes + int(twins[0][3]) + fword_bytes
    for qy in (qa, qb, qa):
        res = qy.run()
        exact(res, query(A), n0)
        res.free()
    qb.free()

    # SYBL_KWORD_MAX=1: a second key set evicts the first word -- qa's, which qa keeps scanning; the filter word stays
    monkeypatch.setenv("SYBL_KWORD_MAX", "1")
    monkeypatch.setenv("SYBL_FWORD_MAX", "1")
    held = tb.hbm_bytes
    res, st, err = _run(tb, query(B), capfd)
    assert [w[0] for w in KWORD.findall(err)] == ["g1,g3,v0"] and KFREED.findall(err) == ["g1,g2,v0"], err[-2000:]
    assert "filter word" not in err and _plans(err) == [([10, 10, 10], [3, 6, 19], 4 + 4 + 3)], err[-2000:]
    exact(res, query(B), n0)
    res.free()
    assert tb.hbm_bytes == held                      # one key word in, one out; the filter word neither evicted nor counted
    res = qa.run()
    exact(res, query(A), n0)
    res.free()
    qa.free()
    monkeypatch.delenv("SYBL_KWORD_MAX")
    monkeypatch.delenv("SYBL_FWORD_MAX")
    res, st, err = _run(tb, query(A), capfd)         # (default cap of 2: A's is built anew beside B's)
    res.free()
    assert [w[0] for w in KWORD.findall(err)] == ["g1,g2,v0"] and not KFREED.findall(err), err[-2000:]

    # a block inside the fields: the word is extended by that block's rows alone
    tb.append_block(n1, {c: cols[c][n0:n0 + n1] for c in names})
    res, st, err = _run(tb, query(A), capfd)
    words = KWORD.findall(err)
    assert len(words) == 1 and words[0][:2] == ("g1,g2,v0", "3,6,19") and int(words[0][2]) >= n0 + n1 and n1 <= int(words[0][3]) < n1 + 32 + 4, err[-2000:]
    assert [p[1] for p in _plans(err)] == [[3, 6, 19]] and not KFREED.findall(err)
    exact(res, query(A), n0 + n1)
    res.free()

    # a block with a key of 4 bits: the word is freed and this prepare plans on the columns ...
    tb.append_block(n2, {c: cols[c][n0 + n1:n0 + n1 + n2] for c in names})
    res, st, err = _run(tb, query(A), capfd)
    assert KFREED.findall(err) == ["g1,g2,v0"] and not KWORD.findall(err) and [p[1] for p in _plans(err)] == [None], err[-2000:]
    exact(res, query(A), n0 + n1 + n2)
    res.free()
    # ... and the next prepare lays out a new word with the fields the columns need now
    tb.append_block(n3, {c: cols[c][n0 + n1 + n2:] for c in names})
    res, st, err = _run(tb, query(A), capfd)
    words = KWORD.findall(err)
    assert len(words) == 1 and words[0][:2] == ("g1,g2,v0", "4,6,19") and int(words[0][2]) == int(words[0][3]) >= n, err[-2000:]
    exact(res, query(A), n)
    res.free()
    tb.free()


# ---------------------------------------------------------------- 8. defaults
@pytest.mark.parametrize("how", ["SYBL_NO_KWORD", "default_min_rows"])
def test_small_tables_stay_on_the_column_plan(main_table, ctx, capfd, monkeypatch, how):
    T = main_table
    n = 4096 * 3 + 5
    if how == "SYBL_NO_KWORD":
        monkeypatch.setenv("SYBL_NO_KWORD", "1")
    else:
        monkeypatch.delenv("SYBL_KWORD_MIN_ROWS")     # (SYBL_FWORD_MIN_ROWS and SYBL_NARROW_MIN_ROWS stay at 1: they do not enable key words)
        assert n < 1 << 25
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "kword_off", cols)
    hbm0 = tb.hbm_bytes
    res, st, err = _run(tb, Q3, capfd)
    res.free()
    # today's line and today's bytes: the filter word and both twins
    assert "narrow: f=word(10,10,10) a0=3 a1=3 bytes_per_row=12" in err and "key word:" not in err and "k=word" not in err, err[-2000:]
    fword_bytes = int(re.search(r"^filter word: .* bytes=(\d+)$", err, re.M)[1])
    assert tb.hbm_bytes - hbm0 == fword_bytes + sum(int(t[3]) for t in TWIN.findall(err)) and len(TWIN.findall(err)) == 2
    tb.free()
