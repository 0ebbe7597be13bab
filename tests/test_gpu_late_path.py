"""GPU: the late-materialisation kernels where whole waves skip a tile.

Four kernel families read the filter columns a tile ahead and request the key, value and time columns of a tile only when some
row of the wave's 256-row window passed: k_scan_hash_packed<.., LATE> hashed (`hash_packed`) and direct-mapped with run-time
column counts (`packed_n`; csrc/hashpacked.hip), k_count_packed / k_emit_packed<.., LATE> (`count_emit`) and k_scan_packed's
late loop (`packed`; csrc/scan_packed.h).  What defines them is a wave that skips tile t and then needs t + 1 while its
neighbours in the workgroup do the opposite: the zero-record descriptor, the hand-over of the predicate bits across a skipped
tile, registers left over from the tile before.  The tables of tests/late_layout.py PLACE that -- all sixteen pass / skip
sequences of four tiles in every workgroup, five positions of the passing rows inside a window, ragged and one-tile tables --
and its failing rows carry keys and values that change the answer when accumulated, one key column (gx) outside its declared
range, so that a leaked row fails the query as an overflow.  tests/test_late_layout.py checks the placement on the CPU.

Every case runs with SYBL_LATE_PATH=1, =0 and unset: each against the numpy group-by of late_layout.reference (count, sum, min,
max per group, `matched`, the number of groups; the overflow count is zero or the query fails), hist queries against the CPU
oracle too (parity.compare), and the two forced runs equal field for field.  Which kernel ran is read from the planner's
`late path:` trace line (SYBL_PLAN_TRACE=1); the last test of the file asserts that every family ran in LATE form.

The estimate (FastPlan::late, planner.cpp: fill_packed; "below 0.5 %" in DESIGN 3.6) is pinned on a 200 000-row table with an
exactly uniform filter column: 0.4 % takes the late form, 0.5 % does not, two filters of 7 % do, and with a neq beside them the
NUL body -- which has no late form -- runs.

Not covered: the NUL variants and the canonical-storage kernels (no late form: asserted for the canonical copy only), multi-rank.
The columns are built once per module (numpy: about as long as the scans of all cases together).
"""
import contextlib
import re
import types

import numpy as np
import pytest

import sybil_amd
from tests import late_layout as LL
from tests import parity

pytestmark = pytest.mark.gpu

LATE_LINE = re.compile(r"late path: kernel=(\w+) late=(\d) estimate=(\S+)")
HASH_LINE = re.compile(r"hash tables: slots=(\d+) staging=(\d+) words_per_slot=(\d+) kernel=(\w+) late=(\d)")
SEEN = {}            # (kernel family, late) -> the first trace line that showed it, over the whole file
WAYS3 = ("1", "0", None)
WAYS2 = ("1", "0")


def _q(**kw):
    return dict(dict(op="avg", want_percentiles=False, order_by=None), **kw)      # (order_by None: canonical key order)


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _env(monkeypatch, unset=(), **kv):
    with monkeypatch.context() as m:
        for k in unset:
            m.delenv(k, raising=False)
        for k, v in kv.items():
            m.setenv(k, v)
        yield


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _build(ctx, layout, compact=True, columns=LL.COLUMN_ORDER):
    tb = ctx.create_table(layout.name)
    for c in columns:
        tb.add_column(c, "int", *LL.INFO.get(c, (1, 0)))
    r0 = 0
    for b in layout.blocks:
        tb.append_block(b, {c: layout.cols[c][r0:r0 + b] for c in columns})
        r0 += b
    for c in columns:
        if c in LL.DECLARED:
            tb.set_bounds(c, *LL.DECLARED[c])
    if compact:
        tb.compact()
    return tb


@pytest.fixture(scope="module")
def world(ctx):
    """The workgroup count of the device (one workgroup per CU: stats()["n_workgroups"] of a first query), then every table."""
    W = types.SimpleNamespace(layouts={}, tb={}, refs={}, oracles={})
    probe = LL.tiny(LL.TINY_ROWS[-1])
    ptb = _build(ctx, probe)
    qy = ptb.query(**_q(groups=["ga"], aggs=["a1"]))
    qy.run().free()
    W.n_wg = qy.stats()["n_workgroups"]
    qy.free()
    ptb.free()
    for layout in [LL.main(W.n_wg), LL.ragged(W.n_wg)] + [LL.tiny(r) for r in LL.TINY_ROWS]:
        W.layouts[layout.name] = layout
        W.tb[layout.name] = _build(ctx, layout)
    m = W.tb["main"]
    for c, nbytes in LL.STORED_BYTES.items():       # the widths the layout promises, as stored
        assert m.column_storage(c)[0] == nbytes, (c, m.column_storage(c))
    yield W
    for tb in W.tb.values():
        tb.free()


# ---------------------------------------------------------------------------------------------- running and checking
def _traced(tb, q, capfd, monkeypatch, late, env):
    """prepare + scan + finalize under the plan trace: (result or None, error text or None, stats, trace)."""
    e = dict(env, SYBL_PLAN_TRACE="1")
    if late is not None:
        e["SYBL_LATE_PATH"] = late
    with _env(monkeypatch, unset=("SYBL_LATE_PATH",), **e):
        capfd.readouterr()
        qy = tb.query(**q)
        res = err = None
        try:
            try:
                res = qy.run()
            except sybil_amd.SyblError as ex:
                err = str(ex)
            st = qy.stats()
        finally:
            qy.free()
        text = capfd.readouterr().err
    lines = [(k, int(l), float(s)) for k, l, s in LATE_LINE.findall(text)]
    hashed = [(k, int(l)) for _, _, _, k, l in HASH_LINE.findall(text)]
    for k, l, s in lines:
        SEEN.setdefault((k, l), "late path: kernel=%s late=%d estimate=%g  [%s %s]" % (k, l, s, tb.name, q.get("groups")))
    return res, err, st, types.SimpleNamespace(lines=lines, hashed=hashed, text=text)


def _check_numpy(res, ref, q, what):
    """Every group of the reference and no other: Count, each aggregation's count, sum, min and max; `matched`; Cumulative.
    BasicHist.Min / Max start at 0 in avg mode and at Info.Min / Info.Max in hist mode (hist_basic.go:34-40)."""
    time_mode = bool(q.get("time_col"))
    rows = res.rows(1 if time_mode else 0, want_values=False)
    got = {}
    for r in rows:
        key = tuple(_signed(v) for v in r["key_vals"])
        got[((r["time_bucket"],) + key) if time_mode else key] = r
    assert ref["overflow"] == 0, what
    assert res.matched == ref["matched"], (what, res.matched, ref["matched"])
    assert len(rows) == len(got) == len(ref["groups"]), (what, len(rows), len(got), len(ref["groups"]))
    assert set(got) == set(ref["groups"]), (what, sorted(set(got) ^ set(ref["groups"]))[:8])
    bad = []
    for key, (count, aggs) in ref["groups"].items():
        g = got[key]
        if g["count"] != count:
            bad.append((key, "count", g["count"], count))
        for a, (name, (total, lo, hi)) in enumerate(zip(q["aggs"], aggs)):
            h = g["hists"][a]
            start = LL.INFO[name] if q["op"] == "hist" else (0, 0)
            if not h["present"] or (h["count"], h["sum"]) != (count, total):
                bad.append((key, name, "sum", h["present"], h["count"], h["sum"], count, total))
            if (h["min"], h["max"]) != (min(lo, start[0]), max(hi, start[1])):
                bad.append((key, name, "extrema", h["min"], h["max"], lo, hi))
            if abs(h["avg"] - total / count) > parity.REL * max(abs(total / count), 1.0):
                bad.append((key, name, "avg", h["avg"], total / count))
    assert not bad, (what, len(bad), bad[:6])
    c = res.cumulative
    inside = sum(cnt for cnt, _ in ref["groups"].values())
    assert c["count"] == inside == ref["matched"], (what, c["count"], inside)
    if not time_mode:
        for a in range(len(q["aggs"])):
            grand = sum(aggs[a][0] for _, aggs in ref["groups"].values())
            assert (c["hists"][a]["count"], c["hists"][a]["sum"]) == (inside, grand), (what, a)


def _oracle_ref(W, oracle, table, q):
    cols = W.layouts[table].cols
    names = list(dict.fromkeys(list(q.get("groups", [])) + list(q["aggs"]) + [f[0] for f in q.get("filters", [])] +
                               ([q["time_col"]] if q.get("time_col") else [])))
    ocols = [{"type": "int", "data": cols[c]} for c in names]
    return oracle.run_query(ocols, n_threads=16, want_values=bool(q.get("want_percentiles")), **parity.oracle_query_kwargs(names, LL.INFO, q))


def _snapshot(res, time_mode):
    """Everything a result says, in the order it says it, floats bit for bit: what the forced runs must agree on."""
    def row(r):
        return (r["key"], r["time_bucket"], r["count"], r["samples"],
                tuple(tuple((k, v.hex() if isinstance(v, float) else (v.tobytes() if isinstance(v, np.ndarray) else v)) for k, v in h.items())
                      for h in r["hists"]))
    return (res.matched, [[row(r) for r in res.rows(w)] for w in ((0, 1, 2) if time_mode else (0, 2))])


def _key(table, q, env):
    return (table, repr(sorted(q.items())), repr(sorted(env.items())))


def _ways(W, oracle, capfd, monkeypatch, table, q, env, kernel, ways=WAYS3, strategy=None, follows_estimate=True, expect_text=()):
    """One query on one table with SYBL_LATE_PATH forced on, forced off and (WAYS3) unset.  follows_estimate: the launch takes
    the LATE form iff FastPlan::late says so (k_scan_packed runs its late loop whatever it says).  expect_text: what the plan
    trace of every run must contain."""
    tb = W.tb[table]
    time_mode = bool(q.get("time_col"))
    rk = _key(table, q, {})
    if rk not in W.refs:
        W.refs[rk] = LL.reference(W.layouts[table].cols, q)
        if q["op"] == "hist":
            W.oracles[rk] = _oracle_ref(W, oracle, table, q)
    ref = W.refs[rk]
    snaps = {}
    for late in ways:
        what = (table, kernel, q.get("filters"), q.get("groups"), q["aggs"], q["op"], env, late)
        res, err, st, tr = _traced(tb, q, capfd, monkeypatch, late, env)
        assert err is None, (what, err)
        try:
            # (packed_kernel: the direct-mapped and strategy-5 plans' flag; a hashed query's body is in the trace alone)
            assert st["n_workgroups"] == W.n_wg and st["packed_kernel"] == (0 if kernel == "hash_packed" else 1), (what, st)
            if strategy is not None:
                assert st["strategy"] == strategy, (what, st)
            assert len(tr.lines) == 1 and tr.lines[0][0] == kernel, (what, tr.lines, tr.text)
            if not follows_estimate:
                assert tr.lines[0][1] == 1, (what, tr.lines)
            elif late is not None:
                assert tr.lines[0][1] == int(late), (what, tr.lines)
            for text in expect_text:
                assert text in tr.text, (what, text, tr.text)
            if kernel == "hash_packed":
                assert tr.hashed == [("packed", tr.lines[0][1])], (what, tr.hashed)
            _check_numpy(res, ref, q, what)
            if q["op"] == "hist":
                parity.compare(res, W.oracles[rk], op="hist", full=bool(q.get("want_percentiles")), n_aggs=len(q["aggs"]), time_mode=time_mode)
            snaps[late] = _snapshot(res, time_mode)
        finally:
            res.free()
    assert snaps["1"] == snaps["0"], (table, kernel, q)
    return ref


HASH = {"SYBL_FORCE_HASH": "1"}
F = LL.FILTERS
TIME = dict(time_col="t", time_bucket=LL.TB)

# ---------------------------------------------------------------------------------------------- main: hashed, packed body
HASHED = {
    "g1-count-f1": _q(filters=F["f1"], groups=["gx"], aggs=[]),
    "g1-avg1-f2": _q(filters=F["f2"], groups=["ga"], aggs=["a1"]),
    "g2-minmax2-f4": _q(filters=F["f4"], groups=["gc", "gx"], aggs=["a2", "a4"]),
    "g2-avg3-and": _q(filters=F["and"], groups=["ga", "gx"], aggs=["a1", "a2b", "a4"]),
    "g1-moments4-f1": _q(filters=F["f1"], groups=["gx"], aggs=["a1", "a2", "a2b", "a4"], op="hist"),
    "g2-moments2-and": _q(filters=F["and"], groups=["gc", "gx"], aggs=["a2", "a4"], op="hist"),
    "g2-avg1-time-f2": _q(filters=F["f2"], groups=["ga", "gx"], aggs=["a4"], **TIME),
}


@pytest.mark.parametrize("case", list(HASHED))
def test_hashed_packed_body(world, oracle, capfd, monkeypatch, case):
    """k_scan_hash_packed<.., HASH, LATE>: one and two group columns, 0..4 aggregations, avg / tracked extrema / moments, a time
    series, the pattern through each filter width and the conjunction."""
    q = HASHED[case]
    ref = _ways(world, oracle, capfd, monkeypatch, "main", q, HASH, "hash_packed", strategy=7)
    assert ref["matched"] == int(world.layouts["main"].passing.sum()) and len(ref["groups"]) >= 2


# ---------------------------------------------------------------------------------------------- main: direct-mapped, run-time counts
PACKED_N = {
    "g3-minmax2-f1": _q(filters=F["f1"], groups=["ga", "gc", "gx"], aggs=["a1", "a2"]),
    "g4-avg1-f2": _q(filters=F["f2"], groups=["ga", "gb", "gc", "gx"], aggs=["a4"]),
    "g2-avg3-f4": _q(filters=F["f4"], groups=["gc", "gx"], aggs=["a1", "a2b", "a4"]),
    "g2-moments4-and": _q(filters=F["and"], groups=["ga", "gx"], aggs=["a1", "a2", "a2b", "a4"], op="hist"),
    "g3-moments2-f2": _q(filters=F["f2"], groups=["ga", "gb", "gx"], aggs=["a2b", "a4"], op="hist"),
    "g2-minmax3-time-f1": _q(filters=F["f1"], groups=["ga", "gx"], aggs=["a1", "a2", "a4"], **TIME),
}


@pytest.mark.parametrize("case", list(PACKED_N))
def test_direct_mapped_run_time_counts(world, oracle, capfd, monkeypatch, case):
    """k_scan_hash_packed<.., HASH = false, LATE> (packed_n_mode): three and four group columns, three and four aggregations."""
    q = PACKED_N[case]
    assert len(q["groups"]) > 2 or len(q["aggs"]) > 2
    _ways(world, oracle, capfd, monkeypatch, "main", q, {}, "packed_n", strategy=2)


# ---------------------------------------------------------------------------------------------- main: strategy 5
PARTHIST = {
    "a1-f1": _q(filters=F["f1"], groups=["gh"], aggs=["a4"], op="hist", want_percentiles=True),
    "a2-and": _q(filters=F["and"], groups=["gh"], aggs=["a4", "a2b"], op="hist", want_percentiles=True),
    "a1-f4": _q(filters=F["f4"], groups=["gh"], aggs=["a2"], op="hist", want_percentiles=True),
}


@pytest.mark.parametrize("case", list(PARTHIST))
def test_partitioned_histograms(world, oracle, capfd, monkeypatch, case):
    """k_count_packed / k_emit_packed<.., LATE>: config 4's shape; every bucket of every group equals the oracle's (full), so
    the emit filled the regions the count pass sized."""
    ref = _ways(world, oracle, capfd, monkeypatch, "main", PARTHIST[case], {}, "count_emit", strategy=5)
    assert len(ref["groups"]) > 2000


# ---------------------------------------------------------------------------------------------- main: k_scan_packed, the control
def _cfg3(groups, filters=LL.ALL3):
    return _q(filters=filters, groups=groups, aggs=["a2b", "a4"], op="hist")


# (four tiles a workgroup are below the planner's threshold for dynamic dealing, and the table below the one for filter words:
# asked for, the same layout runs through packed_scan_dyn's late loop -- two-tile pieces, so that every workgroup draws some)
DYN = {"SYBL_DYN_MIN_TILES": "1", "SYBL_DYN_PIECE_TILES": "2"}
FWORD = dict(DYN, SYBL_FWORD_MIN_ROWS="1")
# case -> (query, environment, what the plan trace must say)
SCAN_PACKED = {
    "default": (_cfg3(["ga", "gx"]), {}, ("dealing: dynamic=0",)),
    "default-2byte-key": (_cfg3(["gc", "gx"]), {}, ()),
    "default-proved-keys": (_cfg3(["ga", "gb"]), {}, ()),
    "no-dyn": (_cfg3(["ga", "gx"]), {"SYBL_NO_DYN": "1"}, ("dealing: dynamic=0",)),
    "no-fword": (_cfg3(["ga", "gx"]), {"SYBL_NO_FWORD": "1"}, ()),
    "dyn": (_cfg3(["ga", "gx"]), DYN, ("dealing: dynamic=1",)),
    "dyn-fword": (_cfg3(["ga", "gx"], LL.WORD3), FWORD, ("dealing: dynamic=1", "narrow: f=word(")),
    "dyn-fword-off": (_cfg3(["ga", "gx"], LL.WORD3), dict(FWORD, SYBL_NO_FWORD="1"), ("dealing: dynamic=1",)),
}


@pytest.mark.parametrize("case", list(SCAN_PACKED))
def test_scan_packed_late_loop(world, oracle, capfd, monkeypatch, case):
    """Config 3's shape (three filters, two groups, two aggregations, moments) through k_scan_packed: the late loop that has
    been measured most, on the same layout -- static (the default at four tiles a workgroup) and dynamic, from the filter
    columns and from a filter word."""
    q, env, text = SCAN_PACKED[case]
    _ways(world, oracle, capfd, monkeypatch, "main", q, env, "packed", follows_estimate=False, expect_text=text)


# ---------------------------------------------------------------------------------------------- ragged and tiny
SMALL = {
    "hashed": (_q(filters=F["f1"], groups=["ga", "gx"], aggs=["a2", "a4"]), HASH, "hash_packed", True),
    "packed_n": (_q(filters=F["f2"], groups=["ga", "gx"], aggs=["a1", "a2", "a4"]), {}, "packed_n", True),
    "parthist": (_q(filters=F["f1"], groups=["gh"], aggs=["a4"], op="hist", want_percentiles=True), {}, "count_emit", True),
    "scan_packed": (_cfg3(["ga", "gx"]), {}, "packed", False),
}


@pytest.mark.parametrize("body", list(SMALL))
@pytest.mark.parametrize("table", ["ragged"] + ["tiny%d" % r for r in LL.TINY_ROWS])
def test_ragged_and_tiny_tables(world, oracle, capfd, monkeypatch, table, body):
    """Partial tiles, partial windows, tiles past n in the look-ahead (ragged); the prologue alone and n_tiles = 1 (tiny)."""
    q, env, kernel, follows = SMALL[body]
    ref = _ways(world, oracle, capfd, monkeypatch, table, q, env, kernel, ways=WAYS2, follows_estimate=follows)
    assert ref["matched"] == int(world.layouts[table].passing.sum()) >= 1


# ---------------------------------------------------------------------------------------------- degenerate filters
# body -> (group columns, the same with gx among them, environment, kernel family)
BODIES = {
    "hashed": (["gc", "ga"], ["gc", "gx"], HASH, "hash_packed"),
    "packed_n": (["ga", "gb", "gc"], ["ga", "gb", "gx"], {}, "packed_n"),
}


@pytest.mark.parametrize("body", list(BODIES))
def test_a_filter_nothing_passes(world, capfd, monkeypatch, body):
    """A constant no stored value reaches (plo > phi): every window of every wave is skipped."""
    groups, _, env, kernel = BODIES[body]
    q = _q(filters=LL.NOTHING, groups=groups, aggs=["a1", "a2"])
    res, err, st, tr = _traced(world.tb["main"], q, capfd, monkeypatch, "1", env)
    assert err is None and tr.lines == [(kernel, 1, 0.0)], (err, tr.lines)
    assert res.matched == 0 and res.rows(0) == [] and all(r["count"] == 0 for r in res.rows(2))
    res.free()


@pytest.mark.parametrize("body", list(BODIES))
def test_a_filter_everything_passes(world, capfd, monkeypatch, body):
    """No window is skipped: the LATE kernel's answer is the unfiltered query's, field for field, and the reference's.  Through
    gx the failing rows are now live rows outside the declared range: the query fails and says how many."""
    groups, groups_x, env, kernel = BODIES[body]
    main = world.layouts["main"]
    q = _q(filters=LL.EVERYTHING, groups=groups, aggs=["a1", "a2"])
    res, err, st, tr = _traced(world.tb["main"], q, capfd, monkeypatch, "1", env)
    assert err is None and tr.lines[0][:2] == (kernel, 1), (err, tr.lines)
    ref = LL.reference(main.cols, q)
    assert ref["matched"] == main.n
    _check_numpy(res, ref, q, (body, "everything"))
    plain, perr, _, ptr = _traced(world.tb["main"], dict(q, filters=[]), capfd, monkeypatch, None, env)
    assert perr is None and ptr.lines[0][:2] == (kernel, 0), (perr, ptr.lines)
    assert _snapshot(res, False) == _snapshot(plain, False)
    res.free()
    plain.free()
    qx = dict(q, groups=groups_x)
    n_out = LL.reference(main.cols, qx)["overflow"]
    assert n_out == int((~main.passing).sum()) > 0
    for filters, late in ((LL.EVERYTHING, "1"), ([], None)):
        res, err, _, tr = _traced(world.tb["main"], dict(qx, filters=filters), capfd, monkeypatch, late, env)
        assert tr.lines[0][:2] == (kernel, 1 if late else 0), tr.lines
        assert res is None and ("%d rows fell outside the declared column bounds" % n_out) in err, err


@pytest.mark.parametrize("body", list(BODIES))
def test_the_canonical_copy_has_no_late_form(ctx, world, capfd, monkeypatch, body):
    """The same rows, not compacted: no packed plan, so no LATE kernel whatever SYBL_LATE_PATH says -- and the same answer."""
    _, groups_x, env, _ = BODIES[body]
    if not hasattr(world, "canonical"):
        world.canonical = _build(ctx, world.layouts["main"], compact=False, columns=("f1", "ga", "gb", "gc", "gx", "a1", "a2"))
        world.tb["main-canonical"] = world.canonical        # (freed with the others)
    q = _q(filters=F["f1"], groups=groups_x, aggs=["a1", "a2"])
    res, err, st, tr = _traced(world.canonical, q, capfd, monkeypatch, "1", env)
    assert err is None and st["packed_kernel"] == 0, (err, st)
    assert all(late == 0 for _, late, _ in tr.lines) and all(late == 0 for _, late in tr.hashed), (tr.lines, tr.hashed)
    _check_numpy(res, LL.reference(world.layouts["main"].cols, q), q, (body, "canonical"))
    res.free()


# ---------------------------------------------------------------------------------------------- the planner's estimate
N_EST = 200_000
EST_PATHS = {
    "hashed": (_q(groups=["k1"], aggs=["v"]), HASH, "hash_packed", 7),
    "packed_n": (_q(groups=["k1", "k2", "k3"], aggs=["v"]), {}, "packed_n", 2),
    "parthist": (_q(groups=["kh"], aggs=["v"], op="hist", want_percentiles=True), {}, "count_emit", 5),
}
TWO7 = [("e", "gt", 929), ("e2", "gt", 929)]
# filters -> (late, the estimate: fill_packed's product of (hi - lo + 1) / (max - min + 1) over the range filters)
EST_CASES = {
    "gt995": ([("e", "gt", 995)], 1, 4 / 1000),
    "gt994": ([("e", "gt", 994)], 0, 5 / 1000),
    "two-of-7-percent": (TWO7, 1, (70 / 1000) * (70 / 1000)),
    "two-of-7-percent-and-neq": (TWO7 + [("e", "neq", 950)], 0, (70 / 1000) * (70 / 1000)),
}


@pytest.fixture(scope="module")
def est(ctx):
    """200 000 rows, two filter columns EXACTLY uniform over 0..999 (200 of each value, both extremes present)."""
    rng = np.random.default_rng(5)
    cols = {"e": rng.permutation(np.arange(N_EST, dtype=np.int64) % 1000), "e2": rng.permutation(np.arange(N_EST, dtype=np.int64) % 1000),
            "k1": rng.integers(0, 8, N_EST), "k2": rng.integers(0, 4, N_EST), "k3": rng.integers(0, 4, N_EST), "kh": rng.integers(0, 5000, N_EST),
            "v": rng.integers(1, 1_000_001, N_EST)}
    assert all(int(cols[c].min()) == 0 and int(cols[c].max()) == 999 and (np.bincount(cols[c]) == N_EST // 1000).all() for c in ("e", "e2"))
    tb = ctx.create_table("estimate")
    for c in cols:
        tb.add_column(c, "int", *((0, 1_000_000) if c == "v" else (1, 0)))
    for r0 in range(0, N_EST, 50_000):
        tb.append_block(50_000, {c: a[r0:r0 + 50_000] for c, a in cols.items()})
    tb.compact()
    yield types.SimpleNamespace(tb=tb, cols=cols)
    tb.free()


@pytest.mark.parametrize("case", list(EST_CASES))
@pytest.mark.parametrize("path", list(EST_PATHS))
def test_the_estimate_either_side_of_half_a_percent(est, capfd, monkeypatch, path, case):
    """Without SYBL_LATE_PATH: FastPlan::late is `estimate < 0.005` (planner.cpp: fill_packed; DESIGN 3.6 "below 0.5 %" -- the two
    agree: 4 values of 1000 is below, 5 of 1000 is not), and the launch follows it only where the plain body keeps the query --
    a neq constant is the NUL body's, which has no late form, so late=0 at an estimate well below the threshold (strategy 5,
    which has no NUL body, leaves such a query to another kernel)."""
    q0, env, kernel, strategy = EST_PATHS[path]
    filters, late, share = EST_CASES[case]
    q = dict(q0, filters=filters)
    res, err, st, tr = _traced(est.tb, q, capfd, monkeypatch, None, env)
    try:
        assert err is None, err
        assert res.matched == int(LL.keep(est.cols, filters).sum()), (res.matched, tr.lines)
        if "neq" in case:
            assert all(l == 0 for _, l, _ in tr.lines) and all(l == 0 for _, l in tr.hashed), tr.text
            if path != "parthist":
                assert len(tr.lines) == 1 and tr.lines[0][0] == kernel and tr.lines[0][2] < 0.005, tr.lines
            return
        assert st["strategy"] == strategy and st["packed_kernel"] == (0 if kernel == "hash_packed" else 1), st
        assert len(tr.lines) == 1 and tr.lines[0][:2] == (kernel, late), tr.lines
        assert abs(tr.lines[0][2] - share) <= 1e-5 * share, (tr.lines, share)      # (the line prints six significant digits)
        if kernel == "hash_packed":
            assert tr.hashed == [("packed", late)], tr.hashed
    finally:
        if res is not None:
            res.free()


# ---------------------------------------------------------------------------------------------- last in the file
def test_every_family_ran_in_late_form(capfd):
    """The cases above must not collapse onto the plain kernels (needs the rest of the file to have run): the trace lines that
    show each of the four LATE instantiations, printed."""
    with capfd.disabled():
        print()
        for key in sorted(SEEN):
            print("  " + SEEN[key])
    for kernel in ("hash_packed", "packed_n", "count_emit", "packed"):
        assert (kernel, 1) in SEEN, (kernel, sorted(SEEN))
    for kernel in ("hash_packed", "packed_n", "count_emit"):
        assert (kernel, 0) in SEEN, (kernel, sorted(SEEN))
