"""GPU: narrow twins -- a 4-byte aggregation column whose largest stored offset is below 2^24, scanned by k_scan_packed from a
3-byte copy (Column::narrow; table.cpp: column_build_narrow, kernels.hip: k_narrow3, narrow3.h, planner.cpp: plan_narrow,
scan_packed.h: packed_decode) -- bit-exact against the oracle, and field for field against the same query with SYBL_NO_NARROW=1.

A twin is built for tables of at least SYBL_NARROW_MIN_ROWS physical rows (default 2^25); every case here sets it to 1, and the
plan trace (SYBL_PLAN_TRACE=1, `narrow: a0=.. a1=.. bytes_per_row=..`, `narrow twin: col=.. rows=.. converted=.. bytes=..`) says
what the plan reads.  Tables are sized as tests/test_gpu_dynamic_pieces.py sizes them: 4096 * (5 * n_wg + 3) + 1234 rows, the
last tile partial and not a multiple of 4 rows.

What a case places where:
  1. config 3's and config 2's shapes under the settings that choose k_scan_packed's loops: the dynamic late and plain loops
     (SYBL_DYN=1 SYBL_DYN_MIN_TILES=1 SYBL_DYN_PIECE_TILES=2), the static ones (SYBL_NO_DYN=1), the body that is not lean
     (SYBL_NO_LEAN=1) and the ring of two tiles (SYBL_PACKED_RING=2);
  2. byte lanes: values of three distinct bytes at each of a lane's four rows, in lane 63, at a tile's first and last row and in
     the last rows of the partial tile, each under a key of its own -- a swapped byte changes that key's sum;
  3. the range edge: a largest offset of 2^24 - 1 gives a twin, 2^24 does not, over a positive and a negative value base;
  4. a twinned column with a validity bitmap (the NUL kernel) and config 5's shape (an hourly time bucket, the windowed plan);
  5. neighbours: on a table whose aggregation columns have twins, a hashed query and a partitioned-histogram query keep the
     4-byte columns;
  6. life cycle: an appended block inside the range extends the twin by that block's rows, one beyond it frees the twin, two
     prepared queries share one twin;
  7. SYBL_NO_NARROW=1 and the default SYBL_NARROW_MIN_ROWS leave these tables on the 4-byte plan.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import parity

pytestmark = pytest.mark.gpu

NARROW = re.compile(r"^narrow: (.*) bytes_per_row=(\d+)$", re.M)
TWIN = re.compile(r"^narrow twin: col=(\w+) rows=(\d+) converted=(\d+) bytes=(\d+)$", re.M)
FREED = re.compile(r"^narrow twin: col=(\w+) freed$", re.M)
TOP24 = (1 << 24) - 1
NAMES = ["f1", "f2", "f3", "g1", "g2", "a1", "a2", "k2", "tm", "hk", "hj"]
INFO = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 63), "a1": (0, 999_999), "a2": (0, 999_996),
        "k2": (0, 299), "tm": (0, 3 * 86400 - 1), "hk": (0, 65535), "hj": (0, 2999)}
_RANGE3 = [(c, op, v) for c in ("f1", "f2", "f3") for op, v in (("gt", 99), ("lt", 900))]
Q3 = dict(filters=_RANGE3, groups=["g1", "g2"], aggs=["a1", "a2"], op="hist", want_percentiles=False)
Q2 = dict(groups=["g1"], aggs=["a1", "a2"], op="avg")
Q5 = dict(groups=["k2"], aggs=["a1"], op="avg", time_col="tm", time_bucket=3600)
DYN = {"SYBL_DYN": "1", "SYBL_DYN_MIN_TILES": "1", "SYBL_DYN_PIECE_TILES": "2"}


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def small_tables_get_twins(monkeypatch):
    monkeypatch.setenv("SYBL_NARROW_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")


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
    cols["k2"] = rng.integers(0, 300, n)
    cols["tm"] = np.sort(rng.integers(0, 3 * 86400, n))    # in time order, as a digested table is: the windowed plan (72 x 300 cells)
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


class _T:
    pass


@pytest.fixture(scope="module")
def main_table(ctx, n_wg, oracle):
    T = _T()
    T.n = 4096 * (5 * n_wg + 3) + 1234
    assert T.n % 4 == 2
    T.cols = _columns(T.n, 41)
    T.tb = _table(ctx, "twin_main", T.cols)
    assert [T.tb.column_storage(c)[0] for c in NAMES[:7]] == [2, 2, 2, 1, 1, 4, 4]
    T.ocols = [{"type": "int", "data": T.cols[c]} for c in NAMES]
    T.oracle = {}

    def answer(key, q):
        if key not in T.oracle:
            T.oracle[key] = oracle.run_query(T.ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, q))
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


def _widths(err):
    """[(widths per aggregation, bytes per row)] of every `narrow:` line."""
    return [([int(x.split("=")[1]) for x in m[0].split()], int(m[1])) for m in NARROW.findall(err)]


def _run(tb, q, capfd):
    capfd.readouterr()
    qy = tb.query(**q)
    res = qy.run()
    st = qy.stats()
    qy.free()
    return res, st, capfd.readouterr().err


def _check(tb, q, ores, capfd, monkeypatch, want, strategy=2):
    """The query from the twins (trace: the widths in `want`) against the oracle, and against itself with SYBL_NO_NARROW=1."""
    n_aggs = len(q["aggs"])
    res, st, err = _run(tb, q, capfd)
    assert [w for w, _ in _widths(err)] == [want], err[-2000:]
    assert (st["strategy"], st["packed_kernel"]) == (strategy, 1), st
    parity.compare(res, ores, op=q["op"], full=q.get("want_percentiles", True), n_aggs=n_aggs, time_mode=bool(q.get("time_col")))
    got = _fields(res)
    res.free()
    monkeypatch.setenv("SYBL_NO_NARROW", "1")
    res, st0, err0 = _run(tb, q, capfd)
    monkeypatch.delenv("SYBL_NO_NARROW")
    assert [w for w, _ in _widths(err0)] == [[4] * n_aggs], err0[-2000:]
    assert (st0["strategy"], st0["n_workgroups"], st0["replicas"], st0["algorithmic_bytes"]) == \
           (st["strategy"], st["n_workgroups"], st["replicas"], st["algorithmic_bytes"])
    assert _fields(res) == got
    res.free()
    return st, err


SETTINGS = [("default", {}), ("dynamic", DYN), ("static", {"SYBL_NO_DYN": "1"}), ("not_lean", {"SYBL_NO_LEAN": "1"}),
            ("dynamic_not_lean", dict(DYN, SYBL_NO_LEAN="1")), ("ring_of_two", {"SYBL_PACKED_RING": "2"})]


@pytest.mark.parametrize("shape", ["config3", "config2"])
@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_config_shapes_in_every_loop(main_table, capfd, monkeypatch, setting, shape):
    for k, v in setting[1].items():
        monkeypatch.setenv(k, v)
    q = Q3 if shape == "config3" else Q2
    st, err = _check(main_table.tb, q, main_table.answer(shape, q), capfd, monkeypatch, [3, 3])
    assert _widths(err)[0][1] == (14 if shape == "config3" else 7)
    assert ("dealing: dynamic=1" in err) == (setting[0].startswith("dynamic")), err[-1000:]
    assert st["algorithmic_bytes"] == main_table.n * (16 if shape == "config3" else 9)   # the table's stored bytes, as before


def test_byte_lanes(ctx, n_wg, oracle, capfd, monkeypatch):
    n = 4096 * (5 * n_wg + 3) + 1234
    rng = np.random.default_rng(42)
    tile = 4096 * (2 * n_wg + 1)
    special = [0, 1, 2, 3,                          # the four rows of lane 0
               252, 253, 254, 255,                  # ... of lane 63 of the first wave
               4096 - 4, 4096 - 1,                  # the last lane of the last wave of a tile
               tile, tile + 1, tile + 4095,         # a later tile's first rows and its last row
               n - 1234, n - 5, n - 4, n - 3, n - 2, n - 1]   # the partial tile: its first row and the rows around its ragged end
    key = np.zeros(n, dtype=np.int64)
    val = rng.integers(0, 1 << 24, n)
    want = {}
    for j, r in enumerate(special):
        key[r] = j + 1
        val[r] = (0x01 + j) | ((0x40 + j) << 8) | ((0x80 + j) << 16)   # three distinct bytes, distinct from every other special row's
        want[j + 1] = int(val[r])
    val[4], val[n - 6] = 0, TOP24
    f = rng.integers(0, 1000, n)
    f[special] = 500
    names, info = ["f", "key", "val"], {"f": (0, 999), "key": (0, 31), "val": (0, TOP24)}
    cols = {"f": f, "key": key, "val": val}
    tb = _table(ctx, "twin_lanes", cols, names, info)
    assert tb.column_storage("val") == (4, 0)
    ocols = [{"type": "int", "data": cols[c]} for c in names]
    for q, env in ((dict(groups=["key"], aggs=["val"], op="avg"), {}),                                    # the plain loop
                   (dict(filters=[("f", "gt", 99), ("f", "lt", 900)], groups=["key"], aggs=["val"], op="avg"), DYN),   # the dynamic late loop
                   (dict(filters=[("f", "gt", 99), ("f", "lt", 900)], groups=["key"], aggs=["val"], op="avg"), {"SYBL_NO_DYN": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(names, info, q))
        res, st, err = _run(tb, q, capfd)
        assert _widths(err) == [([3], (2 if q.get("filters") else 0) + 1 + 3)], err[-2000:]
        parity.compare(res, ores, op="avg", full=True, n_aggs=1)
        got = {r["key"][0]: (r["count"], r["hists"][0]["sum"]) for r in res.rows(0)}
        assert {k: got[k] for k in want} == {k: (1, v) for k, v in want.items()}
        res.free()
        for k in env:
            monkeypatch.delenv(k)
    tb.free()


@pytest.mark.parametrize("vbase", [7777, -5000])
@pytest.mark.parametrize("top,width", [(TOP24, 3), (TOP24 + 1, 4)])
def test_range_edge(ctx, oracle, capfd, vbase, top, width):
    n = 4096 * 3 + 5
    rng = np.random.default_rng(43)
    g = rng.integers(0, 16, n)
    v = vbase + rng.integers(0, top + 1, n)
    v[7], v[n - 2] = vbase, vbase + top
    names, info = ["g", "v"], {"g": (0, 15), "v": (vbase, vbase + top)}
    tb = _table(ctx, "twin_edge", {"g": g, "v": v}, names, info)
    assert tb.column_storage("v") == (4, vbase)
    q = dict(groups=["g"], aggs=["v"], op="avg")
    ores = oracle.run_query([{"type": "int", "data": g}, {"type": "int", "data": v}], block_rows=65536, n_threads=2,
                            **parity.oracle_query_kwargs(names, info, q))
    hbm0 = tb.hbm_bytes
    res, st, err = _run(tb, q, capfd)
    assert _widths(err) == [([width], 1 + width)], err[-2000:]
    assert len(TWIN.findall(err)) == (1 if width == 3 else 0)
    assert (tb.hbm_bytes > hbm0) == (width == 3)
    parity.compare(res, ores, op="avg", full=True, n_aggs=1)
    res.free()
    tb.free()


def test_validity_bitmap_on_a_twinned_column(main_table, ctx, oracle, capfd, monkeypatch):
    """A column with unpopulated rows: the NUL kernel reads the twin and the parent's validity words."""
    T = main_table
    n = 4096 * 9 + 1234
    rng = np.random.default_rng(44)
    pop = (rng.integers(0, 5, n) != 0).astype(np.uint8)
    pop[:8], pop[n - 3:] = (1, 0, 1, 1, 0, 0, 1, 0), (0, 1, 1)
    cols = {"g1": T.cols["g1"][:n].copy(), "a1": T.cols["a1"][:n].copy()}
    cols["a1"][0], cols["a1"][n - 1] = INFO["a1"]
    tb = ctx.create_table("twin_nul")
    for c in ("g1", "a1"):
        tb.add_column(c, "int", *INFO[c])
    tb.append_block(n, {"g1": cols["g1"], "a1": (cols["a1"], pop)})
    for c in ("g1", "a1"):
        tb.set_bounds(c, *INFO[c], has_missing=(c == "a1"))
    tb.compact()
    assert tb.column_storage("a1")[0] == 4
    q = dict(groups=["g1"], aggs=["a1"], op="avg")
    ores = oracle.run_query([{"type": "int", "data": cols["g1"]}, {"type": "int", "data": cols["a1"], "populated": pop}], block_rows=65536,
                            n_threads=2, **parity.oracle_query_kwargs(["g1", "a1"], INFO, q))
    _check(tb, q, ores, capfd, monkeypatch, [3])
    tb.free()


def test_config5_shape_windowed(main_table, capfd, monkeypatch):
    T = main_table
    st, err = _check(T.tb, Q5, T.answer("config5", Q5), capfd, monkeypatch, [3], strategy=4)
    assert _widths(err)[0][1] == 4 + 2 + 3   # the time column and the key keep their stored widths


def test_neighbours_keep_the_four_byte_column(main_table, ctx, oracle, capfd):
    """The twins exist (the first query builds them); the hash path and the partitioned histograms do not read them.  A table of
    its own, of the size at which tests/test_gpu_compact.py runs config 4: 65 536 groups are what these two answers cost to check."""
    T = main_table
    n = 300_002
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "twin_neighbours", cols)
    ocols = [{"type": "int", "data": cols[c]} for c in NAMES]
    res, st, err = _run(tb, Q2, capfd)
    res.free()
    assert [w for w, _ in _widths(err)] == [[3, 3]] and sorted(t[0] for t in TWIN.findall(err)) == ["a1", "a2"], err[-2000:]
    for key, q, strategy in (("hashed", dict(groups=["hk", "hj"], aggs=["a1", "a2"], op="avg"), 7),
                             ("part_hist", dict(groups=["hk"], aggs=["a1"], op="hist", want_percentiles=True), 5)):
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, q))
        res, st, err = _run(tb, q, capfd)
        assert st["strategy"] == strategy, (key, st)
        assert "narrow" not in err, err[-2000:]   # no `narrow:` line (not k_scan_packed's launch), no twin built or freed
        parity.compare(res, ores, op=q["op"], full=q["op"] == "hist", n_aggs=len(q["aggs"]))
        res.free()
    tb.free()


def test_life_cycle(ctx, oracle, capfd, monkeypatch):
    n0, n1, n2 = 4096 * 5 + 1234, 4096 + 70, 100
    rng = np.random.default_rng(45)
    g = rng.integers(0, 16, n0 + n1 + n2)
    v = 1000 + rng.integers(0, 1 << 20, n0 + n1 + n2)
    v[0], v[n0 - 1] = 1000, 1000 + (1 << 22)
    v[n0 + 5] = 1000 + TOP24               # the second block reaches the last offset a twin holds
    v[n0 + n1 + 7] = 1000 + TOP24 + 1      # the third block goes one beyond it
    names, info = ["g", "v"], {"g": (0, 15), "v": (1000, 1000 + (1 << 25))}

    def build(name):
        tb = ctx.create_table(name)
        for c in names:
            tb.add_column(c, "int", *info[c])
        tb.append_block(n0, {"g": g[:n0], "v": v[:n0]})
        for c in names:
            tb.set_bounds(c, *info[c])
        tb.compact()
        assert tb.column_storage("v") == (4, 1000)
        return tb

    def answer(n):
        return oracle.run_query([{"type": "int", "data": g[:n]}, {"type": "int", "data": v[:n]}], block_rows=65536, n_threads=2,
                                **parity.oracle_query_kwargs(names, info, q))
    q = dict(groups=["g"], aggs=["v"], op="avg")
    tb = build("twin_life")
    monkeypatch.setenv("SYBL_NO_NARROW", "1")
    plain = build("twin_life_plain")     # the same table without a twin: what hbm_bytes is without one
    monkeypatch.delenv("SYBL_NO_NARROW")
    assert tb.hbm_bytes == plain.hbm_bytes

    # two prepared queries share one twin: built once, 3 bytes per reserved row
    capfd.readouterr()
    qa, qb = tb.query(**q), tb.query(**q)
    err = capfd.readouterr().err
    twins = TWIN.findall(err)
    assert len(twins) == 1 and twins[0][0] == "v" and int(twins[0][1]) == int(twins[0][2]) >= n0, err[-2000:]
    assert [w for w, _ in _widths(err)] == [[3], [3]]
    twin_bytes = tb.hbm_bytes - plain.hbm_bytes
    assert twin_bytes == int(twins[0][3]) and twin_bytes % 3 == 0 and twin_bytes >= 3 * int(twins[0][1])
    for qy in (qa, qb, qa):
        res = qy.run()
        parity.compare(res, answer(n0), op="avg", full=True, n_aggs=1)
        res.free()
    qa.free()
    qb.free()

    # a block inside the range: the twin is extended by that block's rows alone
    for t in (tb, plain):
        t.append_block(n1, {"g": g[n0:n0 + n1], "v": v[n0:n0 + n1]})
    assert tb.column_storage("v") == (4, 1000)
    res, st, err = _run(tb, q, capfd)
    twins = TWIN.findall(err)
    assert len(twins) == 1 and int(twins[0][1]) >= n0 + n1 and n1 <= int(twins[0][2]) < n1 + 32 + 4, err[-2000:]
    assert [w for w, _ in _widths(err)] == [[3]]
    parity.compare(res, answer(n0 + n1), op="avg", full=True, n_aggs=1)
    res.free()
    twin_bytes = tb.hbm_bytes - plain.hbm_bytes
    assert twin_bytes == int(twins[0][3]) and twin_bytes % 3 == 0 and twin_bytes >= 3 * int(twins[0][1])

    # a block with a value 2^24 above the base: back on the 4-byte column, the twin's bytes returned
    for t in (tb, plain):
        t.append_block(n2, {"g": g[n0 + n1:], "v": v[n0 + n1:]})
    assert tb.column_storage("v") == (4, 1000)
    res, st, err = _run(tb, q, capfd)
    assert FREED.findall(err) == ["v"] and not TWIN.findall(err), err[-2000:]
    assert [w for w, _ in _widths(err)] == [[4]]
    parity.compare(res, answer(n0 + n1 + n2), op="avg", full=True, n_aggs=1)
    res.free()
    assert tb.hbm_bytes == plain.hbm_bytes
    tb.free()
    plain.free()


@pytest.mark.parametrize("how", ["SYBL_NO_NARROW", "default_min_rows"])
def test_small_tables_stay_on_the_four_byte_plan(main_table, ctx, capfd, monkeypatch, how):
    """A table of its own: main_table's columns carry twins from the cases before, which a plan without twins leaves alone."""
    T = main_table
    n = 4096 * 3 + 5
    if how == "SYBL_NO_NARROW":
        monkeypatch.setenv("SYBL_NO_NARROW", "1")
    else:
        monkeypatch.delenv("SYBL_NARROW_MIN_ROWS")
        assert n < 1 << 25
    cols = {c: T.cols[c][:n].copy() for c in NAMES}
    for c in NAMES:
        cols[c][0], cols[c][n - 1] = INFO[c]
    tb = _table(ctx, "twin_off", cols)
    hbm = tb.hbm_bytes
    for q in (Q3, Q2):
        res, st, err = _run(tb, q, capfd)
        assert [w for w, _ in _widths(err)] == [[4, 4]] and not TWIN.findall(err), err[-2000:]
        res.free()
    assert tb.hbm_bytes == hbm
    tb.free()
