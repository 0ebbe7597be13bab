"""GPU: k_scan_packed with its tiles dealt from a device queue (FastPlan::dyn; scan_packed.h: packed_scan_dyn, pieces.h,
planner.cpp: plan_dynamic) -- bit-exact against the oracle, and field for field against the same query with SYBL_NO_DYN=1.

The planner takes dynamic dealing for tables of at least 128 tiles per workgroup, and by default for the late-materialisation
loop only; every case here sets SYBL_DYN=1 (the plain loop too), SYBL_DYN_MIN_TILES=1 and SYBL_DYN_PIECE_TILES=2, so tables of a few tiles per workgroup take the new loops, in pieces of two tiles, and the plan trace
(SYBL_PLAN_TRACE=1, `dealing: dynamic=..`) says that they did.  The tables are sized from the workgroup count of the device
under test, as tests/test_gpu_word_packing.py does: 4096 * (5 * n_wg + 3) + 1234 rows are 5 * n_wg + 4 tiles, the last one
partial -- several pieces per workgroup, more than one ticket drawn ahead, a piece of one tile and a partial tile at the end.

What a case places where:
  1. config 3's shape (three range filters, two one-byte keys, two aggregations, moments): the late-materialisation loop, with
     the lean body and without (SYBL_NO_LEAN=1);
  2. config 2's shape (no filter, one key, avg, Count packed into the sum word): the plain loop;
  3. a table appended in blocks of unequal size -- blocks start on padded 32-row boundaries, every block a run of its own --,
     half of them skipped through a filter column that is constant per block: many short runs with gaps;
  4. fewer pieces than workgroups, and a table of one row;
  5. every workgroup at its cap (SYBL_DYN_CAP_PCT=100, as many pieces as workgroups): nothing may be left over;
  6. rescans of one prepared query, and two prepared queries scanned in turns: the queue word starts from zero every time;
  7. the proof fallback: Count packed above 2^32 - 1 offsets fits the static share of 10 tiles but not the 18 a workgroup could
     draw -- the plan stays static and keeps its packing.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import parity

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
DEALING = re.compile(r"dealing: dynamic=(\d) pieces=(\d+) piece_tiles=(\d+) cap=(\d+)")
CPACK = re.compile(r"count packing: cshift=(\d+) sum_bits=(\d+) count_bits=(\d+) slot_rows=(\d+)")
LEAN = re.compile(r"lean moments: lean=(\d)")
NAMES = ["f1", "f2", "f3", "g1", "g2", "a1", "a2", "blk", "k2", "tm"]
INFO = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 63), "a1": (0, 999_999), "a2": (0, 999_996), "blk": (0, 9),
        "k2": (0, 299), "tm": (0, 8 * 3600 - 1)}
_RANGE3 = [(c, op, v) for c in ("f1", "f2", "f3") for op, v in (("gt", 99), ("lt", 900))]
Q3 = dict(filters=_RANGE3, groups=["g1", "g2"], aggs=["a1", "a2"], op="hist", want_percentiles=False)
Q2 = dict(groups=["g1"], aggs=["a1", "a2"], op="avg")


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def small_pieces(monkeypatch):
    monkeypatch.setenv("SYBL_DYN_MIN_TILES", "1")
    monkeypatch.setenv("SYBL_DYN_PIECE_TILES", "2")
    monkeypatch.setenv("SYBL_DYN", "1")      # the plain loop too (by default only the late-materialisation loop takes the queue)
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


def _columns(n, seed, block_of_row=None):
    rng = np.random.default_rng(seed)
    cols = {c: rng.integers(0, 1000, n) for c in ("f1", "f2", "f3")}
    cols["g1"] = rng.integers(0, 16, n)
    cols["g2"] = rng.integers(0, 64, n)
    cols["a1"] = rng.integers(0, 1_000_000, n)
    cols["a2"] = np.clip(rng.normal(500_000, 120_000, n).astype(np.int64), 0, 999_996)
    for c in ("f1", "g1", "g2", "a1", "a2"):   # the declared extrema occur: the stored widths and bases are the same in every table
        cols[c][0], cols[c][n - 1] = INFO[c][0], INFO[c][1]
    cols["blk"] = np.zeros(n, dtype=np.int64) if block_of_row is None else (block_of_row * 7) % 10
    cols["k2"] = rng.integers(0, 300, n)          # a key stored in two bytes
    cols["tm"] = rng.integers(0, 8 * 3600, n)     # eight time buckets of an hour: the whole [bucket][cell] table fits the LDS
    for c in ("k2", "tm"):
        cols[c][0], cols[c][n - 1] = INFO[c][0], INFO[c][1]
    return cols


def _table(ctx, name, cols, sizes):
    tb = ctx.create_table(name)
    for c in NAMES:
        tb.add_column(c, "int", *INFO[c])
    r0 = 0
    for s in sizes:
        tb.append_block(s, {c: cols[c][r0:r0 + s] for c in NAMES})
        r0 += s
    assert r0 == len(cols["f1"]) == tb.rows
    for c in NAMES:
        tb.set_bounds(c, *INFO[c])
    tb.compact()
    assert [tb.column_storage(c)[0] for c in NAMES[:7]] == [2, 2, 2, 1, 1, 4, 4]
    return tb


def _even_sizes(n, block=65536):
    return [min(block, n - r0) for r0 in range(0, n, block)]


class _T:
    pass


@pytest.fixture(scope="module")
def main_table(ctx, n_wg, oracle):
    """5 * n_wg + 4 tiles in one run; the oracle's answers to both shapes, computed once."""
    T = _T()
    T.n = 4096 * (5 * n_wg + 3) + 1234
    T.cols = _columns(T.n, 31)
    T.tb = _table(ctx, "dyn_main", T.cols, _even_sizes(T.n))
    T.ocols = [{"type": "int", "data": T.cols[c]} for c in NAMES]
    T.o3 = oracle.run_query(T.ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, Q3))
    T.o2 = oracle.run_query(T.ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, Q2))
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


def _run(tb, q, capfd, dynamic=1, strategy=2):
    """prepare + scan + finalize: (result, stats, trace text); asserts what the `dealing:` line says."""
    capfd.readouterr()
    qy = tb.query(**q)
    res = qy.run()
    st = qy.stats()
    qy.free()
    err = capfd.readouterr().err
    deal = DEALING.findall(err)
    assert len(deal) == 1 and int(deal[0][0]) == dynamic, (deal, err[-2000:])
    if dynamic:
        assert int(deal[0][1]) >= 1 and int(deal[0][2]) == 2 and int(deal[0][3]) >= 1, deal
    assert (st["strategy"], st["packed_kernel"]) == (strategy, 1), st
    return res, st, err


def _check(tb, q, ores, capfd, monkeypatch, n_aggs=2, strategy=2):
    """The query with dynamic dealing against the oracle, and against itself with SYBL_NO_DYN=1."""
    res, st, err = _run(tb, q, capfd, strategy=strategy)
    parity.compare(res, ores, op=q["op"], full=q.get("want_percentiles", True), n_aggs=n_aggs, time_mode=bool(q.get("time_col")))
    dyn = _fields(res)
    res.free()
    monkeypatch.setenv("SYBL_NO_DYN", "1")
    res, st0, _ = _run(tb, q, capfd, dynamic=0, strategy=strategy)
    assert st0["n_workgroups"] == st["n_workgroups"] and st0["replicas"] == st["replicas"]
    assert _fields(res) == dyn
    res.free()
    monkeypatch.delenv("SYBL_NO_DYN")
    return st, err


@pytest.mark.parametrize("lean", [True, False])
def test_config3_shape_late_loop(main_table, capfd, monkeypatch, lean, n_wg):
    if not lean:
        monkeypatch.setenv("SYBL_NO_LEAN", "1")
    st, err = _check(main_table.tb, Q3, main_table.o3, capfd, monkeypatch)
    pieces, cap = (int(x) for x in DEALING.findall(err)[0][1::2])
    assert pieces == (5 * n_wg + 4 + 1) // 2 and cap == -(-pieces * 125 // (100 * n_wg)) + 2
    # (the dynamic plan keeps the lean layout: the proofs hold for cap * 2 tiles a workgroup as well)
    assert LEAN.findall(err) == (["1"] if lean else []), err[-1000:]
    assert st["n_workgroups"] == n_wg


def test_the_plain_loop_is_opt_in(main_table, capfd, monkeypatch):
    """Without SYBL_DYN=1 config 2's shape plans static and config 3's dynamic, whatever the table's size."""
    monkeypatch.delenv("SYBL_DYN")
    res, _, _ = _run(main_table.tb, Q2, capfd, dynamic=0)
    parity.compare(res, main_table.o2, op="avg", full=True, n_aggs=2)
    res.free()
    res, _, _ = _run(main_table.tb, Q3, capfd, dynamic=1)
    parity.compare(res, main_table.o3, op="hist", full=False, n_aggs=2)
    res.free()


def test_config2_shape_plain_loop(main_table, capfd, monkeypatch):
    st, err = _check(main_table.tb, Q2, main_table.o2, capfd, monkeypatch)
    cp = CPACK.findall(err)
    assert len(cp) == 1 and int(cp[0][0]) > 0, cp   # Count rides in the sum word under the cap too


# the other kernels the planner can choose a dynamic loop for: a key wider than one byte (G1 = false: 16-byte key loads), a time
# column on a plan that is not windowed (TIME: one more column in the plain loop, and in the late loop's second half), plain avg
# and the full histogram with its bucket arrays in LDS (strategy 6)
_F1 = [("f1", "gt", 99), ("f1", "lt", 900)]
OTHER_SHAPES = [
    ("two_byte_key_avg", dict(groups=["k2"], aggs=["a1"], op="avg"), 2),
    ("two_byte_key_late", dict(filters=_F1, groups=["k2", "g1"], aggs=["a1"], op="hist", want_percentiles=False), 2),
    ("time_plain", dict(groups=["g1"], aggs=["a1"], op="avg", time_col="tm", time_bucket=3600), 2),
    ("time_late_two_byte_key", dict(filters=_F1, groups=["k2"], aggs=["a1"], op="hist", want_percentiles=False, time_col="tm", time_bucket=3600), 2),
    ("full_hist_in_lds", dict(filters=_F1, groups=["g1"], aggs=["a1"], op="hist", want_percentiles=True), 6),
]


@pytest.mark.parametrize("name,q,strategy", OTHER_SHAPES, ids=[s[0] for s in OTHER_SHAPES])
def test_other_shapes(main_table, oracle, capfd, monkeypatch, name, q, strategy):
    T = main_table
    ores = oracle.run_query(T.ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, q))
    assert ores["matched"] > 0
    _check(T.tb, q, ores, capfd, monkeypatch, n_aggs=1, strategy=strategy)


def test_unequal_blocks_and_skipped_blocks(ctx, n_wg, oracle, capfd, monkeypatch):
    n = 4096 * (5 * n_wg + 3) + 1234
    sizes, left, i = [], n, 0
    while left > 0:
        s = min((65536, 50001, 70007, 33333, 4097, 61, 99999)[i % 7], left)
        sizes.append(s)
        left -= s
        i += 1
    assert sum(1 for s in sizes if s % 32) > len(sizes) // 2
    block_of_row = np.repeat(np.arange(len(sizes)), sizes)
    cols = _columns(n, 32, block_of_row)
    tb = _table(ctx, "dyn_blocks", cols, sizes)
    ocols = [{"type": "int", "data": cols[c]} for c in NAMES]
    q = dict(filters=[("blk", "gt", 4), ("f1", "gt", 99), ("f1", "lt", 900)], groups=["g1", "g2"], aggs=["a1", "a2"], op="hist",
             want_percentiles=False, block_skip=True)
    ores = oracle.run_query(ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, dict(q, block_skip=False)))
    assert ores["matched"] > 0
    st, err = _check(tb, q, ores, capfd, monkeypatch)
    want_skipped = sum(1 for b in range(len(sizes)) if (b * 7) % 10 <= 4)
    assert st["blocks_skipped"] == want_skipped > len(sizes) // 3, (st, want_skipped)
    # without skipping: every block that does not end on a 32-row boundary still ends a run
    q_all = dict(Q3)
    ores = oracle.run_query(ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, q_all))
    _check(tb, q_all, ores, capfd, monkeypatch)
    tb.free()


@pytest.mark.parametrize("n", [4096 * 3 + 5, 1])
def test_fewer_pieces_than_workgroups(ctx, oracle, capfd, monkeypatch, n):
    cols = _columns(max(n, 2), 33)
    cols = {c: v[:n] for c, v in cols.items()}
    cols["f1"][:] = 500   # (the one row passes)
    tb = ctx.create_table("dyn_small")
    for c in NAMES:
        tb.add_column(c, "int", *INFO[c])
    tb.append_block(n, {c: cols[c] for c in NAMES})
    for c in NAMES:
        tb.set_bounds(c, *INFO[c])
    tb.compact()
    ocols = [{"type": "int", "data": cols[c]} for c in NAMES]
    for q in (Q3, Q2):
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=2, **parity.oracle_query_kwargs(NAMES, INFO, q))
        st, err = _check(tb, q, ores, capfd, monkeypatch)
        assert int(DEALING.findall(err)[0][1]) == (2 if n > 1 else 1)
    tb.free()


def test_every_workgroup_at_its_cap(ctx, n_wg, oracle, capfd, monkeypatch):
    """As many pieces as workgroups and a cap of exactly the share: every workgroup draws one ticket and leaves, and every piece
    has been scanned."""
    n = 4096 * 2 * n_wg
    cols = _columns(n, 34)
    tb = _table(ctx, "dyn_cap", cols, _even_sizes(n))
    ocols = [{"type": "int", "data": cols[c]} for c in NAMES]
    monkeypatch.setenv("SYBL_DYN_CAP_PCT", "100")
    for q in (Q3, Q2):
        ores = oracle.run_query(ocols, block_rows=65536, n_threads=16, **parity.oracle_query_kwargs(NAMES, INFO, q))
        st, err = _check(tb, q, ores, capfd, monkeypatch)
        assert DEALING.findall(err)[0][1::2] == (str(n_wg), "1"), err[-1000:]
    tb.free()


def test_rescans_and_two_queries_in_turns(main_table, capfd):
    T = main_table
    capfd.readouterr()
    q3, q2 = T.tb.query(**Q3), T.tb.query(**Q2)
    seen3, seen2 = [], []
    for _ in range(3):           # one prepared query, scanned three times
        r = q3.run()
        seen3.append(_fields(r))
        r.free()
    for _ in range(3):           # two prepared queries in turns
        r = q2.run()
        seen2.append(_fields(r))
        r.free()
        r = q3.run()
        seen3.append(_fields(r))
        r.free()
    r = q3.run()
    parity.compare(r, T.o3, op="hist", full=False, n_aggs=2)
    r.free()
    r = q2.run()
    parity.compare(r, T.o2, op="avg", full=True, n_aggs=2)
    r.free()
    assert all(s == seen3[0] for s in seen3) and all(s == seen2[0] for s in seen2)
    assert [int(d[0]) for d in DEALING.findall(capfd.readouterr().err)] == [1, 1]   # both dynamic, planned once each
    q3.free()
    q2.free()


def test_a_proof_that_fails_under_the_cap_keeps_the_plan_static(ctx, n_wg, oracle, capfd):
    """Ten tiles a workgroup: one replica word takes 10 * 4 * 1024 rows of up to 2^32 - 1 -- 48 bits of offsets under 16 bits of
    Count.  In pieces of two tiles a workgroup may draw ceil(5 * 5/4) + 2 = 9 of them, 18 tiles: 17 bits of Count, which no
    longer fit.  (The widths as tests/test_gpu_word_packing.py derives them.)"""
    T = 10
    static_rows = T * 4 * 1024
    assert static_rows.bit_length() + (static_rows * U32).bit_length() == 16 + 48
    n_pieces = T * n_wg // 2
    cap = -(-n_pieces * 125 // (100 * n_wg)) + 2
    cap_rows = cap * 2 * 4 * 1024
    assert cap == 9 and cap_rows.bit_length() + (cap_rows * U32).bit_length() == 17 + 49 > 64
    n = n_wg * T * 4096
    kc = np.full(n, 7, dtype=np.int64)
    wide = np.full(n, U32, dtype=np.int64)
    wide[12345] = 0
    tb = ctx.create_table("dyn_proof")
    tb.add_column("kc", "int", 0, 4095)     # (4096 cells x (Count, sum, max): one replica is all the LDS holds)
    tb.add_column("wide", "int", 0, U32)
    for r0 in range(0, n, 65536):
        tb.append_block(min(65536, n - r0), {"kc": kc[r0:r0 + 65536], "wide": wide[r0:r0 + 65536]})
    tb.set_bounds("kc", 0, 4095)
    tb.compact()
    assert [tb.column_storage(c) for c in ("kc", "wide")] == [(1, 7), (4, 0)]
    q = dict(groups=["kc"], aggs=["wide"], op="avg")
    res, st, err = _run(tb, q, capfd, dynamic=0)
    assert st["replicas"] == 1, st
    assert [tuple(int(x) for x in m) for m in CPACK.findall(err)] == [(48, 48, 16, static_rows)], err[-1000:]
    ores = oracle.run_query([{"type": "int", "data": kc}, {"type": "int", "data": wide}], block_rows=65536, n_threads=16,
                            **parity.oracle_query_kwargs(["kc", "wide"], {"kc": (0, 4095), "wide": (0, U32)}, q))
    parity.compare(res, ores, op="avg", full=True, n_aggs=1)
    rows = res.rows(0)
    assert len(rows) == 1 and (rows[0]["count"], rows[0]["hists"][0]["sum"]) == (n, (n - 1) * U32)
    res.free()
    tb.free()
