"""GPU: the lean row bodies of k_scan_packed (FastPlan::lean; planner.cpp: plan_lean, scan_packed.h: packed_row<LEAN, PROVED>,
scan_fast.h: fast_finish / sum_of).

In moments mode (op hist without bucket arrays) a (cell, replica) keeps NA + ceil(NA / 2) + NA LDS words instead of 1 + 3 NA:
Count above aggregation 0's sum of stored offsets, sum(b) of two aggregations in the two dwords of one word, sums of offsets
with Count * base added at the end.  Under a second proof the bucket quotient's correction multiplies in 24 bits and the
per-digit range compares go; and every kernel without validity bits derives its overflow count from matched rows and Counts.

Every case runs three ways -- the lean plan, SYBL_NO_LEAN=1, and the CPU oracle over the same host columns (tests/parity.py:
Count, Sum, extrema and bucket arrays exact, avg to 1e-6, stddev to 1e-9 of the oracle's exact one) -- and the two GPU runs
must agree to the last bit.  Tables are sized from the workgroup count of the device under test, as in
test_gpu_word_packing.py: n_wg * T * 4096 rows give every workgroup exactly T tiles.

Three or four aggregations run the body with run-time column counts (hashpacked.hip), which has no lean variant: those
cases check the results and that no lean plan is reported.  So a paired and an unpaired sum(b) word side by side (NA = 3) is
never exercised; the unpaired word alone (NA = 1) and the pair (NA = 2) are.
"""
import re

import numpy as np
import pytest

import sybil_amd
from sybil_amd._native import SyblError
from tests import parity

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
BLOCK = 65536
TILE = 4096
MOMENTS = re.compile(r"lean moments: lean=(\d) proved=(\d) digits=(\d) mul24=(\d) cshift=(\d+) count_bits=(\d+)(.*) slot_rows=(\d+) "
                     r"tried_replicas=(\d+) words=(\d+) replicas=(\d+)")
HIST = re.compile(r"lean hist: proved=(\d) digits=(\d) mul24=(\d)")


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


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


def _moments(err):
    out = []
    for m in MOMENTS.finditer(err):
        lean, proved, digits, mul24, cshift, count_bits, fields, slot_rows, tried, words, replicas = m.groups()
        out.append(dict(lean=int(lean), proved=int(proved), digits=int(digits), mul24=int(mul24), cshift=int(cshift),
                        count_bits=int(count_bits), fields={k: int(v) for k, v in re.findall(r"(\w+)_bits=(\d+)", fields)},
                        slot_rows=int(slot_rows), tried_replicas=int(tried), words=int(words), replicas=int(replicas)))
    return out


def _table(ctx, name, cols, info, bounds, n):
    """cols: {name: int64 array}; info: {name: (info_min, info_max)}; bounds: {name: (lo, hi)} declared for the key columns."""
    tb = ctx.create_table(name)
    for c in cols:
        tb.add_column(c, "int", *info[c])
    for r0 in range(0, n, BLOCK):
        tb.append_block(min(BLOCK, n - r0), {c: v[r0:r0 + BLOCK] for c, v in cols.items()})
    for c, (lo, hi) in bounds.items():
        tb.set_bounds(c, lo, hi)
    tb.compact()
    return tb


def _run(tb, q, capfd):
    capfd.readouterr()
    qy = tb.query(**q)
    try:
        res = qy.run()
        st = qy.stats()
    finally:
        qy.free()
    return res, st, capfd.readouterr().err


def _digest(res, n_aggs):
    """Everything the two GPU runs must agree on to the last bit."""
    rows = sorted((g["key"], g["count"]) + tuple((h["count"], h["sum"], h["min"], h["max"], h["avg"], h["stddev"]) +
                                                 ((h["values"].tolist(),) if "values" in h else ())
                                                 for h in g["hists"][:n_aggs]) for g in res.rows(0))
    c = res.cumulative
    return res.matched, rows, c["count"], [(h["count"], h["sum"], h["stddev"]) for h in c["hists"][:n_aggs]]


def _three_ways(tb, names, cols, info, q, oracle, capfd, monkeypatch, full=False):
    """The query with the lean plan, with SYBL_NO_LEAN=1 and through the oracle: (lean trace text, stats of the lean run)."""
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    monkeypatch.delenv("SYBL_NO_LEAN", raising=False)
    ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in names], n_threads=16, **parity.oracle_query_kwargs(names, info, q))
    res, st, err = _run(tb, q, capfd)
    parity.compare(res, ores, op="hist", full=full, n_aggs=len(q["aggs"]))
    lean = _digest(res, len(q["aggs"]))
    res.free()
    monkeypatch.setenv("SYBL_NO_LEAN", "1")
    res, st0, err0 = _run(tb, q, capfd)
    assert not MOMENTS.search(err0) and not HIST.search(err0), err0    # (switched off before anything is looked at)
    parity.compare(res, ores, op="hist", full=full, n_aggs=len(q["aggs"]))
    assert _digest(res, len(q["aggs"])) == lean
    res.free()
    monkeypatch.delenv("SYBL_NO_LEAN")
    return err, st, st0


# ---------------------------------------------------------------------------------------------- 1. shapes
class _Shapes:
    pass


@pytest.fixture(scope="module")
def shapes(ctx, n_wg):
    """Two tiles per workgroup and a ragged end.  a1 / a2 / a4: aggregation columns stored in 1, 2 and 4 bytes; an: a 2-byte
    column with a negative base; g1, g2: 1-byte keys (g2 never takes the value 5); f1..f3: filter columns."""
    S = _Shapes()
    n = n_wg * 2 * TILE + 777
    rng = np.random.default_rng(4242)
    S.n = n
    S.cols = {
        "g1": rng.integers(0, 7, n), "g2": rng.choice(np.array([0, 1, 2, 3, 4, 6, 7]), n),
        "f1": rng.integers(0, 1000, n), "f2": rng.integers(0, 100, n), "f3": rng.integers(-50, 50, n),
        "a1": rng.integers(10, 250, n), "a2": rng.integers(0, 60000, n), "a4": rng.integers(0, 3_000_000_000, n),
        "an": rng.integers(-5000, 20000, n),
    }
    S.cols["a1"][:3] = (10, 249, 10)
    S.cols["a2"][:2] = (0, 59999)
    S.cols["a4"][:2] = (0, 2_999_999_999)
    S.cols["an"][:2] = (-5000, 19999)
    S.info = {"g1": (0, 6), "g2": (0, 7), "f1": (0, 999), "f2": (0, 99), "f3": (-50, 49), "a1": (10, 249), "a2": (0, 60000),
              "a4": (0, 2_999_999_999), "an": (-5000, 20000)}   # (ranges the bucket size divides: no value can be an outlier)
    S.names = list(S.cols)
    S.tb = _table(ctx, "shapes", S.cols, S.info, {"g1": (0, 6), "g2": (0, 7)}, n)
    assert [S.tb.column_storage(c) for c in ("g1", "g2", "a1", "a2", "a4", "an")] == [(1, 0), (1, 0), (1, 10), (2, 0), (4, 0), (2, -5000)]
    yield S
    S.tb.free()


AGGS = [["a1"], ["a4"], ["a2", "an"], ["an", "a4"], ["a2", "a1", "an"], ["an", "a4", "a2", "a1"]]
FILTERS = [("f1", "gt", 99), ("f2", "lt", 90), ("f3", "gt", -40)]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("aggs", AGGS, ids="+".join)
def test_lean_moments_shapes(shapes, oracle, capfd, monkeypatch, aggs, n_groups, filtered):
    """NA = 1..4 (odd counts: an unpaired sum(b) word), one and two key columns, none and three filters, values stored in 1, 2
    and 4 bytes, a negative storage base (Count * base is added back with base < 0), a group no row reaches.  a4's bucket
    numerators pass 2^24: the lean layout is taken without the 24-bit multiply."""
    S = shapes
    na = len(aggs)
    q = dict(groups=["g1", "g2"][:n_groups], aggs=aggs, op="hist", want_percentiles=False, filters=FILTERS if filtered else [])
    err, st, st0 = _three_ways(S.tb, S.names, S.cols, S.info, q, oracle, capfd, monkeypatch)
    assert st["packed_kernel"] == 1 and st["strategy"] == 2, st
    assert st["n_sum_fields"] == st0["n_sum_fields"] == 1 + 3 * na      # (the published layout does not change)
    tr = _moments(err)
    if na <= 2:
        proved = 0 if "a4" in aggs else 1
        assert tr and all((t["lean"], t["digits"], t["mul24"], t["proved"]) == (1, 1, proved, proved) for t in tr), err
        assert all(t["words"] == 2 * na + (na + 1) // 2 and t["replicas"] == st["replicas"] and t["cshift"] >= 32 for t in tr), tr
        assert st["replicas"] >= st0["replicas"]
    else:
        assert tr == [], err      # (the run-time-count body: no lean plan)
        assert st["replicas"] == st0["replicas"]


# ---------------------------------------------------------------------------------------------- 2. S0 at its boundary
class _Wide:
    pass


@pytest.fixture(scope="module")
def wide(ctx, n_wg):
    """One group of a 4096-cell table (one replica is all the LDS holds, lean or not) over a 4-byte column whose offsets reach
    2^32 - 1: T = 15 tiles per workgroup are 61 440 rows a word -- 48 bits of offsets and 16 of Count."""
    W = _Wide()
    W.n15, W.n16 = n_wg * 15 * TILE, n_wg * 16 * TILE
    rng = np.random.default_rng(99)
    W.cols = {"kc": np.full(W.n16, 7, dtype=np.int64), "wide": rng.integers(0, 1 << 32, W.n16)}
    W.cols["wide"][:] |= 0xFFF00000          # (the sums come close to the bound the planner works with)
    W.cols["wide"][0], W.cols["wide"][1] = 0, U32
    W.info = {"kc": (0, 4095), "wide": (0, U32)}
    W.names = ["kc", "wide"]
    W.tb = W_tb = ctx.create_table("wide")
    W_tb.add_column("kc", "int", 0, 4095)
    W_tb.add_column("wide", "int", 0, U32)

    def append(r0, r1):
        for b in range(r0, r1, BLOCK):
            W_tb.append_block(BLOCK, {c: W.cols[c][b:b + BLOCK] for c in W.names})
    W.append = append
    append(0, W.n15)
    W_tb.set_bounds("kc", 0, 4095)
    W_tb.compact()
    assert [W_tb.column_storage(c) for c in W.names] == [(1, 7), (4, 0)]
    yield W
    W_tb.free()


def test_lean_moments_s0_boundary(wide, oracle, capfd, monkeypatch):
    """T = 15 packs (48 + 16 bits), T = 16 declines (48 + 17) and reports today's four words and one replica.  The bucket size
    is 4 294 967 (1002 buckets), so the numerators are far beyond 2^24: the lean layout runs with the 32-bit multiply."""
    W = wide
    q = dict(groups=["kc"], aggs=["wide"], op="hist", want_percentiles=False)
    assert W.tb.rows == W.n15
    cols15 = {c: v[:W.n15] for c, v in W.cols.items()}
    err, st, st0 = _three_ways(W.tb, W.names, cols15, W.info, q, oracle, capfd, monkeypatch)
    tr = _moments(err)
    assert tr and all((t["lean"], t["proved"], t["mul24"], t["cshift"], t["count_bits"], t["slot_rows"], t["words"], t["replicas"]) ==
                      (1, 0, 0, 48, 16, 61440, 3, 1) for t in tr), err
    assert all(t["fields"]["s0"] == 48 and t["fields"]["b0"] == (1001 * 61440).bit_length() for t in tr), tr
    assert (st["replicas"], st0["replicas"]) == (1, 1)
    W.append(W.n15, W.n16)
    W.tb.compact()
    assert W.tb.rows == W.n16
    err, st, st0 = _three_ways(W.tb, W.names, W.cols, W.info, q, oracle, capfd, monkeypatch)
    tr = _moments(err)
    assert tr and all((t["lean"], t["cshift"], t["count_bits"], t["slot_rows"], t["words"], t["replicas"]) == (0, 0, 17, 65536, 4, 1)
                      for t in tr), err
    assert (st["replicas"], st0["replicas"], st["lds_bytes"]) == (1, 1, st0["lds_bytes"])


# ---------------------------------------------------------------------------------------------- 3. replicas unfold without carrying
def test_lean_moments_replicas_unfold_without_carry(ctx, oracle, capfd, monkeypatch):
    """A 64-cell table replicated as often as the LDS holds it, with one hot cell of 4.4 M rows whose `lo` value sits in bucket
    1000: the cell's sum(b) over all replicas passes 2^32 while every replica's dword stays far below.  `hi`, a different
    column, shares the word: a carry out of the low dword would change its stddev.  Then 8 and 1 replicas.
    What catches such a carry is the bit-exact comparison of the lean run with the SYBL_NO_LEAN=1 run: one carry moves `hi`'s
    stddev by about 4e-7, inside the 1e-9 x scale (5e-7 here) the comparison with the oracle allows.
    (The 64 replicas of a 64-cell table do not exist for two aggregations: 64 x 64 x 5 words are 160 KiB, over the LDS budget.)"""
    n = 5_000_321
    rng = np.random.default_rng(31)
    g = rng.integers(0, 64, n)
    g[rng.random(n) < 0.88] = 21
    lo = rng.integers(0, 50_000, n)
    lo[g == 21] = 50_000                 # bucket 1000 of 0..50 000 in steps of 50
    hi = rng.integers(0, 1000, n)
    assert int((g == 21).sum()) >= 4_300_000 and int((g == 21).sum()) * 1000 > 1 << 32
    cols, info = {"g": g, "lo": lo, "hi": hi}, {"g": (0, 63), "lo": (0, 50_000), "hi": (0, 999)}
    tb = _table(ctx, "unfold", cols, info, {"g": (0, 63)}, n)
    q = dict(groups=["g"], aggs=["lo", "hi"], op="hist", want_percentiles=False)
    # a replica of the lean table is 64 cells x 5 words x 8 bytes = 2560 bytes: 32 of them fit the LDS budget (64 would be
    # 160 KiB), 8 fit 20 KiB, one is all that 2 KiB hold
    for replicas, budget in ((32, None), (8, "20"), (1, "2")):
        if budget:
            monkeypatch.setenv("SYBL_REP_BUDGET_KB", budget)
        err, st, st0 = _three_ways(tb, ["g", "lo", "hi"], cols, info, q, oracle, capfd, monkeypatch)
        tr = _moments(err)
        assert tr and all((t["lean"], t["words"], t["replicas"]) == (1, 5, replicas) for t in tr), err
        assert st["replicas"] == replicas
        for t in tr:   # every replica's sum(b) fits its dword; all of them together do not
            assert t["fields"]["b0"] <= 32 and t["slot_rows"] * 1000 < 1 << 32
    tb.free()


# ---------------------------------------------------------------------------------------------- 4. quotient edges
@pytest.mark.parametrize("bs,proved", [(1, 1), (999, 1), ((1 << 24) - 1, 1), (20000, 0)])
def test_bucket_quotient_edges(ctx, n_wg, oracle, capfd, monkeypatch, bs, proved):
    """Bucket arrays (exact to compare) over k * bs - 1, k * bs, k * bs + 1 for every bucket k the column can hold: with the
    24-bit multiply (numerators below 2^24) and, for bucket size 20 000, beyond it -- the proof declines and the 32-bit
    multiply runs.  With a bucket size just below 2^24 the numerators below 2^24 are buckets 0 and 1."""
    kmax = 1000 if bs * 1000 + 1 < (1 << 24) or not proved else ((1 << 24) - 1) // bs
    edges = np.array(sorted({v for k in range(kmax + 1) for v in (k * bs - 1, k * bs, k * bs + 1) if 0 <= v and (not proved or v < 1 << 24)}),
                     dtype=np.int64)
    n = n_wg * 2 * TILE + 333
    rng = np.random.default_rng(bs)
    x = edges[rng.integers(0, edges.size, n)]
    x[:edges.size] = edges
    g = rng.integers(0, 4, n)
    cols, info = {"g": g, "x": x}, {"g": (0, 3), "x": (0, int(edges.max()))}
    assert (int(edges.max()) >= 1 << 24) == (not proved)
    tb = _table(ctx, "quot", cols, info, {"g": (0, 3)}, n)
    q = dict(groups=["g"], aggs=["x"], op="hist", hist_bucket=bs, want_percentiles=True)
    err, st, st0 = _three_ways(tb, ["g", "x"], cols, info, q, oracle, capfd, monkeypatch, full=True)
    assert st["packed_kernel"] == 1 and st["strategy"] in (2, 6), st
    tr = [tuple(int(v) for v in m.groups()) for m in HIST.finditer(err)]
    assert tr and set(tr) == {(proved, 1, proved)}, err
    # ... and the same values through the lean moments body
    q = dict(q, want_percentiles=False)
    err, st, st0 = _three_ways(tb, ["g", "x"], cols, info, q, oracle, capfd, monkeypatch)
    tm = _moments(err)
    assert tm and all((t["lean"], t["proved"], t["mul24"]) == (1, proved, proved) for t in tm), err
    tb.free()


# ---------------------------------------------------------------------------------------------- 5. matched / overflow
def test_overflow_is_exact_and_the_range_proof_declines(ctx, n_wg, oracle, capfd, monkeypatch):
    """Keys 0..7 under declared bounds 0..5: the rows of keys 6 and 7 that pass the filter are out of bounds -- the range proof
    declines and the kernel's overflow count (derived from matched rows and Counts) is exactly theirs, lean or not.  With
    bounds that cover the keys the proof is taken and the result is the oracle's."""
    n = n_wg * 2 * TILE + 91
    rng = np.random.default_rng(5)
    cols = {"g": rng.integers(0, 8, n), "f": rng.integers(0, 100, n), "v": rng.integers(0, 1000, n)}
    info = {"g": (0, 7), "f": (0, 99), "v": (0, 999)}
    q = dict(groups=["g"], aggs=["v"], op="hist", want_percentiles=False, filters=[("f", "lt", 80)])
    lost = int(((cols["g"] > 5) & (cols["f"] < 80)).sum())
    assert lost > 0
    tb = _table(ctx, "oob", cols, info, {"g": (0, 5)}, n)
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    for no_lean in (False, True):
        if no_lean:
            monkeypatch.setenv("SYBL_NO_LEAN", "1")
        capfd.readouterr()
        qy = tb.query(**q)
        with pytest.raises(SyblError, match=r"\b%d rows fell outside the declared column bounds" % lost):
            qy.run()
        qy.free()
        tr = _moments(capfd.readouterr().err)
        if not no_lean:
            assert tr and all((t["lean"], t["digits"], t["proved"]) == (1, 0, 0) for t in tr), tr
    monkeypatch.delenv("SYBL_NO_LEAN")
    tb.free()
    tb = _table(ctx, "inb", cols, info, {"g": (0, 7)}, n)
    err, st, st0 = _three_ways(tb, ["g", "f", "v"], cols, info, q, oracle, capfd, monkeypatch)
    tr = _moments(err)
    assert tr and all((t["lean"], t["digits"], t["proved"]) == (1, 1, 1) for t in tr), err
    tb.free()
