"""GPU: the LDS time-window scan (strategies 3 and 4, DESIGN 3.2 `lds-window`) at the edges of its windows.

A time series whose [time bucket][group] table does not fit LDS is scanned by workgroups that each hold a window
[wg_cell_base, + lds_cells) of it (planner.cpp: Planner::window), accumulate at lcell = cell - cell_base and flush the touched
cells into the global table with device-scope fetch_add / fetch_max.  Five kernel families share that path: k_scan<.., USE_LDS>
(strategy 3), k_scan_fast plain and GEN, k_scan_packed plain and NUL, k_scan_hash_packed<.., HASH = false> (three or four keys or
aggregations) and fast_finish's flush through sum_of / max_of for the plain, cshift and lean LDS word layouts.  A mistake there
either trips kHdrOverflow or puts a row into the neighbouring time bucket -- silently.

The tables of tests/window_layout.py PLACE rows at a window's first and last bucket, make two workgroups flush into the same
cells, put a window next to the 152 KiB budget (plan.h: kLdsBudgetBytes), give workgroups no segment or no window, skip blocks,
and declare bounds that put wg_cell_base next to fill_packed's 2^24-cell limit; tests/test_window_layout.py checks the placement
and the reference on the CPU.

Every check (`_check`) asserts the strategy and packed_kernel the case expects and the `window:` trace line's wmax against
window_layout.windows(); compares counts, sums, min / max and bucket arrays with window_layout.reference() bit for bit, every
field with the CPU oracle (parity.compare), and field for field with the same query under SYBL_NO_WINDOW=1 -- global atomics, an
independent GPU path, asserted not to be strategy 3 or 4.  What ran is collected in SEEN (printed by the last test).
"""
import re
import types

import numpy as np
import pytest

import sybil_amd
from tests import parity
from tests import window_layout as WL
from tests.test_window_layout import bucket_sizes, check_reference, oracle_answer

pytestmark = pytest.mark.gpu

WINDOW_LINE = re.compile(r"^window: windowed=(\d) wmax=(\d+) cells=(\d+) lds_cells=(\d+) replicas=(\d+) why=(\S+)$", re.M)
CPACK_LINE = re.compile(r"^count packing: cshift=(\d+) ", re.M)
LEAN_LINE = re.compile(r"^lean moments: lean=(\d) ", re.M)
LATE_LINE = re.compile(r"^late path: kernel=(\w+) ", re.M)
SYBL_E_STATE, SYBL_E_NODEVICE = -5, -2
SEEN = {}       # (case, storage, query, settings) -> (strategy, packed_kernel, kernel of the `late path:` line or None)
BUILDERS = {"spike": WL.spike, "straddle": WL.straddle, "small_blocks": WL.small_blocks, "idle": WL.idle, "nullable": WL.nullable,
            "signed": WL.signed, "skips": WL.skips, "wide_below": lambda n_wg: WL.wide_declared(65535),
            "wide_at": lambda n_wg: WL.wide_declared(65536)}


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


def build_table(ctx, L, compact):
    tb = ctx.create_table(L.name)
    for c in WL.COLUMN_ORDER:
        tb.add_column(c, "int", *WL.INFO.get(c, (1, 0)))
    r0 = 0
    for b in L.blocks:
        tb.append_block(b, {c: ((L.cols[c][r0:r0 + b], L.pop[c][r0:r0 + b]) if c in L.pop else L.cols[c][r0:r0 + b]) for c in WL.COLUMN_ORDER})
        r0 += b
    assert tb.rows == L.n
    for c in WL.COLUMN_ORDER:
        tb.set_bounds(c, *L.declared(c), has_missing=c in L.pop)
    if compact:
        tb.compact()
        for c, nbytes in WL.STORED_BYTES.items():
            assert tb.column_storage(c)[0] == nbytes, (L.name, c, tb.column_storage(c))
    return tb


@pytest.fixture(scope="module")
def world(ctx, n_wg, oracle):
    """One layout per case and one resident table per (case, storage), built on first use and kept for the module; the oracle's
    answer and the reference per (case, query), computed once."""
    W = types.SimpleNamespace(n_wg=n_wg, layouts={}, tables={}, answers={})

    def layout(case):
        if case not in W.layouts:
            W.layouts[case] = BUILDERS[case](n_wg)
        return W.layouts[case]

    def table(case, storage):
        if (case, storage) not in W.tables:
            W.tables[(case, storage)] = build_table(ctx, layout(case), storage == "compact")
        return W.tables[(case, storage)]

    def answer(case, qkey, q, L=None):
        if (case, qkey) not in W.answers:
            L = L or layout(case)
            ores = oracle_answer(oracle, L, q)
            ref = WL.reference(L, q, bucket_sizes(ores, q))
            check_reference(ref, ores, q)                # the two references agree at this size too
            W.answers[(case, qkey)] = (ref, ores)
        return W.answers[(case, qkey)]

    W.layout, W.table, W.answer = layout, table, answer
    yield W
    for tb in W.tables.values():
        tb.free()


# ---------------------------------------------------------------------------------------------- running and checking
def _signed64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


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


def _run(tb, q, capfd, monkeypatch, env):
    with monkeypatch.context() as m:
        m.setenv("SYBL_PLAN_TRACE", "1")
        for k, v in env.items():
            m.setenv(k, v)
        capfd.readouterr()
        qy = tb.query(**q)
        try:
            res = qy.run()
            st = qy.stats()
        except sybil_amd.SyblError as ex:
            if ex.code == SYBL_E_NODEVICE:      # a HIP call failed: nothing more is started on a device that may have faulted
                pytest.exit("HIP failure, session ended: %s" % ex, returncode=3)
            raise
        finally:
            qy.free()
        return res, st, capfd.readouterr().err


def _against_reference(res, ref, q, what):
    """Every (time bucket, key) row of the reference and no other: Count, Samples, per aggregation count, sum, min / max and, for a
    full histogram, the bucket array.  BasicHist.Min / Max start at 0 in avg mode, at Info.Min / Info.Max in hist mode."""
    rows = res.rows(1, want_values=True)
    got = {(r["time_bucket"],) + tuple(_signed64(v) for v in r["key_vals"]): r for r in rows}
    assert res.matched == ref["matched"], (what, res.matched, ref["matched"])
    assert len(rows) == len(got) and set(got) == set(ref["groups"]), (what, len(rows), len(ref["groups"]), sorted(set(got) ^ set(ref["groups"]))[:8])
    bad = []
    for key, (count, samples, aggs) in ref["groups"].items():
        g = got[key]
        if (g["count"], g["samples"]) != (count, samples):
            bad.append((key, "count", g["count"], g["samples"], count, samples))
        for name, (total, lo, hi, buckets), h in zip(q["aggs"], aggs, g["hists"]):
            start = WL.INFO[name] if q["op"] == "hist" else (0, 0)
            if not h["present"] or (h["count"], h["sum"]) != (count, total):
                bad.append((key, name, "sum", h["present"], h["count"], h["sum"], count, total))
            if (h["min"], h["max"]) != (min(lo, start[0]), max(hi, start[1])):
                bad.append((key, name, "extrema", h["min"], h["max"], lo, hi))
            if buckets is not None:
                v = h.get("values")
                if v is None or v.size < buckets.size or not np.array_equal(v[:buckets.size], buckets) or v[buckets.size:].any():
                    bad.append((key, name, "buckets"))
    assert not bad, (what, len(bad), bad[:6])
    assert res.cumulative["count"] == sum(g[0] for g in ref["groups"].values()), what


def _check(W, capfd, monkeypatch, case, storage, qkey, expect, env=None, q=None, layout=None, table=None, scanned=None, windowed=True):
    """See the module docstring.  expect: (strategy or a tuple of strategies, packed_kernel).  Returns (stats, trace)."""
    env = env or {}
    q = q or WL.QUERIES[qkey]
    L = layout or W.layout(case)
    tb = table or W.table(case, storage)
    what = (case, storage, qkey, sorted(env.items()))
    ref, ores = W.answer(L.name, qkey, q, L)
    res, st, err = _run(tb, q, capfd, monkeypatch, env)
    try:
        late = LATE_LINE.findall(err)
        SEEN[(case, storage, qkey, " ".join("%s=%s" % kv for kv in sorted(env.items())))] = (st["strategy"], st["packed_kernel"], late[0] if late else None)
        strategies = expect[0] if isinstance(expect[0], tuple) else (expect[0],)
        assert st["strategy"] in strategies and st["packed_kernel"] == expect[1] and st["n_workgroups"] == W.n_wg, (what, st, err[-1500:])
        lines = WINDOW_LINE.findall(err)
        assert len(lines) == 1, (what, err[-1500:])
        _, wmax, inside = WL.layout_windows(L, W.n_wg, scanned)
        cells = WL.cells_of(q, L)
        fields = st["n_sum_fields"] + st["n_max_fields"]
        assert inside
        if windowed:
            assert lines[0][:3] == ("1", str(wmax), str(cells)) and lines[0][5] == "ok", (what, lines, wmax, cells)
            assert int(lines[0][3]) == wmax * cells and WL.window_bytes(wmax, cells, fields) <= WL.LDS_BUDGET, (what, lines, fields)
        else:
            assert lines[0][:3] == ("0", str(wmax), str(cells)) and lines[0][5] == "budget", (what, lines, wmax, cells)
            assert WL.window_bytes(wmax, cells, fields) > WL.LDS_BUDGET, (what, lines, fields)
        _against_reference(res, ref, q, what)
        parity.compare(res, ores, op=q["op"], full=bool(q.get("want_percentiles")), n_aggs=len(q["aggs"]), time_mode=True)
        got = _fields(res)
    finally:
        res.free()
    res, st0, err0 = _run(tb, q, capfd, monkeypatch, dict(env, SYBL_NO_WINDOW="1"))
    try:
        assert st0["strategy"] not in (3, 4), (what, st0)
        if windowed:
            assert [l[5] for l in WINDOW_LINE.findall(err0)] == ["SYBL_NO_WINDOW"], (what, err0[-1500:])
        assert _fields(res) == got, what
    finally:
        res.free()
    return st, err


COMPACT_MATRIX = {
    # query: (strategy, packed_kernel), the kernel family of the `late path:` line (None: no packed plan)
    "avg": ((4, 1), "packed"),
    "signed_agg": ((4, 1), "packed"),
    "lean1": ((4, 1), "packed"),
    "lean2": ((4, 1), "packed"),
    "full": ((4, 1), "packed"),
    "weighted": ((4, 0), None),             # a weight column: the GEN body of k_scan_fast over compact storage
    "keys3": ((4, 1), "packed_n"),          # k_scan_hash_packed<.., HASH = false>
    "aggs3": ((4, 1), "packed_n"),
    "range": ((4, 1), "packed"),
    "five": ((4, 1), "packed"),             # the pre-pass bitmap (Planner::prefilter) and a window
}


@pytest.mark.parametrize("qkey", list(COMPACT_MATRIX))
@pytest.mark.parametrize("case", ["spike", "straddle"])
def test_matrix_on_compact_storage(world, capfd, monkeypatch, case, qkey):
    expect, kernel = COMPACT_MATRIX[qkey]
    st, err = _check(world, capfd, monkeypatch, case, "compact", qkey, expect)
    assert LATE_LINE.findall(err) == ([kernel] if kernel else []), err[-1500:]
    if qkey == "avg":
        # Count packed into the sum word (FastPlan::cshift), then the plain word layout
        assert int(CPACK_LINE.findall(err)[0]) > 0, err[-1500:]
        st, err = _check(world, capfd, monkeypatch, case, "compact", qkey, expect, env={"SYBL_NO_CPACK": "1"})
        assert not CPACK_LINE.findall(err) or int(CPACK_LINE.findall(err)[0]) == 0
    if qkey in ("lean1", "lean2"):
        assert LEAN_LINE.findall(err) == ["1"], err[-1500:]
        st, err = _check(world, capfd, monkeypatch, case, "compact", qkey, expect, env={"SYBL_NO_LEAN": "1"})
        assert LEAN_LINE.findall(err) in ([], ["0"])
    if qkey == "full":
        assert st["strategy"] != 5          # (q->time_mode keeps the partitioned histograms away)
    if qkey == "five":
        # five filter columns are one more than the packed row bodies evaluate: packed_kernel == 1 means the pre-pass ran
        assert len({f[0] for f in WL.QUERIES[qkey]["filters"]}) == 5


@pytest.mark.parametrize("case", ["spike", "straddle"])
def test_canonical_storage(world, capfd, monkeypatch, case):
    _check(world, capfd, monkeypatch, case, "canonical", "avg", (4, 0))             # k_scan_fast


@pytest.mark.parametrize("case", ["spike", "straddle"])
def test_generic_kernel(world, capfd, monkeypatch, case):
    _check(world, capfd, monkeypatch, case, "compact", "avg", (3, 0), env={"SYBL_NO_FAST": "1"})      # k_scan<.., USE_LDS>


@pytest.mark.parametrize("qkey", WL.FIRST_TWO)
@pytest.mark.parametrize("case", ["small_blocks", "idle"])
def test_small_blocks_and_idle_workgroups(world, capfd, monkeypatch, case, qkey):
    _check(world, capfd, monkeypatch, case, "compact", qkey, (4, 1))
    if case == "idle":
        assert sum(1 for s in WL.shares(world.layout(case).blocks, world.n_wg) if s) == 6


@pytest.mark.parametrize("qkey", ["avg", "nullable_key", "nullable_key_signed"])
@pytest.mark.parametrize("storage", ["compact", "canonical"])
def test_nullable_time_and_key(world, capfd, monkeypatch, storage, qkey):
    """Missing time values, a block and a whole share without any, the MISSING digit: k_scan_packed<NUL> / k_scan_fast<GEN>."""
    _check(world, capfd, monkeypatch, "nullable", storage, qkey, (4, 1 if storage == "compact" else 0))
    wins = WL.layout_windows(world.layout("nullable"), world.n_wg)[0]
    assert [g for g, w in enumerate(wins) if w is None] == [2 * world.n_wg // 3]


@pytest.mark.parametrize("qkey", WL.FIRST_TWO)
@pytest.mark.parametrize("storage", ["compact", "canonical"])
def test_signed_times(world, capfd, monkeypatch, storage, qkey):
    """Negative times: bucket 0 is double width; compact storage declines the packed body (exact_min < 0)."""
    _check(world, capfd, monkeypatch, "signed", storage, qkey, ((3, 4), 0))


def test_skipped_blocks(world, capfd, monkeypatch):
    L = world.layout("skips")
    for qkey, q in (("skip_s", WL.QUERIES["skip_s"]),
                    ("skip_t", WL._q(filters=[("t", "gt", WL.T0 + (world.n_wg // 4) * WL.TB - 1)], groups=["k2"], aggs=["a4"], block_skip=True))):
        scanned = WL.skips_scanned(L, q["filters"])
        assert 0 < scanned.count(False) < len(scanned)
        st, err = _check(world, capfd, monkeypatch, "skips", "compact", qkey, (4, 1), q=q, scanned=scanned)
        assert st["blocks_skipped"] == scanned.count(False), (qkey, st)
        assert world.answer("skips", qkey, q)[1]["blocks_skipped"] == scanned.count(False)
    for qkey in WL.FIRST_TWO:
        _check(world, capfd, monkeypatch, "skips", "compact", qkey, (4, 1))


@pytest.mark.parametrize("case,packed", [("wide_below", 1), ("wide_at", 0)])
def test_wide_declared_bounds(world, capfd, monkeypatch, case, packed):
    """wg_cell_base next to the top of a 2^24-cell table: below fill_packed's limit on k_scan_packed, at it off it."""
    st, err = _check(world, capfd, monkeypatch, case, "compact", "wide", (4, packed))
    assert st["n_cells"] == WL.PACKED_CELL_LIMIT - (256 if packed else 0)


def test_budget(world, ctx, capfd, monkeypatch):
    """A window next to kLdsBudgetBytes: the widest that fits is windowed and takes exactly its bytes, one bucket more is not."""
    q = WL.QUERIES["avg"]
    res, st, _ = _run(world.table("spike", "compact"), q, capfd, monkeypatch, {})
    res.free()
    fields = st["n_sum_fields"] + st["n_max_fields"]
    cells = WL.cells_of(q)
    w_fit = WL.fit(cells, fields)
    assert w_fit * cells * fields * 8 <= 152 * 1024 < (w_fit + 1) * cells * fields * 8 and w_fit >= 3
    for W_, windowed in ((w_fit, True), (w_fit + 1, False)):
        L = WL.budget(world.n_wg, W_)
        assert WL.layout_windows(L, world.n_wg)[1] == W_
        tb = build_table(ctx, L, True)
        try:
            if windowed:
                st, err = _check(world, capfd, monkeypatch, L.name, "compact", "avg", (4, 1), layout=L, table=tb)
                assert st["lds_bytes"] // st["replicas"] == WL.window_bytes(W_, cells, fields) and st["lds_bytes"] % st["replicas"] == 0, st
            else:
                st, err = _check(world, capfd, monkeypatch, L.name, "compact", "avg", (1, 0), layout=L, table=tb, windowed=False)
        finally:
            tb.free()


def test_rescan_and_replan(world, ctx, capfd, monkeypatch):
    L = world.layout("spike")
    q = WL.QUERIES["avg"]
    ref, ores = world.answer("spike", "avg", q)
    tb = build_table(ctx, L, True)
    try:
        monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
        qy = tb.query(**q)
        snaps = []
        for _ in range(3):
            res = qy.run()
            _against_reference(res, ref, q, "rescan")
            snaps.append(_fields(res))
            res.free()
        assert qy.stats()["strategy"] == 4 and snaps[0] == snaps[1] == snaps[2]
        # a block of later times: the prepared query is stale, a fresh one is windowed again over the grown table
        last = int(L.cols["t"].max()) // WL.TB
        grown, extra = WL.appended(L, WL._spread((last + 2) * WL.TB - 1, (last + 3) * WL.TB + 1, WL.SHARE), seed=99)
        tb.append_block(WL.SHARE, {c: extra[c] for c in WL.COLUMN_ORDER})
        with pytest.raises(sybil_amd.SyblError) as ei:
            qy.run()
        assert ei.value.code == SYBL_E_STATE
        qy.free()
        grown.name = "spike_grown"
        st, err = _check(world, capfd, monkeypatch, "spike_grown", "compact", "avg", (4, 1), layout=grown, table=tb)
        assert WL.layout_windows(grown, world.n_wg)[1] >= 3        # (four more units: the shares no longer end where the blocks do)
    finally:
        tb.free()


def test_what_ran(world):
    """Not a check of the engine: prints what the cases above were seen to run (pytest -s)."""
    for k in sorted(SEEN):
        print("SEEN %-14s %-9s %-20s %-18s strategy=%d packed_kernel=%d late_path_kernel=%s" % (k + SEEN[k]))
    assert {v[0] for v in SEEN.values()} >= {3, 4} or not SEEN
