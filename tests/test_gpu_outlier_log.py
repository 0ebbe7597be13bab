"""GPU: the outlier log (csrc/plan.h, csrc/outlog.h, k_outlog_gather in csrc/kernels.hip, out_log_begin / out_log_end in
csrc/engine.cpp, csrc/result.cpp at "outlier values") where its stripes fill, spill and run out.

The rest of the suite runs the log at its default 2^20 records (no stripe ever fills) and at SYBL_OUTLIER_LOG_CAP=16 (one
place per stripe, nearly everything dropped).  Here the capacity is set between those, on tables (tests/outlog_cases.py, checked
on the CPU by tests/test_outlog_cases.py) whose outlier values are all distinct and, for the one-wave tables, all belong to
wave 0 of one workgroup -- so that what the log must do follows from a model of ONE wave (outlog_cases.one_wave_outcome).

Paths (PATHS; every case asserts the one it ran through, from stats() and the SYBL_PLAN_TRACE lines of its own prepare):
  scan          k_scan (scan_generic.h: row_accumulate)              SYBL_NO_FAST=1 SYBL_NO_PARTHIST=1     strategy 0
  part_few      k_part_hist, 256 workgroups sharing ONE partition    SYBL_NO_FAST=1                        strategy 5
  fast         k_scan_fast, GEN body (scan_fast.h: fast_accumulate)  canonical storage                     strategy 6
  packed        k_scan_packed (scan_packed.h: packed_row)            compact storage                       strategy 6, packed
  hash_compact  SYBL_FORCE_HASH=1 over compact storage                                                      strategy 7
  hash_generic  k_scan_hash (hashgroup.hip)                          SYBL_FORCE_HASH=1 SYBL_NO_FAST=1      strategy 7
  part1, part3  k_part_hist (kernels.hip: part_outlier)              65 536 / 1024 declared groups         strategy 5
scan: SYBL_NO_FAST=1 alone does NOT reach k_scan with this query -- select_part_hist (planner.cpp) steps aside only for a fast
plan with LDS bucket arrays (`q->fast && q->fplan.hist_lds`), so a five-group histogram query without the fast path becomes
partitioned histograms (by the same rule the SYBL_NO_FAST leg of test_outlier_values_are_kept_and_printed, which asserts no
strategy, is k_part_hist's as well).  That is path part_few here; k_scan takes SYBL_NO_PARTHIST=1 besides.
hash_compact: a query that keeps a log keeps bucket arrays (planner.cpp: `any_out && q->want_percentiles`), and
select_hash_fast leaves such a query to k_scan_hash_fast (`try_packed` excludes `op == hist && want_percentiles`; so does the
run-time-column-count form, select_fast_path) -- over compact storage too.  k_scan_hash_packed's call of log_outlier
(hashpacked.hip) is therefore never reached with a log; what runs, and what this path asserts (`hash tables: .. kernel=fast`),
is k_scan_hash_fast with fast_accumulate's call, the log naming groups by composite key.
part3 is config 3's 1024 groups with three aggregations in the order c07, c09, c08 at -hist-bucket 940: two passes of
count -> emit -> k_part_hist append to one log, the first with agg0 = 0 (c07's outliers), the second with agg0 = 2 (c08's).

Every run, whatever the capacity (_examine):
* counts, bucket arrays, percentiles, n_outliers and stddev equal the oracle's (parity.compare, op="hist", full=True);
* the completeness flag is all-or-nothing: every histogram with outliers has n_outlier_values == n_outliers, or every one -1
  (result.cpp skips a record whose cell is not live or whose aggregation is out of range: a misplaced record shows up here as
  a histogram with fewer values than outliers);
* complete: outlier_values equal the oracle's per group and aggregation -- asserted here, not left to compare_hist's
  conditional --, and the table's own claim (outlog_cases.claimed_outliers); render("json") and encode() succeed, and for the
  placed tables every outlier is printed under its own value; not complete: render("json") and encode() raise SyblError.

A. test_one_wave_thresholds: capacity 64 * per for per in {1, 4}, set exactly (64, 256) and reached by the planner's rounding
   (1 -> 64, 193 -> 256: planner.cpp `(cap + kOutStripes - 1) / kOutStripes * kOutStripes`), tables of n = per, per + 1,
   8 * per and 8 * per + 1 outliers in one wave.
   - n = per complete: the home stripe alone takes them -- `if (i < per)` of outlog.h stores ranks up to per - 1, the last
     place of the stripe included.
   - n = per + 1 complete: the first spill -- the lane with `i >= per` stays `pending`, goes round the `for (t < kOutSpill)`
     loop and reserves in stripe home + 1; the gather reads the home cursor at per + something and takes `per` of it.
   - n = 8 * per complete with exact values: every one of the stripes home .. home + 7 is filled to its last place
     (`(home + t) & (kOutStripes - 1)`, t up to kOutSpill - 1 = 7), at least one reservation straddles a stripe's end (the
     fetch-add of `popcount(here)` takes the cursor past `per`; test_outlog_cases: replay()["straddles"] >= 1 under both row
     mappings), and k_outlog_gather's `n = c < per ? c : per` is what makes `kept`, `before` and `mine` right: without the clamp
     the header counts more records than were written and the stripes behind an over-run one land too far up the dense log.
     A record stored one place off (`i <= per`, `stripe * per + i` with another stride) or a spill loop one step short loses
     or misattributes a distinct value.
   - n = 8 * per + 1 must come out -1 with exact counts: the ninth stripe is not tried, the lane left `pending` after the loop
     stores the home stripe's `dropped` word, and the gather's `dropped != 0 ? cap + 1 : kept` turns it into "more than the
     capacity" (result.cpp: `n_out_log <= q->out_cap`).
   hash_generic (path e) and hash_compact keep the mapping `row = seg.start + tid * kRowsPerThread`, so they run here too;
   part1 / part3 (k_part_hist walks records sorted by partition, not rows) are left to part B.
B. test_many_waves_bounds: N outliers over many waves; capacity 64 * N (per >= N: no stripe can fill, must be complete), the
   largest multiple of 64 below N (pigeonhole: must be -1), and N, 2 N and 8 N, where the outcome depends on how many
   workgroups the device runs: printed (`outlier log: ...` in the captured output), not asserted -- a run that reports complete
   has exact values all the same.  (At N rounded up a stripe holds the AVERAGE share: unless every stripe received exactly
   that, some filled and their waves went on to the next -- the spill between waves of different workgroups.)
C. test_rescans: one Query run twice at the exact fit (both complete and identical: out_log_begin zeroes cursors AND flags --
   a cursor left standing makes the second run spill further and drop) and twice at 8 * per + 1 (both -1 with exact counts),
   then a fresh query at the default capacity on the same table (complete).
D. test_time_series: outliers in two time buckets of the same group land in the right (time_bucket, key) row of time_results,
   at the default capacity and at the one-wave exact fit.

One process, one Context; tables and oracle results are built once per module.
"""
import json
import re
import types

import numpy as np
import pytest

import sybil_amd
from sybil_amd import synth
from tests import outlog_cases as OC
from tests import parity

pytestmark = pytest.mark.gpu

# every switch that moves a query between the paths below, or changes the log: unset unless the path sets it
SWITCHES = ("SYBL_NO_FAST", "SYBL_FORCE_HASH", "SYBL_OUTLIER_LOG_CAP", "SYBL_NO_OUTLIER_LOG", "SYBL_NO_PARTHIST", "SYBL_NO_LDSHIST",
            "SYBL_NO_FASTGEN", "SYBL_NO_HASH_FAST", "SYBL_NO_HASH_PACKED", "SYBL_NO_PACKED_N", "SYBL_LAZY_ROWS")
REJECTED = r"fast path: rejected at"
PATHS = {
    "scan": dict(env={"SYBL_NO_FAST": "1", "SYBL_NO_PARTHIST": "1"}, compact=False, strategy=0, packed=0, trace=[REJECTED],
                 absent=[r"hash tables:", r"part hist: pass="]),
    "part_few": dict(env={"SYBL_NO_FAST": "1"}, compact=False, strategy=5, packed=0,
                     trace=[REJECTED, r"part hist: pass=0 aggs=1 packed=0 .* parts=1 .* out=1 "], absent=[r"part hist: pass=1"]),
    "fast": dict(env={}, compact=False, strategy=6, packed=0, trace=[], absent=[REJECTED, r"hash tables:", r"late path:"]),
    "packed": dict(env={}, compact=True, strategy=6, packed=1, trace=[r"late path: kernel=packed "], absent=[REJECTED, r"hash tables:"]),
    "hash_compact": dict(env={"SYBL_FORCE_HASH": "1"}, compact=True, strategy=7, packed=0, trace=[r"hash tables: .* kernel=fast "], absent=[]),
    "hash_generic": dict(env={"SYBL_FORCE_HASH": "1", "SYBL_NO_FAST": "1"}, compact=False, strategy=7, packed=0,
                         trace=[r"hash tables: .* kernel=generic "], absent=[]),
    "part1": dict(env={}, compact=False, strategy=5, packed=0, trace=[r"part hist: pass=0 aggs=1 packed=0 .* out=1 "], absent=[r"part hist: pass=1"]),
    "part3": dict(env={}, compact=True, strategy=5, packed=1,
                  trace=[r"part hist: pass=0 aggs=2 packed=1 .* out=1 ", r"part hist: pass=1 aggs=1 packed=1 .* out=1 "], absent=[]),
}
WAVE_PATHS = ("scan", "fast", "packed", "hash_compact", "hash_generic")
PART1_ROWS, PART3_ROWS = 30_000, 300_000


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """Tables (built on first use, per storage) and oracle results (once per table), shared by every test of the file."""
    W = types.SimpleNamespace(tables={}, cases={}, oracles={})

    def case(name):
        if name not in W.cases:
            kind, n = re.match(r"([a-z]+)(\d*)", name).groups()
            W.cases[name] = {"wave": OC.one_wave, "time": OC.time_wave}[kind](int(n)) if n else OC.many_waves()
        return W.cases[name]

    def table(name, compact):
        if (name, compact) not in W.tables:
            if name in ("part1", "part3"):
                cols, rows = _part_columns(name)
                tb = ctx.synth_table(name, synth.SEED, rows, 0, rows, synth.synth_cols(cols))
            else:
                c = case(name)
                names = ["g", "v"] + (["t"] if "t" in c.cols else [])
                tb = ctx.create_table(name)
                tb.add_column("g", "int")
                tb.add_column("v", "int", *OC.INFO)
                if "t" in c.cols:
                    tb.add_column("t", "int")
                r0 = 0
                for b in c.blocks:
                    tb.append_block(b, {k: c.cols[k][r0:r0 + b] for k in names})
                    r0 += b
            if compact:
                tb.compact()
            W.tables[(name, compact)] = tb
        return W.tables[(name, compact)]

    def reference(name):
        if name not in W.oracles:
            if name in ("part1", "part3"):
                cols, rows = _part_columns(name)
                info = {k: (synth.COLUMNS[k][4], synth.COLUMNS[k][5]) for k in cols}
                W.oracles[name] = oracle.run_query(parity.oracle_synth_cols(oracle, cols, rows, 0, rows), block_rows=65536, n_threads=4,
                                                   **parity.oracle_query_kwargs(cols, info, _part_query(name)))
            else:
                W.oracles[name] = OC.oracle_result(oracle, case(name), time=name.startswith("time"))
        return W.oracles[name]

    W.case, W.table, W.reference = case, table, reference
    yield W
    for tb in W.tables.values():
        tb.free()


def _part_columns(name):
    wl = synth.WORKLOADS["cfg4_hist_highcard" if name == "part1" else "cfg3_filter3_group2_stddev"]
    return (wl["columns"], PART1_ROWS) if name == "part1" else (wl["columns"] + ["c09"], PART3_ROWS)


def _part_query(name):
    if name == "part1":
        return dict(synth.WORKLOADS["cfg4_hist_highcard"]["query"], hist_bucket=990)
    return dict(synth.WORKLOADS["cfg3_filter3_group2_stddev"]["query"], aggs=["c07", "c09", "c08"], want_percentiles=True, hist_bucket=940)


def _n_logged(ores, n_aggs, time_mode=False):
    """Records a complete log holds: the outliers of every histogram of the rows the log serves."""
    return sum(r["hists"][a]["n_outliers"] + r["hists"][a]["n_underliers"] for r in ores["time_results" if time_mode else "results"]
               for a in range(n_aggs) if r["hists"][a]["present"])


# ---------------------------------------------------------------------------------------------- running and checking
def _examine(res, ores, n_aggs, time_mode, claim, what):
    """The assertions of every run (module docstring).  Returns (complete, a digest of everything the rows carry)."""
    parity.compare(res, ores, op="hist", full=True, n_aggs=n_aggs, time_mode=time_mode)
    grows = {(r["time_bucket"], r["key"]): r for r in res.rows(1 if time_mode else 0)}
    orows = {(r["time_bucket"], r["key"]): r for r in ores["time_results" if time_mode else "results"]}
    assert set(grows) == set(orows), what
    flags, digest = [], {}
    empty = np.zeros(0, dtype=np.int64)
    for k, o in orows.items():
        for a in range(n_aggs):
            oh, gh = o["hists"][a], grows[k]["hists"][a]
            if not oh["present"]:
                continue
            no = oh["n_outliers"] + oh["n_underliers"]
            assert gh["n_outliers"] == no, (what, k, a)
            digest[(k, a)] = (gh["count"], gh["sum"], no, gh["n_outlier_values"], gh.get("outlier_values", empty).tolist(),
                              gh["values"].tolist(), gh.get("percentiles", empty).tolist(), gh["stddev"])
            if no:
                flags.append((gh["n_outlier_values"], no, k, a))
    assert flags, what
    complete = all(got == no for got, no, _, _ in flags)
    assert complete or all(got == -1 for got, _, _, _ in flags), (what, [f for f in flags if f[0] not in (-1, f[1])][:5], len(flags))
    if not complete:
        with pytest.raises(sybil_amd.SyblError):
            res.render("json")
        with pytest.raises(sybil_amd.SyblError):
            res.encode()
        return False, digest
    for k, o in orows.items():
        for a in range(n_aggs):
            oh, gh = o["hists"][a], grows[k]["hists"][a]
            if not oh["present"]:
                continue
            got = gh.get("outlier_values", empty)
            assert np.array_equal(got, np.sort(oh["outlier_values"])), (what, k, a, got[:8], np.sort(oh["outlier_values"])[:8])
            assert gh["n_outlier_values"] == got.size
    out = json.loads(res.render("json"))
    assert len(out) > 0 and len(res.encode()) > 0, what
    if claim is not None:
        got = {(tb if time_mode else 0, r["key_vals"][0]): r["hists"][0]["outlier_values"].tolist()
               for (tb, _), r in grows.items() if "outlier_values" in r["hists"][0]}
        assert got == claim, what
        if not time_mode:       # the visible effect: every outlier on a bucket line of its own in `-json`
            for jr in out:
                for x in claim.get((0, int(jr["g"])), ()):
                    assert jr["v"]["buckets"].get(str(x)) == 1, (what, jr["g"], x)
    return True, digest


def _run(world, name, path, cap, capfd, monkeypatch, runs=1, query=None, n_aggs=1, time_mode=False):
    """Prepares `query` over table `name` on `path` with SYBL_OUTLIER_LOG_CAP=cap (None: the default), asserts the path from the
    prepare's own trace and stats, runs it `runs` times and examines every run: [(complete, digest)]."""
    spec = PATHS[path]
    tb = world.table(name, spec["compact"])
    ores = world.reference(name)
    claim = OC.claimed_outliers(world.case(name), time_mode) if name not in PATHS else None
    what = "%s %s cap=%s" % (name, path, cap)
    out = []
    with monkeypatch.context() as m:
        for k in SWITCHES:
            m.delenv(k, raising=False)
        for k, v in spec["env"].items():
            m.setenv(k, v)
        m.setenv("SYBL_PLAN_TRACE", "1")
        if cap is not None:
            m.setenv("SYBL_OUTLIER_LOG_CAP", str(cap))
        capfd.readouterr()
        qy = tb.query(**(query or OC.QUERY))
        try:
            trace = capfd.readouterr().err
            st = qy.stats()
            assert (st["strategy"], st["packed_kernel"]) == (spec["strategy"], spec["packed"]), (what, st, trace)
            for pat in spec["trace"]:
                assert re.search(pat, trace), (what, pat, trace)
            for pat in spec["absent"]:
                assert not re.search(pat, trace), (what, pat, trace)
            for i in range(runs):
                res = qy.run()
                try:
                    assert qy.stats()["strategy"] == spec["strategy"], what
                    out.append(_examine(res, ores, n_aggs, time_mode, claim, "%s run %d" % (what, i)))
                finally:
                    res.free()
        finally:
            qy.free()
    return out


# ---------------------------------------------------------------------------------------------- A. one wave
@pytest.mark.parametrize("cap", [64, 1, 256, 193])
@pytest.mark.parametrize("path", WAVE_PATHS)
def test_one_wave_thresholds(world, capfd, monkeypatch, path, cap):
    per = OC.per_of(cap)
    assert OC.rounded_cap(cap) == 64 * per and per in (1, 4)
    for n in OC.wave_ns(per):
        placed, dropped = OC.one_wave_outcome(n, per)
        assert (dropped == 0) == (n <= OC.SPILL * per)
        (complete, _), = _run(world, "wave%d" % n, path, cap, capfd, monkeypatch)
        assert complete == (dropped == 0), "%d outliers of one wave, stripes of %d on %s: model says placed=%d dropped=%d" % (n, per, path, placed, dropped)


# ---------------------------------------------------------------------------------------------- B. many waves
@pytest.mark.parametrize("kind", ["roomy", "short", "1N", "2N", "8N"])
@pytest.mark.parametrize("path", WAVE_PATHS + ("part_few", "part1", "part3"))
def test_many_waves_bounds(world, capfd, monkeypatch, path, kind):
    name = path if path in ("part1", "part3") else "many"
    n_aggs = 3 if path == "part3" else 1
    N = _n_logged(world.reference(name), n_aggs)
    assert N > 64
    if name == "many":
        assert N == world.case(name).n_outliers
    if path == "part3":     # both passes have something to append
        by_agg = [sum(r["hists"][a]["n_outliers"] for r in world.reference(name)["results"]) for a in range(3)]
        assert by_agg[0] > 0 and by_agg[2] > 0, by_agg
    cap = {"roomy": 64 * N, "short": (N - 1) // 64 * 64, "1N": N, "2N": 2 * N, "8N": 8 * N}[kind]
    query = _part_query(name) if name != "many" else None
    (complete, _), = _run(world, name, path, cap, capfd, monkeypatch, query=query, n_aggs=n_aggs)
    capfd.readouterr()
    print("outlier log: path=%s N=%d cap=%d (rounded %d, %d per stripe) -> %s" % (path, N, cap, OC.rounded_cap(cap), OC.per_of(cap),
                                                                               "complete" if complete else "overflowed"))
    if kind == "roomy":
        assert OC.per_of(cap) >= N and complete      # no stripe can fill, whatever the number of workgroups
    if kind == "short":
        assert 0 < OC.rounded_cap(cap) < N and not complete     # pigeonhole


# ---------------------------------------------------------------------------------------------- C. rescans
@pytest.mark.parametrize("cap", [64, 256])
@pytest.mark.parametrize("path", ["fast", "packed"])
def test_rescans(world, capfd, monkeypatch, path, cap):
    per = OC.per_of(cap)
    fit, over = "wave%d" % (OC.SPILL * per), "wave%d" % (OC.SPILL * per + 1)
    first, second = _run(world, fit, path, cap, capfd, monkeypatch, runs=2)
    assert first[0] and second[0], "exact fit, run twice: %s" % ((first[0], second[0]),)
    assert first[1] == second[1]
    first, second = _run(world, over, path, cap, capfd, monkeypatch, runs=2)
    assert not first[0] and not second[0]
    assert first[1] == second[1]
    for name in (fit, over):
        (complete, _), = _run(world, name, path, None, capfd, monkeypatch)
        assert complete


# ---------------------------------------------------------------------------------------------- D. time series
@pytest.mark.parametrize("n,cap", [(32, None), (32, 256), (8, 64), (9, 64)])
@pytest.mark.parametrize("path", ["fast", "packed"])
def test_time_series(world, capfd, monkeypatch, path, n, cap):
    query = dict(OC.QUERY, time_col="t", time_bucket=OC.TB)
    (complete, digest), = _run(world, "time%d" % n, path, cap, capfd, monkeypatch, query=query, time_mode=True)
    per = OC.per_of(cap if cap is not None else OC.DEFAULT_CAP)
    assert complete == (n <= OC.SPILL * per)
    if complete:
        claim = OC.claimed_outliers(world.case("time%d" % n), time=True)
        assert {tb for tb, _ in claim} == {OC.T0, OC.T0 + OC.TB}
        logged = {k[0]: d[4] for k, d in digest.items() if d[2]}
        assert {tb for tb, _ in logged} == {OC.T0, OC.T0 + OC.TB} and sum(len(v) for v in logged.values()) == n
