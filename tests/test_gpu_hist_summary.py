"""GPU: the device histogram summaries -- k_hist_summary (percentiles and bucket moments, one wave per (cell, aggregation)),
k_hist_total (Cumulative's bucket arrays), k_hist_gather / the per-row copies (the printed rows' arrays) -- at the edges of
the bucket array.  A query takes them once its group table has 2048 or more cells (query_wants_hist_summary, result.cpp);
every case of tests/hist_summary_cases.py that is run here as a summary query gets there by two anchor keys, with a
handful of live groups, so a case is a 16-35 MB table and a few hundred rows.  tests/test_oracle_hist_summary.py holds
the oracle against a Python big-integer reference on the same inputs.

Per case, on canonical int64 storage and after compact():
  a. the default path: the sb2 probe answers (the summary ran on the device), parity.compare in full against the oracle,
     sb and sb2 of every cell bit for bit against the reference mod 2^64 (0 for an empty cell);
  b. SYBL_NO_HISTSUMMARY=1, the host walk of the same query: the probe refuses, the same parity.compare, percentiles
     equal to (a), stddev within 1e-9 of (a) by the scale-aware rule of parity.compare_hist.
The W cases also run as moments queries (want_percentiles=False, few groups) on both storages and through the hash
group-by with and without LDS staging; their 2^33 weights carry sum(b^2 * w) past 2^63 and past 2^64, where stddev has to
come from the recovered true moment (true_moments, result.cpp).  The printers' tables (700 live groups) take the per-row
copies (limit 25), the gather kernel (limit 600, and limit 25 under SYBL_TOP_GATHER_KERNEL=1), with printed_only off and on,
and the snapshot without its copy stream."""
import numpy as np
import pytest

import sybil_amd
from sybil_amd import _native as N
from tests import hist_summary_cases as H
from tests import parity
from tests.test_oracle_hist_summary import MOMENTS_CASES, SUMMARY_CASES, reference, run_oracle

pytestmark = pytest.mark.gpu

STRATEGIES = {"summary": {}, "moments": {}}  # kind -> {variant: strategies seen}, over the whole file
_ORACLE = {}  # case name -> oracle result (computed once, shared, never modified)
MOMENT_VARIANTS = {"int64": {}, "compact": {}, "hash": {"SYBL_FORCE_HASH": "1"},
                   "hash_nolds": {"SYBL_FORCE_HASH": "1", "SYBL_NO_HASH_LDS": "1"}}


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


def _oracle(orc, case):
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = run_oracle(orc, case)
    return _ORACLE[case["name"]]


def _table(ctx, case, compact):
    cols, pop = case["cols"], case.get("pop", {})
    n = len(next(iter(cols.values())))
    tb = ctx.create_table("hs")
    for c in cols:
        lo, hi = case["info"].get(c, (1, 0))
        tb.add_column(c, "int", lo, hi)
    for r0 in range(0, n, case["block_rows"]):
        r1 = min(r0 + case["block_rows"], n)
        tb.append_block(r1 - r0, {c: (cols[c][r0:r1], pop[c][r0:r1]) if c in pop else cols[c][r0:r1] for c in cols})
    if compact:
        tb.compact()
    return tb


def _stddev_close(a, b, h):
    return parity._close(a, b, 1e-9, max(abs(h["avg"]), abs(h["bucket_size"]), 1.0))


def _check_moments(query, case, cell_of_key, n_cells):
    """sb and sb2 of every cell against the big-integer reference mod 2^64; 0 in every cell without a group."""
    ref = reference(case)["groups"]
    for a in range(len(case["q"]["aggs"])):
        for which in ("sb", "sb2"):
            got = query.debug_cells(which, a)
            want = np.zeros(n_cells, dtype=np.int64)
            for k, g in ref.items():
                want[cell_of_key[k[0]]] = g["hists"][a][which]
            assert got.size == n_cells, (case["name"], got.size)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (case["name"], which, a, bad[:5], got[bad[:5]], want[bad[:5]])


def _run_summary_case(ctx, orc, case, compact, monkeypatch, kind="summary"):
    ores = _oracle(orc, case)
    n_aggs = len(case["q"]["aggs"])
    n_cells = case["far"] + 1
    q = dict(case["q"], want_percentiles=True)
    tb = _table(ctx, case, compact)
    try:
        # a. the default path
        query = tb.query(**q)
        try:
            gres = query.run()
            assert query.debug_cells("sb2").size == n_cells  # (raises on the host walk: the summary ran on the device)
            STRATEGIES.setdefault(kind, {}).setdefault("compact" if compact else "int64", set()).add(query.stats()["strategy"])
            parity.compare(gres, ores, op="hist", full=True, n_aggs=n_aggs)
            _check_moments(query, case, {k: k for k in range(n_cells)}, n_cells)
        finally:
            query.free()
        # b. the host walk of the same query
        monkeypatch.setenv("SYBL_NO_HISTSUMMARY", "1")
        query = tb.query(**q)
        try:
            hres = query.run()
            with pytest.raises(N.SyblError, match="keeps no bucket moments"):
                query.debug_cells("sb2")
            parity.compare(hres, ores, op="hist", full=True, n_aggs=n_aggs)
        finally:
            query.free()
        monkeypatch.delenv("SYBL_NO_HISTSUMMARY")
        hrows = {r["key"]: r for r in hres.rows(0)}
        for g, w in [(g, hrows[g["key"]]) for g in gres.rows(0)] + [(gres.cumulative, hres.cumulative)]:
            for a in range(n_aggs):
                gh, wh = g["hists"][a], w["hists"][a]
                assert ("percentiles" in gh) == ("percentiles" in wh), (case["name"], g["key_vals"], a)
                if "percentiles" in gh:
                    assert np.array_equal(gh["percentiles"], wh["percentiles"]), (case["name"], g["key_vals"], a)
                if gh["present"]:
                    assert _stddev_close(gh["stddev"], wh["stddev"], gh), (case["name"], g["key_vals"], a, gh["stddev"], wh["stddev"])
        gres.free()
        hres.free()
    finally:
        tb.free()


# ---------------------------------------------------------------- G, M, E, W through the device summary
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "compact"])
@pytest.mark.parametrize("case", SUMMARY_CASES, ids=lambda c: c["name"])
def test_summary_path_against_oracle_reference_and_host_walk(ctx, oracle, monkeypatch, case, compact):
    _run_summary_case(ctx, oracle, case, compact, monkeypatch)


@pytest.mark.parametrize("name", ["G-1002", "M-4"])
def test_summary_snapshot_without_the_copy_stream(ctx, oracle, monkeypatch, name):
    """SYBL_NO_COPY_STREAM=1: the 16-20 MB snapshot of these cases leaves on the main stream instead of the copy stream."""
    monkeypatch.setenv("SYBL_NO_COPY_STREAM", "1")
    case = [c for c in SUMMARY_CASES if c["name"] == name][0]
    _run_summary_case(ctx, oracle, case, False, monkeypatch, kind="nocopystream")


def test_w_big_stddev_beyond_2_63_and_2_64(ctx, oracle):
    """The three groups of 2^33-weighted rows at value 1000 (true sum(b^2 * w) just below 2^63, between 2^63 and 2^64, above
    2^64) have stddev 0 around the mean 1000 -- which a variance gone negative is reported as, too; the two that alternate
    between 1000 and 900 (past 2^63, past 2^64) have 50, the one spread over buckets 0..1000 one near 289.  All are inside
    the documented bound ((n_values - 1) * sb - sb^2 / Count < 2^64, include/sybilgpu.h at `stddev`), so stddev is asserted in
    full against the big-integer reference, on the summary path and as a moments query."""
    for case in (H.case_w_big(True), H.case_w_big(False)):
        ref = reference(case)["groups"]
        tb = _table(ctx, case, False)
        try:
            query = tb.query(**case["q"])
            gres = query.run()
            query.free()
            rows = {r["key_vals"]: r["hists"][0] for r in gres.rows(0)}
            assert set(rows) == set(ref)
            for k, r in ref.items():
                print(case["name"], k, "sb2/2^63 = %.4f" % (r["hists"][0]["sb2_true"] / 2.0 ** 63), "stddev", rows[k]["stddev"], "reference", r["hists"][0]["stddev"])
            for k, r in ref.items():
                assert parity._close(rows[k]["stddev"], r["hists"][0]["stddev"], 1e-9, 1000.0), (case["name"], k, rows[k]["stddev"], r["hists"][0]["stddev"])
            gres.free()
        finally:
            tb.free()


# ---------------------------------------------------------------- W as moments queries
@pytest.mark.parametrize("variant", list(MOMENT_VARIANTS))
@pytest.mark.parametrize("case", MOMENTS_CASES, ids=lambda c: c["name"])
def test_w_moments_queries(ctx, oracle, monkeypatch, case, variant):
    for k, v in MOMENT_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    ores = _oracle(oracle, case)
    tb = _table(ctx, case, variant == "compact")
    try:
        query = tb.query(**case["q"])
        try:
            gres = query.run()
            STRATEGIES["moments"].setdefault(variant, set()).add(query.stats()["strategy"])
            parity.compare(gres, ores, op="hist", full=False, n_aggs=1)
            keys = sorted(k[0] for k in reference(case)["groups"])  # dense keys 0..n-1: the direct-mapped cell, and the hash path's key order
            assert keys == list(range(len(keys)))
            _check_moments(query, case, {k: k for k in keys}, len(keys))
            gres.free()
        finally:
            query.free()
    finally:
        tb.free()


# ---------------------------------------------------------------- the printed rows
PRINTERS = {"dma25": (25, {}), "gather600": (600, {}), "gather25": (25, {"SYBL_TOP_GATHER_KERNEL": "1"}),
            "dma25_nocopystream": (25, {"SYBL_NO_COPY_STREAM": "1"})}


@pytest.fixture(scope="module", params=[1, 4], ids=["P-1", "P-4"])
def printer(request, ctx, oracle):
    """(case, table, oracle result): the one-aggregation table on canonical storage, the four-aggregation table compacted."""
    case = H.printer_table(request.param)
    tb = _table(ctx, case, request.param == 4)
    yield case, tb, run_oracle(oracle, case)
    tb.free()


@pytest.mark.parametrize("printed_only", [False, True], ids=["all_rows", "printed_only"])
@pytest.mark.parametrize("mode", list(PRINTERS))
def test_printed_rows(printer, monkeypatch, mode, printed_only):
    case, tb, ores = printer
    limit, env = PRINTERS[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n_aggs = len(case["q"]["aggs"])
    query = tb.query(**dict(case["q"], want_percentiles=True, order_by="$COUNT", limit=limit, printed_only=printed_only))
    try:
        gres = query.run()
        if not printed_only:  # (a printer's query computes no moments)
            assert query.debug_cells("sb2").size == case["far"] + 1
    finally:
        query.free()
    omap = {r["key"]: r for r in ores["results"]}
    rows = gres.results
    assert len(rows) == len(omap) == 700 and [r["count"] for r in rows] == sorted((r["count"] for r in rows), reverse=True)
    none = np.zeros(0, dtype=np.int64)
    for i, g in enumerate(rows):
        o = omap[g["key"]]
        assert g["count"] == o["count"]
        for a in range(n_aggs):
            h, oh = g["hists"][a], o["hists"][a]
            ctx_ = (mode, printed_only, i, g["key_vals"], a)
            assert (h["count"], h["sum"], h["min"], h["max"], h["n_outliers"]) == (oh["count"], oh["sum_exact"], oh["min"], oh["max"], oh["n_outliers"]), ctx_
            if i < limit:
                assert np.array_equal(h["values"], oh["values"]), ctx_
            else:
                assert "values" not in h, ctx_
            if i < limit or not printed_only:
                assert np.array_equal(h.get("percentiles", none), oh["percentiles"]), ctx_
                assert _stddev_close(h["stddev"], oh["stddev_exact"], oh), (ctx_, h["stddev"], oh["stddev_exact"])
            else:
                assert "percentiles" not in h and h["stddev"] != h["stddev"], ctx_
    for a in range(n_aggs):
        parity.compare_hist(gres.cumulative["hists"][a], ores["cumulative"]["hists"][a], "hist", True, ctx=(mode, "cumulative", a), cumulative=True)
    gres.free()


def test_the_file_ran_the_summary_on_several_kernels():
    """Last in the file (needs the rest of it to have run): the summary-path cases and the moments queries must each have
    been scanned by two strategies at least, so that the bucket table k_hist_summary reads was laid down by more than one
    kernel."""
    print("strategies:", {kind: {k: sorted(v) for k, v in d.items()} for kind, d in STRATEGIES.items()})
    for kind in ("summary", "moments"):
        seen = set().union(*STRATEGIES[kind].values()) if STRATEGIES[kind] else set()
        assert len(seen) >= 2, (kind, STRATEGIES[kind])
