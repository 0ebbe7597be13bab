"""GPU: aggregates at the int64 edges against the oracle (which tests/test_oracle_int64_edges.py holds against a Python
big-integer reference on the same inputs, tests/int64_edges.py): group sums that leave int64, keys / values / filter
constants at INT64_MIN and INT64_MAX, the reject gate, count distinct of the extremes, and the exact-division branch of
the bucket and time-bucket divides (spans from 2^51 - 1 to 2^61).  Every case runs on canonical int64 storage, after
compact(), through the hash group-by with and without LDS staging, and through the plan interpreter."""
import numpy as np
import pytest

import sybil_amd
from tests import int64_edges as E
from tests import parity
from tests.test_oracle_int64_edges import run_oracle

pytestmark = pytest.mark.gpu

VARIANTS = {"int64": {}, "compact": {}, "hash": {"SYBL_FORCE_HASH": "1"},
            "hash_nolds": {"SYBL_FORCE_HASH": "1", "SYBL_NO_HASH_LDS": "1"}, "nofast": {"SYBL_NO_FAST": "1"}}
STRATEGIES = {}  # variant -> strategies seen, over the whole file
_ORACLE = {}     # case name -> oracle result (computed once, shared by the variants, never modified)


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(params=list(VARIANTS))
def variant(request, monkeypatch):
    for k, v in VARIANTS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def _table(ctx, case, variant):
    cols = case["cols"]
    n = len(next(iter(cols.values())))
    tb = ctx.create_table("e")
    for c in cols:
        lo, hi = case["info"].get(c, (1, 0))
        tb.add_column(c, "int", lo, hi)
    for r0 in range(0, n, case["block_rows"]):
        r1 = min(r0 + case["block_rows"], n)
        tb.append_block(r1 - r0, {c: cols[c][r0:r1] for c in cols})
    if variant == "compact":
        tb.compact()
    return tb


def _oracle(orc, case, **kw):
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = run_oracle(orc, case, **kw)
    return _ORACLE[case["name"]]


def _run(ctx, orc, case, variant, compare=True, tb=None, **qextra):
    """One case on one storage / path: (result, oracle result); the caller frees the result."""
    own = tb is None
    tb = tb or _table(ctx, case, variant)
    try:
        q = dict(case["q"], want_percentiles=case["q"].get("op") == "hist", **qextra)
        query = tb.query(**q)
        try:
            gres = query.run()
            STRATEGIES.setdefault(variant, set()).add(query.stats()["strategy"])
        finally:
            query.free()
        ores = _oracle(orc, case)
        if compare:
            op = case["q"].get("op", "avg")
            parity.compare(gres, ores, op=op, full=op == "hist", n_aggs=len(case["q"].get("aggs", [])),
                           time_mode=bool(case["q"].get("time_col")), loghist=bool(case["q"].get("loghist")))
        return gres, ores
    finally:
        if own:
            tb.free()


def _check_exact_means(gres, case, ores):
    """avg against the exact mean of the Python reference: true sum / count through one long double division and one
    rounding to double, 2^-52 relative at the most (parity.compare holds it against the reference-order mean at 1e-6)."""
    h = ores["cumulative"]["hists"][0]
    ref = E.reference(case, (h["bucket_size"], h["n_values"]) if case["q"]["op"] == "hist" else None)
    for r in gres.rows(0):
        g = ref["groups"][(0, r["key_vals"])]
        assert abs(r["hists"][0]["avg"] - float(g["mean"])) <= 2.0 ** -51 * abs(float(g["mean"])), (case["name"], r["key_vals"])
    t = ref["total"]
    assert abs(gres.cumulative["hists"][0]["avg"] - float(t["mean"])) <= 2.0 ** -51 * abs(float(t["mean"])), case["name"]
    return ref


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("op", ["avg", "hist"])
@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4"])
def test_sums_that_leave_int64(ctx, oracle, variant, name, op):
    case = E.case_a(name, op)
    gres, ores = _run(ctx, oracle, case, variant)
    _check_exact_means(gres, case, ores)
    gres.free()


@pytest.mark.parametrize("asc", [False, True])
def test_a1_order_by_mean_follows_the_exact_mean(ctx, oracle, variant, asc):
    case = E.case_a("A1", "avg")
    gres, ores = _run(ctx, oracle, case, variant, order_by="v", order_asc=asc)
    ref = E.reference(case)
    want = sorted(ref["groups"], key=lambda k: ref["groups"][k]["mean"], reverse=not asc)
    assert [r["key_vals"] for r in gres.rows(0)] == [k[1] for k in want]
    gres.free()


@pytest.mark.parametrize("op", ["avg", "hist"])
def test_a5_sum_beyond_the_recoverable_bound(ctx, oracle, variant, op):
    """Four rows of 9e18 and one of -4e18 under Info (-2^62, 9e17): 5 * (hi - lo) >= 2^64, so the true sum (3.2e19) cannot be
    recovered from 64 bits plus the count -- the documented limit (include/sybilgpu.h at `sum`).  Asserted: count,
    sum mod 2^64, min and max ONLY; avg and stddev are not (the engine reports -3.2e18 where the oracle's mean is 6.4e18)."""
    case = E.case_a("A5", op)
    gres, ores = _run(ctx, oracle, case, variant, compare=False)
    assert gres.matched == 5
    for g, o in ((gres.rows(0)[0]["hists"][0], ores["results"][0]["hists"][0]), (gres.cumulative["hists"][0], ores["cumulative"]["hists"][0])):
        assert (g["count"], g["sum"], g["min"], g["max"]) == (o["count"], o["sum_exact"], o["min"], o["max"])
        assert (g["count"], g["sum"]) == (5, E.wrap64(32 * 10 ** 18))
    gres.free()


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("two_groups", [False, True])
def test_b1_extreme_keys_and_values(ctx, oracle, variant, two_groups):
    case = E.case_b1(two_groups)
    gres, ores = _run(ctx, oracle, case, variant)
    rows = {r["key_vals"][-1]: r["hists"][0] for r in gres.rows(0)}
    kmin = E.MIN & (E.M64 - 1)
    assert (rows[kmin]["count"], rows[kmin]["sum"], rows[kmin]["min"]) == (2, E.MIN, E.MIN)
    assert rows[E.MAX]["sum"] == E.MIN + 5 and rows[E.MAX]["min"] == E.MIN
    assert rows[7]["sum"] == 0 and rows[7]["avg"] == -2.0 ** 63 and rows[7]["min"] == E.MIN
    _check_exact_means(gres, case, ores)
    gres.free()


@pytest.mark.parametrize("which", ["edges", "wrap"])
def test_b2_reject_gate(ctx, oracle, variant, which):
    case = E.case_b2(which)
    gres, ores = _run(ctx, oracle, case, variant)
    counts = {r["key_vals"][0]: (r["hists"][0]["present"], r["hists"][0]["count"]) for r in gres.rows(0)}
    if which == "wrap":
        assert counts == {g: (1, 0) for g in range(4)}
    else:
        assert counts == {g: (1, c) for g, c in {0: 1, 1: 0, 2: 1, 3: 0, 4: 1, 5: 1, 6: 1, 7: 0, 8: 0}.items()}
    gres.free()


@pytest.mark.parametrize("col", ["wide", "near"])
def test_b3_filters_at_the_extremes(ctx, oracle, variant, col):
    tb = _table(ctx, E.case_b3(col, "gt", 0), variant)
    try:
        for op in ("gt", "lt", "eq", "neq"):
            for const in E.B3_CONSTANTS:
                case = E.case_b3(col, op, const)
                gres, ores = _run(ctx, oracle, case, variant, tb=tb)
                assert gres.matched == E.reference(case)["matched"], case["name"]
                gres.free()
    finally:
        tb.free()


def test_b4_count_distinct_of_extreme_values(ctx, oracle, variant):
    cols = E.cols_b4()
    case = {"name": "B4", "cols": cols, "info": {}, "block_rows": 4, "q": dict(groups=["g"], distincts=["d"])}
    tb = _table(ctx, case, variant)
    try:
        query = tb.query(groups=["g"], distincts=["d"])
        gres = query.run()
        STRATEGIES.setdefault(variant, set()).add(query.stats()["strategy"])
        query.free()
    finally:
        tb.free()
    ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in cols], groups=[0], distincts=[1], n_threads=2, want_registers=True)
    omap = {r["key"]: r for r in ores["results"]}
    grows = gres.rows(0)
    assert gres.matched == ores["matched"] and len(grows) == len(omap) == 3
    for i, g in enumerate(grows):
        card, regs = gres.distinct(0, i, registers=True)
        assert np.array_equal(regs, omap[g["key"]]["registers"]), g["key_vals"]
        assert card == omap[g["key"]]["distinct"] == g["distinct"] and g["count"] == omap[g["key"]]["count"]
    card, regs = gres.distinct(2, 0, registers=True)
    assert np.array_equal(regs, ores["cumulative"]["registers"]) and card == ores["cumulative"]["distinct"]
    gres.free()


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("negative_min", [False, True])
@pytest.mark.parametrize("span", E.C_SPANS)
def test_c_bucket_divide_either_side_of_2_51(ctx, oracle, variant, span, negative_min):
    """Buckets and percentiles bit for bit (parity.compare, full) where udiv_fast switches from the double reciprocal to
    the exact n / d: values one below, on and one above 200 random bucket edges, plus both ends of the range."""
    for bs in E.c_bucket_sizes(span):
        case = E.case_c(span, bs, E.c_min(span, negative_min))
        gres, ores = _run(ctx, oracle, case, variant)
        _check_exact_means(gres, case, ores)
        gres.free()


def test_c_loghist_beyond_2_53(ctx, oracle, variant):
    """-loghist on the 2^53 + 12345 span (MultiSub::big_div).  Parity unpinned, like every -loghist figure: the oracle restates
    hist_multi.go, no reference binary has confirmed it."""
    span = (1 << 53) + 12345
    gres, ores = _run(ctx, oracle, E.case_c(span, E.c_bucket_sizes(span)[0], 0, loghist=True), variant)
    gres.free()


@pytest.mark.parametrize("which", ["big", "usec", "negative"])
def test_c_time_buckets(ctx, oracle, variant, which):
    gres, ores = _run(ctx, oracle, E.case_c_time(which), variant)
    gres.free()


def test_the_file_ran_on_several_kernels():
    """Last in the file: the cases above must not collapse onto one kernel.  (Needs the rest of the file to have run.)"""
    seen = set().union(*STRATEGIES.values()) if STRATEGIES else set()
    print("strategies by variant:", {k: sorted(v) for k, v in STRATEGIES.items()})
    assert len(seen) >= 4, STRATEGIES
