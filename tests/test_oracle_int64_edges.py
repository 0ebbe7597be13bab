"""CPU: the oracle at the int64 edges against a plain Python big-integer reference (tests/int64_edges.py) -- sums that
leave int64, keys and values at INT64_MIN / INT64_MAX, the reject gate with Go's wrapping Info.Max*10, filters at the
extremes, and bucket / time-bucket division beyond 2^51.  tests/test_gpu_int64_edges.py holds the engine against the
oracle on the same inputs, so the oracle has to be right here first: its exact mean and stddev used to come from a sum
that wraps mod 2^64."""
import numpy as np
import pytest

from tests import int64_edges as E
from tests import parity


def run_oracle(orc, case, **kw):
    names = list(case["cols"])
    info = {n: case["info"].get(n, (0, 0)) for n in names}
    ocols = [{"type": "int", "data": case["cols"][n]} for n in names]
    return orc.run_query(ocols, block_rows=case["block_rows"], n_threads=2, **dict(parity.oracle_query_kwargs(names, info, case["q"]), **kw))


def check_hist(o, r, op, ctx, sums_only=False):
    assert o["present"] == (1 if r["pop"] else 0), ctx
    if not r["pop"]:
        return
    assert (o["count"], o["samples"], o["sum_exact"]) == (r["count"], r["samples"], r["sum64"]), (ctx, o, r)
    if r["count"]:
        assert (o["true_min"], o["true_max"]) == (r["min"], r["max"]), ctx
    else:
        # (0.0, or NaN once two empty hists were combined: 0/0 in hist_basic.go:264-265)
        assert (o["avg"] == 0.0 or o["avg"] != o["avg"]) and o["sum_exact"] == 0, ctx
    if sums_only or not r["count"]:
        return
    mean = float(r["mean"])
    # the reference-order running mean (hist_basic.go:118) against the exact mean: a property of the inputs
    assert abs(o["avg"] - mean) <= parity.REL * abs(mean), (ctx, o["avg"], mean)
    if op == "hist":
        assert np.array_equal(o["values"], r["values"]), ctx
        # (the project's bar, parity.compare_hist: 1e-9 of the magnitude the doubles of GetStdDev work at)
        scale = max(abs(mean), o["bucket_size"], 1.0)
        assert parity._close(o["stddev_exact"], r["stddev"], 1e-9, scale), (ctx, o["stddev_exact"], r["stddev"])


def check_case(orc, case, sums_only=False):
    ores = run_oracle(orc, case)
    op = case["q"].get("op", "avg")
    geo = None
    if op == "hist":
        h = (ores["time_results"][0] if case["q"].get("time_col") else ores["cumulative"])["hists"][0]
        geo = (h["bucket_size"], h["n_values"])
    ref = E.reference(case, geo)
    assert ores["matched"] == ref["matched"]
    timed = bool(case["q"].get("time_col"))
    orows = {(r["time_bucket"], r["key_vals"]): r for r in ores["time_results" if timed else "results"]}
    assert set(orows) == set(ref["groups"]), (case["name"], sorted(set(orows) ^ set(ref["groups"])))
    for k, r in ref["groups"].items():
        assert (orows[k]["count"], orows[k]["samples"]) == (r["rows"], r["row_samples"]), (case["name"], k)
        check_hist(orows[k]["hists"][0], r, op, (case["name"], k), sums_only)
    if not timed:
        check_hist(ores["cumulative"]["hists"][0], ref["total"], op, (case["name"], "cumulative"), sums_only)
    return ores, ref


@pytest.mark.parametrize("op", ["avg", "hist"])
@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4"])
def test_sums_that_leave_int64(oracle, name, op):
    ores, ref = check_case(oracle, E.case_a(name, op))
    # the point of the case: some group's true sum is not its low 64 bits
    assert any(g["sum"] != g["sum64"] for g in ref["groups"].values())


@pytest.mark.parametrize("op", ["avg", "hist"])
def test_a5_sum_beyond_64_bits_plus_count(oracle, op):
    """Four rows of 9e18 and one of -4e18: the oracle's 128-bit mean is right (6.4e18); only count, sum mod 2^64, min and
    max are asserted on the engine side of this case (tests/test_gpu_int64_edges.py), so the rest is pinned here."""
    case = E.case_a("A5", op)
    ores = run_oracle(oracle, case)
    h = ores["results"][0]["hists"][0]
    assert (h["count"], h["sum_exact"], h["true_min"], h["true_max"]) == (5, E.wrap64(32 * 10 ** 18), -4 * 10 ** 18, 9 * 10 ** 18)
    assert abs(h["avg"] - 6.4e18) <= parity.REL * 6.4e18
    if op == "hist":  # 9e18 - Info.Min wraps negative (hist_basic.go:130): four underliers, clipped into bucket 0
        assert h["n_outliers"] + h["n_underliers"] == 4 and h["stddev_exact"] > 1e18


@pytest.mark.parametrize("two_groups", [False, True])
def test_b1_extreme_keys_and_values(oracle, two_groups):
    ores, ref = check_case(oracle, E.case_b1(two_groups))
    rows = {r["key_vals"][-1]: r["hists"][0] for r in ores["results"] if not two_groups or r["key_vals"][0] != 2}
    kmin, kmax = E.MIN & (E.M64 - 1), E.MAX
    assert (rows[kmin]["count"], rows[kmin]["sum_exact"], rows[kmin]["min"]) == (2, E.MIN, E.MIN)
    assert rows[kmax]["sum_exact"] == E.MIN + 5
    seven = [r["hists"][0] for r in ores["results"] if r["key_vals"][-1] == 7][0]
    assert seven["sum_exact"] == 0 and seven["avg"] == -2.0 ** 63


@pytest.mark.parametrize("which", ["edges", "wrap"])
def test_b2_reject_gate(oracle, which):
    ores, ref = check_case(oracle, E.case_b2(which))
    if which == "wrap":
        assert all(r["hists"][0]["present"] and r["hists"][0]["count"] == 0 for r in ores["results"])
    else:
        counts = {r["key_vals"][0]: r["hists"][0]["count"] for r in ores["results"]}
        assert counts == {0: 1, 1: 0, 2: 1, 3: 0, 4: 1, 5: 1, 6: 1, 7: 0, 8: 0}


@pytest.mark.parametrize("const", E.B3_CONSTANTS)
@pytest.mark.parametrize("op", ["gt", "lt", "eq", "neq"])
@pytest.mark.parametrize("col", ["wide", "near"])
def test_b3_filters_at_the_extremes(oracle, col, op, const):
    check_case(oracle, E.case_b3(col, op, const))


def test_b4_count_distinct_of_extreme_values(oracle):
    cols = E.cols_b4()
    ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in cols], groups=[0], distincts=[1], n_threads=2, want_registers=True)

    def sketch(values):  # the values' 8-byte images, each once (the estimate itself stays "parity unpinned")
        s = oracle.LogLogBeta()
        for v in sorted(set(int(x) for x in values)):
            s.add((v & (E.M64 - 1)).to_bytes(8, "little"))
        return s

    for r in ores["results"]:
        want = sketch(cols["d"][cols["g"] == r["key_vals"][0]])
        assert np.array_equal(r["registers"], want.registers) and r["distinct"] == want.cardinality(), r["key_vals"]
    total = sketch(cols["d"])
    assert int(np.count_nonzero(total.registers)) == 3  # INT64_MIN, INT64_MAX and 0 each left a register
    assert np.array_equal(ores["cumulative"]["registers"], total.registers)


@pytest.mark.parametrize("negative_min", [False, True])
@pytest.mark.parametrize("span", E.C_SPANS)
def test_c_bucket_divide_either_side_of_2_51(oracle, span, negative_min):
    for bs in E.c_bucket_sizes(span):
        case = E.case_c(span, bs, E.c_min(span, negative_min))
        ores, ref = check_case(oracle, case)
        assert ores["cumulative"]["hists"][0]["n_outliers"] + ores["cumulative"]["hists"][0]["n_underliers"] == 0


@pytest.mark.parametrize("which", ["big", "usec", "negative"])
def test_c_time_buckets(oracle, which):
    check_case(oracle, E.case_c_time(which))
