"""CPU: the oracle against the plain Python big-integer reference of tests/hist_summary_cases.py on every input that
tests/test_gpu_hist_summary.py puts through the device histogram summaries: bucket-array geometries from 2 to 1002
buckets (G), several aggregations of different geometry (M), the int64-edge bucket sizes (E) and weights up to a
sum(b^2 * w) beyond 2^64 (W).  Buckets, percentiles, counts, sums, extrema and outliers are compared exactly, stddev by the
1e-9 scale-aware rule of parity.compare_hist.  The oracle has to be right on these inputs before a GPU sees them."""
import numpy as np
import pytest

from tests import hist_summary_cases as H
from tests import parity

SUMMARY_CASES = H.summary_cases()
MOMENTS_CASES = H.moments_cases()
_REF = {}  # case name -> reference result (computed once, never modified)


def run_oracle(orc, case):
    names = list(case["cols"])
    info = {n: case["info"].get(n, (0, 0)) for n in names}
    pop = case.get("pop", {})
    ocols = [dict({"type": "int", "data": case["cols"][n]}, **({"populated": pop[n]} if n in pop else {})) for n in names]
    return orc.run_query(ocols, block_rows=case["block_rows"], n_threads=2, **parity.oracle_query_kwargs(names, info, case["q"]))


def reference(case):
    if case["name"] not in _REF:
        _REF[case["name"]] = H.reference(case)
    return _REF[case["name"]]


def check_hist(o, r, ctx, cumulative=False):
    assert bool(o["present"]) == r["present"], ctx
    if not r["present"]:
        return
    assert (o["count"], o["samples"], o["sum_exact"]) == (r["count"], r["samples"], r["sum64"]), (ctx, o, r)
    assert (o["bucket_size"], o["num_buckets"], o["n_values"]) == (r["bucket_size"], r["num_buckets"], r["n_values"]), ctx
    assert (o["min"], o["max"]) == (r["min"], r["max"]), ctx
    assert np.array_equal(o["values"], r["values"]), ctx
    assert o["percentiles"].tolist() == r["percentiles"], ctx
    assert (o["n_outliers"], o["n_underliers"]) == (r["n_outliers"], r["n_underliers"]), ctx
    if not cumulative:  # (Combine merges no outlier lists: Cumulative's are one block's, hist_basic.go:259-279)
        assert sorted(o["outlier_values"].tolist()) == r["outliers"], ctx
    if not r["count"]:
        return
    assert (o["true_min"], o["true_max"]) == (r["true_min"], r["true_max"]), ctx
    mean = float(r["mean"])
    assert abs(o["avg"] - mean) <= parity.REL * abs(mean), (ctx, o["avg"], mean)
    scale = max(abs(mean), o["bucket_size"], 1.0)
    assert parity._close(o["stddev_exact"], r["stddev"], 1e-9, scale), (ctx, o["stddev_exact"], r["stddev"])


def check_case(orc, case):
    ores, ref = run_oracle(orc, case), reference(case)
    assert ores["matched"] == ref["matched"]
    orows = {r["key_vals"]: r for r in ores["results"]}
    assert set(orows) == set(ref["groups"]), case["name"]
    for k, r in ref["groups"].items():
        assert (orows[k]["count"], orows[k]["samples"]) == (r["rows"], r["row_samples"]), (case["name"], k)
        for a, rh in enumerate(r["hists"]):
            check_hist(orows[k]["hists"][a], rh, (case["name"], k, a))
    for a, rh in enumerate(ref["total"]["hists"]):
        check_hist(ores["cumulative"]["hists"][a], rh, (case["name"], "cumulative", a), cumulative=True)
    return ores, ref


@pytest.mark.parametrize("case", SUMMARY_CASES + MOMENTS_CASES, ids=lambda c: c["name"])
def test_oracle_against_the_big_integer_reference(oracle, case):
    check_case(oracle, case)


@pytest.mark.parametrize("nv", H.G_N_VALUES)
def test_g_ranges_give_the_bucket_counts_they_are_named_for(oracle, nv):
    lo, hi = H.G_INFO[nv]
    bs, nb, n_values = H.setup_buckets(lo, hi)
    assert oracle.setup_buckets(lo, hi) == {"bucket_size": bs, "num_buckets": nb, "n_values": nv} and n_values == nv
    ores = run_oracle(oracle, H.case_g(nv))
    assert all(r["hists"][0]["n_values"] == nv for r in ores["results"] if r["hists"][0]["present"])
    assert ores["cumulative"]["hists"][0]["n_values"] == nv


def test_m_queries_mix_the_geometries(oracle):
    for n, aggs in H.M_AGGS.items():
        ores = run_oracle(oracle, H.case_m(n))
        assert [h["n_values"] for h in ores["cumulative"]["hists"]] == [int(a[1:]) for a in aggs]
    assert sorted(int(a[1:]) for a in H.M_AGGS[4]) == [2, 65, 129, 1002]


def test_w_geometry_and_the_three_sides_of_the_moment_bound(oracle):
    assert oracle.setup_buckets(*H.W_INFO) == {"bucket_size": 1, "num_buckets": 1001, "n_values": 1002}
    ref = reference(H.case_w_big(True))["groups"]
    sb2 = [ref[(k,)]["hists"][0]["sb2_true"] for k in H.W_KEYS]
    assert sb2[0] < 1 << 63 < sb2[1] < 1 << 64 < sb2[2] and sb2[3] < 1 << 63
    assert ref[(H.W_KEYS[3],)]["hists"][0]["count"] == ref[(H.W_KEYS[2],)]["hists"][0]["count"]
    split = [ref[(k,)]["hists"][0] for k in H.W_SPLIT_KEYS]
    assert 1 << 63 < split[0]["sb2_true"] < 1 << 64 < split[1]["sb2_true"] and [h["stddev"] for h in split] == [50.0, 50.0]
    for k in H.W_KEYS + H.W_SPLIT_KEYS:
        h = ref[(k,)]["hists"][0]
        assert h["count"] * (H.W_INFO[1] - H.W_INFO[0]) < 1 << 64
        # the bound up to which stddev is exact (include/sybilgpu.h at `stddev`): the groups beyond 2^63 are inside it
        assert 1001 * h["sb_true"] - h["sb_true"] ** 2 // h["count"] < 1 << 64


def test_summary_cases_have_a_partial_last_workgroup_and_block():
    """2048 or more cells, no multiple of 4 (k_hist_summary: four pairs per workgroup), no multiple of 128 (k_hist_total's
    blocks), and one far key whose last block of cells takes both the unrolled-by-8 loop and its remainder."""
    for case in SUMMARY_CASES:
        g = case["cols"]["g"]
        cells = int(g.max()) - int(g.min()) + 1
        assert int(g.min()) == 0 and cells == case["far"] + 1 >= 2048 and cells % 4 and cells % 128, case["name"]
    assert any(8 < (c["far"] + 1) % 128 and (c["far"] + 1) % 128 % 8 for c in SUMMARY_CASES)
    for case in SUMMARY_CASES[:len(H.G_N_VALUES) + len(H.G_HIST_BUCKETS) + len(H.M_AGGS)]:
        assert sorted(set(case["cols"]["g"].tolist())) == sorted(H.keys(case["far"]))
