"""The restatement of rollup percentiles (tests/rollup_pct_ref.py) against answers written out by hand -- no GPU.  What the
GPU tests compare the library with is first held to the definition here: nearest rank (k * n + 99) / 100, n = 1, n = 0
unpopulated, the int64 edges in one group, the column order, the tokens that are refused, the plan of the sort."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import rollup_pct_ref as P

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _one_group(values, ops, pop=None):
    v = np.array(values, dtype=np.int64)
    tl = [(len(v), {"v": ("int", v, None if pop is None else np.array(pop, dtype=bool))})]
    ref = P.rollup_pct_ref(tl, aggs=[("v", ops)])
    assert ref["stats"]["groups"] == 1
    cols = D.concat(ref["blocks"])
    return {n: (int(cols[n][1][0]) if cols[n][2][0] else None) for n, _ in ref["columns"]}, ref


@pytest.mark.parametrize("values,want", [
    ([10, 20, 30, 40], {1: 10, 50: 20, 51: 30, 99: 40}),
    ([40, 10, 30, 20], {1: 10, 50: 20, 51: 30, 99: 40}),                # the input's order does not matter
    ([5, 5, 9], {66: 5, 67: 9}),
    (list(range(1, 101)), {k: k for k in (1, 2, 50, 51, 98, 99)}),
    (list(range(1, 102)), {50: 51, 99: 100}),
    (list(range(1, 201)), {1: 2, 50: 100, 99: 198}),
    ([7], {1: 7, 50: 7, 99: 7}),                                        # n = 1
    ([I64_MAX, I64_MIN], {1: I64_MIN, 50: I64_MIN, 51: I64_MAX, 99: I64_MAX}),
    ([I64_MAX, I64_MIN, 0], {33: I64_MIN, 34: 0, 67: I64_MAX}),
])
def test_nearest_rank_by_hand(values, want):
    got, _ = _one_group(values, ",".join("p%d" % k for k in want))
    assert {k: got["v_p%d" % k] for k in want} == want
    for k, x in want.items():
        assert P.nearest_rank(values, k) == x


def test_every_k_of_1_to_100_is_itself():
    for k in range(1, 100):
        assert P.nearest_rank(list(range(100, 0, -1)), k) == k


def test_n_zero_is_unpopulated_and_stored_zero():
    v = np.array([3, 4, 5, 6], dtype=np.int64)
    tl = [(4, {"g": ("int", np.array([0, 0, 1, 1], dtype=np.int64), None), "v": ("int", v, np.array([True, True, False, False]))})]
    for compact in (True, False):
        ref = P.rollup_pct_ref(tl, groups=["g"], aggs=[("v", "min,p50,p99")], compact=compact)
        cols = D.concat(ref["blocks"])
        assert cols["v_p50"][1].tolist() == [3, 0] and cols["v_p50"][2].tolist() == [True, False]
        assert cols["v_p99"][1].tolist() == [4, 0] and cols["v_min"][2].tolist() == [True, False]
        assert ref["bitmap"]["v_p50"] and ref["bitmap"]["v_min"] and not ref["bitmap"]["count"]
        assert ref["storage"]["v_p50"] == ((1, 3) if compact else (8, 0))
        assert ref["pct_stats"] == dict(columns=1, percentiles=2, variant32=1, variant64=0, variant_pairs=0, key_bits_max=1 + 1, items=2)   # 2 cells; 3 .. 4
    # a column without any populated value: nothing is sorted
    tl = [(2, {"v": ("int", np.zeros(2, dtype=np.int64), np.zeros(2, dtype=bool))})]
    ref = P.rollup_pct_ref(tl, aggs=[("v", "p50")], compact=True)
    assert ref["pct_stats"] == dict(columns=1, percentiles=1, variant32=0, variant64=0, variant_pairs=0, key_bits_max=0, items=0)
    assert ref["bitmap"]["v_p50"] and ref["storage"]["v_p50"] == (1, 0) and D.concat(ref["blocks"])["v_p50"][2].tolist() == [False]


def test_column_order_and_percentile_only_columns():
    i = np.arange(6, dtype=np.int64)
    tl = [(6, {"g": ("int", i % 2, None), "a": ("int", i, None), "b": ("int", i * 10, None), "time": ("int", i * 1000, None)})]
    ref = P.rollup_pct_ref(tl, groups=["g"], aggs=[("a", "p99,max,p5,n"), ("b", "p50")], time_col="time", time_bucket=3600, count_name="rows")
    assert [n for n, _ in ref["columns"]] == ["time", "g", "rows", "a_n", "a_max", "a_p5", "a_p99", "b_p50"]
    assert "b_n" not in ref["storage"] and "b_n" not in ref["bitmap"] and ref["stats"]["fields"] == 9
    cols = D.concat(ref["blocks"])
    assert set(cols) == {n for n, _ in ref["columns"]}
    # hour 0 holds rows 0 .. 3, hour 1 rows 4, 5; g = row % 2
    assert cols["a_p5"][1].tolist() == [0, 1, 4, 5] and cols["a_p99"][1].tolist() == [2, 3, 4, 5] and cols["b_p50"][1].tolist() == [0, 10, 40, 50]
    # the MISSING group has percentiles of its own; filters apply; rows without a time value contribute nothing
    tl = [(6, {"g": ("int", i % 2, i < 4), "a": ("int", i, None), "time": ("int", i, i != 5)})]
    ref = P.rollup_pct_ref(tl, groups=["g"], aggs=[("a", "p50")], filters=[("a", "gt", 0)], time_col="time", time_bucket=100)
    cols = D.concat(ref["blocks"])
    assert cols["g"][2].tolist() == [False, True, True] and cols["a_p50"][1].tolist() == [4, 2, 1] and ref["stats"]["rows_no_time"] == 1


@pytest.mark.parametrize("ops", ["p0", "p100", "p05", "p5.5", "p", "p50,p50", "sum,p50,sum", "p1,p2,p3,p4,p5,p6,p7,p8,p9", "P50", "p-1", "p 5", "",
                                 "p50,", "p500"])
def test_refused_tokens(ops):
    with pytest.raises(ValueError):
        P.split_ops(ops)


def test_accepted_tokens_and_name_collisions():
    assert P.split_ops("p99,sum,p1") == (["sum"], [1, 99]) and P.split_ops("p50") == ([], [50])
    assert P.split_ops("p1,p2,p3,p4,p5,p6,p7,p8") == ([], [1, 2, 3, 4, 5, 6, 7, 8]) and P.split_ops("n,p10,max") == (["n", "max"], [10])
    tl = [(2, {"v": ("int", np.arange(2, dtype=np.int64), None)})]
    with pytest.raises(AssertionError):
        P.rollup_pct_ref(tl, aggs=[("v", "p50")], count_name="v_p50")


def test_the_plan_of_the_sort():
    assert P.plan(1, 5, 5) == (0, 0, P.V32) and P.plan(2, 0, 1) == (1, 1, P.V32) and P.plan(1 << 27, 0, 31) == (27, 5, P.V32)
    assert P.plan(1 << 27, 0, 32) == (27, 6, P.V64) and P.plan(1, I64_MIN, I64_MAX) == (0, 64, P.V64) and P.plan(2, I64_MIN, I64_MAX) == (1, 64, P.PAIRS)
    assert P.plan(3, 0, (1 << 30) - 1) == (2, 30, P.V32) and P.plan(3, 0, 1 << 30) == (2, 31, P.V64)
    assert P.plan(2, 0, 1, "64")[2] == P.V64 and P.plan(2, 0, 1, "pairs")[2] == P.PAIRS and P.plan(2, 0, 1, "32")[2] == P.V32
    assert P.plan(3, 0, 1 << 30, "32")[2] is None and P.plan(2, I64_MIN, I64_MAX, "64")[2] is None and P.plan(2, I64_MIN, I64_MAX, "pairs")[2] == P.PAIRS
