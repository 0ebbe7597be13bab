"""tests/rollup_ref.py -- the checker of tests/test_gpu_rollup.py -- held to answers written out by hand (no GPU)."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import rollup_ref as U

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _int(v, p=None):
    return ("int", np.array(v, dtype=np.int64), None if p is None else np.array(p, dtype=bool))


def _table(ref):
    """{column: [value or None per output row]}"""
    cols = D.concat(ref["blocks"])
    return {n: [x if ok else None for x, ok in zip((v.tolist() if ty == "int" else v), p.tolist())] for n, (ty, v, p) in cols.items()}


def test_time_buckets_truncate_toward_zero():
    """-1 and 1 both fall into bucket 0; -3 / 3 * 3 = -3, -4 / 3 * 3 = -3, -6 -> -6.  A row without time is dropped and counted."""
    blocks = [(4, {"time": _int([-1, 1, -3, -4]), "v": _int([1, 2, 3, 4])}),
              (4, {"time": _int([-6, 5, 0, 9], [1, 1, 1, 0]), "v": _int([5, 6, 7, 8])})]
    ref = U.rollup_ref(blocks, aggs=[("v", "sum,n")], time_bucket=3)
    assert ref["columns"] == [("time", "int"), ("count", "int"), ("v_n", "int"), ("v_sum", "int")]
    assert _table(ref) == {"time": [-6, -3, 0, 3], "count": [1, 2, 3, 1], "v_n": [1, 2, 3, 1], "v_sum": [5, 7, 10, 6]}
    assert ref["stats"]["rows_no_time"] == 1 and ref["stats"]["rows_matched"] == 8 and ref["stats"]["groups"] == 4
    assert U.trunc_div(-1, 3600) == 0 and U.trunc_div(-3600, 3600) == -1 and U.trunc_div(-3601, 3600) == -1 and U.trunc_div(7199, 3600) == 1
    # quotients -2 .. 1 (the unpopulated 9 does not count): 4 cells, one field + 4
    assert ref["product"] == 4 and ref["stats"]["path"] == U.LDS and ref["stats"]["cells_or_slots"] == 4 and ref["stats"]["fields"] == 5


def test_missing_sorts_first_and_str_keys_order_by_dictionary_id():
    blocks = [(5, {"s": ("str", ["b", None, "a", "b", None]), "k": _int([7, 7, 0, 7, 3], [1, 1, 0, 1, 1]), "v": _int([1, 2, 3, 4, 5])})]
    ref = U.rollup_ref(blocks, groups=["s", "k"], aggs={"v": "max,min"})
    # dictionary: b = 0, a = 1.  keys: (MISSING, 3), (MISSING, 7), (b, 7), (a, MISSING)
    assert ref["dicts"] == {"s": ["b", "a"]}
    assert _table(ref) == {"s": [None, None, "b", "a"], "k": [3, 7, 7, None], "count": [1, 1, 2, 1], "v_min": [5, 2, 1, 3], "v_max": [5, 2, 4, 3]}
    assert ref["bitmap"] == {"s": True, "k": True, "count": False, "v_min": False, "v_max": False}
    assert ref["columns"][-2:] == [("v_min", "int"), ("v_max", "int")]   # n, sum, min, max whatever the order asked
    # s: ids 0..1 + MISSING = 3; k: 3..7 + MISSING = 6
    assert ref["product"] == 18


def test_sums_wrap_and_the_int64_edges():
    blocks = [(4, {"k": _int([1, 1, 2, 2]), "v": _int([I64_MAX, 1, I64_MIN, I64_MAX])})]
    ref = U.rollup_ref(blocks, groups=["k"], aggs=[("v", "n,sum,min,max")], compact=True)
    assert _table(ref) == {"k": [1, 2], "count": [2, 2], "v_n": [2, 2], "v_sum": [I64_MIN, -1], "v_min": [1, I64_MIN], "v_max": [I64_MAX, I64_MAX]}
    assert ref["storage"] == {"count": (1, 2), "v_n": (1, 2), "v_sum": (8, 0), "v_min": (8, 0), "v_max": (1, I64_MAX)}


def test_a_group_whose_values_are_all_unpopulated():
    blocks = [(4, {"k": _int([5, 5, 6, 6]), "v": _int([10, 20, 30, 40], [0, 0, 1, 0])})]
    for compact in (False, True):
        ref = U.rollup_ref(blocks, groups=["k"], aggs=[("v", "n,sum,min,max")], compact=compact)
        assert _table(ref) == {"k": [5, 6], "count": [2, 2], "v_n": [0, 1], "v_sum": [None, 30], "v_min": [None, 30], "v_max": [None, 30]}
        assert ref["bitmap"] == {"k": False, "count": False, "v_n": False, "v_sum": True, "v_min": True, "v_max": True}
        assert ref["storage"]["v_sum"] == ((1, 30) if compact else (8, 0)) and ref["storage"]["v_n"] == ((1, 0) if compact else (8, 0))
        # stored 0 where unpopulated
        assert D.concat(ref["blocks"])["v_sum"][1].tolist() == [0, 30]


def test_names_no_key_filters_and_blocks():
    blocks = [(3, {"a": _int([1, 2, 3]), "b": _int([4, 5, 6])}), (0, {}), (2, {"a": _int([4, 5]), "b": _int([7, 8])})]
    ref = U.rollup_ref(blocks, aggs=[("a", "sum"), ("b", "max")], count_name="rows", filters=[("a", "gt", 1)])
    assert ref["columns"] == [("rows", "int"), ("a_sum", "int"), ("b_max", "int")]
    assert _table(ref) == {"rows": [4], "a_sum": [14], "b_max": [8]} and ref["stats"]["rows_in"] == 5 and ref["stats"]["rows_matched"] == 4
    none = U.rollup_ref(blocks, aggs=[("a", "sum")], filters=[("a", "gt", 99)])
    assert none["blocks"] == [] and none["stats"]["groups"] == 0 and none["columns"] == [("count", "int"), ("a_sum", "int")]
    cut = U.rollup_ref(blocks, groups=["a"], block_rows=2)
    assert [n for n, _ in cut["blocks"]] == [2, 2, 1] and cut["stats"]["blocks_out"] == 3
    with pytest.raises(AssertionError):
        U.rollup_ref(blocks, groups=["a"], aggs=[("b", "sum")], count_name="b_sum")
    with pytest.raises(ValueError):
        U.rollup_ref(blocks, aggs=[("a", "avg")])
    with pytest.raises(ValueError):
        U.rollup_ref(blocks, aggs=[("a", "")])


def test_the_path_rule_and_slots():
    assert U.choose_path(1 << 16, 10, 1) == U.GLOBAL and U.choose_path((1 << 16) + 1, 10, 1) == U.HASH
    assert U.choose_path(80000, 20000, 1) == U.GLOBAL and U.choose_path(80001, 20000, 1) == U.HASH
    assert U.choose_path(8192, 10, 1) == U.LDS and U.choose_path(8193, 10, 1) == U.GLOBAL
    assert U.choose_path(1638, 10, 5) == U.LDS and U.choose_path(1639, 10, 5) == U.GLOBAL
    assert U.choose_path(1 << 27, 1 << 26, 1) == U.GLOBAL and U.choose_path((1 << 27) + 1, 1 << 26, 1) == U.HASH
    assert U.choose_path((1 << 27) + 1, 10, 1, "direct") is None and U.choose_path(100, 10, 1, "global") == U.GLOBAL
    assert U.choose_path(100, 10, 1, "hash") == U.HASH and U.choose_path(100000, 10, 1, "direct") == U.GLOBAL
    assert U.slots_for(10, 1 << 40) == 64 and U.slots_for(33, 1 << 40) == 128 and U.slots_for(1000, 40) == 128
    assert U.slots_for(1 << 30, 1 << 40) == 1 << 27 and U.slots_for(1000, 1 << 40, asked=32) == 32 and U.slots_for(5, 5, asked=33) == 64
    with pytest.raises(OverflowError):
        U.rollup_ref([(2, {"k": ("int", np.array([I64_MIN, I64_MAX]), None)})], groups=["k"])
