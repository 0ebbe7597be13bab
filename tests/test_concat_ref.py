"""tests/concat_ref.py held to hand-written answers (no GPU, no library)."""
import numpy as np
import pytest

from tests import concat_ref as R
from tests import digest_ref as D


def _ints(*v):
    return ("int", np.array(v, dtype=np.int64), None)


A = [(2, {"time": _ints(1, 2), "s": ("str", ["x", None])}), (0, {"time": _ints(), "s": ("str", [])}), (1, {"time": _ints(3), "s": ("str", ["y"])})]
B = [(1, {"s": ("str", ["y"]), "extra": _ints(9), "time": _ints(4)})]
EMPTY = [(0, {"time": _ints(), "only_here": _ints()})]


def test_column_order_is_first_seen_and_the_named_order_when_named():
    assert R.output_columns([A, B]) == [("time", "int"), ("s", "str"), ("extra", "int")]
    assert R.output_columns([B, A]) == [("s", "str"), ("extra", "int"), ("time", "int")]
    assert R.output_columns([A, B], ["extra", "time", "extra"]) == [("extra", "int"), ("time", "int")]
    with pytest.raises(KeyError):
        R.output_columns([A, B], ["nope"])
    with pytest.raises(ValueError):
        R.output_columns([A, [(1, {"s": _ints(1)})]])


def test_blocks_are_kept_and_a_missing_column_is_unpopulated():
    out = R.concat_ref([A, B])
    assert [b[0] for b in out] == [2, 1, 1]                       # the empty block is gone, nothing is re-cut
    assert D.rows_of(out) == [{"time": 1, "s": "x"}, {"time": 2}, {"time": 3, "s": "y"}, {"time": 4, "s": "y", "extra": 9}]
    assert D.rows_of(R.concat_ref([A, B], ["extra"])) == [{}, {}, {}, {"extra": 9}]
    assert D.rows_of(R.concat_ref([B, A, B], ["time"])) == [{"time": 4}, {"time": 1}, {"time": 2}, {"time": 3}, {"time": 4}]


def test_an_empty_source_gives_its_columns_and_no_rows():
    assert R.concat_ref([EMPTY, EMPTY]) == []
    assert R.output_columns([EMPTY, A]) == [("time", "int"), ("only_here", "int"), ("s", "str")]
    assert D.rows_of(R.concat_ref([A, EMPTY, B], ["time"])) == [{"time": 1}, {"time": 2}, {"time": 3}, {"time": 4}]


def test_dictionary_with_overlap_and_a_permuted_id_order():
    assert R.merged_dict([["a", "b", "c"], ["c", "d", "a", "e"]]) == ["a", "b", "c", "d", "e"]
    assert R.merged_dict([["a", "b"], ["b", "a"]]) == ["a", "b"]
    assert R.merged_dict([[], ["z", "y"], ["y", "x"]]) == ["z", "y", "x"]
    # table 1 uses "d" and "a" (its ids 1..2): its id table is [2, 3, 0, 4], so the ids 3 and 0 come out
    assert R.str_extrema([["a", "b", "c"], ["c", "d", "a", "e"]], [["b"], ["d", "a"]]) == (0, 3)
    # ... and an id between the tracked extrema counts though no row uses it: ids 0..2 of table 1 -> 2, 3, 0
    assert R.str_extrema([["a", "b", "c"], ["c", "d", "a", "e"]], [[], ["c", "a"]]) == (0, 3)
    assert R.str_extrema([["a"], ["b"]], [[], []]) == (R.INT64_MAX, R.INT64_MIN)


def test_width_thresholds():
    assert R.storage_of(10, 265, "int") == (1, 10) and R.storage_of(10, 266, "int") == (2, 10)
    assert R.storage_of(-5, 65530, "int") == (2, -5) and R.storage_of(-5, 65531, "int") == (4, -5)
    assert R.storage_of(1, 1 << 32, "int") == (4, 1) and R.storage_of(0, 1 << 32, "int") == (8, 0)
    assert R.storage_of(R.INT64_MIN, R.INT64_MAX, "int") == (8, 0)
    assert R.storage_of(R.INT64_MIN, R.INT64_MIN + 255, "int") == (1, R.INT64_MIN)
    assert R.storage_of(7, 7, "int") == (1, 7) and R.storage_of(1, 0, "int") == (1, 0)
    assert R.storage_of(0, 255, "str") == (1, 0) and R.storage_of(0, 256, "str") == (2, 0)
    assert R.storage_of(3, 65538, "str") == (2, 3) and R.storage_of(3, 65539, "str") == (4, 0)     # canonical ids: base 0
