"""tests/select_ref.py (the numpy restatement the GPU select is checked against) held to hand-checked answers."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import select_ref as S


def _blocks():
    """Seven rows in blocks of 3, 0 and 4: v = 10..16, a nullable int, a str and a set."""
    a = (3, {"v": ("int", np.array([10, 11, 12], dtype=np.int64), None),
             "ni": ("int", np.array([5, 0, 7], dtype=np.int64), np.array([True, False, True])),
             "s": ("str", ["a", None, "c"]), "t": ("set", [["x"], [], None])})
    b = (4, {"v": ("int", np.array([13, 14, 15, 16], dtype=np.int64), None),
             "ni": ("int", np.array([0, 5, 0, -1], dtype=np.int64), np.array([False, True, True, True])),
             "s": ("str", ["d", "a", None, "g"]), "t": ("set", [["y", "x"], None, ["z"], ["x"]])})
    return [a, (0, {}), b]


def test_no_filter_recuts_the_table():
    out = S.select_ref(_blocks(), block_rows=2)
    assert [n for n, _ in out] == [2, 2, 2, 1]
    assert [b[1]["v"][1].tolist() for b in out] == [[10, 11], [12, 13], [14, 15], [16]]
    assert D.rows_of(out) == D.rows_of(_blocks())
    assert S.matching_rows(_blocks()).tolist() == [0, 1, 2, 3, 4, 5, 6]
    # the default block size holds them all
    assert [n for n, _ in S.select_ref(_blocks())] == [7]


def test_nothing_matches_gives_no_blocks():
    assert S.select_ref(_blocks(), filters=[("v", "gt", 16)]) == []
    assert S.select_ref(_blocks(), filters=[("v", "gt", 5), ("v", "lt", 3)]) == []
    assert S.select_ref([]) == [] and S.select_ref([(0, {"v": ("int", np.zeros(0, dtype=np.int64), None)})]) == []


def test_a_single_row():
    out = S.select_ref(_blocks(), filters=[("v", "eq", 13)])
    assert len(out) == 1 and out[0][0] == 1
    assert D.rows_of(out) == [{"v": 13, "s": "d", "t": ["y", "x"]}]
    assert S.matching_rows(_blocks(), [("v", "eq", 13)]).tolist() == [3]


def test_block_rows_not_a_multiple_of_32_and_ascending_source_order():
    n = 100
    blocks = [(60, {"v": ("int", np.arange(60, dtype=np.int64), None)}), (40, {"v": ("int", np.arange(60, 100, dtype=np.int64), None)})]
    out = S.select_ref(blocks, filters=[("v", "gt", 9)], block_rows=33)
    assert [b[0] for b in out] == [33, 33, 24]
    assert np.concatenate([b[1]["v"][1] for b in out]).tolist() == list(range(10, n))
    assert out[1][1]["v"][1][0] == 43 and out[2][1]["v"][1][-1] == 99


def test_projection_order_and_duplicate_names():
    out = S.select_ref(_blocks(), filters=[("v", "lt", 12)], columns=["s", "v", "s"])
    assert list(out[0][1]) == ["s", "v"]
    assert D.rows_of(out) == [{"s": "a", "v": 10}, {"v": 11}]
    assert S.output_columns(_blocks()) == ["v", "ni", "s", "t"]
    # a filter column need not be an output column
    out = S.select_ref(_blocks(), filters=[("t", "in", "x")], columns=["v"])
    assert D.rows_of(out) == [{"v": 10}, {"v": 13}, {"v": 16}]
    with pytest.raises(KeyError):
        S.select_ref(_blocks(), columns=["nope"])


def test_an_unpopulated_value_fails_a_filter():
    # ni: 5 - 7 | - 5 0 -1 : the stored 0 of an unpopulated row passes neither lt nor neq
    assert S.matching_rows(_blocks(), [("ni", "lt", 6)]).tolist() == [0, 4, 5, 6]
    assert S.matching_rows(_blocks(), [("ni", "neq", 5)]).tolist() == [2, 5, 6]
    assert S.matching_rows(_blocks(), [("s", "neq", "a")]).tolist() == [2, 3, 6]
    assert S.matching_rows(_blocks(), [("t", "nin", "x")]).tolist() == [1, 5]
    out = S.select_ref(_blocks(), filters=[("ni", "lt", 6), ("v", "gt", 10)], block_rows=2)
    assert D.rows_of(out) == [{"v": 14, "ni": 5, "s": "a"}, {"v": 15, "ni": 0, "t": ["z"]}, {"v": 16, "ni": -1, "s": "g", "t": ["x"]}]
    assert [n for n, _ in out] == [2, 1]
