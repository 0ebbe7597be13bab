"""tests/digest_ref.py (the numpy restatement the GPU digest is checked against) held to hand-checked answers."""
import numpy as np

from tests import digest_ref as D

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _int_block(times, extra=None):
    vals = np.array([0 if t is None else t for t in times], dtype=np.int64)
    pop = np.array([t is not None for t in times], dtype=bool)
    cols = {"time": ("int", vals, pop), "row": ("int", np.arange(len(times), dtype=np.int64), None)}
    cols.update(extra or {})
    return (len(times), cols)


def test_unpopulated_row_sorts_as_zero_and_ties_keep_source_order():
    blocks = [_int_block([5, None, -3, 5, 0])]
    # -3 | the row without a time (key 0, came first) | the real 0 | the two 5s in source order
    assert D.permutation(blocks).tolist() == [2, 1, 4, 0, 3]
    out = D.digest_ref(blocks)
    assert len(out) == 1 and out[0][0] == 5
    assert out[0][1]["row"][1].tolist() == [2, 1, 4, 0, 3]
    assert out[0][1]["time"][2].tolist() == [True, False, True, True, True]
    assert D.rows_of(out) == [{"time": -3, "row": 2}, {"row": 1}, {"time": 0, "row": 4}, {"time": 5, "row": 0}, {"time": 5, "row": 3}]


def test_int64_extremes_around_an_unpopulated_row():
    blocks = [_int_block([I64_MAX, None, I64_MIN]), _int_block([I64_MIN, I64_MAX, None])]
    # keys: MAX 0 MIN | MIN MAX 0  ->  the MINs (rows 2, 3), the zeros (1, 5), the MAXs (0, 4)
    assert D.permutation(blocks).tolist() == [2, 3, 1, 5, 0, 4]
    rows = D.rows_of(D.digest_ref(blocks))
    assert [r.get("time") for r in rows] == [I64_MIN, I64_MIN, None, None, I64_MAX, I64_MAX]


def test_block_rows_cut_2_2_1_and_carry_every_type():
    extra = {"s": ("str", ["a", None, "c", "d", "e"]), "t": ("set", [["x"], [], None, ["y", "z"], ["x"]])}
    blocks = [_int_block([5, None, -3, 5, 0], extra)]
    out = D.digest_ref(blocks, block_rows=2)
    assert [n for n, _ in out] == [2, 2, 1]
    assert [b[1]["s"][1] for b in out] == [["c", None], ["e", "a"], ["d"]]
    assert [b[1]["t"][1] for b in out] == [[None, []], [["x"], ["x"]], [["y", "z"]]]
    assert D.rows_of(out)[1] == {"row": 1, "t": []}
    # several source blocks, one of them without the columns and one without rows
    two = [_int_block([5, None], {"s": ("str", ["a", None])}), (0, {}), (3, {"time": ("int", np.array([-3, 5, 0], dtype=np.int64), None)})]
    out = D.digest_ref(two, block_rows=2)
    assert [n for n, _ in out] == [2, 2, 1]
    assert D.rows_of(out) == [{"time": -3}, {"row": 1}, {"time": 0}, {"time": 5, "row": 0, "s": "a"}, {"time": 5}]


def test_other_time_column_and_default_block_size():
    blocks = [(3, {"time": ("int", np.array([1, 2, 3], dtype=np.int64), None), "ts": ("int", np.array([9, 7, 8], dtype=np.int64), None)})]
    assert D.permutation(blocks, "ts").tolist() == [1, 2, 0]
    n = D.BLOCK_ROWS + 3
    big = [(n, {"time": ("int", np.arange(n, dtype=np.int64)[::-1].copy(), None)})]
    out = D.digest_ref(big)
    assert [b[0] for b in out] == [D.BLOCK_ROWS, 3]
    assert out[1][1]["time"][1].tolist() == [n - 3, n - 2, n - 1]


def test_empty_table():
    assert D.digest_ref([]) == []
    empty = [(0, {"time": ("int", np.zeros(0, dtype=np.int64), None)})]
    assert D.digest_ref(empty) == [] and D.rows_of(empty) == []
