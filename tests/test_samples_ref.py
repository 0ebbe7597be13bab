"""Known answers for tests/samples_ref.py, the numpy restatement the GPU samples tests are held against: the visited
prefix (the reference stops at the first block at which the matched count is STRICTLY greater than the limit,
table_query.go:222-228), the default newest-first order and the sorted order with its tie and missing-value rules
(printer.go:398-456)."""
import numpy as np
import pytest

from tests import samples_ref as R


def _blocks_with_counts(counts, rows_per_block=5):
    """Blocks of rows_per_block rows; `v` is the table-wide row index, `hit` is 1 on the first counts[b] rows of block b."""
    blocks, base = [], 0
    for m in counts:
        v = np.arange(base, base + rows_per_block, dtype=np.int64)
        hit = (np.arange(rows_per_block) < m).astype(np.int64)
        blocks.append((rows_per_block, {"v": ("int", v, None), "hit": ("int", hit, None)}))
        base += rows_per_block
    return blocks


# candidates of counts [3,0,2,4] with 5 rows per block: c0..c8 = rows 0,1,2, 10,11, 15,16,17,18
@pytest.mark.parametrize("limit,P,M,ids", [
    (5, 4, 9, [18, 17, 16, 15, 11]),   # 5 > 5 is false at block 2: the visit goes on
    (4, 3, 5, [11, 10, 2, 1]),         # c4, c3, c2, c1
    (2, 1, 3, [2, 1]),                 # c2, c1
    (0, 1, 3, []),
])
def test_visited_prefix_is_strict(limit, P, M, ids):
    blocks = _blocks_with_counts([3, 0, 2, 4])
    got = R.samples_ref(blocks, filters=[("hit", "eq", 1)], columns=["v"], limit=limit)
    assert (got["blocks_visited"], got["matched"]) == (P, M)
    assert got["row_ids"] == ids
    assert got["rows"] == [{"v": i} for i in ids]


def test_limit_zero_visits_until_the_first_match():
    got = R.samples_ref(_blocks_with_counts([0, 0, 1]), filters=[("hit", "eq", 1)], limit=0)
    assert (got["blocks_visited"], got["matched"], got["rows"]) == (3, 1, [])


def test_no_match_visits_every_block():
    got = R.samples_ref(_blocks_with_counts([0, 0, 0, 0]), filters=[("hit", "eq", 1)], limit=7)
    assert (got["blocks_visited"], got["matched"], got["rows"], got["row_ids"]) == (4, 0, [], [])
    assert R.samples_ref([], limit=3) == {"rows": [], "row_ids": [], "matched": 0, "blocks_visited": 0}


def test_sorted_order_ties_and_missing_rows():
    k = np.array([5, 0, 5, 1, 7], dtype=np.int64)
    pop = np.array([1, 0, 1, 1, 1], dtype=bool)
    blocks = [(5, {"k": ("int", k, pop)})]
    desc = R.samples_ref(blocks, order_by="k", order_asc=False, limit=10)
    assert desc["row_ids"] == [1, 4, 2, 0, 3]   # the row without k, then 7, the two 5s by descending row, 1
    assert desc["rows"] == [{}, {"k": 7}, {"k": 5}, {"k": 5}, {"k": 1}]
    asc = R.samples_ref(blocks, order_by="k", order_asc=True, limit=10)
    assert asc["row_ids"] == [3, 0, 2, 4, 1]
    # the limit cuts after reversing
    assert R.samples_ref(blocks, order_by="k", order_asc=True, limit=2)["row_ids"] == [3, 0]
    assert R.samples_ref(blocks, order_by="k", order_asc=False, limit=2)["row_ids"] == [1, 4]


def test_filters_are_anded_and_unpopulated_rows_fail():
    blocks = [(4, {"a": ("int", np.array([1, 2, 3, 4], dtype=np.int64), np.array([1, 1, 0, 1], dtype=bool)),
                   "s": ("str", ["x", None, "xy", "y"]),
                   "t": ("set", [["p"], [], None, ["p", "q"]])}),
              (2, {"a": ("int", np.array([9, 9], dtype=np.int64), None)})]     # s and t absent from the block
    ids = lambda **kw: R.samples_ref(blocks, limit=10, **kw)["row_ids"]
    assert ids(filters=[("a", "gt", 1)]) == [5, 4, 3, 1]
    assert ids(filters=[("a", "neq", 2)]) == [5, 4, 3, 0]
    assert ids(filters=[("s", "re", "^x")]) == [2, 0]
    assert ids(filters=[("s", "neq", "x")]) == [3, 2]
    assert ids(filters=[("t", "in", "p")]) == [3, 0]
    assert ids(filters=[("t", "nin", "p")]) == [1]
    assert ids(filters=[("t", "in", "p"), ("a", "gt", 1)]) == [3]
    got = R.samples_ref(blocks, limit=10)
    assert got["rows"][0] == {"a": 9} and got["rows"][4] == {"a": 2, "t": []} and got["rows"][3] == {"s": "xy"}
