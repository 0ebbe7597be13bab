"""Known answers, written by hand, for tests/lookup_ref.py -- the restatement tests/test_gpu_lookup.py checks the library
against."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import lookup_ref as L


def ints(v, pop=None):
    return ("int", np.array(v, dtype=np.int64), None if pop is None else np.array(pop, dtype=bool))


def test_first_of_duplicates_absent_keys_and_unpopulated_keys_on_either_side():
    t = [(3, {"k": ints([7, 9, 7]), "x": ints([1, 2, 3])}),
         (0, {"k": ints([]), "x": ints([])}),
         (3, {"k": ints([5, 8, 5], [1, 1, 0]), "x": ints([4, 5, 6])})]
    #                      row: 0   1  2   3            4   5
    dim = [(4, {"k": ints([5, 7, 5, 9], [0, 1, 1, 1]), "v": ints([50, 70, 51, 90])}),
           (2, {"k": ints([7, 9]), "v": ints([71, 91], [1, 0])})]
    ref = L.lookup_ref(t, dim, "k")
    # key 5: row 0 of dim is unpopulated, the first populated one is row 2; key 7: rows 1 and 4, the first wins; key 9: rows 3, 5
    assert L.match_rows(t, dim, "k")[0].tolist() == [1, 3, 1, 2, -1, -1]   # 8 is absent from dim; t's last key is unpopulated
    assert (ref["matched"], ref["dim_keys"], ref["dim_duplicates"]) == (4, 3, 2)
    assert ref["attached"] == [("v", "int")]
    assert [b[0] for b in ref["blocks"]] == [3, 3]           # the empty block is gone, boundaries are kept
    assert D.rows_of(ref["blocks"]) == [{"k": 7, "x": 1, "v": 70}, {"k": 9, "x": 2, "v": 90}, {"k": 7, "x": 3, "v": 70},
                                        {"k": 5, "x": 4, "v": 51}, {"k": 8, "x": 5}, {"x": 6}]
    assert ref["bitmap"] == {"v": True} and ref["storage"] == {"v": (8, 0)}


def test_a_matched_row_whose_dim_value_is_unpopulated_is_unpopulated():
    t = [(2, {"k": ints([1, 2])})]
    dim = [(2, {"k": ints([1, 2]), "v": ints([10, 999], [1, 0])})]
    ref = L.lookup_ref(t, dim, "k")
    assert ref["matched"] == 2
    assert D.rows_of(ref["blocks"]) == [{"k": 1, "v": 10}, {"k": 2}]
    v = ref["blocks"][0][1]["v"]
    assert v[1].tolist() == [10, 0] and v[2].tolist() == [True, False]      # the stored value is 0, not 999
    assert ref["bitmap"] == {"v": True}                                       # dim's column has one


def test_every_row_matches_a_fully_populated_column_no_bitmap_one_miss_a_bitmap():
    dim = [(3, {"k": ints([1, 2, 3]), "v": ints([10, 20, 30])})]
    assert L.lookup_ref([(4, {"k": ints([3, 1, 2, 3])})], dim, "k")["bitmap"] == {"v": False}
    assert L.lookup_ref([(4, {"k": ints([3, 1, 4, 3])})], dim, "k")["bitmap"] == {"v": True}


def test_str_keys_compare_as_strings_not_ids():
    # t's dictionary: b a c z ""; dim's: c "" a q b -- the same strings under other ids, and each side holds strings the other lacks
    t = [(6, {"h": ("str", ["b", "a", "c", None, "z", ""])})]
    dim = [(6, {"host": ("str", ["c", "", None, "a", "q", "b"]), "dc": ("str", ["ams", "fra", "xxx", "sfo", "nrt", None])})]
    ref = L.lookup_ref(t, dim, "h", dim_key="host")
    assert L.match_rows(t, dim, "h", "host")[0].tolist() == [5, 3, 0, -1, -1, 1]
    assert (ref["matched"], ref["dim_keys"], ref["dim_duplicates"]) == (4, 5, 0)
    assert D.rows_of(ref["blocks"]) == [{"h": "b"}, {"h": "a", "dc": "sfo"}, {"h": "c", "dc": "ams"}, {}, {"h": "z"},
                                        {"h": "", "dc": "fra"}]
    assert ref["dicts"] == {"dc": ["ams", "fra", "xxx", "sfo", "nrt"]}       # dim's, id for id, used or not
    assert ref["storage"] == {"dc": (4, 0)}
    assert L.lookup_ref(t, dim, "h", dim_key="host", compact=True)["storage"] == {"dc": (1, 0)}


def test_columns_prefix_and_collisions():
    t = [(1, {"k": ints([1]), "v": ints([0]), "d_w": ints([0])})]
    dim = [(1, {"k": ints([1]), "v": ints([5]), "w": ints([6]), "tags": ("set", [["a", "b"]])})]
    with pytest.raises(L.LookupError_) as e:
        L.lookup_ref(t, dim, "k")                              # v is a column of t
    assert e.value.column == "v"
    with pytest.raises(L.LookupError_) as e:
        L.lookup_ref(t, dim, "k", prefix="d_")                 # d_v is fine, d_w is a column of t
    assert e.value.column == "d_w"
    ref = L.lookup_ref(t, dim, "k", prefix="dim.")
    assert ref["attached"] == [("dim.v", "int"), ("dim.w", "int"), ("dim.tags", "set")]       # every column but the key, dim's order
    assert D.rows_of(ref["blocks"]) == [{"k": 1, "v": 0, "d_w": 0, "dim.v": 5, "dim.w": 6, "dim.tags": ["a", "b"]}]
    ref = L.lookup_ref(t, dim, "k", columns=["w", "k", "w"], prefix="x")                      # a repeated name is ignored; the key may be named
    assert ref["attached"] == [("xw", "int"), ("xk", "int")]
    for bad, col in ((dict(key="nope"), "nope"), (dict(key="k", dim_key="nope"), "nope"), (dict(key="k", columns=["zz"], prefix="p"), "zz"),
                     (dict(key="k", dim_key="tags"), "tags"), (dict(key="v", dim_key="tags"), "tags")):
        with pytest.raises(L.LookupError_) as e:
            L.lookup_ref(t, dim, **bad)
        assert e.value.column == col
    with pytest.raises(L.LookupError_):
        L.lookup_ref([(1, {"k": ("str", ["a"])})], dim, "k")   # str against int


def test_storage_rule():
    dim = [(3, {"k": ints([1, 2, 3]), "b1": ints([1000, 1255, 1100]), "b2": ints([-5, 251, 0]), "b4": ints([0, 65536, 7]),
                "b8": ints([0, 1 << 32, 5]), "none": ints([9, 9, 9], [0, 0, 0]), "part": ints([70000, 5, 6], [0, 1, 1]),
                "s": ("str", ["x", None, "y"]), "s_none": ("str", [None, None, None])})]
    t = [(1, {"k": ints([2])})]
    assert L.lookup_ref(t, dim, "k", compact=True)["storage"] == {
        "b1": (1, 1000), "b2": (2, -5), "b4": (4, 0), "b8": (8, 0), "none": (1, 0), "part": (1, 5), "s": (1, 0), "s_none": (1, 0)}
    ref = L.lookup_ref(t, dim, "k")
    assert set(ref["storage"].values()) == {(8, 0), (4, 0)} and ref["storage"]["s"] == (4, 0)
    # dim's extrema decide, not the rows that were matched: row 1 alone is matched, b4 keeps 4 bytes
    assert ref["matched"] == 1 and D.rows_of(ref["blocks"])[0]["b4"] == 65536


def test_an_empty_dim_and_an_empty_t():
    dim0 = [(0, {"k": ints([]), "v": ints([])})]
    ref = L.lookup_ref([(2, {"k": ints([1, 2])})], dim0, "k", compact=True)
    assert (ref["matched"], ref["dim_keys"], ref["dim_duplicates"]) == (0, 0, 0)
    assert D.rows_of(ref["blocks"]) == [{"k": 1}, {"k": 2}] and ref["bitmap"] == {"v": True} and ref["storage"] == {"v": (1, 0)}
    ref = L.lookup_ref([(0, {"k": ints([])})], [(1, {"k": ints([1]), "v": ints([3])})], "k")
    assert ref["blocks"] == [] and ref["attached"] == [("v", "int")] and ref["matched"] == 0 and ref["dim_keys"] == 1
