"""CPU: tests/chain_ref.py -- the composer of the restatements that tests/test_gpu_derived_chains.py checks the GPU against --
held to answers written by hand on a table of twelve rows, and the three documented routes held to their identities on the
restatements alone, before a GPU is involved."""
import numpy as np
import pytest

from tests import chain_ref as CH
from tests import digest_ref as D
from tests.test_gpu_rollup import MAIN

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NONE = None


def _tiny():
    """row   0    1     2    3     4    5    6     7    8     9    10    11
    time    30   10    20   10    50   40    5    60   25    15    35    45
    k        1    2     1    2     -    1    2     3    1     2     3     1
    v       10    -    30   40    50   60  -75     -   90  -101     -   120
    s        b    a     b    -     c    a    b     a    c     b     a     c      in blocks of 5 and 7 rows"""
    time = np.array([30, 10, 20, 10, 50, 40, 5, 60, 25, 15, 35, 45], dtype=np.int64)
    k = np.array([1, 2, 1, 2, 0, 1, 2, 3, 1, 2, 3, 1], dtype=np.int64)
    kp = np.arange(12) != 4
    v = np.array([10, 0, 30, 40, 50, 60, -75, 0, 90, -101, 0, 120], dtype=np.int64)
    vp = ~np.isin(np.arange(12), (1, 7, 10))
    s = ["b", "a", "b", NONE, "c", "a", "b", "a", "c", "b", "a", "c"]
    out, r0 = [], 0
    for n in (5, 7):
        sl = slice(r0, r0 + n)
        out.append((n, {"time": ("int", time[sl], None), "k": ("int", k[sl], kp[sl]), "v": ("int", v[sl], vp[sl]), "s": ("str", s[sl])}))
        r0 += n
    return out


TINY = _tiny()


def test_select_digest_rollup_orders_str_keys_by_the_carried_dictionary():
    """v > 25 keeps rows 2 3 4 5 8 11; by time they are 3 2 8 5 11 4, whose strings appear in the order b c a -- but the table's
    dictionary is the source's, b a c, and a rollup orders its str key by dictionary id: MISSING, b, a, c."""
    r = CH.run_ref({"t": TINY}, [("select", dict(filters=[("v", "gt", 25)], block_rows=4)), ("digest", dict(block_rows=5)),
                                ("rollup", dict(groups=["s"], aggs=[("v", "n,sum")]))])
    assert [b[0] for b in r[0]["blocks"]] == [4, 2] and [b[0] for b in r[1]["blocks"]] == [5, 1]
    assert [row["time"] for row in D.rows_of(r[0]["blocks"])] == [20, 10, 50, 40, 25, 45]
    assert [row["time"] for row in D.rows_of(r[1]["blocks"])] == [10, 20, 25, 40, 45, 50]
    assert [row.get("s") for row in D.rows_of(r[1]["blocks"])] == [NONE, "b", "c", "a", "c", "c"]
    assert r[0]["blocks"].dicts == r[1]["blocks"].dicts == {"s": ["b", "a", "c"]} == r[2]["dicts"]
    assert D.rows_of(r[2]["blocks"]) == [{"count": 1, "v_n": 1, "v_sum": 40}, {"s": "b", "count": 1, "v_n": 1, "v_sum": 30},
                                         {"s": "a", "count": 1, "v_n": 1, "v_sum": 60}, {"s": "c", "count": 3, "v_n": 3, "v_sum": 260}]
    assert r[2]["stats"]["rows_in"] == 6 and r[2]["stats"]["cells_or_slots"] == 4          # ids 0 .. 2 and the MISSING digit
    # the same rows as a table built block by block would hold another dictionary and give another order
    plain = CH.run_ref({"t": list(r[1]["blocks"])}, [("rollup", dict(groups=["s"], aggs=[("v", "n,sum")]))])
    assert [row.get("s") for row in D.rows_of(plain[0]["blocks"])] == [NONE, "b", "c", "a"]


def test_rollup_compute_lookup_average_truncates_toward_zero_and_a_group_without_values_attaches_nothing():
    """By k: MISSING (row 4), 1 (0 2 5 8 11), 2 (1 3 6 9: 40 - 75 - 101 = -136 over 3 values), 3 (7 10: no value).  The averages
    are 50, 62, -45 (not -46) and unpopulated; looked up by k every row of k = 1 gets 62, of k = 2 gets -45, k = 3 matches and
    gets nothing, and row 4, whose k is unpopulated, matches nothing -- the MISSING group's row takes no part."""
    stages = [("rollup", dict(groups=["k"], aggs=[("v", CH.ALL)], block_rows=3)), ("compute", dict(exprs=[("avg", "v_sum / v_n")])),
              ("lookup_dim", dict(t="t", key="k", columns=["avg", "count"], prefix="g_"))]
    for compact in (False, True):
        r = CH.run_ref({"t": TINY}, stages, compact=compact)
        assert D.rows_of(r[0]["blocks"]) == [{"count": 1, "v_n": 1, "v_sum": 50, "v_min": 50, "v_max": 50},
                                             {"k": 1, "count": 5, "v_n": 5, "v_sum": 310, "v_min": 10, "v_max": 120},
                                             {"k": 2, "count": 4, "v_n": 3, "v_sum": -136, "v_min": -101, "v_max": 40},
                                             {"k": 3, "count": 2, "v_n": 0}]
        assert [b[0] for b in r[0]["blocks"]] == [3, 1] == [b[0] for b in r[1]["blocks"]]
        assert [row.get("avg") for row in D.rows_of(r[1]["blocks"])] == [50, 62, -45, NONE]
        assert r[1]["stats"]["unpopulated"] == 1 and r[1]["extrema"]["avg"] == (-45, 62) and r[1]["has_missing"]["avg"]
        assert r[1]["storage"]["avg"] == ((1, -45) if compact else (8, 0))
        assert (r[2]["matched"], r[2]["dim_keys"], r[2]["dim_duplicates"]) == (11, 3, 0)
        assert [row.get("g_avg") for row in D.rows_of(r[2]["blocks"])] == [62, -45, 62, -45, NONE, 62, -45, NONE, 62, -45, NONE, 62]
        assert [row.get("g_count") for row in D.rows_of(r[2]["blocks"])] == [5, 4, 5, 4, NONE, 5, 4, 2, 5, 4, 2, 5]
        assert [b[0] for b in r[2]["blocks"]] == [5, 7] and r[2]["bitmap"] == {"g_avg": True, "g_count": True}
        assert r[2]["storage"] == ({"g_avg": (1, -45), "g_count": (1, 1)} if compact else {"g_avg": (8, 0), "g_count": (8, 0)})


def test_concat_merges_the_carried_dictionaries_and_a_rollup_of_it_sums_the_parts():
    """Two selects put back together in the other order; then the parts' counts summed: the rows of the source by k."""
    stages = [("select", dict(src="t", filters=[("s", "eq", "c")])), ("select", dict(src="t", filters=[("s", "neq", "c")])),
              ("concat", dict(srcs=[0, 1, "t"])), ("rollup", dict(groups=["k"])), ("rollup", dict(src=2, groups=["s"], block_rows=2))]
    r = CH.run_ref({"t": TINY}, stages)
    assert [b[0] for b in r[2]["blocks"]] == [3, 8, 5, 7] and r[2]["blocks"].dicts == {"s": ["b", "a", "c"]}
    assert [row["time"] for row in D.rows_of(r[2]["blocks"])][:11] == [50, 25, 45, 30, 10, 20, 40, 5, 60, 15, 35]
    assert D.rows_of(r[3]["blocks"]) == [{"count": 2}, {"k": 1, "count": 10}, {"k": 2, "count": 7}, {"k": 3, "count": 4}]
    assert D.rows_of(r[4]["blocks"]) == [{"count": 1}, {"s": "b", "count": 8}, {"s": "a", "count": 8}, {"s": "c", "count": 6}]
    assert [b[0] for b in r[4]["blocks"]] == [2, 2]


def test_a_table_without_rows_keeps_its_columns_and_dictionaries():
    none = [("v", "gt", 1000)]
    r = CH.run_ref({"t": TINY}, [("select", dict(filters=none, columns=["s", "k", "v"])), ("rollup", dict(groups=["s"], aggs=[("v", "sum")])),
                                ("digest", dict(src=0, time_col="k")), ("compute", dict(src=0, exprs=[("w", "v + k")])),
                                ("lookup_dim", dict(src=0, t="t", key="k", columns=["v"], prefix="d_")),
                                ("concat", dict(srcs=[0, 1])), ("rollup_pct", dict(src=1, groups=["s"], aggs=[("v_sum", "p50")]))], compact=True)
    for k, cols in ((0, ["s", "k", "v"]), (1, ["s", "count", "v_sum"]), (2, ["s", "k", "v"]), (3, ["s", "k", "v", "w"]),
                    (5, ["s", "k", "v", "count", "v_sum"]), (6, ["s", "count", "v_sum_p50"])):
        assert [c for c, _ in r[k]["columns"]] == cols == list(D.column_types(r[k]["blocks"]))
        assert [b[0] for b in r[k]["blocks"]] == [0] and CH.live(r[k]["blocks"]) == [] and r[k]["blocks"].dicts == {"s": ["b", "a", "c"]}, k
    assert r[1]["stats"] == dict(rows_in=0, rows_matched=0, rows_no_time=0, groups=0, blocks_out=0, path=0, fields=5, cells_or_slots=0)
    assert r[1]["storage"] == {"count": (1, 0), "v_sum": (1, 0)} and r[3]["storage"] == {"w": (1, 0)} and r[6]["storage"]["v_sum_p50"] == (1, 0)
    assert (r[4]["matched"], r[4]["dim_keys"]) == (0, 0) and r[4]["storage"] == {"d_v": (1, 0)} and r[4]["bitmap"] == {"d_v": True}
    assert D.rows_of(r[4]["blocks"]) == D.rows_of(TINY) and [b[0] for b in r[4]["blocks"]] == [5, 7]
    assert CH.exact_extrema(r[0]["blocks"], "k") == (I64_MAX, I64_MIN) == CH.exact_extrema(r[0]["blocks"], "s")
    assert CH.fitted_storage(r[0]["blocks"], "k", True) == (1, 0) and CH.fitted_storage(r[0]["blocks"], "s", False) == (4, 0)


def test_a_bitmap_is_carried_and_gives_a_rollup_key_the_missing_digit():
    """k has a bitmap (row 4).  k == 1 keeps populated rows only, and the select's column keeps the bitmap: a rollup by k then has
    the one value and the MISSING digit, 2 cells; the same rows as a table built block by block have no bitmap, 1 cell.  A rollup's
    key has a bitmap iff the MISSING group occurs; concat: iff a source has one or a source with rows lacks the column."""
    stages = [("select", dict(filters=[("k", "eq", 1)])), ("rollup", dict(groups=["k"])), ("concat", dict(srcs=[1, "t"])),
              ("compute", dict(src=0, exprs=[("w", "v / (v - 10)")])), ("rollup", dict(src="t", groups=["k", "s"], filters=[("v", "gt", 45)]))]
    r = CH.run_ref({"t": TINY}, stages)
    assert not CH.has_unpopulated(r[0]["blocks"], "k") and r[0]["blocks"].bitmap == {"time": False, "k": True, "v": True, "s": True}
    assert (r[1]["stats"]["cells_or_slots"], r[1]["stats"]["groups"]) == (2, 1) and r[1]["blocks"].bitmap == {"k": False, "count": False}
    assert CH.run_ref({"t": list(r[0]["blocks"])}, stages[1:2])[0]["stats"]["cells_or_slots"] == 1
    assert r[2]["blocks"].bitmap == {"k": True, "count": True, "time": True, "v": True, "s": True}
    assert r[3]["blocks"].bitmap["w"] and [row.get("w") for row in D.rows_of(r[3]["blocks"])] == [NONE, 1, 1, 1, 1]     # 10 / 0: unpopulated
    assert r[4]["blocks"].bitmap == {"k": True, "s": False, "count": False} and CH.bitmap_of(TINY, "s") and not CH.bitmap_of(TINY, "time")


def test_the_helpers_that_compare_tables():
    assert CH.exact_extrema(TINY, "v") == (-101, 120) and CH.exact_extrema(TINY, "s") == (0, 2) and CH.exact_extrema(TINY, "k") == (1, 3)
    assert CH.has_unpopulated(TINY, "k") and CH.has_unpopulated(TINY, "s") and not CH.has_unpopulated(TINY, "time")
    assert CH.fitted_storage(TINY, "v", True) == (1, -101) and CH.fitted_storage(TINY, "v", False) == (8, 0)
    assert CH.fitted_storage(TINY, "s", True) == (1, 0)
    sel = CH.run_ref({"t": TINY}, [("select", dict(filters=[("s", "eq", "c")]))])[0]["blocks"]
    assert CH.exact_extrema(sel, "s") == (2, 2) and CH.dicts_of(sel) == {"s": ["b", "a", "c"]}     # the id the source gave "c"
    assert CH.renamed_rows(TINY[:1], {"k": "key", "s": "s"})[3:] == [{"key": 2}, {"s": "c"}]


class _FakeTable:
    """What run_gpu needs of a Table: the seven calls (recorded) and free."""
    log = []

    def __init__(self, name, fail_on=None):
        self.name, self.ctx, self.freed, self.fail_on = name, self, 0, fail_on

    def _new(self, op, *a, **kw):
        import os
        if op == self.fail_on:
            raise RuntimeError(op)
        _FakeTable.log.append((op, self.name, a, kw, os.environ.get("SYBL_ROLLUP_PATH"), os.environ.get("SYBL_ROLLUP_PCT")))
        made = _FakeTable("%s>%s" % (self.name, op), self.fail_on)
        _FakeTable.made.append(made)
        return made

    def free(self):
        self.freed += 1

    digest = lambda self, **kw: self._new("digest", **kw)
    select = lambda self, **kw: self._new("select", **kw)
    compute = lambda self, **kw: self._new("compute", **kw)
    rollup = lambda self, **kw: self._new("rollup", **kw)
    lookup = lambda self, dim, **kw: self._new("lookup", dim.name, **kw)
    concat = lambda self, tables, **kw: self._new("concat", [t.name for t in tables], **kw)


def test_run_gpu_makes_the_same_calls_and_frees_what_it_made_on_every_exit(monkeypatch):
    import os
    monkeypatch.setenv("SYBL_ROLLUP_PATH", "global")
    stages = [("select", dict(filters=[("v", "gt", 1)])), ("rollup_pct", dict(groups=["k"], force="hash", pct_force="64")),
              ("lookup_dim", dict(t="t", key="k")), ("lookup", dict(src="t", dim=1, key="k")), ("concat", dict(srcs=[0, "u", 0])),
              ("digest", dict(src=4, block_rows=7)), ("compute", dict(exprs=[("a", "1")])), ("rollup", dict(groups=[]))]
    _FakeTable.log, _FakeTable.made = [], []
    t, u = _FakeTable("t"), _FakeTable("u")
    with CH.run_gpu({"t": t, "u": u}, stages) as made:
        assert [m.name for m in made] == ["t>select", "t>select>rollup", "t>lookup", "t>lookup", "t>select>concat", "t>select>concat>digest",
                                          "t>select>concat>digest>compute", "t>select>concat>digest>compute>rollup"]
        assert not any(m.freed for m in made)
    assert _FakeTable.log == [("select", "t", (), dict(filters=[("v", "gt", 1)]), NONE, NONE), ("rollup", "t>select", (), dict(groups=["k"]), "hash", "64"),
                              ("lookup", "t", ("t>select>rollup",), dict(key="k"), NONE, NONE), ("lookup", "t", ("t>select>rollup",), dict(key="k"), NONE, NONE),
                              ("concat", "t>select", (["t>select", "u", "t>select"],), {}, NONE, NONE), ("digest", "t>select>concat", (), dict(block_rows=7), NONE, NONE),
                              ("compute", "t>select>concat>digest", (), dict(exprs=[("a", "1")]), NONE, NONE),
                              ("rollup", "t>select>concat>digest>compute", (), dict(groups=[]), NONE, NONE)]
    assert [m.freed for m in made] == [1] * 8 and (t.freed, u.freed) == (0, 0)
    assert os.environ["SYBL_ROLLUP_PATH"] == "global" and "SYBL_ROLLUP_PCT" not in os.environ          # the switches are put back
    # a stage that fails: what was made before it is freed, the error passes
    _FakeTable.log, _FakeTable.made = [], []
    t = _FakeTable("t", fail_on="compute")
    with pytest.raises(RuntimeError):
        with CH.run_gpu({"t": t}, stages[:1] + stages[6:]):
            raise AssertionError("the block is not entered")
    assert [m.freed for m in _FakeTable.made] == [1] and t.freed == 0
    # an exception inside the block
    _FakeTable.made = []
    with pytest.raises(KeyError):
        with CH.run_gpu({"t": _FakeTable("t")}, stages[:2]):
            raise KeyError("x")
    assert [m.freed for m in _FakeTable.made] == [1, 1]


# ------------------------------------------------------------------ the three documented routes, on the restatements

@pytest.mark.parametrize("compact", [True, False])
def test_merge_of_ranks_equals_one_rollup_of_all_rows(compact):
    sources, stages = CH.merge_route(MAIN)
    assert sum(b[0] for k in range(3) for b in sources["rank%d" % k]) == sum(b[0] for b in MAIN) == 3161
    r = CH.run_ref(sources, stages, compact=compact)
    assert [x["stats"]["path"] for x in r[:4]] == [2, 2, 3, 3] and r[3]["stats"]["groups"] == 0 and CH.live(r[3]["blocks"]) == []
    parts, merged, one = r[4]["blocks"], r[5], r[6]
    assert len(CH.live(parts)) == 3 and sum(b[0] for b in parts) == sum(x["stats"]["groups"] for x in r[:3]) == merged["stats"]["rows_in"] == 144
    assert parts.dicts["s"] == one["dicts"]["s"] == merged["dicts"]["s"] and len(parts.dicts["s"]) == 6
    assert merged["stats"]["groups"] == one["stats"]["groups"] == 88 and merged["stats"]["fields"] == 33
    assert CH.renamed_rows(merged["blocks"], CH.MERGED) == CH.renamed_rows(one["blocks"], {v: v for v in CH.MERGED.values()})
    c = D.concat(one["blocks"])
    assert int((c["nb_n"][1] == 0).sum()) == 5 and int((~c["k2"][2]).sum()) == 36 and int((~c["nb_min"][2]).sum()) == 5
    # an unpopulated nb_min of one rank does not enter the merged minimum: some group has it unpopulated in one part, populated in another
    p = D.concat(CH.live(parts))
    key = lambda cols, i: (cols["time"][1][i], cols["k2"][1][i] if cols["k2"][2][i] else NONE, cols["s"][1][i])
    empty = {key(p, i) for i in range(144) if not p["nb_min"][2][i]}
    full = {key(p, i) for i in range(144) if p["nb_min"][2][i]}
    assert empty & full
    # the sums wrapped: some v8_sum of the parts is not the true sum
    assert any(abs(x) > (1 << 62) for x in p["v8_sum"][1].tolist())
    for name, want in CH.MERGED.items():
        if name not in ("time", "k2", "s"):
            assert merged["storage"][name] == one["storage"][want], name     # the same values, the same storage rule
            assert merged["bitmap"][name] == one["bitmap"][want], name


@pytest.mark.parametrize("compact", [True, False])
def test_average_by_compute(compact):
    r = CH.run_ref(*CH.average_route(MAIN), compact=compact)
    roll, avg, top = r
    c = D.concat(avg["blocks"])
    n0 = c["nb_n"][1] == 0
    assert int(n0.sum()) == 5 == avg["stats"]["unpopulated"] and np.array_equal(~c["nb_avg"][2], n0) and c["v8_avg"][2].all()
    sums, ns, got = c["nb_sum"][1].tolist(), c["nb_n"][1].tolist(), c["nb_avg"][1].tolist()
    toward_zero = 0
    for s, n, g in zip(sums, ns, got):
        if n:
            q = abs(s) // n * (1 if s >= 0 else -1)
            assert g == q
            toward_zero += s < 0 and s % n != 0 and q != s // n
    assert toward_zero > 0                                            # negative sums that do not divide: floor would differ
    assert avg["has_missing"] == {"nb_avg": True, "v8_avg": False} and avg["storage"]["nb_avg"] == ((2, -368) if compact else (8, 0))
    assert top["stats"]["groups"] == 7 and top["stats"]["rows_in"] == 88 and top["pct_stats"]["items"] == 83
    assert [n for n, _ in top["columns"]] == ["s", "count", "nb_avg_min", "nb_avg_max", "nb_avg_p50"]
    assert D.rows_of(top["blocks"])[:2] == [{"count": 20, "nb_avg_min": -294, "nb_avg_max": 358, "nb_avg_p50": 12},
                                            {"s": "host01", "count": 12, "nb_avg_min": -121, "nb_avg_max": 139, "nb_avg_p50": -7}]


@pytest.mark.parametrize("key,groups,dim_keys,matched", [("k2", 4, 3, 2833), ("s", 6, 5, 2479)])
@pytest.mark.parametrize("compact", [True, False])
def test_rollup_as_the_small_side_of_a_lookup(compact, key, groups, dim_keys, matched):
    small, out = CH.run_ref(*CH.lookup_route(MAIN, key), compact=compact)
    c = D.concat(small["blocks"])
    assert small["stats"]["groups"] == groups and small["stats"]["rows_matched"] == 10
    assert c[key][2].tolist() == [False] + [True] * (groups - 1)                               # the MISSING group's row comes first
    assert not c["nb_min"][2][0] and c["nb_min"][2][1:].any() and not c["nb_min"][2][1:].all()  # partly unpopulated under populated keys
    assert (out["matched"], out["dim_keys"], out["dim_duplicates"]) == (matched, dim_keys, 0)
    assert [n for n, _ in out["attached"]] == ["g_count", "g_v1_sum", "g_nb_min", "g_v4_p50"] and all(out["bitmap"].values())
    if compact:
        assert small["storage"]["v1_sum"][0] == 2 and out["storage"]["g_v1_sum"][0] == 2 and out["storage"]["g_v4_p50"][0] == 4
    # every row of the big side: nothing where its key is unpopulated or not in the small side, else its group's row
    big, got = D.concat(MAIN), D.concat(out["blocks"])
    by_key = {(c[key][1][i] if key == "s" else int(c[key][1][i])): i for i in range(1, groups)}
    kv = big[key][1] if key == "s" else big[key][1].tolist()
    hits = 0
    for r in range(3161):
        g = by_key.get(kv[r]) if big[key][2][r] else NONE
        assert bool(got["g_count"][2][r]) == (g is not NONE)
        if g is not NONE:
            hits += 1
            assert got["g_count"][1][r] == c["count"][1][g] and bool(got["g_nb_min"][2][r]) == bool(c["nb_min"][2][g])
            assert got["g_v4_p50"][1][r] == c["v4_p50"][1][g] and got["g_v1_sum"][1][r] == c["v1_sum"][1][g]
    assert hits == matched
