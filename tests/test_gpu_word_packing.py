"""GPU: two quantities in one LDS word, at the row counts where the word is full.

Two scan paths pack a pair of counters into one LDS word and rest on an argument that the pair cannot run into each other:

* Count in the high bits of aggregation 0's sum word (FastPlan::cshift; planner.cpp: plan_count_packing, scan_packed.h:
  packed_row, scan_fast.h: fast_finish / sum_of).  The planner takes it when the rows one replica word can receive, and that
  many times the column's largest stored offset, fit 64 bits together.
* the -limit pushdown's 15-bit group counters, two to a word with a guard bit each (pushdown.hip: k_pd_count / k_pd_fold): a
  field that fills hands 32 768 over to a device-side carry word.

Both boundaries are per WORKGROUP, and the planner launches one workgroup per CU, so they move with the device: the tables here
are sized from the workgroup count of the device under test.  work() deals the 2048-row tiles of the single contiguous run out
evenly, so a table of n_wg * T * 4096 rows gives every workgroup exactly T packed tiles, and for T = 16 workgroup w owns rows
[w * 65536, (w + 1) * 65536).  The tests use that only to PLACE data where the paths must run; every expected value is a plain
numpy int64 / Python int computation over the whole column and holds whatever the split is.

Not covered: the same boundary for 1- and 2-byte aggregation columns (sum_bits + count_bits reaches 64 only near 4e9 rows per
workgroup set there).  The windowed flush (strategy 4) through sum_of / max_of, for the plain, cshift and lean word layouts, is
tests/test_gpu_time_window.py's.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import parity

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
BLOCK = 65536                    # rows per appended block == rows of one workgroup's share at T = 16
T_PACKED, T_DECLINED = 15, 16    # packed 4096-row tiles per workgroup: the last count that packs, the first that does not
N_KEYS = 4096
K_CONST = 7                      # column "kc": every row
K_LO, K_HI = 100, 101            # the two fields of one counter word
K_TWICE, K_ODD, K_ALL, K_TIE = 2000, 2001, 3000, 50
NEVER = range(3500, 3600)        # keys no row has
TRACE = re.compile(r"count packing: cshift=(\d+) sum_bits=(\d+) count_bits=(\d+) slot_rows=(\d+)")


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


def _trace(err):
    """The planner's `count packing:` lines (SYBL_PLAN_TRACE=1) as (cshift, sum_bits, count_bits, slot_rows) tuples."""
    return [tuple(int(x) for x in m.groups()) for m in TRACE.finditer(err)]


def _group_ref(key, val):
    """{key: (count, sum, min, max)} of val per key, exact: counts with bincount, the rest over a stable sort by key with
    reduceat -- int64 throughout, and shown not to wrap.  min / max are the values' own (BasicHist's start value is applied by
    _check_avg)."""
    key = np.asarray(key, dtype=np.int64)
    val = np.asarray(val, dtype=np.int64)
    cnt = np.bincount(key, minlength=int(key.max()) + 1)
    assert int(cnt.max()) * max(abs(int(val.min())), abs(int(val.max()))) < 1 << 63   # no per-group sum can wrap int64
    assert 0 <= int(key.min()) and int(key.max()) < 65536
    order = np.argsort(key.astype(np.uint16), kind="stable")
    ks, vs = key[order], val[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    sums, mins, maxs = np.add.reduceat(vs, starts), np.minimum.reduceat(vs, starts), np.maximum.reduceat(vs, starts)
    ref = {int(k): (int(cnt[k]), int(s), int(lo), int(hi)) for k, s, lo, hi in zip(ks[starts], sums, mins, maxs)}
    assert sum(c for c, _, _, _ in ref.values()) == key.size
    return ref


def _one_group_ref(key, val):
    """_group_ref for a key column of one value (no sort needed)."""
    assert int(key.min()) == int(key.max()) and key.size * max(abs(int(val.min())), abs(int(val.max()))) < 1 << 63
    assert np.bincount(key).tolist()[-1] == key.size
    return {int(key[0]): (int(key.size), int(val.sum(dtype=np.int64)), int(val.min()), int(val.max()))}


def _check_avg(res, ref, n_rows):
    """An avg-mode result of one group column and one aggregation against _group_ref: every group that has a row and no other,
    Count, Sum, min and max exact, avg to 1e-9.  BasicHist.Min / Max start at 0 in avg mode (hist_basic.go:34-40)."""
    rows = res.rows(0)
    got = {g["key_vals"][0]: g for g in rows}
    assert len(got) == len(rows)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:8]
    assert res.matched == n_rows
    for k, (count, total, lo, hi) in ref.items():
        g, h = got[k], got[k]["hists"][0]
        assert h["present"], k
        assert (g["count"], h["count"], h["sum"]) == (count, count, total), (k, g["count"], h["count"], h["sum"], count, total)
        assert (h["min"], h["max"]) == (min(lo, 0), max(hi, 0)), (k, h["min"], h["max"], lo, hi)
        assert abs(h["avg"] - total / count) <= 1e-9 * max(abs(total / count), 1.0), (k, h["avg"], total / count)
    c = res.cumulative
    grand = sum(t for _, t, _, _ in ref.values())
    assert abs(grand) < 1 << 63
    assert (c["count"], c["hists"][0]["count"], c["hists"][0]["sum"]) == (n_rows, n_rows, grand)
    return {k: (g["count"], g["hists"][0]["sum"], g["hists"][0]["min"], g["hists"][0]["max"]) for k, g in got.items()}


def _run_avg(tb, groups, aggs, capfd):
    """prepare + scan + finalize with the plan trace on: (result, stats, the trace's tuples)."""
    capfd.readouterr()
    qy = tb.query(groups=groups, aggs=aggs, op="avg")
    res = qy.run()
    st = qy.stats()
    qy.free()
    return res, st, _trace(capfd.readouterr().err)


# ---------------------------------------------------------------------------------------------- the table, grown once
class _Big:
    pass


@pytest.fixture(scope="module")
def big(ctx):
    """The table at T = 15 tiles per workgroup, and the host columns of all 16 (grown: appends the rest)."""
    tiny = ctx.create_table("probe")
    tiny.add_column("g", "int", 0, 3)
    tiny.add_column("v", "int", 0, 9)
    tiny.append_block(8, {"g": np.arange(8) % 4, "v": np.arange(8)})
    qy = tiny.query(groups=["g"], aggs=["v"])
    qy.run().free()
    n_wg = qy.stats()["n_workgroups"]
    qy.free()
    tiny.free()
    # (10 whole shares are laid out below; beyond 512 workgroups the table is no longer a few seconds' work)
    assert 16 <= n_wg <= 512, "n_workgroups = %d: this file is sized for one workgroup per CU of a 16..512-CU device" % n_wg
    B = _Big()
    B.n_wg = n_wg
    B.n15, B.n16 = n_wg * T_PACKED * 4096, n_wg * T_DECLINED * 4096
    n = B.n16
    rng = np.random.default_rng(20250)
    special = {K_CONST, K_LO, K_HI, K_TWICE, K_ODD, K_ALL, K_TIE} | set(NEVER)
    allowed = np.array([x for x in range(N_KEYS) if x not in special], dtype=np.int64)
    k = allowed[rng.integers(0, allowed.size, n)]
    S = BLOCK
    k[0:32767] = K_LO                      # share 0: the low field stops at 0x7FFF ...
    k[32767:S] = K_HI                      # ... the high field of the same word wraps once (32 769 rows)
    k[S:S + 32768] = K_LO                  # share 1: both fields end at 0 with a carry each
    k[S + 32768:2 * S] = K_HI
    k[2 * S:3 * S] = K_TWICE               # share 2: two wraps of one field
    k[3 * S:4 * S - 1] = K_ODD             # share 3: 65 535 rows of an odd cell (+ one row of the random fill)
    k[4 * S:10 * S] = K_ALL                # shares 4-9: every lane on one field, in several workgroups
    # 65 535 rows spread thinly over the rest (no field fills): ties with K_LO and K_ODD, whose counts went through carries
    stride = (n - 10 * S) // 65535
    assert stride >= 1
    k[10 * S + stride * np.arange(65535)] = K_TIE
    B.k = k
    B.kc = np.full(n, K_CONST, dtype=np.int64)
    B.v = rng.integers(0, 1000, n)
    B.wide = np.full(n, U32, dtype=np.int64)
    B.wide[12345] = 0
    B.wide2 = rng.integers(0, 1 << 32, n)
    B.wide2[0], B.wide2[1] = 0, U32
    B.names = ["kc", "k", "v", "wide", "wide2"]
    tb = ctx.create_table("words")
    tb.add_column("kc", "int", 0, N_KEYS - 1)
    tb.add_column("k", "int", 0, N_KEYS - 1)
    tb.add_column("v", "int", 0, 999)      # (BucketSize 1, no value can be an outlier: what the pushdown asks for)
    tb.add_column("wide", "int", 0, U32)
    tb.add_column("wide2", "int", 0, U32)
    B.tb = tb

    def append(r0, r1):
        for b in range(r0, r1, S):
            tb.append_block(S, {c: getattr(B, c)[b:b + S] for c in B.names})
    B.append = append
    append(0, B.n15)
    for c in ("kc", "k"):
        tb.set_bounds(c, 0, N_KEYS - 1)
    tb.set_bounds("v", 0, 999)
    tb.compact()
    assert [tb.column_storage(c) for c in B.names] == [(1, K_CONST), (2, 0), (2, 0), (4, 0), (4, 0)]
    yield B
    tb.free()


@pytest.fixture
def at15(big):
    assert big.tb.rows == big.n15, "the T = 15 tests run before the table is grown: run this file in its own order"
    return big


@pytest.fixture(scope="module")
def grown(big):
    """The same table at T = 16: n_wg * 4096 more rows, packed into place."""
    if big.tb.rows == big.n15:
        big.append(big.n15, big.n16)
        big.tb.compact()
    assert big.tb.rows == big.n16
    assert [big.tb.column_storage(c) for c in big.names] == [(1, K_CONST), (2, 0), (2, 0), (4, 0), (4, 0)]
    return big


# ---------------------------------------------------------------------------------------------- A. Count in the sum word
def _expect_plan(st):
    # (4096 cells x (Count, sum, max) x 8 bytes = 96 KiB: one replica is all the LDS holds)
    assert (st["strategy"], st["packed_kernel"], st["replicas"]) == (2, 1, 1), st


def test_count_packing_is_taken_where_sum_and_count_exactly_fill_the_word(at15, capfd, monkeypatch):
    """T = 15: every lane of a workgroup sees 60 rows, the one replica word of the only group 61 440 -- 16 bits of Count above
    48 bits of offsets, each of which is 2^32 - 1 but one.  The extreme the planner's argument allows, and really reached."""
    B = at15
    slot_rows = T_PACKED * 4 * 1024
    assert slot_rows == 61440 and slot_rows.bit_length() == 16 and (slot_rows * U32).bit_length() == 48
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    res, st, tr = _run_avg(B.tb, ["kc"], ["wide"], capfd)
    with capfd.disabled():
        print("case A trace:", tr, "n_wg", B.n_wg)
    _expect_plan(st)
    assert tr and set(tr) == {(48, 48, 16, 61440)}, tr
    ref = _one_group_ref(B.kc[:B.n15], B.wide[:B.n15])
    assert ref == {K_CONST: (B.n15, (B.n15 - 1) * U32, 0, U32)}
    _check_avg(res, ref, B.n15)
    res.free()


def test_random_keys_with_and_without_count_packing(at15, capfd, monkeypatch):
    """The same table through its random key column and a random 4-byte column (shares 0-9 are single-key runs: up to 61 440
    rows a word there too): packed Count, Count in its own word (SYBL_NO_CPACK=1) and numpy agree."""
    B = at15
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    ref = _group_ref(B.k[:B.n15], B.wide2[:B.n15])
    assert not set(ref) & set(NEVER)
    res, st, tr = _run_avg(B.tb, ["k"], ["wide2"], capfd)
    _expect_plan(st)
    assert tr and set(tr) == {(48, 48, 16, 61440)}, tr
    packed = _check_avg(res, ref, B.n15)
    res.free()
    monkeypatch.setenv("SYBL_NO_CPACK", "1")
    res, st, tr = _run_avg(B.tb, ["k"], ["wide2"], capfd)
    _expect_plan(st)
    assert tr == []          # (switched off before the widths are looked at)
    plain = _check_avg(res, ref, B.n15)
    res.free()
    assert packed == plain


def test_count_packing_is_declined_one_tile_later(grown, capfd, monkeypatch):
    """T = 16: 65 536 rows a word would need 17 bits above the 48: Count keeps its own word, and 65 536 rows of 2^32 - 1 in one
    workgroup's cell come out exact (packed all the same, Count << 48 would have wrapped to 0)."""
    B = grown
    slot_rows = T_DECLINED * 4 * 1024
    assert slot_rows == 65536 and slot_rows.bit_length() == 17 and (slot_rows * U32).bit_length() == 48
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    res, st, tr = _run_avg(B.tb, ["kc"], ["wide"], capfd)
    with capfd.disabled():
        print("case B trace:", tr, "n_wg", B.n_wg)
    _expect_plan(st)
    assert tr and set(tr) == {(0, 48, 17, 65536)}, tr
    ref = _one_group_ref(B.kc, B.wide)
    assert ref == {K_CONST: (B.n16, (B.n16 - 1) * U32, 0, U32)}
    _check_avg(res, ref, B.n16)
    res.free()
    # ... and the random columns, whole shares of one key among them
    ref = _group_ref(B.k, B.wide2)
    res, st, tr = _run_avg(B.tb, ["k"], ["wide2"], capfd)
    _expect_plan(st)
    assert tr and set(tr) == {(0, 48, 17, 65536)}, tr
    first = _check_avg(res, ref, B.n16)
    res.free()
    monkeypatch.setenv("SYBL_NO_CPACK", "1")
    res, st, tr = _run_avg(B.tb, ["k"], ["wide2"], capfd)
    assert tr == []
    assert _check_avg(res, ref, B.n16) == first
    res.free()


@pytest.mark.parametrize("base", [0, -(1 << 31), 7])
def test_replicas_of_a_packed_word_fold_without_carrying_into_the_count(ctx, capfd, monkeypatch, base):
    """64, 8 and 1 lane replicas of a 64-cell table (SYBL_REP_BUDGET_KB): a replica's word holds Count << cshift + offsets, and the
    replicas' offset sums together pass bit cshift -- fast_finish unfolds them one by one.  Four of the 64 keys occur.  One
    group's only value is the column minimum: its offsets are all 0 while its Count is not, and its maximum is rebuilt from
    the storage base (max_of) -- visible where the base is above BasicHist's start value 0 (base 7).  A negative base tracks a
    minimum beside the maximum."""
    n = 2_500_077
    rng = np.random.default_rng(606 + (base & 0xFF))
    g = np.array([3, 17, 63], dtype=np.int64)[rng.choice(3, n, p=[0.8, 0.15, 0.05])]
    wide = rng.integers(0, 1 << 32, n)
    wide[g == 3] |= 1 << 31          # (the hot group's offsets in the upper half)
    wide += base
    only_min = rng.choice(n, 1000, replace=False)
    g[only_min], wide[only_min] = 40, base
    wide[np.flatnonzero(g == 3)[0]] = base + U32
    assert int(wide.min()) == base and int(wide.max()) == base + U32
    tb = ctx.create_table("rep")
    tb.add_column("g", "int", 0, 63)
    tb.add_column("wide", "int", base, base + U32)
    for r0 in range(0, n, BLOCK):
        tb.append_block(min(BLOCK, n - r0), {"g": g[r0:r0 + BLOCK], "wide": wide[r0:r0 + BLOCK]})
    tb.set_bounds("g", 0, 63)
    tb.compact()
    assert tb.column_storage("wide") == (4, base)
    ref = _group_ref(g, wide)
    assert sorted(ref) == [3, 17, 40, 63] and ref[40][2:] == (base, base)
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    # one replica of the cell table: 64 cells x (Count, sum, max[, -min]) x 8 bytes = 1536 or 2048 bytes; the planner doubles
    # the replicas while they fit the budget: 2 KiB -> 1, 16 KiB -> 8, the whole LDS -> 64
    seen = []
    for replicas, budget in ((64, None), (8, "16"), (1, "2")):
        if budget:
            monkeypatch.setenv("SYBL_REP_BUDGET_KB", budget)
        for packing in (True, False):
            if packing:
                monkeypatch.delenv("SYBL_NO_CPACK", raising=False)
            else:
                monkeypatch.setenv("SYBL_NO_CPACK", "1")
            res, st, tr = _run_avg(tb, ["g"], ["wide"], capfd)
            assert (st["strategy"], st["packed_kernel"], st["replicas"]) == (2, 1, replicas), st
            if packing:
                assert tr and len(set(tr)) == 1, tr
                cshift, sum_bits, count_bits, slot_rows = tr[0]
                # (the words of one replica take the rows of 1024 / replicas lanes)
                assert slot_rows % (4 * 1024 // replicas) == 0 and slot_rows * replicas >= -(-n // st["n_workgroups"])
                assert (sum_bits, count_bits) == ((slot_rows * U32).bit_length(), slot_rows.bit_length())
                assert cshift == sum_bits and sum_bits + count_bits <= 64
                if replicas == 64:   # the fold matters: the hot group's offsets, all replicas together, pass bit cshift
                    assert ref[3][1] - ref[3][0] * base >= st["n_workgroups"] << cshift
            else:
                assert tr == []
            seen.append(_check_avg(res, ref, n))
            if base > 0:
                assert seen[-1][40][3] == base
            res.free()
    assert all(s == seen[0] for s in seen)
    tb.free()


# ---------------------------------------------------------------------------------------------- B. pushdown counters that carry
@pytest.fixture(scope="module")
def pd_oracle(grown, oracle):
    B = grown
    q = dict(groups=["k"], aggs=["v"], op="hist")
    ores = oracle.run_query([{"type": "int", "data": B.k}, {"type": "int", "data": B.v}], n_threads=16,
                            **parity.oracle_query_kwargs(["k", "v"], {"k": (0, N_KEYS - 1), "v": (0, 999)}, q))
    return ores


@pytest.mark.parametrize("limit", [1, 5, 50])
def test_pushdown_counters_that_fill_and_carry(grown, pd_oracle, limit):
    """T = 16, so a share is one 65 536-row block: single-key runs of 32 767, 32 768, 32 769, 65 535, 65 536 rows and six whole
    shares of one key take the 15-bit fields of k_pd_count to their guard bit, low field and high field, once and twice; k_pd_fold
    adds the carries back; k_pd_select ranks carried counts, three of them tied at 65 535 across the limit of 5."""
    B = grown
    counts = np.bincount(B.k, minlength=N_KEYS)
    vals, cnts = np.unique(B.k, return_counts=True)
    assert np.array_equal(vals, np.flatnonzero(counts)) and np.array_equal(cnts, counts[vals])
    assert [int(counts[x]) for x in (K_LO, K_HI, K_TWICE, K_ODD, K_ALL, K_TIE)] == [65535, 65537, 65536, 65535, 6 * 65536, 65535]
    assert not counts[NEVER.start:NEVER.stop].any()
    by_count = sorted(cnts.tolist(), reverse=True)
    assert by_count[:6] == [6 * 65536, 65537, 65536, 65535, 65535, 65535] and by_count[6] < 32768   # the tie straddles limit 5
    q = dict(groups=["k"], aggs=["v"], op="hist", want_percentiles=True, limit=limit, order_by="$COUNT")
    runs = []
    for level in (1, 2):
        qy = B.tb.query(**dict(q, printed_only=level))
        r = qy.run()
        runs.append((r, qy, qy.stats()))
    (r1, q1, s1), (r2, q2, s2) = runs
    assert (s1["strategy"], s2["strategy"]) == (5, 8), (s1["strategy"], s2["strategy"])
    assert s2["n_workgroups"] == B.n_wg
    text1, json1 = r1.render("text"), r1.render("json")
    assert r2.render("text") == text1
    assert r2.render("json") == json1
    assert r2.matched == r1.matched == B.n16

    def check(res):
        rows = res.rows(0)
        got = {g["key_vals"][0]: g["count"] for g in rows}
        assert len(got) == len(rows)
        assert got == dict(zip(vals.tolist(), cnts.tolist())), [(x, got.get(x), int(counts[x])) for x in vals.tolist() if got.get(x) != counts[x]][:8]
        assert [g["count"] for g in rows] == by_count
        return rows

    rows1, rows2 = check(r1), check(r2)
    assert [g["key"] for g in rows2[:limit]] == [g["key"] for g in rows1[:limit]]
    if limit == 5:
        printed = [g["key_vals"][0] for g in rows2[:5]]
        assert printed[:3] == [K_ALL, K_HI, K_TWICE] and set(printed[3:]) < {K_TIE, K_LO, K_ODD}, printed
    omap = {r["key"]: r for r in pd_oracle["results"]}
    assert len(omap) == len(rows2)
    for i, g in enumerate(rows2):
        assert g["count"] == omap[g["key"]]["count"]
        if i < limit:
            parity.compare_hist(g["hists"][0], omap[g["key"]]["hists"][0], "hist", True, ctx=(limit, i))
    parity.compare_hist(r2.cumulative["hists"][0], pd_oracle["cumulative"]["hists"][0], "hist", True, ctx=("cumulative", limit), cumulative=True)
    # a rescan of the same prepared query: the carries and the list of printed cells start from zero again
    r3 = q2.run()
    assert r3.render("text") == text1 and r3.render("json") == json1
    assert r3.matched == B.n16
    check(r3)
    for r in (r1, r2, r3):
        r.free()
    q1.free()
    q2.free()
