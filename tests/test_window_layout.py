"""CPU: the claims tests/window_layout.py makes about its tables, from the arrays (no GPU, no library), and its reference
against the CPU oracle on every case and every query of the GPU matrix (tests/test_gpu_time_window.py)."""
import numpy as np
import pytest

from tests import parity
from tests import window_layout as WL

N_WG = 16
TB, T0, SHARE, UNIT = WL.TB, WL.T0, WL.SHARE, WL.UNIT


# ---------------------------------------------------------------------------------------------- shares and windows by hand
def test_shares_by_hand():
    # three workgroups, unequal blocks: 5000 rows at 0, 100 at 5024 (5000 rounded up to 32), 4096 at 5152 (5124 rounded up),
    # 2048 at 9248 -- the last two touch and are one run.  Units: 3 + 1 + 3 = 7, dealt 2 / 2 / 3.
    assert WL.block_starts([5000, 100, 4096, 2048]) == [0, 5024, 5152, 9248]
    assert WL.shares([5000, 100, 4096, 2048], 3) == [[(0, 4096)], [(4096, 904), (5024, 100)], [(5152, 6144)]]
    # the second block skipped: 3 + 3 units, 2 / 2 / 2
    assert WL.shares([5000, 100, 4096, 2048], 3, scanned=[True, False, True, True]) == \
        [[(0, 4096)], [(4096, 904), (5152, 2048)], [(7200, 4096)]]
    # fewer units than workgroups: total * (w + 1) / n - total * w / n
    assert WL.shares([2048, 7], 3) == [[], [(0, 2048)], [(2048, 7)]]
    assert WL.shares([], 3) == [[], [], []]


def test_windows_by_hand():
    blocks = [5000, 100, 4096, 2048]
    # block extrema (min, max, populated rows); the second block has no time value at all
    mn, mx, pop = [10, 0, 250, 399], [199, 0, 330, 405], [5000, 0, 4096, 2048]
    wins, wmax, inside = WL.windows(blocks, 3, mn, mx, pop, 100, (0, 499))
    # workgroup 1 overlaps blocks 0 and 1 -- block 1 is left out; workgroup 2's run is blocks 2 and 3
    assert wins == [(0, 1), (0, 1), (2, 4)] and wmax == 3 and inside
    # skipped block 1: workgroup 1 now holds rows of blocks 0 and 2, workgroup 2 of blocks 2 and 3
    wins, wmax, inside = WL.windows(blocks, 3, mn, mx, pop, 100, (0, 499), scanned=[True, False, True, True])
    assert wins == [(0, 1), (0, 3), (2, 4)] and wmax == 4 and inside
    # a workgroup whose only block has no time value has no window; one without a segment neither
    wins, wmax, inside = WL.windows([2048, 2048, 7], 4, [5, 0, 7], [6, 0, 7], [2048, 0, 7], 100, (0, 99))
    assert wins == [None, (0, 0), None, (0, 0)] and wmax == 1 and inside
    # negative times truncate towards zero; data outside the declared bounds is reported
    wins, wmax, inside = WL.windows([2048], 1, [-150], [150], [2048], 100, (-199, 199))
    assert wins == [(-1, 1)] and wmax == 3 and inside
    assert not WL.windows([2048], 1, [-150], [150], [2048], 100, (-99, 199))[2]


# ---------------------------------------------------------------------------------------------- the cases at n_wg = 16
CASES = {
    "spike": lambda: WL.spike(N_WG),
    "straddle": lambda: WL.straddle(N_WG),
    "small_blocks": lambda: WL.small_blocks(N_WG),
    "idle": lambda: WL.idle(N_WG),
    "nullable": lambda: WL.nullable(N_WG),
    "signed": lambda: WL.signed(N_WG),
    "budget": lambda: WL.budget(N_WG, WL.fit(300, 3)),
    "skips": lambda: WL.skips(N_WG),
    "wide_below": lambda: WL.wide_declared(65535),
    "wide_at": lambda: WL.wide_declared(65536),
}
# the queries each case runs on the GPU
MATRIX = [k for k in WL.QUERIES if k not in ("nullable_key", "nullable_key_signed", "wide", "skip_s")]
CASE_QUERIES = {
    "spike": MATRIX,
    "nullable": ["avg", "nullable_key", "nullable_key_signed"],
    "skips": ["avg", "signed_agg", "skip_s"],
    "wide_below": ["wide"],
    "wide_at": ["wide"],
    "budget": ["avg"],
}
CASE_QUERIES["straddle"] = CASE_QUERIES["spike"]
_built = {}


def _layout(case):
    if case not in _built:
        _built[case] = CASES[case]()
    return _built[case]


def _bucket(t):
    return WL.trunc_div(int(t), TB)


@pytest.mark.parametrize("case", list(CASES))
def test_columns(case):
    L = _layout(case)
    assert set(L.cols) == set(WL.COLUMN_ORDER) and all(a.dtype == np.int64 and a.size == L.n for a in L.cols.values())
    for name in WL.COLUMN_ORDER:
        lo, hi = L.declared(name)
        v = L.cols[name][L.pop[name] != 0] if name in L.pop else L.cols[name]
        assert lo <= int(v.min()) and int(v.max()) <= hi, name
    for a in WL.INFO:
        assert (L.cols[a] != 0).all(), a
    assert int(L.cols["sg"].min()) < 0 < int(L.cols["sg"].max())
    for name, nbytes in WL.STORED_BYTES.items():
        span = int(L.cols[name].max()) - int(L.cols[name].min())
        assert {1: span < 256, 2: 256 <= span < 65536, 4: 65536 <= span < 1 << 32}[nbytes], (name, span)
    if "t" not in L.pop:
        assert (np.diff(L.cols["t"]) >= 0).all()
    # the filters fail a fair share of the rows, and every failing row would count
    for f in (WL.F_RANGE, WL.F_FIVE):
        share = WL.keep(L, f).mean()
        assert 0.5 < share < 0.9, share
    assert (L.t_bounds[1] + 1 - L.t_bounds[0]) % TB == 0 and L.t_bounds[0] % TB == 0


def _fits(L, wmax, queries, layout_for_cells=None):
    for k in queries:
        assert WL.window_bytes(wmax, WL.cells_of(WL.QUERIES[k], L), WL.FIELDS[k]) <= WL.LDS_BUDGET, (k, wmax)
        # ... and the whole table does not (what makes the plan a windowed one)
        n_tb = (L.t_bounds[1] + 1 - L.t_bounds[0]) // TB
        assert WL.window_bytes(n_tb, WL.cells_of(WL.QUERIES[k], L), WL.FIELDS[k]) > WL.LDS_BUDGET, k


def test_spike_shape():
    L = _layout("spike")
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    s = N_WG // 2
    assert inside and wmax == 3 and L.blocks == [SHARE] * N_WG
    assert [w[1] - w[0] + 1 for w in wins] == [3 if g == s else 1 for g in range(N_WG)]
    t = L.cols["t"]
    k = _bucket(t[s * SHARE + 1])
    assert (t[s * SHARE], t[s * SHARE + 1], t[s * SHARE + 2]) == (k * TB - 1, k * TB, k * TB + 1)
    assert wins[s] == (k - 1, k + 1) and wins[s - 1] == (k - 1, k - 1) and wins[s + 1] == (k + 1, k + 1)
    # shares pair up in one bucket: the cells of that bucket get two workgroups' flushes
    shared = [g for g in range(N_WG - 1) if wins[g][1] == wins[g + 1][0]]
    assert len(shared) >= N_WG // 2 and s - 1 in shared and s in shared
    # ... and the larger maximum of a cell sits in the later workgroup for some cells, in the earlier for others
    g = 0
    assert wins[g] == wins[g + 1]
    a, b = slice(g * SHARE, (g + 1) * SHARE), slice((g + 1) * SHARE, (g + 2) * SHARE)
    first = np.zeros(300, dtype=np.int64)
    second = np.zeros(300, dtype=np.int64)
    np.maximum.at(first, L.cols["k2"][a], L.cols["a4"][a])
    np.maximum.at(second, L.cols["k2"][b], L.cols["a4"][b])
    assert (first > second).sum() >= 5 and (second > first).sum() >= 5 and ((first > 0) & (second > 0)).sum() == WL.K2_VALUES.size
    _fits(L, wmax, CASE_QUERIES["spike"])


def test_budget_shape():
    W = WL.fit(300, 3)
    assert W == 21 and WL.window_bytes(W, 300, 3) <= WL.LDS_BUDGET < WL.window_bytes(W + 1, 300, 3)
    for w in (W, W + 1):
        L = WL.budget(N_WG, w)
        wins, wmax, inside = WL.layout_windows(L, N_WG)
        assert inside and wmax == w and sorted(x[1] - x[0] + 1 for x in wins)[-2] == 1
        assert (np.diff(L.cols["t"]) >= 0).all()
        # one row in each bucket between the first and the last
        got = np.unique(L.cols["t"][N_WG // 2 * SHARE:(N_WG // 2 + 1) * SHARE] // TB, return_counts=True)
        assert got[0].size == w and got[1][0] == 1 and got[1][1] == 2 and (got[1][2:-1] == 1).all()


def test_straddle_shape():
    L = _layout("straddle")
    assert L.n % UNIT != 0 and all(b == 12288 for b in L.blocks[:-1]) and 0 < L.blocks[-1] < 12288
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    sh = WL.shares(L.blocks, N_WG)
    assert inside and wmax == 3 and all(len(s) == 1 for s in sh)
    t = L.cols["t"]
    wider = 0
    for g, (((r0, rn),), win) in enumerate(zip(sh, wins)):
        mine = np.unique(t[r0:r0 + rn] // TB)             # (blocks of 12288 rows touch: physical rows are logical rows)
        assert win[0] <= mine.min() and mine.max() <= win[1]
        wider += mine.size < win[1] - win[0] + 1
    assert wider >= N_WG // 2       # windows with buckets the workgroup has no row in
    assert sh[-1][0][1] == SHARE + 777
    _fits(L, wmax, CASE_QUERIES["straddle"])


def test_small_blocks_shape():
    L = _layout("small_blocks")
    sh = WL.shares(L.blocks, N_WG)
    assert all(len(s) in (8, 9) and all(n == 1000 for _, n in s) for s in sh) and sum(len(s) for s in sh) == len(L.blocks)
    assert any(r0 % UNIT for s in sh for r0, _ in s)
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    assert inside and 2 <= wmax <= 3
    _fits(L, wmax, WL.FIRST_TWO)


def test_idle_shape():
    L = _layout("idle")
    assert L.n == 5 * UNIT + 7
    sh = WL.shares(L.blocks, N_WG)
    assert sum(1 for s in sh if s) == 6 and sum(n for s in sh for _, n in s) == L.n
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    assert inside and wmax == 2 and [w is None for w in wins] == [not s for s in sh]
    _fits(L, wmax, WL.FIRST_TWO)


def test_nullable_shape():
    L = _layout("nullable")
    mn, mx, cnt = WL.block_extrema(L.blocks, L.cols["t"], L.pop["t"])
    a, b = N_WG // 3, 2 * N_WG // 3
    empty = [j for j, c in enumerate(cnt) if c == 0]
    assert empty == [4 * a + 1] + [4 * b + j for j in range(4)]
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    assert inside and wmax == 1 and [g for g, w in enumerate(wins) if w is None] == [b] and wins[a] == (T0 // TB + a,) * 2
    assert 0.05 < 1 - L.pop["t"].mean() < 0.2 and 0.1 < 1 - L.pop["kn"].mean() < 0.2
    _fits(L, wmax, CASE_QUERIES["nullable"])


def test_signed_shape():
    L = _layout("signed")
    t = L.cols["t"]
    assert (int(t.min()), int(t.max())) == (-3 * TB - 1, 3 * TB + 1)
    assert np.isin(np.array(WL.SIGNED_PLACED), t).all()
    tb = WL.time_buckets(t, TB)
    assert sorted(np.unique(tb).tolist()) == [-3 * TB, -2 * TB, -TB, 0, TB, 2 * TB, 3 * TB]
    assert (tb == 0).sum() > 1.9 * (tb == TB).sum()            # bucket 0: (-TB, TB), twice as wide as any other
    assert set(tb[t == -TB + 1].tolist()) == {0} and set(tb[t == -TB].tolist()) == {-TB} and set(tb[t == -TB - 1].tolist()) == {-TB}
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    assert inside and wmax <= 3
    _fits(L, wmax, WL.FIRST_TWO)


def test_skips_shape():
    L = _layout("skips")
    scanned = WL.skips_scanned(L, [("s", "gt", 0)])
    nb = len(L.blocks)
    assert [j for j, k in enumerate(scanned) if not k] == [j for j in range(nb // 4, nb // 2) if j % 2 == 1]
    sh = WL.shares(L.blocks, N_WG, scanned)
    assert any(len(s) > 1 and s[1][0] > s[0][0] + s[0][1] for s in sh)      # a share of segments that are not neighbours
    wins, wmax, inside = WL.layout_windows(L, N_WG, scanned)
    assert inside and wmax <= 3
    _fits(L, wmax, ["skip_s"])
    # a filter on the time column itself drops the blocks below it
    cut = T0 + (N_WG // 4) * TB - 1
    by_time = WL.skips_scanned(L, [("t", "gt", cut)])
    assert by_time == [j >= 2 * (N_WG // 4) for j in range(nb)]
    assert WL.layout_windows(L, N_WG, by_time)[1] <= 3


@pytest.mark.parametrize("case,n_tb", [("wide_below", 65535), ("wide_at", 65536)])
def test_wide_declared_shape(case, n_tb):
    L = _layout(case)
    cells = WL.cells_of(WL.QUERIES["wide"])
    assert cells == 256 and n_tb * cells == WL.PACKED_CELL_LIMIT - (cells if case == "wide_below" else 0)
    assert (L.t_bounds[1] + 1 - L.t_bounds[0]) // TB == n_tb and int(L.cols["t"].max()) == L.t_bounds[1]
    wins, wmax, inside = WL.layout_windows(L, N_WG)
    first = T0 // TB + n_tb - 3
    assert inside and wmax == 1 and sorted(set(w for w in wins if w)) == [(first + j, first + j) for j in range(3)]
    assert (first - T0 // TB) * cells >= (1 << 24) - 4 * cells                # wg_cell_base: next to the top of the table
    _fits(L, wmax, ["wide"])


# ---------------------------------------------------------------------------------------------- reference() against the oracle
def oracle_answer(oracle, L, q):
    names = list(WL.COLUMN_ORDER)
    ocols = [dict({"type": "int", "data": L.cols[c]}, **({"populated": L.pop[c]} if c in L.pop else {})) for c in names]
    return oracle.run_query(ocols, block_rows=L.block_rows, n_threads=16, want_values=bool(q.get("want_percentiles")),
                            **parity.oracle_query_kwargs(names, WL.INFO, q))


def _signed64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def check_reference(ref, ores, q):
    """reference() and an oracle answer agree on matched, the set of (time bucket, key) rows, counts, samples, sums, extrema
    (BasicHist.Min / Max start at 0 in avg mode, at Info.Min / Info.Max in hist mode: hist_basic.go:34-40) and bucket arrays."""
    assert ref["matched"] == ores["matched"]
    omap = {(r["time_bucket"],) + tuple(_signed64(v) for v in r["key_vals"]): r for r in ores["time_results"]}
    assert len(omap) == len(ores["time_results"]) and set(omap) == set(ref["groups"])
    for key, (count, samples, aggs) in ref["groups"].items():
        o = omap[key]
        assert (o["count"], o["samples"]) == (count, samples), key
        for name, (total, lo, hi, buckets), h in zip(q["aggs"], aggs, o["hists"]):
            start = WL.INFO[name] if q["op"] == "hist" else (0, 0)
            assert h["present"] and (h["count"], h["sum_exact"]) == (count, total), (key, name)
            assert (h["min"], h["max"]) == (min(lo, start[0]), max(hi, start[1])), (key, name)
            if buckets is not None:
                v = h["values"]
                assert v.size >= buckets.size and np.array_equal(v[:buckets.size], buckets) and not v[buckets.size:].any(), (key, name)


def bucket_sizes(ores, q):
    return [ores["time_results"][0]["hists"][a]["bucket_size"] for a in range(len(q["aggs"]))] if q["op"] == "hist" else None


@pytest.mark.parametrize("case", list(CASES))
def test_reference_against_the_oracle(oracle, case):
    L = _layout(case)
    queries = {k: WL.QUERIES[k] for k in list(MATRIX) + [k for k in CASE_QUERIES.get(case, ()) if k not in MATRIX]}
    if case == "skips":
        queries["skip_t"] = WL._q(filters=[("t", "gt", T0 + (N_WG // 4) * TB - 1)], groups=["k2"], aggs=["a4"], block_skip=True)
    for k, q in queries.items():
        ores = oracle_answer(oracle, L, q)
        ref = WL.reference(L, q, bucket_sizes(ores, q))
        assert len(ref["groups"]) > 1 and ref["matched"] > 0, k
        check_reference(ref, ores, q)
        if q.get("block_skip"):
            assert ores["blocks_skipped"] == WL.skips_scanned(L, q["filters"]).count(False) > 0


def test_reference_against_a_row_loop():
    L = WL.nullable(16)
    q = WL._q(filters=WL.F_RANGE, groups=["k3", "kn"], aggs=["sg"], weight_col="w")
    ref = WL.reference(L, q)
    want, matched = {}, 0
    c = L.cols
    for i in range(0, L.n):
        if not 99 < c["f1"][i] < 900:
            continue
        matched += 1
        if not L.pop["t"][i]:
            continue
        key = (WL.trunc_div(int(c["t"][i]), TB) * TB, int(c["k3"][i]), int(c["kn"][i]) if L.pop["kn"][i] else WL.MISSING)
        g = want.setdefault(key, [0, 0, 0, None, None])
        v, w = int(c["sg"][i]), int(c["w"][i])
        g[0], g[1], g[2] = g[0] + w, g[1] + 1, g[2] + v * w
        g[3], g[4] = v if g[3] is None else min(g[3], v), v if g[4] is None else max(g[4], v)
    assert ref["matched"] == matched and any(k[2] == WL.MISSING for k in want)
    assert ref["groups"] == {k: (g[0], g[1], ((g[2], g[3], g[4], None),)) for k, g in want.items()}


def test_a_row_in_the_neighbouring_bucket_is_visible():
    """The mistake the GPU file exists for: a row of the window's first or last bucket accumulated one bucket off."""
    L = _layout("spike")
    q = WL.QUERIES["avg"]
    good = WL.reference(L, q)
    s = N_WG // 2 * SHARE
    for row in (s, s + 1):
        moved = WL.Layout.__new__(WL.Layout)
        moved.__dict__.update(L.__dict__)
        moved.cols = dict(L.cols, t=L.cols["t"].copy())
        moved.cols["t"][row] += TB if row == s else -TB
        assert WL.reference(moved, q)["groups"] != good["groups"]
