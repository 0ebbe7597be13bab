"""CPU: the claims tests/late_layout.py makes about its tables, from the arrays (no GPU, no library)."""
import collections

import numpy as np
import pytest

from tests import late_layout as LL

N_WGS = (16, 256, 304)


@pytest.fixture(scope="module", params=N_WGS)
def main(request):
    return request.param, LL.main(request.param)


def test_main_is_four_whole_tiles_of_one_block_per_workgroup(main):
    n_wg, m = main
    assert m.n == n_wg * LL.SHARE and m.n % (n_wg * LL.UNIT) == 0
    assert all(b == LL.BLOCK for b in m.blocks[:-1]) and 0 < m.blocks[-1] <= LL.BLOCK and m.blocks[-1] % LL.SHARE == 0
    assert LL.SHARE == 4 * LL.TILE and LL.TILE == 16 * LL.WINDOW and LL.WINDOW == 64 * LL.LANE_ROWS and LL.TILE == 2 * LL.UNIT


def test_every_workgroup_runs_all_sixteen_sequences_and_they_rotate(main):
    n_wg, m = main
    needed = m.passing.reshape(n_wg, 4, LL.WAVES, LL.WINDOW).any(axis=3)          # [g, it, w]
    seq = sum(needed[:, it, :].astype(np.int64) << it for it in range(4))          # [g, w]
    for g in range(n_wg):
        assert sorted(seq[g].tolist()) == list(range(16)), g
        assert seq[g].tolist() == [(w + g) % 16 for w in range(16)], g
    # never passing and always passing, in every workgroup; and from one workgroup to the next every wave changes its sequence
    assert (seq == 0).sum(axis=1).tolist() == [1] * n_wg and (seq == 15).sum(axis=1).tolist() == [1] * n_wg
    assert (seq[1:] != seq[:-1]).all()
    # a wave that skips tile t and needs t + 1 beside one that does the opposite, in every workgroup and at every t
    for it in range(3):
        a = ~needed[:, it, :] & needed[:, it + 1, :]
        b = needed[:, it, :] & ~needed[:, it + 1, :]
        assert a.any(axis=1).all() and b.any(axis=1).all()
    # skips at the first and at the last tile of a share, beside fifteen / eight waves that pass there
    assert (~needed[:, 0, :]).any(axis=1).all() and (~needed[:, 3, :]).any(axis=1).all()
    assert (needed.sum(axis=2) == 8).all()


def test_every_position_class_occurs_at_every_tile(main):
    n_wg, m = main
    win = m.passing.reshape(n_wg, 4, LL.WAVES, LL.WINDOW)
    seen = collections.Counter()
    by_rows = {(tuple(range(LL.WINDOW)) if pos is None else tuple(pos)): name for name, pos in LL.POSITIONS.items()}
    for g in range(n_wg):
        for it in range(4):
            for w in range(LL.WAVES):
                rows = tuple(np.flatnonzero(win[g, it, w]).tolist())
                if rows:
                    assert rows in by_rows, (g, it, w, rows[:8])
                    seen[(by_rows[rows], it)] += 1
    assert set(seen) == {(name, it) for name in LL.CLASSES for it in range(4)}
    # what the classes are: the first and the last row of a window, row 3 of a lane, two lanes, every lane
    P = LL.POSITIONS
    assert P["row0"] == (0,) and P["row255"] == (LL.WINDOW - 1,) and P["k3"][0] % LL.LANE_ROWS == 3
    assert P["two_lanes"][0] // LL.LANE_ROWS != P["two_lanes"][1] // LL.LANE_ROWS and P["all"] is None


def _windows_of(layout):
    """[(first row, rows)] of every wave window, counted from the start of each block."""
    out, r0 = [], 0
    for b in layout.blocks:
        out += [(r0 + o, min(LL.WINDOW, b - o)) for o in range(0, b, LL.WINDOW)]
        r0 += b
    return out


def _check_columns(layout, check_widths):
    c, p = layout.cols, layout.passing
    assert set(c) == set(LL.COLUMN_ORDER) and all(a.dtype == np.int64 and a.size == layout.n for a in c.values())
    # every filter width reproduces the pattern, and so does the conjunction -- of which neither half does
    for name, f in LL.FILTERS.items():
        assert np.array_equal(LL.keep(c, f), p), name
    assert np.array_equal(LL.keep(c, LL.ALL3), p) and np.array_equal(LL.keep(c, LL.WORD3), p)
    assert not LL.keep(c, LL.NOTHING).any() and LL.keep(c, LL.EVERYTHING).all()
    if layout.n > 1:
        for half in LL.FILTERS["and"]:
            alone = LL.keep(c, [half])
            assert not np.array_equal(alone, p)
            for r0, rows in _windows_of(layout):
                if rows >= 2:
                    assert alone[r0:r0 + rows].any(), (half, r0)
    # passing rows: inside every declared range; failing rows: inside the key ranges but for gx, and never a zero value
    for g, (lo, hi) in LL.DECLARED.items():
        inside = (c[g] >= lo) & (c[g] <= hi)
        assert inside[p].all(), g
        assert inside[~p].all() if g != "gx" else not inside[~p].any(), g
    assert (c["gx"][~p] == LL.GX_LEAK).all() and 0 <= LL.GX_LEAK - LL.DECLARED["gx"][0] < 256
    for a, (lo, hi) in LL.INFO.items():
        assert ((c[a] >= lo) & (c[a] <= hi) & (c[a] != 0)).all(), a
    assert (np.diff(c["t"]) >= 0).all() and c["t"].min() >= LL.T0 and c["t"].max() < LL.T0 + LL.N_TB * LL.TB
    if check_widths:
        for name, nbytes in LL.STORED_BYTES.items():
            span = int(c[name].max()) - int(c[name].min())
            assert {1: span < 256, 2: 256 <= span < 65536, 4: 65536 <= span < 1 << 32}[nbytes], (name, span)
        assert int(c["a2"].min()) < 0 < int(c["a2"].max())
        assert len(np.unique(c["t"] // LL.TB)) == LL.N_TB
        for g, (lo, hi) in LL.DECLARED.items():
            if g != "gx":
                assert (int(c[g].min()), int(c[g].max())) == (lo, hi), g


def test_main_columns(main):
    _check_columns(main[1], check_widths=True)


def test_a_leaked_row_is_visible():
    """The verdict of tile t + 1 applied to the rows of tile t (the hand-over the kernels could get wrong) changes the
    reference: as an overflow through gx, as a wrong count and sum in every group without it.  (One size: the property is the
    columns', which test_main_columns checks at every size.)"""
    m = LL.main(16)
    q = dict(filters=LL.FILTERS["f1"], groups=["ga", "gx"], aggs=["a1", "a2"])
    ref = LL.reference(m.cols, q)
    assert ref["overflow"] == 0 and ref["matched"] == int(m.passing.sum()) and len(ref["groups"]) == 8
    shifted = dict(m.cols, f1=np.roll(m.cols["f1"], -LL.TILE))
    bad = LL.reference(shifted, q)
    assert bad["overflow"] > 0 and bad["groups"] != ref["groups"]
    # without gx the same mistake is a wrong count and sum in every group
    q2 = dict(q, groups=["ga"])
    good2, bad2 = LL.reference(m.cols, q2), LL.reference(shifted, q2)
    assert bad2["overflow"] == 0 and all(bad2["groups"][k] != v for k, v in good2["groups"].items())
    # a query every row passes: the failing rows ARE the overflow
    assert LL.reference(m.cols, dict(q, filters=LL.EVERYTHING))["overflow"] == int((~m.passing).sum())


@pytest.mark.parametrize("n_wg", N_WGS)
def test_ragged(n_wg):
    r = LL.ragged(n_wg)
    k = len(LL.RAGGED_BLOCKS)
    assert len(r.blocks) % k == 0 and all(tuple(r.blocks[j:j + k]) == LL.RAGGED_BLOCKS for j in range(0, len(r.blocks), k))
    units = sum((b + LL.UNIT - 1) // LL.UNIT for b in r.blocks)
    assert units >= 2 * n_wg > units - sum((b + LL.UNIT - 1) // LL.UNIT for b in LL.RAGGED_BLOCKS)
    assert LL.RAGGED_BLOCKS == (65536, 12293, 1, 2303, 40961, 4095, 4097)
    r0 = 0
    for b in r.blocks:
        assert r.passing[r0] and r.passing[r0 + b - 1] and r.passing[max(r0, r0 + b - 2)]
        r0 += b
    inner = r.passing.sum() - sum(min(b, 3) for b in r.blocks)
    assert 0.001 < inner / r.n < 0.003
    wins = _windows_of(r)
    skipped = sum(1 for w0, rows in wins if not r.passing[w0:w0 + rows].any())
    assert skipped > len(wins) // 2
    # partial windows (needed, every one: a block's last two rows pass), partial tiles, and a tile's worth of look-ahead past n
    assert any(rows < LL.WINDOW for _, rows in wins) and any(b % LL.TILE for b in r.blocks) and any(b < LL.TILE for b in r.blocks)
    _check_columns(r, check_widths=False)


@pytest.mark.parametrize("rows", LL.TINY_ROWS)
def test_tiny(rows):
    t = LL.tiny(rows)
    assert t.blocks == [rows] and t.n == rows and np.flatnonzero(t.passing).tolist() == [rows - 1]
    _check_columns(t, check_widths=False)


def test_reference_against_a_row_loop():
    t = LL.ragged(16)
    c = {k: v[:20_000] for k, v in t.cols.items()}
    q = dict(filters=[("f1", "gt", 99)], groups=["gb", "gx"], aggs=["a2", "a4"], time_col="t", time_bucket=LL.TB)
    ref = LL.reference(c, q)
    want, matched, overflow = {}, 0, 0
    for i in range(20_000):
        if not c["f1"][i] > 99:
            continue
        matched += 1
        if not 0 <= c["gx"][i] <= 1:
            overflow += 1
            continue
        key = (int(c["t"][i]) // LL.TB * LL.TB, int(c["gb"][i]), int(c["gx"][i]))
        cnt, aggs = want.get(key, (0, [[0, None, None], [0, None, None]]))
        for a, name in zip(aggs, q["aggs"]):
            v = int(c[name][i])
            a[0], a[1], a[2] = a[0] + v, v if a[1] is None else min(a[1], v), v if a[2] is None else max(a[2], v)
        want[key] = (cnt + 1, aggs)
    assert (ref["matched"], ref["overflow"]) == (matched, overflow) and overflow > 0 and len(want) > 1
    assert ref["groups"] == {k: (cnt, tuple(tuple(a) for a in aggs)) for k, (cnt, aggs) in want.items()}
    none = LL.reference(c, dict(q, filters=LL.NOTHING))
    assert none == {"matched": 0, "overflow": 0, "groups": {}}
