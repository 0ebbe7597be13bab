"""CPU: the claims tests/outlog_cases.py makes about its tables (through the oracle) and about one wave's appends to the
outlier log (the model against itself, and the planner's rounding of the capacity restated)."""
import itertools

import numpy as np
import pytest

from tests import outlog_cases as OC

PERS = (1, 2, 4)
WAVE_NS = sorted({n for per in PERS for n in OC.wave_ns(per)})


@pytest.fixture(scope="module")
def many():
    return OC.many_waves()


def _check_table(orc, case, time=False):
    """The oracle finds exactly the outliers the case claims: in all, per group (and time bucket), value for value."""
    claim = OC.claimed_outliers(case, time)
    assert sum(len(v) for v in claim.values()) == case.n_outliers == case.outlier_rows.size
    v = case.cols["v"]
    mask = np.zeros(case.n, dtype=bool)
    mask[case.outlier_rows] = True
    assert (v[mask] >= OC.FIRST_OUTLIER).all() and (v[mask] <= OC.INFO[1]).all() and np.unique(v[mask]).size == case.n_outliers
    assert ((v[~mask] >= 0) & (v[~mask] < OC.IN_RANGE)).all() and OC.IN_RANGE <= OC.FIRST_OUTLIER
    assert sum(case.blocks) == case.n and all(b == case.block for b in case.blocks[:-1])
    ores = OC.oracle_result(orc, case, time)
    assert ores["matched"] == case.n
    got = {}
    for r in ores["time_results" if time else "results"]:
        h = r["hists"][0]
        assert h["n_underliers"] == 0
        assert h["n_outliers"] == len(h["outlier_values"])
        if h["n_outliers"]:
            got[(r["time_bucket"] if time else 0, r["key_vals"][0])] = sorted(h["outlier_values"].tolist())
    assert got == claim
    return ores


@pytest.mark.parametrize("n", WAVE_NS)
def test_one_wave_tables_hold_their_outliers_in_the_first_64_rows(oracle, n):
    case = OC.one_wave(n)
    assert case.n == OC.ONE_WAVE_BLOCK * OC.ONE_WAVE_BLOCKS and case.blocks == [OC.ONE_WAVE_BLOCK] * OC.ONE_WAVE_BLOCKS
    assert case.n_outliers == n and (case.outlier_rows < 64).all() and np.unique(case.outlier_rows).size == n
    assert sorted(case.outlier_rows.tolist()) == sorted(OC.WAVE_ROWS[:n])
    _check_table(oracle, case)
    # the outliers of a wave go to several groups as soon as there are several
    assert len(OC.claimed_outliers(case)) >= (3 if n >= 8 else 1)


def test_the_first_value_beyond_the_buckets(oracle):
    """FIRST_OUTLIER is the first outlier and FIRST_OUTLIER - 1 the last value of the last bucket (hist_basic.go:130-135)."""
    case = OC.one_wave(0)
    assert case.n_outliers == 0
    case.cols["v"][5] = OC.FIRST_OUTLIER - 1
    case.cols["v"][6] = OC.FIRST_OUTLIER
    ores = OC.oracle_result(oracle, case)
    outs = [x for r in ores["results"] for x in r["hists"][0]["outlier_values"].tolist()]
    assert outs == [OC.FIRST_OUTLIER]


def test_many_waves_table(oracle, many):
    assert many.n == OC.MANY_ROWS <= 300_000 and len(many.blocks) == OC.MANY_ROWS // OC.MANY_BLOCK
    assert 0.018 < many.n_outliers / many.n < 0.022
    _check_table(oracle, many)
    claim = OC.claimed_outliers(many)
    assert sorted(g for _, g in claim) == list(range(OC.GROUPS))
    # every block holds outliers, and many waves of it: 64-row stretches with at least one
    r0 = 0
    for b in many.blocks:
        rows = many.outlier_rows[(many.outlier_rows >= r0) & (many.outlier_rows < r0 + b)]
        assert np.unique(rows // 64).size > 100
        r0 += b


@pytest.mark.parametrize("n", [OC.SPILL * 1, OC.SPILL * 4])
def test_time_wave_tables(oracle, n):
    case = OC.time_wave(n)
    assert (case.outlier_rows < 64).all()
    _check_table(oracle, case, time=True)
    claim = OC.claimed_outliers(case, time=True)
    # two time buckets of the same group (at 32 outliers: of both groups)
    both = [g for g in (1, 3) if {tb for tb, gg in claim if gg == g} == {OC.T0, OC.T0 + OC.TB}]
    assert both if n < 32 else both == [1, 3]
    assert {gg for _, gg in claim} == {1, 3}
    assert set(np.unique(case.cols["t"] // OC.TB * OC.TB).tolist()) == {OC.T0, OC.T0 + OC.TB}


@pytest.mark.parametrize("per", PERS)
def test_one_wave_keeps_everything_up_to_eight_stripes(per):
    for n in range(0, OC.SPILL * per + 1):
        assert OC.one_wave_outcome(n, per) == (n, 0), n
    placed, dropped = OC.one_wave_outcome(OC.SPILL * per + 1, per)
    assert placed == OC.SPILL * per and dropped == 1
    assert OC.one_wave_outcome(64, per) == (OC.SPILL * per, 64 - OC.SPILL * per)
    # the home stripe wraps round the 64
    for home in (0, 57, 63):
        assert OC.one_wave_outcome(OC.SPILL * per, per, home) == (OC.SPILL * per, 0)
        assert OC.one_wave_outcome(OC.SPILL * per + 1, per, home)[1] == 1


@pytest.mark.parametrize("per", PERS)
def test_replay_agrees_with_the_model_however_the_lanes_meet(per):
    """log_outlier restated with its cursors gives the model's answer for every kernel's row mapping, for lanes that arrive one
    by one and for all of them at once -- and says what the exact fit exercises: a reservation that straddles a stripe's end,
    cursors beyond their share, a gather whose sum is right only with the clamp."""
    for n in OC.wave_ns(per):
        rows = OC.WAVE_ROWS[:n]
        want_placed, want_dropped = OC.one_wave_outcome(n, per)
        for calls in (OC.calls_of(rows, 2), OC.calls_of(rows, 4), [1] * n, [n]):
            assert sum(calls) == n
            for home in (0, 60):
                r = OC.replay(calls, per, home)
                assert r["placed"] == want_placed and bool(r["flag"]) == (want_dropped > 0), (n, calls)
                assert r["kept"] == want_placed
                assert r["header"] == (want_placed if not want_dropped else OC.STRIPES * per + 1)
    for rows_per_lane in (2, 4):
        full = OC.replay(OC.calls_of(OC.WAVE_ROWS[:OC.SPILL * per], rows_per_lane), per)
        assert full["straddles"] >= 1 and full["overrun"] >= 1 and full["unclamped"] > full["kept"] == OC.SPILL * per
        assert sorted(full["cursor"], reverse=True)[OC.SPILL - 1] >= per and sorted(full["cursor"], reverse=True)[OC.SPILL] == 0
        spill = OC.replay(OC.calls_of(OC.WAVE_ROWS[:per + 1], rows_per_lane), per)
        assert spill["placed"] == per + 1 and sum(1 for c in spill["cursor"] if c) == 2
        home = OC.replay(OC.calls_of(OC.WAVE_ROWS[:per], rows_per_lane), per)
        assert home["placed"] == per and sum(1 for c in home["cursor"] if c) == 1 and home["overrun"] == 0


def test_calls_of():
    assert OC.calls_of([0, 2, 4, 5, 63], 2) == [3, 2]
    assert OC.calls_of([0, 2, 4, 5, 63], 4) == [2, 1, 1, 1]
    assert OC.calls_of([], 2) == []
    assert sorted(OC.WAVE_ROWS) == list(range(64))
    # every call of the exact-fit tables is made by several lanes, under both mappings
    for per in (1, 4):
        for rows_per_lane in (2, 4):
            assert max(OC.calls_of(OC.WAVE_ROWS[:OC.SPILL * per], rows_per_lane)) >= 2


def test_rounded_capacity():
    assert [OC.rounded_cap(c) for c in (-5, 0, 1, 16, 63, 64, 65, 193, 256, 257)] == [64, 64, 64, 64, 64, 64, 128, 256, 256, 320]
    assert [OC.per_of(c) for c in (1, 64, 193, 256, 1 << 20)] == [1, 1, 4, 4, 1 << 14]
    for c, k in itertools.product((1, 100, 4000), (1, 2, 8, 64)):
        cap = OC.rounded_cap(c * k)
        assert cap % OC.STRIPES == 0 and cap >= c * k and cap - c * k < OC.STRIPES
    assert OC.rounded_cap(OC.DEFAULT_CAP) == OC.DEFAULT_CAP
