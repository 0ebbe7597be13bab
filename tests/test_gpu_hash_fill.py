"""GPU: hash group-by (strategy 7) at the fill levels where its two table levels hand over.

Every hashed row goes through a per-workgroup LDS staging table of L slots (planner.cpp: window() sizes L from kLdsBudgetBytes and
the words of one slot; filled to 3/4 L, at most kHashLdsProbes probes) and, when it finds no room there, straight into the global
open-addressing table in HBM, where the flush of every staging table lands too (hash_table.h: hash_find_or_insert, probe bound
min(slots, kHashMaxProbes)).  A key is then partly staged and partly direct, in one workgroup and across them, and the adds and
maxes of both routes have to meet in one slot.  tests/test_gpu_hash.py stages every row or almost none; this file pins the levels
in between, for each of the three row bodies (k_scan_hash_packed, k_scan_hash_fast, k_scan_hash):

A. the staging table, swept across L: K = L/2, 3L/4, L, 3L/2, 2L live keys per workgroup, for count-only, avg with tracked
   minima and maxima, moments with outliers, missing keys and values (NUL), a range filter (packed: the plain and the LATE
   instantiation), a time series and two group columns.
B. the global table at 4095, 4096 and 4097 keys in 4096 slots and at 90 % of 8192, through the flush and without staging;
   once with the 4096th key arriving last and needing every one of its 4096 probes.

Both boundaries are per WORKGROUP and the planner launches one workgroup per CU, so the tables are sized from the workgroup count
of the device under test: n_workgroups shares of S contiguous rows, key columns cyclic (key[i] = values[i mod K]), so every window of
S >= 2K rows holds each of the K keys at least twice however the rows are dealt, and for K > L no staging table can hold a
workgroup's keys.  L is read from the planner's `hash tables:` trace line (SYBL_PLAN_TRACE=1) and every K is asserted against it:
a change of the LDS budget moves the cases or fails them, it cannot silently take them off the boundary.  The layout only PLACES
rows where the paths must run; every expected value is a numpy int64 group-by over the whole column (tests/hash_fill_ref.py) or
the CPU oracle's, and holds whatever the split is.

Not covered: the multi-rank union, -loghist through the table, tables above 4096 slots beyond 90 % load (early "full" verdicts
there are documented behaviour), lazy rows (tests/test_gpu_hash.py).
"""
import contextlib
import re

import numpy as np
import pytest

import sybil_amd
from tests import hash_fill_ref as H
from tests import parity

pytestmark = pytest.mark.gpu

BLOCK = 65536
S_MIN = 16384                    # rows of one workgroup's share (more where a shape's 2L keys need it)
T0, TB, N_TB = 1_700_000_000 - 1_700_000_000 % 3600, 3600, 6
# v and w: declared bounds that hold the data (the bucket geometry alone makes the top 10 % of the range outliers);
# u: data up to 69 999 beyond the declared 49 999 -- outliers AND a tracked maximum, which the packed body does not keep in hist mode
V_INFO, U_INFO, W_INFO = (-5000, 4999), (0, 49_999), (0, 9999)
TRACE = re.compile(r"hash tables: slots=(\d+) staging=(\d+) words_per_slot=(\d+) kernel=(\w+) late=(\d)")
KERNELS = {"packed": {}, "fast": {"SYBL_NO_HASH_PACKED": "1"}, "generic": {"SYBL_NO_HASH_FAST": "1"}}
LEVELS = {"L/2": (1, 2), "3L/4": (3, 4), "L": (1, 1), "3L/2": (3, 2), "2L": (2, 1)}
SWEEP5, SWEEP3 = ("L/2", "3L/4", "L", "3L/2", "2L"), ("L/2", "L", "2L")
MAX_PROBES = 4096                # hash_table.h: kHashMaxProbes


def _q(**kw):
    return dict(dict(op="avg", want_percentiles=False, order_by=None), **kw)      # (order_by None: canonical key order)


# shape -> (table, key columns of one K, query over them, levels, reference)
SHAPES = {
    "count": ("count", lambda k: ["k%d" % k], lambda kc: _q(groups=kc, aggs=[]), SWEEP3, "numpy"),
    "avg": ("main", lambda k: ["k%d" % k], lambda kc: _q(groups=kc, aggs=["v"]), SWEEP5, "numpy"),
    "moments": ("main", lambda k: ["k%d" % k], lambda kc: _q(groups=kc, aggs=["v", "u"], op="hist"), SWEEP5, "oracle"),
    "moments_in": ("main", lambda k: ["k%d" % k], lambda kc: _q(groups=kc, aggs=["v", "w"], op="hist"), SWEEP5, "oracle"),
    "nul": ("main", lambda k: ["kn%d" % k], lambda kc: _q(groups=kc, aggs=["vn"]), SWEEP3, "oracle"),
    "filter": ("main", lambda k: ["k%d" % k], lambda kc: _q(filters=[("f", "gt", 49)], groups=kc, aggs=["v"]), SWEEP3, "numpy"),
    "time": ("main", lambda k: ["k%d" % k], lambda kc: _q(groups=kc, aggs=["v"], time_col="t", time_bucket=TB), SWEEP3, "oracle"),
    "two": ("main", lambda k: ["a%d" % k, "b%d" % k], lambda kc: _q(groups=kc, aggs=["v"]), SWEEP3, "numpy"),
}
CASES = [(shape, level) for shape, spec in SHAPES.items() for level in spec[3]]
# The row body the planner takes where it is not the one asked for.  `moments` is the shape with declared bounds narrower than
# the data: in hist mode a maximum above Info.Max is tracked by the GEN body only (planner.cpp: fill_fast_columns, "h.Max
# lives in the GEN body"), so the compact table runs k_scan_hash_fast too; `moments_in` is the same query with the outliers
# inside the declared bounds, which k_scan_hash_packed takes.
TAKEN = {("moments", "packed"): "fast"}


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _env(monkeypatch, **kv):
    with monkeypatch.context() as m:
        for k, v in kv.items():
            m.setenv(k, v)
        yield


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _value_columns(n, guard):
    """The columns every K shares, a function of the row count alone (the first rows carry the extremes, so a short table plans
    like the long one).  Rows of the even `guard`-row blocks always pass the filter and always have a key; the other blocks
    lose about 4 rows in 5 to the filter and 1 key in 4: a window of 3 guard blocks holds a whole even one."""
    rng = np.random.default_rng(4242)
    i = np.arange(n, dtype=np.int64)
    even = (i // guard) % 2 == 0
    c = {}
    c["v"] = rng.integers(-5000, 5000, n)
    c["v"][:2] = V_INFO
    c["u"] = rng.integers(0, 70_000, n)
    c["u"][:2] = 0, 69_999
    c["w"] = rng.integers(0, 10_000, n)
    c["w"][:2] = W_INFO
    c["vn"] = rng.integers(-5000, 5000, n)
    c["vn"][:2] = V_INFO
    c["f"] = np.where(even, rng.integers(50, 100, n), rng.integers(0, 63, n))
    c["t"] = T0 + i * (N_TB * TB) // n
    pops = {"vn": (rng.random(n) > 0.2).astype(np.uint8), "key": (even | (rng.random(n) > 0.25)).astype(np.uint8)}
    pops["vn"][:2] = 1
    return c, pops


def _key_columns(shape_keys, n):
    """{column: values} of the key columns the shapes need: {(kind, K)} with kind k (one column), kn (the same, rows without a
    key: _value_columns' mask) or ab (two columns whose K live combinations are the K values' high and low bytes)."""
    out = {}
    for kind, k in sorted(shape_keys):
        vals = H.key_values(k, seed=k)
        col = H.cyclic_column(vals, n)
        if kind == "ab":
            out["a%d" % k], out["b%d" % k] = (col >> 8) - 7, col & 255
        else:
            out["%s%d" % (kind, k)] = col
    return out


def _build(ctx, name, n, cols, pops, info):
    tb = ctx.create_table(name)
    for c in cols:
        tb.add_column(c, "int", *info.get(c, (1, 0)))
    for r0 in range(0, n, BLOCK):
        r1 = min(r0 + BLOCK, n)
        tb.append_block(r1 - r0, {c: ((a[r0:r1], pops[c][r0:r1]) if c in pops else a[r0:r1]) for c, a in cols.items()})
    tb.compact()
    return tb


INFO = {"v": V_INFO, "u": U_INFO, "w": W_INFO, "vn": V_INFO}


def _pops_for(cols, pops):
    return {c: (pops["key"] if c.startswith("kn") else pops[c]) for c in cols if c.startswith("kn") or c in pops}


def _kinds(shape):
    return {"nul": "kn", "two": "ab"}.get(shape, "k")


def _traced(tb, q, capfd, monkeypatch, **env):
    """prepare + scan + finalize with the plan trace on: (result, stats, the one `hash tables:` line as a dict)."""
    with _env(monkeypatch, SYBL_FORCE_HASH="1", SYBL_PLAN_TRACE="1", **env):
        capfd.readouterr()
        qy = tb.query(**q)
        try:
            res = qy.run()
            st = qy.stats()
        finally:
            qy.free()
        lines = TRACE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    slots, staging, words, kernel, late = lines[0]
    return res, st, dict(slots=int(slots), staging=int(staging), words=int(words), kernel=kernel, late=int(late))


class _Fill:
    pass


def _c_stderr_of(fn):
    """What fn() makes the library write to the C stderr (a module-scoped fixture has no capfd)."""
    import os
    import tempfile
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode("utf-8", "replace")


@pytest.fixture(scope="module")
def fill(ctx):
    """L of every shape from a short table of the same columns, then the two tables: `main` and, for the count-only shape
    (two words a slot: the largest L, so the longest shares), `count`."""
    probe_n = 8192
    pc, pp = _value_columns(probe_n, 4096)
    pc.update(_key_columns({(k, 64) for k in ("k", "kn", "ab")}, probe_n))
    ptb = _build(ctx, "fillprobe", probe_n, pc, _pops_for(pc, pp), INFO)
    F = _Fill()
    F.L, F.words = {}, {}
    order = []

    def probe():
        for shape, (_, keys, query, _, _) in SHAPES.items():
            qy = ptb.query(**query(keys(64)))
            if shape == "count":
                qy.run().free()
                F.n_wg = qy.stats()["n_workgroups"]
            assert qy.stats()["strategy"] == 7, (shape, qy.stats())
            qy.free()
            order.append(shape)

    mp = pytest.MonkeyPatch()
    mp.setenv("SYBL_FORCE_HASH", "1")
    mp.setenv("SYBL_PLAN_TRACE", "1")
    try:
        lines = TRACE.findall(_c_stderr_of(probe))
    finally:
        mp.undo()
    ptb.free()
    assert len(lines) == len(order), lines
    for shape, (_, staging, words, _, _) in zip(order, lines):
        F.L[shape], F.words[shape] = int(staging), int(words)
        assert 64 <= F.L[shape] <= 16384 and F.L[shape] & (F.L[shape] - 1) == 0, (shape, lines)
    # (whole shares are laid out below; beyond 512 workgroups the tables are no longer a few seconds' work)
    assert 16 <= F.n_wg <= 512, "n_workgroups = %d: this file is sized for one workgroup per CU of a 16..512-CU device" % F.n_wg
    F.K = {(shape, level): F.L[shape] * LEVELS[level][0] // LEVELS[level][1] for shape, level in CASES}
    F.guard = max(F.K[c] for c in CASES if c[0] in ("nul", "filter"))
    F.S, F.n, F.cols, F.pops, F.tb = {}, {}, {}, {}, {}
    for table in ("main", "count"):
        mine = [c for c in CASES if SHAPES[c[0]][0] == table]
        S = max([S_MIN, 3 * F.guard if table == "main" else 0] + [2 * F.K[c] for c in mine])
        n = F.n_wg * S
        cols, pops = _value_columns(n, F.guard) if table == "main" else ({}, {})
        cols.update(_key_columns({(_kinds(c[0]), F.K[c]) for c in mine}, n))
        F.S[table], F.n[table], F.cols[table], F.pops[table] = S, n, cols, _pops_for(cols, pops)
        F.tb[table] = _build(ctx, "fill" + table, n, cols, F.pops[table], INFO)
    F.summary = "hash fill: n_wg=%d L=%s words_per_slot=%s S=%s rows=%s" % (F.n_wg, F.L, F.words, F.S, F.n)
    F.refs = {}
    yield F
    for tb in F.tb.values():
        tb.free()


# ---------------------------------------------------------------------------------------------- expected values
def _numpy_ref(F, shape, table, kc, q):
    cols = F.cols[table]
    if shape == "two":
        key = (cols[kc[0]] + 7) * 256 + cols[kc[1]]
    else:
        key = cols[kc[0]]
    keep = cols["f"] > 49 if q.get("filters") else None
    return H.group_ref(key, cols[q["aggs"][0]] if q["aggs"] else None, keep)


def _check_numpy(res, ref, shape, has_agg, what):
    """Every group that has a row and no other; Count, Sum, min and max exact, avg to parity.REL.  BasicHist.Min / Max start at
    0 in avg mode (hist_basic.go:34-40)."""
    rows = res.rows(0)
    if shape == "two":
        got = {(_signed(g["key_vals"][0]) + 7) * 256 + g["key_vals"][1]: g for g in rows}
    else:
        got = {g["key_vals"][0]: g for g in rows}
    assert len(got) == len(rows), what
    assert set(got) == set(ref), (what, len(got), len(ref), sorted(set(got) ^ set(ref))[:8])
    n_rows = sum(c for c, _, _, _ in ref.values())
    assert res.matched == n_rows, (what, res.matched, n_rows)
    bad = []
    for k, (count, total, lo, hi) in ref.items():
        g = got[k]
        if g["count"] != count:
            bad.append((k, "count", g["count"], count))
        if not has_agg:
            continue
        h = g["hists"][0]
        if not h["present"] or (h["count"], h["sum"]) != (count, total):
            bad.append((k, "sum", h["present"], h["count"], h["sum"], count, total))
        if (h["min"], h["max"]) != (min(lo, 0), max(hi, 0)):
            bad.append((k, "extrema", h["min"], h["max"], lo, hi))
        if abs(h["avg"] - total / count) > parity.REL * max(abs(total / count), 1.0):
            bad.append((k, "avg", h["avg"], total / count))
    assert not bad, (what, len(bad), bad[:6])
    c = res.cumulative
    assert c["count"] == n_rows, what
    if has_agg:
        grand = sum(t for _, t, _, _ in ref.values())
        assert abs(grand) < 1 << 63
        assert (c["hists"][0]["count"], c["hists"][0]["sum"]) == (n_rows, grand), what


def _oracle_ref(F, oracle, table, kc, q):
    cols, pops = F.cols[table], F.pops[table]
    names = list(kc) + [c for c in ("v", "u", "w", "vn", "f", "t") if c in q["aggs"] or c == q.get("time_col")]
    ocols = [{"type": "int", "data": cols[c], **({"populated": pops[c]} if c in pops else {})} for c in names]
    kw = parity.oracle_query_kwargs(names, INFO, q)
    return oracle.run_query(ocols, n_threads=16, want_values=False, **kw)


def _snapshot(res, time_mode):
    """Everything a result says, in the order it says it, floats bit for bit: what the three row bodies must agree on."""
    def row(r):
        return (r["key"], r["time_bucket"], r["count"], r["samples"],
                tuple(tuple((k, v.hex() if isinstance(v, float) else v) for k, v in h.items()) for h in r["hists"]))
    return [[row(r) for r in res.rows(w, want_values=False)] for w in ((0, 1, 2) if time_mode else (0, 2))]


# ---------------------------------------------------------------------------------------------- A. the staging table
@pytest.mark.parametrize("shape,level", CASES, ids=["%s-%s" % (s, lv.replace("/", "_")) for s, lv in CASES])
def test_staging_table_fill_levels(fill, oracle, capfd, monkeypatch, shape, level):
    """One query shape at one fill level through the three row bodies (and, for the filter, the packed body's LATE
    instantiation): each against the reference, and all of them equal."""
    F = fill
    table, keys, query, _, reference = SHAPES[shape]
    K, L, S, tb = F.K[(shape, level)], F.L[shape], F.S[table], F.tb[table]
    kc = keys(K)
    q = query(kc)
    time_mode = bool(q.get("time_col"))
    assert S >= 2 * K and K * LEVELS[level][1] == L * LEVELS[level][0]
    if shape in ("nul", "filter"):       # every even guard block holds every key, and every share a whole even guard block
        assert F.guard % K == 0 and S >= 3 * F.guard
    if (shape, K) not in F.refs:
        F.refs[(shape, K)] = _numpy_ref(F, shape, table, kc, q) if reference == "numpy" else _oracle_ref(F, oracle, table, kc, q)
    ref = F.refs[(shape, K)]
    if q["op"] == "hist":                # (outliers of both aggregations, in every group: whichever level a row lands on)
        assert all(h["n_outliers"] > 0 for r in ref["results"] for h in r["hists"])
    runs = [(name, env, 0) for name, env in KERNELS.items()]
    if shape == "filter":
        runs.append(("packed", {"SYBL_LATE_PATH": "1"}, 1))
    snaps = {}
    for kernel, env, late in runs:
        what = (shape, level, K, L, kernel, late)
        res, st, tr = _traced(tb, q, capfd, monkeypatch, **env)
        try:
            assert st["strategy"] == 7 and st["lds_bytes"] > 0 and st["n_workgroups"] == F.n_wg, (what, st)
            assert (tr["kernel"], tr["late"]) == (TAKEN.get((shape, kernel), kernel), late), (what, tr)
            assert tr["staging"] == L and tr["words"] == F.words[shape] and st["lds_bytes"] == 8 * L * tr["words"], (what, tr, st)
            assert S >= 2 * K, what
            if level in ("3L/2", "2L"):
                assert K > tr["staging"], what           # more keys in every share than slots: some rows MUST go direct
            elif level == "L/2":
                assert 2 * K <= tr["staging"], what
            if reference == "numpy":
                _check_numpy(res, ref, shape, bool(q["aggs"]), what)
            else:
                parity.compare(res, ref, op=q["op"], full=False, n_aggs=len(q["aggs"]), time_mode=time_mode)
            snaps[(kernel, late)] = _snapshot(res, time_mode)
        finally:
            res.free()
    first = snaps[("packed", 0)]
    assert len(first[0]) >= K
    for k, s in snaps.items():
        assert s == first, (shape, level, K, k)


def test_the_sweep_saw_what_it_was_built_for(fill, capfd):
    """The shapes' L as traced on this device (printed), and the rows the shapes rely on: values of both signs, outliers, a filter
    that passes about half, a sorted time column of a handful of buckets, rows without a key and without a value."""
    F = fill
    with capfd.disabled():
        print("\n" + F.summary)
    assert F.L["count"] == max(F.L.values()) and F.L["moments"] == min(F.L.values()), F.L
    main = F.cols["main"]
    assert int(main["v"].min()) < 0 < int(main["v"].max()) and int(main["u"].max()) > U_INFO[1] and int(main["w"].max()) == W_INFO[1]
    passing = float((main["f"] > 49).mean())
    assert 0.4 < passing < 0.7, passing
    assert np.all(np.diff(main["t"]) >= 0) and len(np.unique(main["t"] // TB)) == N_TB
    pk, pv = F.pops["main"]["kn%d" % F.K[("nul", "L")]], F.pops["main"]["vn"]
    assert 0.05 < 1 - pk.mean() < 0.2 and 0.1 < 1 - pv.mean() < 0.3


# ---------------------------------------------------------------------------------------------- B. the global table
N_B = 100_000
SEED_90 = 29         # (chosen on the CPU: longest run 212 of 8192 slots, one run across the table end)


def _cap_keys(k, seed):
    """k distinct keys of [0, 2^20), 0 among them (the declared minimum: the composite key is the value itself)."""
    rng = np.random.default_rng(seed)
    return np.r_[0, 1 + rng.choice((1 << 20) - 1, k - 1, replace=False)].astype(np.int64)


def _cap_table(ctx, keys, compact, by_key):
    """N_B rows over the keys, each at least N_B // len(keys) times: in key order (a 2048-row tile then holds a few dozen keys,
    all of them staged, and the global table is filled by the flushes) or cyclic (every tile holds 2048 keys)."""
    rng = np.random.default_rng(len(keys))
    k = H.cyclic_column(rng.permutation(keys), N_B)
    cols = {"k": np.sort(k) if by_key else k, "v": rng.integers(-300, 1000, N_B)}
    tb = ctx.create_table("cap")
    tb.add_column("k", "int")
    tb.add_column("v", "int", -300, 999)
    for r0 in range(0, N_B, 50_000):
        tb.append_block(50_000, {c: a[r0:r0 + 50_000] for c, a in cols.items()})
    tb.set_bounds("k", 0, (1 << 20) - 1)
    if compact:
        tb.compact()
    return tb, cols


def _cap_env(kernel, staging, slots):
    env = dict(KERNELS[kernel], SYBL_HASH_SLOTS=str(slots))
    if not staging:
        env["SYBL_NO_HASH_LDS"] = "1"
    return env


@pytest.mark.parametrize("staging", [True, False], ids=["flush", "direct"])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("slots,n_keys", [(4096, 4095), (4096, 4096), (8192, 7372)])
def test_global_table_at_capacity_is_exact(ctx, capfd, monkeypatch, slots, n_keys, kernel, staging):
    """4096 slots: the probe bound is the whole table, so a key that has walked it all has seen 4096 OTHER keys -- with 4095 or
    4096 keys every insertion order succeeds, the last key into the last free slot.  8192 slots at 90 %: the bound is half the
    table; the keys are chosen (on the CPU, from the restated hash) so that no run of occupied slots comes near it.  Inserts
    arrive through the flush of the staging tables (rows in key order: a tile's few dozen keys all stage) or row by row."""
    keys = _cap_keys(n_keys, SEED_90 if slots == 8192 else n_keys)
    occ = H.occupied_slots(keys, slots)
    run = H.longest_run(occ)
    assert H.wraps(occ), "no run of occupied slots crosses the table end"
    if slots > MAX_PROBES:
        assert run < MAX_PROBES // 8, run
    else:
        assert min(slots, MAX_PROBES) == slots and n_keys <= slots and run >= slots - 1
    tb, cols = _cap_table(ctx, keys, compact=kernel == "packed", by_key=staging)
    try:
        res, st, tr = _traced(tb, _q(groups=["k"], aggs=["v"]), capfd, monkeypatch, **_cap_env(kernel, staging, slots))
        what = (slots, n_keys, kernel, staging)
        assert st["strategy"] == 7 and (st["lds_bytes"] > 0) == staging, (what, st)
        assert (tr["slots"], tr["kernel"], tr["staging"] > 0) == (slots, kernel, staging), (what, tr)
        ref = H.group_ref(cols["k"], cols["v"])
        assert len(ref) == n_keys
        _check_numpy(res, ref, "cap", True, what)
        res.free()
    finally:
        tb.free()


class _Walk:
    pass


@pytest.fixture(scope="module")
def walk(ctx):
    """4096 keys for 4096 slots of which the last to arrive has to read every slot.  The slots 4095 keys take do not depend on
    their order, so the one they leave free, f, is known here; the last key X is picked with its home at f + 1, the far end of
    the walk.  The rows favour that order without needing it: every workgroup has eight tiles, the 4095 keys cycle through all
    of them and X is in the last 64 rows of the table alone, seven tiles after its workgroup met every other key.  In any other
    order the query has to succeed just the same; in this one a probe bound of 4095 reports a table with a free slot as full."""
    others = _cap_keys(4095, 4095)
    occ = H.occupied_slots(others, 4096)
    free = np.flatnonzero(~occ)
    assert free.size == 1
    cand = np.setdiff1d(np.arange(1, 1 << 20, dtype=np.int64), others)
    last = int(cand[H.home_slots(cand, 4096) == (int(free[0]) + 1) % 4096][0])
    n_wg = ctx.device_info()["n_cus"]
    assert 16 <= n_wg <= 512, n_wg
    W = _Walk()
    W.n_wg, W.n = n_wg, n_wg * 8 * 2048
    rng = np.random.default_rng(4096)
    W.cols = {"k": H.cyclic_column(rng.permutation(others), W.n), "v": rng.integers(-300, 1000, W.n)}
    W.cols["k"][-64:] = last
    assert np.flatnonzero(W.cols["k"] == last)[0] == W.n - 64 and np.unique(W.cols["k"][:4095]).size == 4095
    W.keys = np.r_[others, last]
    assert H.occupied_slots(W.keys, 4096).all() and int(H.home_slots(W.keys[-1:], 4096)[0]) == (int(free[0]) + 1) % 4096
    tb = ctx.create_table("walk")
    tb.add_column("k", "int")
    tb.add_column("v", "int", -300, 999)
    for r0 in range(0, W.n, BLOCK):
        tb.append_block(BLOCK, {c: a[r0:r0 + BLOCK] for c, a in W.cols.items()})
    tb.set_bounds("k", 0, (1 << 20) - 1)
    tb.compact()
    W.tb = tb
    W.ref = H.group_ref(W.cols["k"], W.cols["v"])
    yield W
    tb.free()


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_the_last_key_may_have_to_read_every_slot(walk, capfd, monkeypatch, kernel):
    """hash_find_or_insert's bound is the WHOLE table: the 4096th key, arriving last with its home just behind the only free
    slot, finds it with its 4096th probe (no staging: the rows insert in the order the workgroups reach them)."""
    W = walk
    res, st, tr = _traced(W.tb, _q(groups=["k"], aggs=["v"]), capfd, monkeypatch, **_cap_env(kernel, False, 4096))
    assert st["strategy"] == 7 and st["lds_bytes"] == 0 and st["n_workgroups"] == W.n_wg, st
    assert (tr["slots"], tr["kernel"], tr["staging"]) == (4096, kernel, 0), tr
    assert len(W.ref) == 4096 and W.ref[int(W.keys[-1])][0] == 64
    _check_numpy(res, W.ref, "cap", True, ("walk", kernel))
    res.free()


@pytest.mark.parametrize("n_keys", [4095, 4096])
def test_bucket_arrays_of_a_full_global_table(ctx, oracle, capfd, monkeypatch, n_keys):
    """hist with percentiles: the bucket arrays live in the global table only and are gathered slot by slot (k_hash_gather_hist),
    here from every slot of the table."""
    keys = _cap_keys(n_keys, n_keys)
    tb, cols = _cap_table(ctx, keys, compact=False, by_key=False)
    try:
        q = _q(groups=["k"], aggs=["v"], op="hist", want_percentiles=True)
        res, st, tr = _traced(tb, q, capfd, monkeypatch, SYBL_HASH_SLOTS="4096")
        assert st["strategy"] == 7 and st["lds_bytes"] == 0 and tr["slots"] == 4096 and tr["staging"] == 0, (st, tr)
        ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in ("k", "v")], n_threads=4, block_rows=50_000,
                                **parity.oracle_query_kwargs(["k", "v"], {"v": (-300, 999)}, q))
        assert len(ores["results"]) == n_keys
        parity.compare(res, ores, op="hist", full=True, n_aggs=1)
        res.free()
    finally:
        tb.free()


@pytest.mark.parametrize("staging", [True, False], ids=["flush", "direct"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_one_key_more_than_slots_fails_and_the_context_survives(ctx, capfd, monkeypatch, kernel, staging):
    """4097 keys in 4096 slots: "more distinct group keys", from the flush's `full` branch (rows in key order: the keys stage, so
    the inserts are the flushes') and from the rows' own; a fresh query on the same context and table, with room, is exact."""
    keys = _cap_keys(4097, 4097)
    tb, cols = _cap_table(ctx, keys, compact=kernel == "packed", by_key=staging)
    try:
        q = _q(groups=["k"], aggs=["v"])
        with _env(monkeypatch, SYBL_FORCE_HASH="1", **_cap_env(kernel, staging, 4096)):
            qy = tb.query(**q)
            assert qy.stats()["strategy"] == 7 and qy.stats()["n_cells"] == 4096 and (qy.stats()["lds_bytes"] > 0) == staging
            for _ in range(2):           # (a rescan starts from an empty table and fails the same way)
                with pytest.raises(sybil_amd.SyblError) as e:
                    qy.run()
                assert "more distinct group keys" in str(e.value)
            qy.free()
        res, st, tr = _traced(tb, q, capfd, monkeypatch, **_cap_env(kernel, staging, 8192))
        assert tr["slots"] == 8192 and tr["kernel"] == kernel
        _check_numpy(res, H.group_ref(cols["k"], cols["v"]), "cap", True, (kernel, staging))
        res.free()
    finally:
        tb.free()
