"""GPU: the PROVED row bodies of k_scan_packed after their vector-instruction diet (scan_packed.h: packed_bucket, packed_row<PROVED>,
PackedRowRegs, packed_scan_dyn's loop-carried operands; scan_fast.h: FastPlan::qmul / qshift / qoff2 / kfold; planner.cpp:
fill_packed, plan_lean; udiv_magic.h).  Under kLeanProved the bucket number is an exact multiply-shift on planner constants, the
cell index runs over the keys' STORED offsets plus one folded constant, and the dynamic loops keep the words' field widths and
the lean addends' high halves in vector registers.

Every case runs three ways -- the plan as planned (the trace says which family: `dealing: dynamic=`, `narrow: f=word(..) k=word(..)`,
`lean moments: .. proved=` / `lean hist: proved=`, and the new `quotient: a0 d=.. mul=.. shift=.. off2=.. kfold=..`, whose constants
are recomputed here), the same query under SYBL_NO_LEAN=1 (the f64 quotient, the digits' offsets added per row), which must equal
the first field for field and floats bit for bit, and the CPU oracle (tests/parity.py).  Tables are n_wg * T * 4096 + ragged rows
with T <= 4, from the workgroup count of the device under test; small tables get words and the dynamic loops through the settings
of tests/test_gpu_key_word.py.

  1. quotient edges in moments mode on the headline's kernel shape (3 filters in a word, 2 one-byte keys, 2 aggregations): values
     at k d - 1, k d, k d + 1 of every bucket k for the divisors 1, 999, 1000, 4096 and 2^23 + 1 (numerators up to 2^24 - 1), two
     different divisors per query in both orders, storage bases at and above h.Min (off2 = 0 and > 0) -- and, through a select
     that drops the rows below h.Min, BELOW it (off2 "negative": the sum wraps back).  An aggregation 0 whose stored range fits
     two bytes gets no key word (d = 1: values within 1001 of h.Min): that case runs the filter-word kernel on the key columns;
  2. quotient edges in full-histogram mode, bucket arrays compared exactly: 16 divisors of the CPU test's list
     (tests/test_gpu_lean_moments.py's test_bucket_quotient_edges keeps 4, 1000, 20 000 and 2^24 - 1000);
  3. the folded key constant: one and two key columns (three have no templated kernel: kFastTemplatedG = 2), declared lower bounds
     below, at and -- through a select -- above the storage base (gdoff > 0, = 0, < 0), rows in the first and the last cell the
     data can reach, one and two replicas; and a key whose stored offsets reach 2^24 reports proved=0 and agrees all the same;
  4. loop-carried operands and masks: tests/late_layout.py's `main` (every one of the sixteen pass / skip sequences per wave, whole
     waves skipping tiles) and `ragged` tables, and last tiles that leave 1, 2 and 3 rows in a lane; `matched` exact.
"""
import re

import numpy as np
import pytest

import sybil_amd
from tests import late_layout as LL
from tests import parity

pytestmark = pytest.mark.gpu

TILE = 4096
BLOCK = 65536
U32 = 1 << 32
LIMIT = 1 << 24
MOMENTS = re.compile(r"^lean moments: lean=(\d) proved=(\d) digits=(\d) mul24=(\d) ", re.M)
HIST = re.compile(r"^lean hist: proved=(\d) digits=(\d) mul24=(\d)$", re.M)
QUOT = re.compile(r"^quotient:((?: a\d+ d=\d+ mul=\d+ shift=\d+ off2=\d+)+) kfold=(\d+)$", re.M)
QAGG = re.compile(r" a(\d+) d=(\d+) mul=(\d+) shift=(\d+) off2=(\d+)")
NARROW = re.compile(r"^narrow:(.*) bytes_per_row=(\d+)$", re.M)
DYN = {"SYBL_DYN": "1", "SYBL_DYN_MIN_TILES": "1", "SYBL_DYN_PIECE_TILES": "2"}
RANGE3 = [(c, op, v) for c in ("f1", "f2", "f3") for op, v in (("gt", 99), ("lt", 900))]
NEAR = (1 << 23) + 1


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def small_tables_get_words_and_the_dynamic_loops(monkeypatch):
    monkeypatch.setenv("SYBL_KWORD_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_FWORD_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_NARROW_MIN_ROWS", "1")
    monkeypatch.setenv("SYBL_PLAN_TRACE", "1")
    for k, v in DYN.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def n_wg(ctx):
    tiny = ctx.create_table("probe")
    tiny.add_column("g", "int", 0, 3)
    tiny.add_column("v", "int", 0, 9)
    tiny.append_block(8, {"g": np.arange(8) % 4, "v": np.arange(8)})
    qy = tiny.query(groups=["g"], aggs=["v"])
    qy.run().free()
    n = qy.stats()["n_workgroups"]
    qy.free()
    tiny.free()
    assert 16 <= n <= 512, "n_workgroups = %d: this file is sized for one workgroup per CU of a 16..512-CU device" % n
    return n


def magic(d):
    """(mul, shift) of udiv_magic.h, in Python's integers."""
    s = d.bit_length() - 1
    return -((-(1 << (31 + s))) // d), s


def test_magic_is_the_header_s():
    assert magic(1) == (1 << 31, 0) and magic(1000) == (1099511628, 9) and magic(LIMIT - 1)[1] == 23
    for d in (1, 2, 3, 999, 1000, 4096, NEAR, LIMIT - 1):
        mul, s = magic(d)
        assert 1 << 30 < mul <= 1 << 31
        for n in (0, d - 1, d, 2 * d - 1, 2 * d, LIMIT - 1):
            if n < LIMIT:
                assert ((2 * n * mul) >> 32) >> s == n // d


def _table(ctx, name, cols, info, bounds):
    n = len(next(iter(cols.values())))
    tb = ctx.create_table(name)
    for c in cols:
        tb.add_column(c, "int", *info[c])
    for r0 in range(0, n, BLOCK):
        tb.append_block(min(BLOCK, n - r0), {c: v[r0:r0 + BLOCK] for c, v in cols.items()})
    assert tb.rows == n
    for c, (lo, hi) in bounds.items():
        tb.set_bounds(c, lo, hi)
    tb.compact()
    return tb


def _run(tb, q, capfd):
    capfd.readouterr()
    qy = tb.query(**q)
    try:
        res = qy.run()
        st = qy.stats()
    finally:
        qy.free()
    return res, st, capfd.readouterr().err


def _fields(res):
    """Every field of every row and of Cumulative, in an order and a form that compares with == (floats by their repr)."""
    def norm(v):
        if hasattr(v, "tolist"):
            return tuple(v.tolist())
        return repr(v) if isinstance(v, float) else v
    out = []
    for which in (0, 1, 2):
        for r in res.rows(which):
            out.append((which, r["key"], r["time_bucket"], r["count"], r["samples"],
                        tuple(tuple(sorted((k, norm(v)) for k, v in h.items())) for h in r["hists"])))
    return res.matched, sorted(out)


def _three_ways(tb, names, cols, info, q, oracle, capfd, monkeypatch, full=False):
    """As planned, under SYBL_NO_LEAN=1 and through the oracle.  Returns (trace of the planned run, its stats, its Result's
    matched count, the keys of its rows)."""
    monkeypatch.delenv("SYBL_NO_LEAN", raising=False)
    ores = oracle.run_query([{"type": "int", "data": cols[c]} for c in names], n_threads=16, **parity.oracle_query_kwargs(names, info, q))
    res, st, err = _run(tb, q, capfd)
    parity.compare(res, ores, op="hist", full=full, n_aggs=len(q["aggs"]))
    planned, matched = _fields(res), res.matched
    keys = {tuple(r["key_vals"]) for r in res.rows(0)}
    res.free()
    monkeypatch.setenv("SYBL_NO_LEAN", "1")
    res, st0, err0 = _run(tb, q, capfd)
    monkeypatch.delenv("SYBL_NO_LEAN")
    assert not MOMENTS.search(err0) and not HIST.search(err0) and "quotient:" not in err0, err0[-2000:]
    assert (st0["strategy"], st0["n_workgroups"], st0["packed_kernel"]) == (st["strategy"], st["n_workgroups"], st["packed_kernel"])
    parity.compare(res, ores, op="hist", full=full, n_aggs=len(q["aggs"]))
    assert _fields(res) == planned
    res.free()
    assert matched == ores["matched"]
    return err, st, matched, keys


def _quotients(err):
    """[({aggregation: (d, mul, shift, off2)}, kfold)] of every `quotient:` line."""
    return [({int(a): (int(d), int(m), int(s), int(o)) for a, d, m, s, o in QAGG.findall(body)}, int(k)) for body, k in QUOT.findall(err)]


def _edges(d, drop):
    """Numerators k d - 1, k d, k d + 1 of every bucket k a column of bucket size d can hold without outliers and below 2^24 (and
    2^24 - 1 itself where the buckets reach it); drop: without those below 3 d - 1 (d - 1 for a bucket size beyond 2^22) -- the
    storage base is then that far above h.Min."""
    kmax = min(1000, (LIMIT - 1) // d)
    e = {v for k in range(kmax + 1) for v in (k * d - 1, k * d, k * d + 1) if 0 <= v < LIMIT and v <= 1000 * d + 1}
    if (LIMIT - 1) // d <= 1000:
        e.add(LIMIT - 1)
    if drop:
        e = {v for v in e if v >= (3 * d - 1 if kmax >= 4 else d - 1)}
    return np.array(sorted(e), dtype=np.int64)


def _headline_columns(n, seed, keys=((0, 15), (0, 15))):
    rng = np.random.default_rng(seed)
    cols = {c: rng.integers(0, 1000, n) for c in ("f1", "f2", "f3")}
    for i, (lo, hi) in enumerate(keys):
        cols["g%d" % (i + 1)] = rng.integers(lo, hi + 1, n)
    for c in ("f1", "f2", "f3"):
        cols[c][0], cols[c][1] = 0, 999
    return cols, rng


def _place(col, values, rng):
    """Every value of `values` at least once, the rest drawn from them."""
    col[:] = values[rng.integers(0, values.size, col.size)]
    col[:values.size] = values


# ---------------------------------------------------------------- 1. quotient edges, moments mode, the headline's kernel shape
H0, H1 = 7777, -500           # h.Min of the two aggregations (Info.Max stays positive: the reference gates values at Info.Max * 10)
PAIRS = [(1, 999), (999, 1), (1000, 4096), (4096, 1000), (NEAR, 1000), (1000, NEAR)]


def _moments_case(n, d0, d1, drop0, drop1, seed, below=(0, 0)):
    """Columns, info and the expected quotient constants.  below: rows whose aggregation lies that far under h.Min (to be dropped
    by a select) -- the storage base is then that far below h.Min."""
    cols, rng = _headline_columns(n, seed)
    info = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 15)}
    want = {}
    for a, (name, d, h, drop, bel) in enumerate((("a0", d0, H0, drop0, below[0]), ("a1", d1, H1, drop1, below[1]))):
        e = _edges(d, drop)
        cols[name] = np.empty(n, dtype=np.int64)
        _place(cols[name], h + e, rng)
        if bel:
            cols[name][3100 + 40 * a:3140 + 40 * a] = h - bel  # (beyond the placed edges: every edge stays; 40 rows of their own each)
        info[name] = (h, h + 1000 * d + 1)
        want[a] = (d,) + magic(d) + ((2 * (int(e.min()) - bel)) % U32,)
    for c in ("f1", "f2", "f3"):                              # the rows that carry the edges pass the filters
        cols[c][2:3100] = 500
    return cols, info, want


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_quotient_edges_in_moments_mode(ctx, n_wg, oracle, capfd, monkeypatch, pair):
    d0, d1 = pair
    n = n_wg * 2 * TILE + 1234 + 1
    i = PAIRS.index(pair)
    cols, info, want = _moments_case(n, d0, d1, i % 2 == 0, i % 2 == 1, 100 + i)
    names = list(cols)
    tb = _table(ctx, "diet_q", cols, info, {"g1": (0, 15), "g2": (0, 15)})
    q = dict(filters=RANGE3, groups=["g1", "g2"], aggs=["a0", "a1"], op="hist", want_percentiles=False)
    err, st, matched, keys = _three_ways(tb, names, cols, info, q, oracle, capfd, monkeypatch)
    tb.free()
    assert "dealing: dynamic=1" in err and st["packed_kernel"] == 1, err[-2000:]
    tr = MOMENTS.findall(err)
    assert tr and all(t[1] == "1" for t in tr), err[-2000:]                     # proved
    plan = NARROW.findall(err)
    assert len(plan) == 1 and "f=word(10,10,10)" in plan[0][0], err[-2000:]
    # the key word: aggregation 0 beside two 1-byte keys is worth one iff its stored range needs more than two bytes
    wide0 = int(cols["a0"].max() - cols["a0"].min()) >= 65536
    assert ("k=word(" in plan[0][0]) == wide0, err[-2000:]
    qs = _quotients(err)
    assert qs and all(x == (want, 0) for x in qs), (qs, want)                    # (both keys stored at their declared minimum: kfold 0)
    assert matched > 3000


def test_quotient_with_storage_bases_below_h_min(ctx, n_wg, oracle, capfd, monkeypatch):
    """A select keeps the columns' storage (width, base) and drops the rows under h.Min: base - h.Min is negative, off2 wraps."""
    n = n_wg * 2 * TILE + 1234 + 2
    cols, info, want = _moments_case(n, 1000, 999, False, False, 120, below=(3000, 12345))
    names = list(cols)
    src = _table(ctx, "diet_src", cols, info, {"g1": (0, 15), "g2": (0, 15)})
    keep = (cols["a0"] >= H0) & (cols["a1"] >= H1)
    tb = src.select(filters=[("a0", "gt", H0 - 1), ("a1", "gt", H1 - 1)])
    src.free()
    assert tb.rows == int(keep.sum()) == n - 80
    assert tb.column_storage("a0")[1] == H0 - 3000 and tb.column_storage("a1")[1] == H1 - 12345
    kept = {c: v[keep] for c, v in cols.items()}
    q = dict(filters=RANGE3, groups=["g1", "g2"], aggs=["a0", "a1"], op="hist", want_percentiles=False)
    err, st, matched, keys = _three_ways(tb, names, kept, info, q, oracle, capfd, monkeypatch)
    tb.free()
    tr = MOMENTS.findall(err)
    assert "dealing: dynamic=1" in err and tr and all(t[1] == "1" for t in tr), err[-2000:]
    assert want[0][3] == U32 - 6000 and want[1][3] == U32 - 24690
    qs = _quotients(err)
    assert qs and all(x[0] == want for x in qs), (qs, want)
    assert matched > 3000


# ---------------------------------------------------------------- 2. quotient edges, full-histogram mode
HIST_DIVISORS = [1, 2, 3, 7, 641, 999, 1001, 4095, 4097, 65535, 65536, (1 << 23) - 1, 1 << 23, NEAR, LIMIT - 2, LIMIT - 1]


@pytest.mark.parametrize("bs", HIST_DIVISORS)
def test_quotient_edges_in_full_histogram_mode(ctx, n_wg, oracle, capfd, monkeypatch, bs):
    drop = HIST_DIVISORS.index(bs) % 2 == 1
    hmin = -77
    e = _edges(bs, drop)
    n = n_wg * 2 * TILE + 333
    rng = np.random.default_rng(bs)
    x = np.empty(n, dtype=np.int64)
    _place(x, hmin + e, rng)
    cols, info = {"g": rng.integers(0, 4, n), "x": x}, {"g": (0, 3), "x": (hmin, hmin + int(e.max()))}
    tb = _table(ctx, "diet_h", cols, info, {"g": (0, 3)})
    q = dict(groups=["g"], aggs=["x"], op="hist", hist_bucket=bs, want_percentiles=True)
    err, st, matched, keys = _three_ways(tb, ["g", "x"], cols, info, q, oracle, capfd, monkeypatch, full=True)
    tb.free()
    assert st["packed_kernel"] == 1, st
    tr = HIST.findall(err)
    assert tr and set(tr) == {("1", "1", "1")}, err[-2000:]
    qs = _quotients(err)
    assert qs and all(x == ({0: (bs,) + magic(bs) + (2 * int(e.min()),)}, 0) for x in qs), qs
    assert matched == n


# ---------------------------------------------------------------- 3. the folded key constant
K1, K2 = (3, 42), (5, 14)      # what the kept rows' keys span: the storage bases are 3 and 5 unless a select keeps lower ones


def _key_case(ctx, n, n_keys, sign, seed, far=False):
    """(table, its host columns, names, info, declared bounds, gdoff per key).  sign > 0: declared lower bounds 2 and 3 below
    the storage bases; 0: at them; < 0: the source holds keys from 0, a select keeps those from the declared bounds on -- the
    bases stay 0 (far: key 1 of one source row at 3 - 2^24, so the kept rows' stored offsets start at 2^24)."""
    spans = (K1, K2)[:n_keys]
    lows = [0 if sign < 0 else lo for lo, hi in spans]
    cols, rng = _headline_columns(n, seed, keys=[(lo0, hi) for lo0, (lo, hi) in zip(lows, spans)])
    cols["a0"], cols["a1"] = rng.integers(0, 1_000_000, n), rng.integers(0, 999_997, n)
    cols["a0"][0], cols["a0"][1], cols["a1"][0], cols["a1"][1] = 0, 999_999, 0, 999_996
    gnames = ["g1", "g2"][:n_keys]
    for j, r in enumerate((5, 6)):                            # a passing row in the lowest and in the highest cell the data reaches
        for c in ("f1", "f2", "f3"):
            cols[c][r] = 500
        for g, (lo, hi) in zip(gnames, spans):
            cols[g][r] = (lo, hi)[j]
    if far:
        cols["g1"][7] = K1[0] - LIMIT
    info = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "a0": (0, 999_999), "a1": (0, 999_996)}
    info.update({g: span for g, span in zip(gnames, spans)})
    step = (2, 3)
    bounds = {g: ((lo - step[k], hi) if sign > 0 else (lo, hi)) for k, (g, (lo, hi)) in enumerate(zip(gnames, spans))}
    gdoff = [step[k] if sign > 0 else 0 if sign == 0 else -(lo if not (far and k == 0) else LIMIT) for k, (lo, hi) in enumerate(spans)]
    tb = _table(ctx, "diet_k", cols, info, bounds)
    if sign < 0:
        keep = np.ones(n, dtype=bool)
        for g, (lo, hi) in zip(gnames, spans):
            keep &= cols[g] >= lo
        src, tb = tb, tb.select(filters=[(g, "gt", lo - 1) for g, (lo, hi) in zip(gnames, spans)])
        src.free()
        assert tb.rows == int(keep.sum()) < n
        cols = {c: v[keep] for c, v in cols.items()}
        assert [tb.column_storage(g)[1] for g in gnames] == [lo + d for (lo, hi), d in zip(spans, gdoff)]
    return tb, cols, list(cols), info, bounds, gdoff


def _rep_budget_kb(cells, na, reps):
    """A SYBL_REP_BUDGET_KB under which the lean table of `cells` cells gets exactly `reps` replicas (planner.cpp: plan_lean)."""
    bytes1 = (na + (na + 1) // 2 + na) * cells * 8
    kb = -(-bytes1 * reps // 1024)
    assert bytes1 * reps <= kb * 1024 < 2 * bytes1 * reps
    return kb


@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("sign", [1, 0, -1], ids=["gdoff_pos", "gdoff_zero", "gdoff_neg"])
@pytest.mark.parametrize("n_keys", [1, 2])
def test_folded_key_constant(ctx, n_wg, oracle, capfd, monkeypatch, n_keys, sign, reps):
    n = n_wg * 2 * TILE + 1234 + 3
    tb, cols, names, info, bounds, gdoff = _key_case(ctx, n, n_keys, sign, 200 + 10 * n_keys + sign)
    gnames = ["g1", "g2"][:n_keys]
    card = [bounds[g][1] - bounds[g][0] + 1 for g in gnames]
    monkeypatch.setenv("SYBL_REP_BUDGET_KB", str(_rep_budget_kb(int(np.prod(card)), 2, reps)))
    q = dict(filters=RANGE3, groups=gnames, aggs=["a0", "a1"], op="hist", want_percentiles=False)
    err, st, matched, keys = _three_ways(tb, names, cols, info, q, oracle, capfd, monkeypatch)
    tb.free()
    assert "dealing: dynamic=1" in err and st["packed_kernel"] == 1 and st["replicas"] == reps, (st, err[-2000:])
    tr = MOMENTS.findall(err)
    assert tr and all(t[:2] == ("1", "1") for t in tr), err[-2000:]             # lean and proved
    plan = NARROW.findall(err)
    # (one 1-byte key and a 3-byte aggregation 0 cost the 4 bytes a key word costs: no word, the filter-word kernel on columns)
    assert len(plan) == 1 and "f=word(10,10,10)" in plan[0][0] and ("k=word(" in plan[0][0]) == (n_keys == 2), err[-2000:]
    # kfold = sum of gdoff * stride (mod 2^32): the strides of two keys are (card 2, 1) or (1, card 1)
    folds = {gdoff[0] % U32} if n_keys == 1 else {(gdoff[0] * card[1] + gdoff[1]) % U32, (gdoff[0] + gdoff[1] * card[0]) % U32}
    qs = _quotients(err)
    assert qs and all(k in folds for _, k in qs), (qs, folds)
    assert (sign == 0) == all(k == 0 for _, k in qs)
    lowest, highest = tuple(lo for lo, hi in (K1, K2)[:n_keys]), tuple(hi for lo, hi in (K1, K2)[:n_keys])
    assert lowest in keys and highest in keys


def test_key_offsets_of_2_24_decline_the_proof(ctx, n_wg, oracle, capfd, monkeypatch):
    """Digits in range, cells few -- and stored offsets from 2^24 on (the base is that far below the declared bound): no 24-bit
    product over the stored offset, so no proof; the unproved body adds gdoff per row and agrees."""
    n = n_wg * 2 * TILE + 1234 + 3
    tb, cols, names, info, bounds, gdoff = _key_case(ctx, n, 2, -1, 290, far=True)
    assert tb.column_storage("g1") == (4, K1[0] - LIMIT) and int(cols["g1"].min()) == K1[0]
    q = dict(filters=RANGE3, groups=["g1", "g2"], aggs=["a0", "a1"], op="hist", want_percentiles=False)
    err, st, matched, keys = _three_ways(tb, names, cols, info, q, oracle, capfd, monkeypatch)
    tb.free()
    tr = MOMENTS.findall(err)
    assert tr and all(t[1:3] == ("0", "0") for t in tr) and not QUOT.search(err), err[-2000:]   # proved=0 digits=0
    assert st["packed_kernel"] == 1 and (K1[0], K2[0]) in keys and (K1[1], K2[1]) in keys


# ---------------------------------------------------------------- 4. loop-carried operands and masks
@pytest.fixture(scope="module")
def late_tables(ctx, n_wg):
    layouts = {"main": LL.main(n_wg), "ragged": LL.ragged(n_wg)}
    tbs = {}
    for name, layout in layouts.items():
        tb = ctx.create_table("diet_" + name)
        for c in LL.COLUMN_ORDER:
            tb.add_column(c, "int", *LL.INFO.get(c, (1, 0)))
        r0 = 0
        for b in layout.blocks:
            tb.append_block(b, {c: layout.cols[c][r0:r0 + b] for c in LL.COLUMN_ORDER})
            r0 += b
        for c in LL.COLUMN_ORDER:
            if c in LL.DECLARED:
                tb.set_bounds(c, *LL.DECLARED[c])
        tb.compact()
        tbs[name] = tb
    yield layouts, tbs
    for tb in tbs.values():
        tb.free()


@pytest.mark.parametrize("filters", ["f1", "word3"])
@pytest.mark.parametrize("table", ["main", "ragged"])
def test_pass_and_skip_patterns_through_the_proved_loop(late_tables, oracle, capfd, monkeypatch, table, filters):
    """ga and gb (in range in every row: the proof holds) and a4 in one key word; every wave of `main` runs one of the sixteen
    pass / skip sequences of four tiles, whole waves skip tiles, `ragged` ends windows and tiles anywhere."""
    layouts, tbs = late_tables
    flt = LL.FILTERS["f1"] if filters == "f1" else LL.WORD3
    q = dict(filters=flt, groups=["ga", "gb"], aggs=["a4", "a2b"], op="hist", want_percentiles=False, order_by=None)
    cols = layouts[table].cols
    names = ["f1", "gc", "gh", "ga", "gb", "a4", "a2b"]
    info = dict(LL.INFO, **{c: (1, 0) for c in names if c not in LL.INFO})
    err, st, matched, keys = _three_ways(tbs[table], names, cols, info, q, oracle, capfd, monkeypatch)
    tr = MOMENTS.findall(err)
    assert "dealing: dynamic=1" in err and tr and all(t[:2] == ("1", "1") for t in tr), err[-2000:]
    plan = NARROW.findall(err)
    assert len(plan) == 1 and "k=word(2,1,20)" in plan[0][0] and ("f=word(8,9,12)" in plan[0][0]) == (filters == "word3"), err[-2000:]
    ref = LL.reference(cols, q)
    assert ref["overflow"] == 0 and matched == ref["matched"] == int(layouts[table].passing.sum()) >= 1
    res, st, err = _run(tbs[table], q, capfd)
    got = {tuple(r["key_vals"]): (r["count"], tuple(h["sum"] for h in r["hists"][:2])) for r in res.rows(0)}
    res.free()
    assert got == {k: (cnt, tuple(a[0] for a in aggs)) for k, (cnt, aggs) in ref["groups"].items()}


@pytest.mark.parametrize("left", [1, 2, 3])
def test_last_lane_with_rows_left(ctx, n_wg, oracle, capfd, monkeypatch, left):
    """The table ends `left` rows into a lane's four; those rows pass, carry the largest values and sit in a cell of their own."""
    n = n_wg * TILE + 4 * 77 + left
    cols, rng = _headline_columns(n, 300 + left, keys=((0, 14), (0, 15)))
    cols["a0"], cols["a1"] = rng.integers(0, 900_000, n), rng.integers(0, 900_000, n)
    tail = np.arange(n - left, n)
    for c in ("f1", "f2", "f3"):
        cols[c][tail] = 500
    cols["g1"][tail], cols["g2"][tail] = 15, 15
    cols["a0"][tail], cols["a1"][tail] = 999_999 - np.arange(left), 999_996 - np.arange(left)
    cols["a0"][0], cols["a1"][0] = 0, 0
    info = {"f1": (0, 999), "f2": (0, 999), "f3": (0, 999), "g1": (0, 15), "g2": (0, 15), "a0": (0, 999_999), "a1": (0, 999_996)}
    tb = _table(ctx, "diet_tail", cols, info, {"g1": (0, 15), "g2": (0, 15)})
    q = dict(filters=RANGE3, groups=["g1", "g2"], aggs=["a0", "a1"], op="hist", want_percentiles=False)
    err, st, matched, keys = _three_ways(tb, list(cols), cols, info, q, oracle, capfd, monkeypatch)
    tr = MOMENTS.findall(err)
    assert "dealing: dynamic=1" in err and tr and all(t[:2] == ("1", "1") for t in tr) and "k=word(4,4,20)" in err, err[-2000:]
    res, st, err = _run(tb, q, capfd)
    last = [r for r in res.rows(0) if tuple(r["key_vals"]) == (15, 15)]
    assert len(last) == 1 and last[0]["count"] == left and last[0]["hists"][0]["sum"] == int(cols["a0"][tail].sum())
    assert last[0]["hists"][1]["sum"] == int(cols["a1"][tail].sum())
    assert res.matched == int(LL.keep(cols, RANGE3).sum())
    res.free()
    tb.free()
