"""GPU: rollup percentiles (the p<k> tokens of Table.rollup / sybl_table_rollup, csrc/rollup.hip) against the restatement in
tests/rollup_pct_ref.py.  Tables are built block by block through append_block from the very block lists the restatement
reads; the output is read back whole with samples(limit=G) and read_int.  Every comparison is exact.

Shapes: a few thousand rows in blocks of 1, 70, 33, 2049, 31, 64, 777, 32 rows -- padding rows, a one-row first block, blocks on
both sides of 32 and of a 1024-row tile.  The radix sort's single-workgroup size sits in the sort library's compiled
configuration, where a test cannot read it: the sort sizes are 300 and 300 000 items, the latter in 65536-row blocks."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import rollup_pct_ref as P
from tests.test_gpu_concat import _against_oracle, _cut, _rows
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

E_INVAL = -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
T_SIZES = (1, 70, 33, 2049, 31, 64, 777, 32)
N_T = sum(T_SIZES)
LDS, GLOBAL, HASH = 1, 2, 3
COUNTS = ("rows_in", "rows_matched", "rows_no_time", "groups", "blocks_out", "path", "fields", "cells_or_slots")
PCT_COUNTS = ("columns", "percentiles", "variant32", "variant64", "variant_pairs", "key_bits_max", "items")
P3 = "p1,p50,p99"


@pytest.fixture(scope="module")
def ctx():
    import sybil_amd
    c = sybil_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc
    return orc


@pytest.fixture
def env(monkeypatch):
    """Sets the diagnostic switches for one test (the library reads them at call time)."""
    def set_(path=None, slots=None, pct=None):
        for name, v in (("SYBL_ROLLUP_PATH", path), ("SYBL_ROLLUP_SLOTS", slots), ("SYBL_ROLLUP_PCT", pct)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    set_()
    return set_


def _check(t, tl, compact, path=None, force=None, slots=0, pct=None, ref=None, rolled=False, **kw):
    """t.rollup(**kw) against rollup_pct_ref: the counts of both stats, columns, every row, storage, bitmaps, extrema folded from
    the block statistics, the stored values of unpopulated rows, the order of the percentiles, the untouched source.  Returns
    (table, pct stats, ref)."""
    if ref is None:
        ref = P.rollup_pct_ref(tl, compact=compact, force=force, slots=slots, pct_force=pct, **kw)
    G = ref["stats"]["groups"]
    before = (t.rows, t.blocks)
    own = t.rollup_pct_stats()                                         # rolled: t is itself a percentile rollup's output
    out = t.rollup(**kw)
    try:
        st, ps = out.rollup_stats(), out.rollup_pct_stats()
        assert {k: st[k] for k in COUNTS} == ref["stats"], (st, ref["stats"])          # fields stays 1 + 4 per aggregated column
        assert {k: ps[k] for k in PCT_COUNTS} == ref["pct_stats"], (ps, ref["pct_stats"])
        if path is not None:
            assert st["path"] == path, st
        assert (out.rows, out.blocks) == (G, len(ref["blocks"])) and (t.rows, t.blocks) == before
        assert t.rollup_pct_stats() == (own if rolled else {k: 0 for k in ps})         # zeros for a table no percentile rollup made
        assert out.samples(limit=1).columns == [c for c, _ in ref["columns"]]
        assert _rows(out) == D.rows_of(ref["blocks"])
        cols = D.concat(ref["blocks"]) if G else {}
        keys = list(kw.get("groups", ()))
        for name, ty in ref["columns"]:
            info = out.column_info(name)
            assert info["has_missing"] == ref["bitmap"][name], (name, info)
            if name not in keys:
                assert out.column_storage(name) == ref["storage"][name], (name, out.column_storage(name), ref["storage"][name])
            if not G or ty != "int":
                continue
            _, v, p = cols[name]
            base = out.column_storage(name)[1]
            assert np.array_equal(out.read_int(name, 0, G), np.where(p, v, base)), name  # an unpopulated row stores 0
            want = (int(v[p].min()), int(v[p].max())) if p.any() else (I64_MAX, I64_MIN)
            assert (info["exact_min"], info["exact_max"]) == want, (name, info)          # the block statistics are exact
        # _min <= _p<k> ascending in k <= _max on every row that has values
        for c, ops in (P.U.agg_pairs(kw.get("aggs", ())) if G else ()):
            base, ks = P.split_ops(ops)
            chain = (["%s_min" % c] if "min" in base else []) + ["%s_p%d" % (c, k) for k in ks] + (["%s_max" % c] if "max" in base else [])
            for a, b in zip(chain, chain[1:]):
                pa, pb = cols[a][2], cols[b][2]
                assert np.array_equal(pa, pb) and (cols[a][1][pa] <= cols[b][1][pb]).all(), (a, b)
        if ps["items"]:
            assert ps["keys_bytes"] > 0 and ps["sort_bytes"] > 0 and ps["pick_bytes"] > 0 and ps["sort_ms"] > 0
    except BaseException:
        out.free()
        raise
    return out, ps, ref


def _same_table(a, b):
    assert (a.rows, a.blocks) == (b.rows, b.blocks)
    names = a.samples(limit=1).columns
    assert names == b.samples(limit=1).columns
    for name in names:
        assert a.column_storage(name) == b.column_storage(name) and a.column_info(name) == b.column_info(name), name
        if a.column_info(name)["type"] == 1 and a.rows:
            assert np.array_equal(a.read_int(name, 0, a.rows), b.read_int(name, 0, b.rows)), name
    assert _rows(a) == _rows(b)


# ------------------------------------------------------------------ 1. every path, every kind of value column

def _main_blocks():
    rng = np.random.default_rng(41)
    n = N_T
    i = np.arange(n, dtype=np.int64)
    time = -9000 + (i * 11) % 20000                                   # hours -2 .. 3 with truncation toward zero
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[5], w8[n - 7], w8[n // 2], w8[9] = I64_MIN, I64_MAX, I64_MAX, I64_MIN
    flat = {"time": (time, rng.random(n) > 0.03), "k1": (-1 + (i * 7) % 5, None), "k2": (1000 + (i % 3) * 30000, rng.random(n) > 0.1),
            "k8": ((i % 3) * (1 << 40) - 5, None), "v1": (100 + (i * 37) % 200, None), "v2": (-3 + (i * 7) % 60000, None),
            "v4": (5 + (i * 100003) % (1 << 31), None), "v8": (w8, None), "nb": (rng.integers(-500, 500, n).astype(np.int64), rng.random(n) > 0.6),
            "none": (np.full(n, 77, dtype=np.int64), np.zeros(n, dtype=bool)), "f": (i % 10, None), "same": ((i % 97 == 0) * 5, None)}
    strs = {"s": [("host%02d" % (k % 6) if k % 17 else None) for k in range(n)]}
    return _cut(flat, strs, {}, T_SIZES)


MAIN = _main_blocks()
MAIN_AGGS = [("v1", "n,sum,min,max," + P3), ("v2", "p50"), ("v4", "p67,max,p66"), ("v8", "min,max," + P3), ("nb", "p50,n"), ("none", "p50,sum")]


@pytest.fixture(scope="module")
def main(ctx):
    made = {}

    def get(compact):
        if compact not in made:
            made[compact] = build(ctx, MAIN, compact=compact, name="events")
        return made[compact]
    yield get
    for tb in made.values():
        tb.free()


@pytest.mark.parametrize("force,path", [(None, LDS), ("direct", LDS), ("global", GLOBAL), ("hash", HASH)])
@pytest.mark.parametrize("compact", [True, False])
def test_every_path_and_every_kind_of_value_column(main, env, compact, force, path):
    """Hourly x an int key x a str key with MISSING on each path, forced and by default; value columns stored at 1 / 2 / 4 / 8
    bytes (compact) and 8 (canonical), a column with a bitmap, a column without any populated value (no sort runs, every value
    unpopulated), INT64_MIN and INT64_MAX in one column with many cells (the pairs variant); unpopulated times dropped."""
    env(path=force)
    t = main(compact)
    if compact:
        assert [t.column_storage(c)[0] for c in ("v1", "v2", "v4", "v8", "none")] == [1, 2, 4, 8, 1]
    out, ps, ref = _check(t, MAIN, compact, path=path, force=force, groups=["k1", "s"], aggs=MAIN_AGGS, time_col="time", time_bucket=3600)
    try:
        assert ref["stats"]["rows_no_time"] > 0 and ref["stats"]["fields"] == 25
        assert (ps["columns"], ps["percentiles"]) == (6, 11) and ps["variant_pairs"] == 1 and ps["variant32"] + ps["variant64"] == 4
        assert ref["bitmap"]["none_p50"] and ref["bitmap"]["nb_p50"] and not ref["bitmap"]["v8_p50"] and ref["bitmap"]["s"]
        tb = {n: v for n, (_, v, p) in D.concat(ref["blocks"]).items()}
        assert I64_MIN in tb["v8_p1"].tolist() and I64_MAX in tb["v8_p99"].tolist()
        assert not D.concat(ref["blocks"])["none_p50"][2].any()
    finally:
        out.free()


@pytest.mark.parametrize("groups,force,path", [(["k2"], None, GLOBAL), (["k8"], None, HASH), (["k2", "k1"], "hash", HASH), ([], None, LDS)])
def test_default_paths_and_the_missing_group(main, env, groups, force, path):
    """direct-global and hash by default; k2 has a bitmap: the MISSING group has percentiles of its own; no key: one row."""
    env(path=force)
    out, ps, ref = _check(main(True), MAIN, True, path=path, force=force, groups=groups, aggs=[("v2", "sum," + P3), ("same", "p50,p99")])
    try:
        if "k2" in groups:
            cols = D.concat(ref["blocks"])
            missing = ~cols["k2"][2]
            assert ref["bitmap"]["k2"] and missing.any() and cols["v2_p50"][2][missing].all()
    finally:
        out.free()


def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def test_a_64_slot_table_whose_chains_wrap(ctx, env):
    """Seven keys whose home slot is 62 or 63 of 64: their chain runs over the end of the table into slots 0 ..; the find-only
    probe of the key pass walks the same chains.  Slot order is not key order: a group's values only have to be contiguous."""
    home = lambda c: (_splitmix64(c) >> 32) & 63
    late = [c for c in range(1, 200000) if home(c) >= 62][:7]
    rest = [c for c in range(1, 400) if 8 <= home(c) < 56][:20]
    one = [0] + late + rest + late[:3] + [199999]
    keys = np.array(one * 4, dtype=np.int64) + 1000                    # composite = value - 1000; every key four times or more
    n = len(keys)
    tl = _cut({"k": (keys, None), "v": ((np.arange(n, dtype=np.int64) * 7919) % 1000 - 500, None)}, {}, {}, (1, 31, n - 32))
    t = build(ctx, tl, compact=True)
    try:
        env(path="hash", slots=64)
        out, ps, ref = _check(t, tl, True, path=HASH, force="hash", slots=64, groups=["k"], aggs=[("v", "min,max,p1,p50,p66,p67,p99")])
        assert out.rollup_stats()["cells_or_slots"] == 64 and out.rollup_stats()["groups"] == 29 and ps["items"] == n
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 2. every variant

def _bits_blocks(cells, vbits, lo=-12345, rows=3000):
    """`cells` keys 0 .. cells - 1 and values that span exactly `vbits` bits from `lo`."""
    rng = np.random.default_rng(cells + vbits)
    i = np.arange(rows, dtype=np.int64)
    span = (1 << vbits) - 1
    off = [int(x) for x in rng.integers(0, 1 << 62, rows)]
    v = np.array([lo + (o % (span + 1)) for o in off], dtype=np.int64)
    v[3], v[rows - 2] = lo, lo + span
    return _cut({"k": (i % cells, None), "v": (v, None)}, {}, {}, (1, 70, 33, 2049, rows - 2153))


@pytest.mark.parametrize("vbits,variant", [(22, "variant32"), (23, "variant64"), (54, "variant64"), (55, "variant_pairs")])
def test_each_variant_reached_by_its_bits(ctx, env, vbits, variant):
    """1024 cells are 10 bits: value spans of 22, 23, 54 and 55 bits put the key at exactly 32, 33, 64 and 65."""
    tl = _bits_blocks(1024, vbits)
    t = build(ctx, tl, compact=True)
    try:
        out, ps, ref = _check(t, tl, True, groups=["k"], aggs=[("v", "min,max," + P3)])
        assert ps[variant] == 1 and ps["key_bits_max"] == 10 + vbits and out.rollup_stats()["cells_or_slots"] == 1024
        out.free()
    finally:
        t.free()


@pytest.mark.parametrize("force", [None, "global", "hash"])
def test_all_variants_forced_on_one_input_give_identical_tables(ctx, env, force):
    tl = _bits_blocks(300, 12)
    t = build(ctx, tl, compact=True)
    outs = []
    try:
        for pct, variant in (("32", "variant32"), ("64", "variant64"), ("pairs", "variant_pairs"), (None, "variant32")):
            env(path=force, pct=pct)
            out, ps, ref = _check(t, tl, True, force=force, pct=pct, groups=["k"], aggs=[("v", "n,min,max,p1,p50,p66,p67,p99")])
            outs.append(out)
            assert ps[variant] == 1 and ps["variant32"] + ps["variant64"] + ps["variant_pairs"] == 1
        for o in outs[1:]:
            _same_table(outs[0], o)
    finally:
        for o in outs:
            o.free()
        t.free()


def test_int64_edges_in_one_column(ctx, env):
    """INT64_MIN and INT64_MAX in one column: 64 value bits.  One cell: the 64-bit variant; more cells: the pairs variant."""
    n = 500
    i = np.arange(n, dtype=np.int64)
    v = (i * 2654435761) % (1 << 50) - (1 << 49)
    v[:12:2], v[1:12:2] = I64_MIN, I64_MAX                              # six of each: ranks 1 .. 6 and 495 .. 500 of 500
    tl = _cut({"k": (i % 3, None), "v": (v, None)}, {}, {}, (70, 33, n - 103))
    for compact in (True, False):
        t = build(ctx, tl, compact=compact)
        try:
            out, ps, ref = _check(t, tl, compact, aggs=[("v", "min,max,p1,p50,p99")])
            assert ps["variant64"] == 1 and ps["key_bits_max"] == 64
            assert _rows(out)[0]["v_p1"] == I64_MIN and _rows(out)[0]["v_p99"] == I64_MAX     # ranks 5 and 495
            out.free()
            out, ps, ref = _check(t, tl, compact, groups=["k"], aggs=[("v", "min,max,p1,p50,p99")])
            assert ps["variant_pairs"] == 1 and ps["key_bits_max"] == 66
            out.free()
        finally:
            t.free()


# ------------------------------------------------------------------ 3. group sizes

GROUP_NS = (0, 1, 2, 3, 99, 100, 101, 199, 200, 201)


@pytest.mark.parametrize("equal", [False, True])
@pytest.mark.parametrize("force", [None, "hash"])
def test_group_sizes_around_the_rank_rule(ctx, env, force, equal):
    """Groups of 0, 1, 2, 3, 99, 100, 101, 199, 200, 201 populated values with p1, p50, p99 and the neighbours p66, p67; once with
    distinct values in shuffled order, once with many equal ones.  The group of 0 has rows, none with a value."""
    rng = np.random.default_rng(7)
    g = np.concatenate([np.full(max(n, 4), k, dtype=np.int64) for k, n in enumerate(GROUP_NS)])
    pop = np.concatenate([np.arange(max(n, 4)) < n for n in GROUP_NS])
    order = rng.permutation(len(g))
    g, pop = g[order], pop[order]
    v = (rng.integers(0, 4, len(g)) * 1000 if equal else rng.permutation(len(g)) * 3 - 700).astype(np.int64)
    tl = _cut({"g": (g, None), "v": (v, pop)}, {}, {}, (1, 70, 33, len(g) - 104))
    t = build(ctx, tl, compact=True)
    try:
        env(path=force)
        out, ps, ref = _check(t, tl, True, force=force, groups=["g"], aggs=[("v", "n,min,max,p1,p50,p66,p67,p99")])
        cols = D.concat(ref["blocks"])
        assert tuple(cols["v_n"][1].tolist()) == GROUP_NS and ps["items"] == sum(GROUP_NS)
        assert cols["v_p50"][2].tolist() == [n > 0 for n in GROUP_NS] and ref["bitmap"]["v_p50"]
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 4. ops and names

def test_ops_and_names(main, env):
    import sybil_amd
    t = main(True)
    out, ps, ref = _check(t, MAIN, True, groups=["k1"], aggs=[("v1", "p50")])                      # percentile tokens only
    assert [c for c, _ in ref["columns"]] == ["k1", "count", "v1_p50"] and out.rollup_stats()["fields"] == 5
    out.free()
    out, ps, ref = _check(t, MAIN, True, groups=["k1"], aggs=[("v1", "p99,max,p5"), ("v2", "p50,p25,p75,n")])   # different lists
    assert [c for c, _ in ref["columns"]] == ["k1", "count", "v1_max", "v1_p5", "v1_p99", "v2_n", "v2_p25", "v2_p50", "v2_p75"]
    assert (ps["columns"], ps["percentiles"]) == (2, 5)
    out.free()
    eight = "p8,p7,p6,p5,p4,p3,p2,p1"
    out, ps, ref = _check(t, MAIN, True, groups=["s"], aggs=[("v4", eight)], count_name="rows")
    assert [c for c, _ in ref["columns"]] == ["s", "rows"] + ["v4_p%d" % k for k in range(1, 9)] and ps["percentiles"] == 8
    out.free()
    cases = [(dict(aggs=[("v4", eight + ",p9")]), eight + ",p9"), (dict(aggs=[("v1", "p50")], count_name="v1_p50"), "v1_p50"),
             (dict(aggs=[("v1", "p50"), ("v1", "p50,sum")]), "v1_p50"), (dict(aggs=[("s", "p50")]), "'s'")]
    for tok in ("p0", "p100", "p05", "p5.5", "p", "p50,p50", "sum,p50,sum", "P50", "p50,", "p500", "p-1"):
        cases.append((dict(aggs=[("v1", tok)]), "'%s'" % tok))
    for kw, word in cases:
        with pytest.raises(sybil_amd.SyblError) as ei:
            t.rollup(groups=["k1"], **kw)
        assert ei.value.code == E_INVAL and "sybl_table_rollup: " in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
    assert t.rows == N_T


def test_the_switch_and_its_refusals(ctx, main, env):
    import sybil_amd
    t = main(True)
    env(pct="sideways")
    with pytest.raises(sybil_amd.SyblError) as ei:
        t.rollup(groups=["k1"], aggs=[("v1", "p50")])
    assert ei.value.code == E_INVAL and "SYBL_ROLLUP_PCT" in str(ei.value) and "sideways" in str(ei.value)
    tl = _bits_blocks(1024, 23)                                        # 33 bits
    big = build(ctx, tl, compact=True)
    try:
        env(pct="32")
        with pytest.raises(sybil_amd.SyblError) as ei:
            big.rollup(groups=["k"], aggs=[("v", "p50")])
        assert ei.value.code == E_INVAL and "SYBL_ROLLUP_PCT=32" in str(ei.value) and "sybl_table_rollup: " in str(ei.value)
        out = big.rollup(groups=["k"], aggs=[("v", "sum")])            # without percentiles the switch forces nothing
        out.free()
    finally:
        big.free()
    env(pct="64")
    with pytest.raises(sybil_amd.SyblError) as ei:                     # v8 over the whole int64 range with 5 cells: 67 bits
        t.rollup(groups=["k1"], aggs=[("v8", "p50")])
    assert ei.value.code == E_INVAL and "SYBL_ROLLUP_PCT=64" in str(ei.value)


# ------------------------------------------------------------------ 5. filters

@pytest.mark.parametrize("force", ["direct", "global", "hash"])
def test_filters_that_empty_waves_tiles_and_blocks(ctx, env, force):
    """Rows 256 .. 511 (a wave's), 1024 .. 3071 (two whole tiles: the whole second block) and 3072 .. 3075 (a lane's) fail the
    filter; rows without a time value are dropped as rows_no_time and contribute nothing; the key has a bitmap."""
    n = 4096 + 100
    i = np.arange(n, dtype=np.int64)
    keep = ~(((i >= 256) & (i < 512)) | ((i >= 1024) & (i < 3072)) | ((i >= 3072) & (i < 3076)))
    tl = _cut({"k": (i % 7, i % 11 != 0), "keep": (keep.astype(np.int64), None), "v": ((i * 7919) % 1000, i % 5 != 0),
               "time": (i * 3, i % 13 != 0)}, {}, {}, (1024, 2048, n - 3072))
    t = build(ctx, tl, compact=True)
    try:
        env(path=force)
        out, ps, ref = _check(t, tl, True, force=force, groups=["k"], aggs=[("v", "n,min,max," + P3)], filters=[("keep", "eq", 1)],
                              time_col="time", time_bucket=5000)
        st = out.rollup_stats()
        assert st["rows_matched"] == int(keep.sum()) and st["rows_no_time"] > 0 and ref["bitmap"]["k"]
        assert ps["items"] == int(D.concat(ref["blocks"])["v_n"][1].sum()) < st["rows_matched"] - st["rows_no_time"]
        out.free()
    finally:
        t.free()


def test_a_filter_that_matches_nothing(main, env):
    t = main(True)
    # the first the planner proves (no kernel runs; the restatement does not model the proof), the second the kernels find
    for filters, proven in (([("f", "gt", I64_MAX)], True), ([("f", "gt", 5), ("f", "lt", 3)], False)):
        if proven:
            out = t.rollup(groups=["k1", "s"], aggs=[("v1", "max," + P3)], filters=filters)
            ps = out.rollup_pct_stats()
        else:
            out, ps, ref = _check(t, MAIN, True, groups=["k1", "s"], aggs=[("v1", "max," + P3)], filters=filters)
        try:
            assert (out.rows, out.blocks) == (0, 0) and (out.rollup_stats()["path"] == 0) == proven
            assert {k: ps[k] for k in PCT_COUNTS} == dict(columns=1, percentiles=3, variant32=0, variant64=0, variant_pairs=0, key_bits_max=0, items=0)
            assert out.samples(limit=1).columns == ["k1", "s", "count", "v1_max", "v1_p1", "v1_p50", "v1_p99"]
            assert out.column_storage("v1_p50") == (1, 0) and (ps["columns"], ps["percentiles"], ps["items"]) == (1, 3, 0)
        finally:
            out.free()


def test_rows_match_and_none_of_them_has_a_value(ctx, env):
    """The column has values, none in a row that passes: no sort runs, every percentile is unpopulated."""
    i = np.arange(400, dtype=np.int64)
    tl = _cut({"k": (i % 3, None), "f": (i % 10, None), "v": (i * 5, i % 10 != 3)}, {}, {}, (70, 330))
    t = build(ctx, tl, compact=True)
    try:
        out, ps, ref = _check(t, tl, True, groups=["k"], aggs=[("v", "n," + P3)], filters=[("f", "eq", 3)])
        assert out.rows == 3 and (ps["items"], ps["variant32"], ps["key_bits_max"]) == (0, 0, 0) and ref["bitmap"]["v_p50"]
        assert out.column_storage("v_p50") == (1, 0) and out.read_int("v_p50", 0, 3).tolist() == [0, 0, 0]
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 6. sort sizes

@pytest.mark.parametrize("pct", ["32", "64", "pairs"])
def test_300_items(ctx, env, pct):
    n = 300
    i = np.arange(n, dtype=np.int64)
    tl = _cut({"k": (i % 3, None), "v": ((i * 7919) % 1000 - 500, None)}, {}, {}, (1, 70, 33, n - 104))
    t = build(ctx, tl, compact=True)
    try:
        env(pct=pct)
        out, ps, ref = _check(t, tl, True, pct=pct, groups=["k"], aggs=[("v", "min,max," + P3)])
        assert ps["items"] == 300
        out.free()
    finally:
        t.free()


def test_300000_items_in_65536_row_blocks(ctx, env):
    """Beyond the sort's single-workgroup size, with 4- and with 8-byte keys (and the pairs variant), from 65536-row blocks."""
    n = 300000
    i = np.arange(n, dtype=np.int64)
    sizes = (65536, 65536, 65536, 65536, n - 4 * 65536)
    tl = _cut({"time": (1700000000 + i // 40, None), "host": ((i * 31) % 100, None), "lat": ((i * 7919 + i // 1000) % 5000, None)}, {}, {}, sizes)
    kw = dict(groups=["host"], aggs=[("lat", "n,min,max," + P3)], time_col="time", time_bucket=3600)
    ref = P.rollup_pct_ref(tl, compact=True, **kw)
    assert ref["pct_stats"]["variant32"] == 1 and ref["pct_stats"]["items"] == n and ref["stats"]["groups"] == 300
    t = build(ctx, tl, compact=True)
    outs = []
    try:
        for pct, variant in ((None, "variant32"), ("64", "variant64"), ("pairs", "variant_pairs")):
            env(pct=pct)
            want = dict(ref, pct_stats=dict(ref["pct_stats"], variant32=0))
            want["pct_stats"][variant] = 1
            out, ps, _ = _check(t, tl, True, path=LDS, ref=want, **kw)
            outs.append(out)
        for o in outs[1:]:
            _same_table(outs[0], o)
    finally:
        for o in outs:
            o.free()
        t.free()


# ------------------------------------------------------------------ 7. the output as a table

def test_two_calls_the_second_level_and_a_saved_table(ctx, main, env, oracle, tmp_path):
    t = main(True)
    kw = dict(groups=["v1"], aggs=[("v2", "n,p50,p99")])
    plain = a = b = back = None
    try:
        plain = t.rollup(groups=["v1"], aggs=[("v2", "n")])
        a, ps, ref = _check(t, MAIN, True, **kw)
        b = t.rollup(**kw)
        _same_table(a, b)                                              # determinism
        # the counts of rollup_stats are those of the same rollup without percentiles
        assert {k: plain.rollup_stats()[k] for k in COUNTS} == {k: a.rollup_stats()[k] for k in COUNTS}
        assert plain.rollup_pct_stats() == {k: 0 for k in ps}
        # second level: a histogram over the per-group p99 = the oracle fed the restatement's rows
        p99 = D.concat(ref["blocks"])["v2_p99"][1]
        q = dict(groups=[], aggs=["v2_p99"], op="hist", want_percentiles=True)
        matched = _against_oracle(oracle, a, ref["blocks"], ref["columns"], {}, q, {"v2_p99": (int(p99.min()), int(p99.max()))}, full=True)
        assert matched == a.rows == 200
        a.save(str(tmp_path))
        back = ctx.open_table(str(tmp_path), "events")
        assert (back.rows, back.blocks) == (a.rows, a.blocks) and _rows(back) == D.rows_of(ref["blocks"])
    finally:
        for tb in (back, a, b, plain):
            if tb is not None:
                tb.free()
