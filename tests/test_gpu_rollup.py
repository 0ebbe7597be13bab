"""GPU: table rollup (Table.rollup / sybl_table_rollup, csrc/rollup.hip) against the restatement in tests/rollup_ref.py.
Tables are built block by block through append_block from the very block lists the restatement reads; the output is read
back whole with samples(limit=G) and read_int.  Every comparison is exact.

Shapes: a few thousand rows in blocks of 1, 70, 33, 2049, 31, 64, 777, 32 rows (repeating) -- padding rows, a one-row first
block, blocks on both sides of 32 and of a 1024-row tile --; one case has a 65536-row block, one 20000 rows where the path rule
needs 4 x rows > 2^16."""
import numpy as np
import pytest

from tests import digest_ref as D
from tests import parity
from tests import rollup_ref as U
from tests.test_gpu_concat import _against_oracle, _cut, _ocols, _rows
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

E_INVAL, E_NOMEM = -1, -3
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
T_SIZES = (1, 70, 33, 2049, 31, 64, 777, 32, 1, 70, 33)
N_T = sum(T_SIZES)
LDS, GLOBAL, HASH = U.LDS, U.GLOBAL, U.HASH
ALL = "n,sum,min,max"
COUNTS = ("rows_in", "rows_matched", "rows_no_time", "groups", "blocks_out", "path", "fields", "cells_or_slots")


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
    def set_(path=None, slots=None, merge=None):
        for name, v in (("SYBL_ROLLUP_PATH", path), ("SYBL_ROLLUP_SLOTS", slots), ("SYBL_ROLLUP_MERGE", merge)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    set_()
    return set_


def _check(t, tl, compact, path=None, force=None, slots=0, rows=True, ref=None, rolled=False, **kw):
    """t.rollup(**kw) against rollup_ref: counts, columns, every row, storage, bitmaps, dictionaries, extrema, the stored values
    of unpopulated rows, the untouched source.  ref: the restatement's result where the caller has it; rolled: t is itself a
    rollup's output (its own stats are then not zeros: they stay what they were).  Returns (table, stats, ref)."""
    if ref is None:
        ref = U.rollup_ref(tl, compact=compact, force=force, slots=slots, **kw)
    G = ref["stats"]["groups"]
    before = (t.rows, t.blocks)
    own = t.rollup_stats()
    out = t.rollup(**kw)
    try:
        st = out.rollup_stats()
        assert {k: st[k] for k in COUNTS} == ref["stats"], (st, ref["stats"])
        if path is not None:
            assert st["path"] == path, st
        assert (out.rows, out.blocks) == (G, len(ref["blocks"])) and (t.rows, t.blocks) == before
        assert t.rollup_stats() == (own if rolled else {k: 0 for k in st})      # zeros for a table no rollup made
        assert out.samples(limit=1).columns == [c for c, _ in ref["columns"]]
        if rows:
            assert _rows(out) == D.rows_of(ref["blocks"])
        cols = D.concat(ref["blocks"]) if G else {}
        src_types = D.column_types(tl)
        keys = [g for g in kw.get("groups", ())]
        for name, ty in ref["columns"]:
            info = out.column_info(name)
            assert info["type"] == {"int": 1, "str": 2}[ty] and info["has_missing"] == ref["bitmap"][name], (name, info)
            if name in keys:
                assert out.column_storage(name) == t.column_storage(name), name     # the source's (width, base)
                assert ty == src_types[name]
            else:
                assert out.column_storage(name) == ref["storage"][name], (name, out.column_storage(name), ref["storage"][name])
            if ty == "str":
                assert out.column_dict(name) == ref["dicts"][name] == t.column_dict(name), name
            if not G:
                continue
            _, v, p = cols[name]
            if ty == "int":
                base = out.column_storage(name)[1]
                # the stored bytes of an unpopulated row are 0: it reads as the column's base
                assert np.array_equal(out.read_int(name, 0, G), np.where(p, v, base)), name
                want = (int(v[p].min()), int(v[p].max())) if p.any() else (I64_MAX, I64_MIN)
            else:
                ids = [ref["dicts"][name].index(s) for s in v if s is not None]
                want = (min(ids), max(ids)) if ids else (I64_MAX, I64_MIN)
            assert (info["exact_min"], info["exact_max"]) == want, (name, info)      # folded from the block statistics
        if G:
            assert st["accumulate_bytes"] > 0 and st["order_bytes"] > 0 and st["emit_bytes"] > 0
    except BaseException:
        out.free()
        raise
    return out, st, ref


# ------------------------------------------------------------------ 1. every kind of column, both storage modes, every path

def _main_blocks():
    rng = np.random.default_rng(33)
    n = N_T
    i = np.arange(n, dtype=np.int64)
    time = -9000 + (i * 11) % 20000                                   # hours -2 .. 3 with truncation toward zero
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[5], w8[n - 7], w8[n // 2] = I64_MIN, I64_MAX, I64_MAX
    flat = {"time": (time, rng.random(n) > 0.03), "k1": (-1 + (i * 7) % 5, None), "k2": (1000 + (i % 3) * 30000, rng.random(n) > 0.1),
            "k4": ((i % 4) * (1 << 20), None), "k8": ((i % 3) * (1 << 40) - 5, None),
            "v1": (100 + (i * 37) % 200, None), "v2": (-3 + (i * 7) % 60000, None), "v4": (5 + (i * 100003) % (1 << 31), None),
            "v8": (w8, None), "nb": (rng.integers(-500, 500, n).astype(np.int64), rng.random(n) > 0.6),
            "none": (np.full(n, 77, dtype=np.int64), np.zeros(n, dtype=bool)), "f": (i % 10, None)}
    strs = {"s": [("host%02d" % (k % 6) if k % 17 else None) for k in range(n)]}
    tags = {"tags": [["a"] if k % 2 else None for k in range(n)]}
    return _cut(flat, strs, tags, T_SIZES)


MAIN = _main_blocks()
MAIN_AGGS = [("v1", ALL), ("v2", ALL), ("v4", ALL), ("v8", ALL), ("nb", ALL), ("none", ALL)]


@pytest.fixture(scope="module")
def main(ctx):
    made = {}

    def get(compact):
        if compact not in made:
            made[compact] = build(ctx, MAIN, compact=compact, name="main")
        return made[compact]
    yield get
    for tb in made.values():
        tb.free()


@pytest.mark.parametrize("force,path", [(None, LDS), ("direct", LDS), ("global", GLOBAL), ("hash", HASH)])
@pytest.mark.parametrize("compact", [True, False])
def test_every_column_kind_by_time_int_and_str_keys(main, env, compact, force, path):
    """Hourly x an int key with key -1 x a str key with MISSING; value columns at stored widths 1 / 2 / 4 / 8 (compact) and 8
    (canonical), INT64_MIN / INT64_MAX as values and a wrapped sum, a column with a bitmap, an all-unpopulated column;
    negative times, unpopulated times dropped and counted."""
    env(path=force)
    t = main(compact)
    if compact:
        assert [t.column_storage(c)[0] for c in ("k1", "k2", "k4", "k8", "s", "v1", "v2", "v4", "v8", "none")] == [1, 2, 4, 8, 1, 1, 2, 4, 8, 1]
    out, st, ref = _check(t, MAIN, compact, path=path, force=force, groups=["k1", "s"], aggs=MAIN_AGGS, time_col="time", time_bucket=3600)
    try:
        assert st["rows_no_time"] > 0 and st["fields"] == 25 and ref["bitmap"]["s"] and ref["bitmap"]["nb_sum"] and ref["bitmap"]["none_max"]
        assert not ref["bitmap"]["v8_sum"] and not ref["bitmap"]["none_n"]
        tb = {n: v for n, (_, v, p) in D.concat(ref["blocks"]).items()}
        assert I64_MIN in tb["v8_min"].tolist() and I64_MAX in tb["v8_max"].tolist() and min(tb["time"].tolist()) == -7200
        if compact:
            assert ref["storage"]["none_sum"] == (1, 0) and ref["storage"]["v8_min"] == (8, 0) and ref["storage"]["time"] == (2, -7200)
            assert sorted({ref["storage"][c][0] for c in ref["storage"]}) == [1, 2, 4, 8]     # _sum columns at every width among them
            assert {ref["storage"][c][0] for c in ("v1_sum", "v2_sum", "v4_sum", "v8_sum")} >= {2, 4, 8}
    finally:
        out.free()


@pytest.mark.parametrize("groups,aggs,force,path", [
    (["k1"], [("v1", "sum")], None, LDS), (["k1"], [("v1", "sum")], "global", GLOBAL), (["k1"], [("v1", "sum")], "hash", HASH),
    (["k2"], [("v2", "max,n")], None, GLOBAL), (["k2", "k4"], [("v2", "max,n")], None, HASH), (["k8"], [("v4", "min")], None, HASH), (["k4", "k2", "k1", "s"], [], None, HASH), (["v1"], [("f", "sum")], None, LDS),
    (["s"], [("nb", ALL)], None, LDS), (["k4", "k2"], {"v8": "sum", "v1": "sum"}, "hash", HASH)])
@pytest.mark.parametrize("compact", [True, False])
def test_key_columns_at_every_stored_width(main, env, compact, groups, aggs, force, path):
    """Key columns stored at 1 / 2 / 4 / 8 bytes, one to four of them, a bitmap on an int key (k2) and on a str key; _sum columns
    that fit 1, 2, 4 and 8 bytes; bucket 1 on the time column in one of them."""
    env(path=force)
    out, st, ref = _check(main(compact), MAIN, compact, path=path, force=force, groups=groups, aggs=aggs)
    out.free()


def test_time_bucket_one_and_other_time_column(main, env):
    out, st, ref = _check(main(True), MAIN, True, groups=[], aggs=[("v1", "n")], time_col="k1", time_bucket=1, count_name="rows")
    try:
        assert st["groups"] == 5 and ref["columns"][0] == ("k1", "int") and ref["columns"][1] == ("rows", "int")
    finally:
        out.free()
    out, st, ref = _check(main(False), MAIN, False, groups=["f"], time_col=None, time_bucket=3600, filters=[("f", "lt", 3)])
    out.free()


# ------------------------------------------------------------------ 2. the default path on both sides of each rule

def _span_blocks(rows, span, lo=-12345, sizes=None, with_v=False):
    rng = np.random.default_rng(rows + span)
    k = lo + rng.integers(0, span, rows).astype(np.int64)
    k[0], k[-1] = lo, lo + span - 1
    flat = {"k": (k, None)}
    if with_v:
        flat["v"] = (np.arange(rows, dtype=np.int64) * 3 - 50, None)
    return _cut(flat, {}, {}, sizes or (33, rows - 33))


@pytest.mark.parametrize("rows,span,aggs,path", [
    (100, 1 << 16, (), GLOBAL), (100, (1 << 16) + 1, (), HASH), (20000, 80000, (), GLOBAL), (20000, 80001, (), HASH),
    (100, 8192, (), LDS), (100, 8193, (), GLOBAL), (100, 1638, (("v", ALL),), LDS), (100, 1639, (("v", ALL),), GLOBAL)])
def test_default_path_rule(ctx, env, rows, span, aggs, path):
    """direct iff product <= max(2^16, 4 x live rows); the LDS body iff cells x fields x 8 B <= 64 KiB."""
    tl = _span_blocks(rows, span, with_v=bool(aggs))
    t = build(ctx, tl, compact=True)
    try:
        out, st, ref = _check(t, tl, True, path=path, groups=["k"], aggs=list(aggs))
        assert st["cells_or_slots"] == (span if path != HASH else max(64, 1 << (2 * rows - 1).bit_length()))
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 3. the hash table

def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def test_a_64_slot_table_whose_chains_wrap(ctx, env):
    """Seven keys whose home slot is 62 or 63 of 64: their chain runs over the end of the table into slots 0 ..; 20 keys elsewhere."""
    home = lambda c: (_splitmix64(c) >> 32) & 63
    late = [c for c in range(1, 200000) if home(c) >= 62][:7]
    rest = [c for c in range(1, 400) if 8 <= home(c) < 56][:20]
    keys = np.array([0] + late + rest + late[:3] + [199999], dtype=np.int64) + 1000     # composite = value - 1000
    assert len(keys) == 32
    tl = _cut({"k": (keys, None), "v": (np.arange(32, dtype=np.int64), None)}, {}, {}, (1, 31))
    t = build(ctx, tl, compact=True)
    try:
        env(path="hash")
        out, st, ref = _check(t, tl, True, path=HASH, force="hash", groups=["k"], aggs=[("v", ALL)])
        assert st["cells_or_slots"] == 64 and st["groups"] == 29
        out.free()
    finally:
        t.free()


def test_a_table_that_fills_is_an_error(ctx, env):
    import sybil_amd
    tl = _cut({"k": (np.arange(33, dtype=np.int64) * 1000, None)}, {}, {}, (33,))
    t = build(ctx, tl, compact=True)
    try:
        env(path="hash", slots=32)
        with pytest.raises(sybil_amd.SyblError) as ei:
            t.rollup(groups=["k"])
        assert ei.value.code == E_NOMEM and "sybl_table_rollup: " in str(ei.value) and "32 slots" in str(ei.value)
        tl32 = _cut({"k": (np.arange(32, dtype=np.int64) * 1000, None)}, {}, {}, (32,))
        t32 = build(ctx, tl32, compact=True)
        try:
            out, st, _ = _check(t32, tl32, True, path=HASH, force="hash", slots=32, groups=["k"])     # exactly full: every key finds a slot
            out.free()
        finally:
            t32.free()
    finally:
        t.free()


def test_a_key_range_of_2_61_and_the_refusals_beyond_2_62(ctx, env):
    import sybil_amd
    n = 200
    i = np.arange(n, dtype=np.int64)
    big = np.where(i % 2 == 0, i, (1 << 61) - 1 - i)
    big[1] = (1 << 61) - 1
    for vals, ok in ((big, True), (np.where(i % 2 == 0, i, (1 << 62) + i), False), (np.where(i % 2 == 0, I64_MIN, I64_MAX), False)):
        tl = _cut({"k": (vals.astype(np.int64), None), "v": (i, None)}, {}, {}, (70, 130))
        for compact in (True, False):
            t = build(ctx, tl, compact=compact)
            try:
                if ok:
                    out, st, ref = _check(t, tl, compact, path=HASH, groups=["k"], aggs=[("v", "sum")])
                    assert ref["product"] == 1 << 61
                    out.free()
                else:
                    for force in (None, "hash"):
                        env(path=force)
                        with pytest.raises(sybil_amd.SyblError) as ei:
                            t.rollup(groups=["k"])
                        assert ei.value.code == E_INVAL and "sybl_table_rollup: " in str(ei.value) and "2^62" in str(ei.value)
                    env()
            finally:
                t.free()


# ------------------------------------------------------------------ 4. contention shapes

def _shape_keys(kind, n):
    i = np.arange(n, dtype=np.int64)
    if kind == "one":
        return np.zeros(n, dtype=np.int64)
    if kind == "alternating":
        return i % 2
    if kind == "each":
        return i
    # runs of equal keys that end at rows 63 / 64 / 65 of a wave's 256 rows, at a lane's four-row boundary and one row either
    # side of it, and at the wave and tile boundaries
    ends = sorted({3, 4, 5, 63, 64, 65, 127, 128, 255, 256, 257, 256 + 63, 256 + 64, 256 + 65, 1023, 1024, 1025, 1024 + 64, 2047, 2048, 2300})
    return np.searchsorted(np.array(ends), i, side="right").astype(np.int64)


@pytest.mark.parametrize("merge", [None, "0"])
@pytest.mark.parametrize("force,path", [("direct", LDS), ("global", GLOBAL), ("hash", HASH)])
@pytest.mark.parametrize("kind", ["one", "alternating", "runs", "each"])
def test_contention_shapes(ctx, env, kind, force, path, merge):
    """Every row in one group; two alternating keys; runs that end around wave, lane and tile boundaries; every row its own
    group (G = N) -- in the LDS body, the global body and the hash body, with the wave-uniform merge and without."""
    n = 2500
    k = _shape_keys(kind, n)
    v = (np.arange(n, dtype=np.int64) * 7919) % 1000 - 500
    tl = _cut({"k": (k, None), "v": (v, np.arange(n) % 5 != 0)}, {}, {}, (2049, 31, 420))
    t = build(ctx, tl, compact=True)
    try:
        env(path=force, merge=merge)
        if kind == "each" and force == "direct":
            path = GLOBAL                                              # 2500 cells x 5 fields do not fit 64 KiB
        out, st, ref = _check(t, tl, True, path=path, force=force, groups=["k"], aggs=[("v", ALL)])
        assert st["groups"] == {"one": 1, "alternating": 2, "each": n}.get(kind, st["groups"])
        out.free()
    finally:
        t.free()


@pytest.mark.parametrize("force", ["direct", "global", "hash"])
def test_whole_waves_and_whole_tiles_filtered_out(ctx, env, force):
    n = 4096 + 100
    i = np.arange(n, dtype=np.int64)
    keep = ~(((i >= 256) & (i < 512)) | ((i >= 1024) & (i < 2048)) | ((i >= 3072) & (i < 3076)))
    tl = _cut({"k": (i % 7, None), "keep": (keep.astype(np.int64), None), "v": (i, None)}, {}, {}, (n,))
    t = build(ctx, tl, compact=True)
    try:
        env(path=force)
        out, st, ref = _check(t, tl, True, force=force, groups=["k"], aggs=[("v", "sum,n")], filters=[("keep", "eq", 1)])
        assert st["rows_matched"] == int(keep.sum()) and st["filter_bytes"] > 0
        out.free()
    finally:
        t.free()


def test_a_65536_row_block(ctx, env):
    n = 65536 + 70
    i = np.arange(n, dtype=np.int64)
    tl = _cut({"time": (1700000000 + i // 8, None), "host": ((i * 31) % 100, None), "lat": ((i * 37) % 500, None)}, {}, {}, (65536, 70))
    t = build(ctx, tl, compact=True)
    try:
        for force, path in ((None, LDS), ("global", GLOBAL), ("hash", HASH)):
            env(path=force)
            out, st, ref = _check(t, tl, True, path=path, force=force, groups=["host"], aggs=[("lat", "sum,max")], time_col="time", time_bucket=3600)
            assert st["groups"] == 300 and st["rows_matched"] == n
            out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 5. the shape of the output

def test_block_rows_no_key_and_nothing_matches(main, env):
    t = main(True)
    G = U.rollup_ref(MAIN, groups=["k1", "k2"])["stats"]["groups"]
    assert G == 20
    for br in (1, 33, G - 1, G, G + 1):
        out, st, ref = _check(t, MAIN, True, groups=["k1", "k2"], aggs=[("v1", "sum")], block_rows=br)
        assert st["blocks_out"] == (G + br - 1) // br
        out.free()
    out, st, ref = _check(t, MAIN, True, aggs=[("v8", ALL), ("none", "sum")])                       # no key: one row
    assert st["groups"] == 1 and st["path"] == LDS and st["cells_or_slots"] == 1
    out.free()
    # nothing can match: the columns and no blocks.  The first the planner proves (no kernel runs), the second the kernels find
    for filters, proven in (([("f", "gt", I64_MAX)], True), ([("f", "gt", 5), ("f", "lt", 3)], False)):
        for groups in ([], ["k1", "s"]):
            out = t.rollup(groups=groups, aggs=[("v1", ALL)], filters=filters)
            try:
                ref = U.rollup_ref(MAIN, groups=groups, aggs=[("v1", ALL)], filters=filters, compact=True)
                st = out.rollup_stats()
                assert (out.rows, out.blocks, st["groups"], st["rows_in"], st["rows_matched"]) == (0, 0, 0, N_T, 0)
                assert (st["path"] == 0) == proven
                assert out.samples(limit=1).columns == [c for c, _ in ref["columns"]]
                assert [out.column_storage(c) for c in ("count", "v1_sum")] == [(1, 0), (1, 0)]
                if groups:
                    assert out.column_storage("s") == t.column_storage("s") and out.column_dict("s") == t.column_dict("s")
            finally:
                out.free()


def test_the_same_call_twice_gives_identical_columns(main, env):
    t = main(True)
    for force in ("hash", None):
        env(path=force)
        a = t.rollup(groups=["v1", "s"], aggs=MAIN_AGGS)
        b = t.rollup(groups=["v1", "s"], aggs=MAIN_AGGS)
        assert a.rollup_stats()["path"] == (HASH if force else GLOBAL)
        try:
            G = a.rows
            assert G == b.rows > 10 and a.blocks == b.blocks
            names = a.samples(limit=1).columns
            assert names == b.samples(limit=1).columns
            for name in names:
                assert a.column_storage(name) == b.column_storage(name) and a.column_info(name) == b.column_info(name), name
                if name != "s":
                    assert np.array_equal(a.read_int(name, 0, G), b.read_int(name, 0, G)), name
            assert _rows(a) == _rows(b)
        finally:
            a.free()
            b.free()


def test_refusals(main, env):
    import sybil_amd
    t = main(True)
    cases = [(dict(groups=["tags"]), "tags"), (dict(groups=["nope"]), "nope"), (dict(groups=["k1", "k1"]), "k1"),
             (dict(groups=["k1", "k2", "k4", "k8", "s"]), "4"), (dict(aggs=[("s", "sum")]), "'s'"), (dict(aggs=[("nope", "sum")]), "nope"),
             (dict(aggs=[("v1", "avg")]), "avg"), (dict(aggs=[("v1", "")]), "v1"), (dict(aggs=[("v1", "sum,sum")]), "sum,sum"),
             (dict(aggs=[("v%d" % w, "n") for w in (1, 2, 4, 8)] * 2 + [("nb", "n")]), "8"),
             (dict(time_bucket=-1), "time_bucket"), (dict(time_bucket=60, time_col="s"), "'s'"), (dict(time_bucket=60, time_col="nope"), "nope"),
             (dict(time_bucket=60, groups=["time"]), "time"), (dict(groups=["k1"], count_name="k1"), "k1"),
             (dict(aggs=[("v1", "sum")], count_name="v1_sum"), "v1_sum"), (dict(aggs=[("v1", "sum"), ("v1", "sum")]), "v1_sum"),
             (dict(block_rows=-1), "block_rows"), (dict(block_rows=65537), "block_rows"),
             (dict(filters=[("nope", "eq", 1)]), "nope")]
    for kw, word in cases:
        with pytest.raises(sybil_amd.SyblError) as ei:
            t.rollup(**kw)
        assert ei.value.code == E_INVAL and "sybl_table_rollup: " in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
    env(path="direct")
    tl = _span_blocks(100, (1 << 27) + 1)
    big = build(ctx_of(t), tl, compact=True)
    try:
        with pytest.raises(sybil_amd.SyblError) as ei:
            big.rollup(groups=["k"])
        assert ei.value.code == E_INVAL and "2^27" in str(ei.value)
    finally:
        big.free()
    env(path="sideways")
    with pytest.raises(sybil_amd.SyblError) as ei:
        t.rollup(groups=["k1"])
    assert ei.value.code == E_INVAL and "SYBL_ROLLUP_PATH" in str(ei.value)
    assert t.rows == N_T


def ctx_of(table):
    return table.ctx


# ------------------------------------------------------------------ 6. against the oracle

def test_two_level_and_conservation_against_the_oracle(main, oracle):
    t = main(True)
    # two-level: the histogram of `count` over a rollup by one key = the oracle fed the restatement's rows
    out, st, ref = _check(t, MAIN, True, groups=["v1"])
    try:
        counts = D.concat(ref["blocks"])["count"][1]
        q = dict(groups=[], aggs=["count"], op="hist", want_percentiles=True)
        matched = _against_oracle(oracle, out, ref["blocks"], ref["columns"], {}, q, {"count": (int(counts.min()), int(counts.max()))}, full=True)
        assert matched == st["groups"] == 200
    finally:
        out.free()
    # conservation: a query of the rollup by (k1, k4) grouped by k1 and weighted by count gives the Counts of the oracle's query
    # over the SOURCE rows
    out, st, ref = _check(t, MAIN, True, groups=["k1", "k4"], aggs=[("v1", "sum")])
    try:
        query = out.query(groups=["k1"], aggs=["v1_sum"], weight_col="count")
        try:
            gres = query.run()
            names = [("k1", "int"), ("v1", "int")]
            okw = parity.oracle_query_kwargs([c for c, _ in names], {"v1": (100, 299)}, dict(groups=["k1"], aggs=["v1"]))
            ores = oracle.run_query(_ocols(MAIN, names, {}), n_threads=4, **okw)
            got = {r["key"]: r["count"] for r in gres.rows(0)}
            want = {r["key"]: r["count"] for r in ores["results"]}
            assert got == want and sum(want.values()) == N_T and len(want) == 5
            gres.free()
        finally:
            query.free()
    finally:
        out.free()
