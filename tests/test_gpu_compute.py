"""GPU: table compute (Table.compute / sybl_table_compute, csrc/compute.hip) against the restatement in tests/compute_ref.py.
Tables are built block by block through append_block from the very block lists the restatement reads; the output is read back
whole with samples(limit=N) and read_int.  Every comparison is exact.

Shapes: a few thousand rows in blocks of 1, 70, 33, 2049, 31, 64, 777, 32 rows (repeating) -- padding rows, a one-row first
block, blocks on both sides of 32 and of the kernel's 1024-row tile --, blocks of 1023 / 1024 / 1025 rows, one 65536-row block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import compute_ref as R
from tests import digest_ref as D
from tests.test_gpu_concat import _against_oracle, _cut, _rows
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
T_SIZES = (1, 70, 33, 2049, 31, 64, 777, 32, 1, 70, 33)
N_T = sum(T_SIZES)
TILE = 2048        # csrc/plan.h: kTileRows, the slack table_reserve / valid_reserve keep behind a table's rows
CX_TILE = 1024     # csrc/compute.hip: kCxTileRows, the rows of one block a workgroup evaluates at a time


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


def _phys(blocks):
    sizes = [n for n, _ in blocks if n > 0]
    return sum((n + 31) // 32 * 32 for n in sizes[:-1]) + (sizes[-1] if sizes else 0)


def _check(t, tl, exprs, compact):
    """t.compute(exprs) against compute_ref: rows, blocks, stats, every row, and per computed column the type, has_missing, the
    exact extrema, the storage and the stored values of unpopulated rows.  Returns (table, stats, ref)."""
    ref = R.compute_ref(tl, exprs, compact=compact)
    n = ref["stats"]["rows"]
    before = (t.rows, t.blocks)
    out = t.compute(exprs)
    try:
        st = out.compute_stats()
        assert (out.rows, out.blocks) == (n, ref["stats"]["blocks"]) and (t.rows, t.blocks) == before
        assert {k: st[k] for k in ref["stats"]} == ref["stats"], st
        assert out.samples(limit=1).columns == list(D.column_types(tl)) + ref["computed"]
        assert _rows(out) == D.rows_of(ref["blocks"])
        cols = D.concat(ref["blocks"]) if n else {}
        for name in ref["computed"]:
            info = out.column_info(name)
            assert info["type"] == 1 and info["has_missing"] == ref["has_missing"][name], (name, info)
            assert (info["exact_min"], info["exact_max"]) == ref["extrema"][name], (name, info)
            assert out.column_storage(name) == ref["storage"][name], name
            if n:
                _, v, p = cols[name]
                # the stored bytes of an unpopulated row are 0: it reads as the column's base
                assert np.array_equal(out.read_int(name, 0, n), np.where(p, v, ref["storage"][name][1])), name
    except BaseException:
        out.free()
        raise
    return out, st, ref


# ------------------------------------------------------------------ 1. the main table: every stored width on both sides

def _main_table():
    rng = np.random.default_rng(33)
    n = N_T
    i = np.arange(n, dtype=np.int64)
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[3], w8[n - 2] = I64_MIN, I64_MAX
    last_of_2049 = sum(T_SIZES[:4]) - 1
    one = np.zeros(n, dtype=bool)
    one[last_of_2049] = True                                           # one populated row: the last before a block's padding
    half = np.ones(n, dtype=bool)
    first_of_2049 = sum(T_SIZES[:3])
    half[first_of_2049 + CX_TILE:first_of_2049 + 2 * CX_TILE] = False   # a whole tile of unpopulated rows between populated ones
    flat = {"w1": (1000 + (i * 37) % 200, None), "w2": (-3 + (i * 7) % 60000, None), "w4": (5 + (i * 100003) % (1 << 31), None),
            "w8": (w8, None), "w8b": (w8 ^ (i & 0x7F), None), "nb": (rng.integers(-500, 500, n).astype(np.int64), rng.random(n) > 0.3),
            "z": (rng.integers(-2, 3, n).astype(np.int64), rng.random(n) > 0.1), "none": (np.full(n, 77, dtype=np.int64), np.zeros(n, dtype=bool)),
            "one": (i + 1, one), "half": (i % 1000, half), "a.b": (i % 5, rng.random(n) > 0.5), "min": (i % 9 - 4, None)}
    strs = {"s": [("user%03d" % (k % 40) if k % 13 else None) for k in range(n)]}
    tags = {"tags": [(["tag%d" % (k % 3)] * (k % 3 + 1) if k % 5 else None) for k in range(n)]}
    return _cut(flat, strs, tags, T_SIZES)


MAIN = _main_table()


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


WIDTHS = [("d1", "w8 - w8b"), ("d4", "w4 - w2"), ("m8", "w1 * 1000000007"), ("r2", "w2 % 1000 * 60"), ("r1", "w4 % 200"), ("r4", "w1 * 100000"),
          ("x8", "w8 + 0"), ("n2", "nb * 60"), ("q1", "w8 / 9223372036854775807"), ("q2", "w2 - w1")]


@pytest.mark.parametrize("compact", [True, False])
def test_source_widths_against_result_widths(main, compact):
    """Sources stored at 1 / 2 / 4 / 8 bytes (compact) or 8 (canonical), results landing at 1 / 2 / 4 / 8 bytes: two wide columns
    whose difference fits a byte, a narrow one widened to 8 by a product, int64 extremes carried through."""
    t = main(compact)
    if compact:
        assert [t.column_storage(c)[0] for c in ("w1", "w2", "w4", "w8", "w8b", "nb")] == [1, 2, 4, 8, 8, 2]
    out, st, ref = _check(t, MAIN, WIDTHS, compact)
    try:
        if compact:
            assert [ref["storage"][c][0] for c, _ in WIDTHS] == [1, 4, 8, 2, 1, 4, 8, 2, 1, 2]
            assert ref["storage"]["r4"] == (4, 100000000) and ref["storage"]["x8"] == (8, 0)
        assert ref["extrema"]["x8"] == (I64_MIN, I64_MAX) and ref["has_missing"]["n2"] and not ref["has_missing"]["d1"]
        assert st["range_bytes"] > 0 and st["store_bytes"] > st["range_bytes"] and st["range_ms"] > 0 and st["store_ms"] > 0
        assert t.compute_stats() == {k: 0 for k in st}                 # zeros for a table no compute made
        assert out.concat_stats()["rows"] == 0 and out.lookup_stats()["rows"] == 0
    finally:
        out.free()


# ------------------------------------------------------------------ 2. populated or not

POPULATED = [("full", "w1 + 1"), ("gone", "w1 / 0"), ("gone2", "none + 1"), ("last", "one + 5"), ("tile", "half * 2"), ("zdiv", "w2 / z"),
             ("zmod", "w2 % z"), ("co", "coalesce(nb, 0 - 1)"), ("pick", "if(z, w1 / z, none)"), ("both", "nb && z || 1")]


@pytest.mark.parametrize("compact", [True, False])
def test_populated_bits_bitmaps_and_stored_zeros(main, compact):
    """Sources with and without bitmaps; a result with no unpopulated row (no bitmap), all unpopulated (width 1, base 0), one
    populated row that is the last before padding, a whole tile of unpopulated rows between populated ones, zero divisors."""
    t = main(compact)
    out, st, ref = _check(t, MAIN, POPULATED, compact)
    try:
        assert ref["has_missing"] == {"full": False, "gone": True, "gone2": True, "last": True, "tile": True, "zdiv": True, "zmod": True,
                                      "co": False, "pick": True, "both": True}
        assert ref["extrema"]["gone"] == (I64_MAX, I64_MIN) and ref["extrema"]["last"][0] == ref["extrema"]["last"][1]
        if compact:
            assert ref["storage"]["gone"] == ref["storage"]["gone2"] == (1, 0) and ref["storage"]["last"][0] == 1
    finally:
        out.free()
    # a bitmap exists iff some live row is unpopulated: seen through sybl_table_hbm_bytes, which counts bitmaps
    phys = _phys(MAIN)
    words = ((phys + TILE + 31) // 32 * 32) // 32 + 1
    a, b = t.compute([("v", "w1 + 1")]), t.compute([("v", "w1 + has(nb) / has(nb)")])
    try:
        assert a.column_storage("v")[0] == b.column_storage("v")[0] and not a.column_info("v")["has_missing"] and b.column_info("v")["has_missing"]
        assert b.hbm_bytes - a.hbm_bytes == words * 4
    finally:
        a.free()
        b.free()


# ------------------------------------------------------------------ 3. every op and function, the wraps and the division cases, from columns

EDGE_X = [7, -7, -7, 7, I64_MAX, I64_MIN, I64_MIN, 3037000500, 1, 0, 0, I64_MIN, I64_MAX, I64_MIN, -1, 5, 0, 9, I64_MAX, 2]
EDGE_Y = [-2, 2, 2, -2, 1, -1, -1, 3037000500, 0, 0, 5, I64_MIN, I64_MAX, I64_MAX, -1, 0, -3, 9, -1, I64_MIN]
EDGE_XP = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1]
EDGE_YP = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1]
EVERY_OP = [("o_div", "x / y"), ("o_mod", "x % y"), ("o_add", "x + y"), ("o_sub", "x - y"), ("o_mul", "x * y"), ("o_abs", "abs(x)"), ("o_neg", "-x"),
            ("o_not", "!x"), ("o_lt", "x < y"), ("o_le", "x <= y"), ("o_gt", "x > y"), ("o_ge", "x >= y"), ("o_eq", "x == y"), ("o_ne", "x != y"),
            ("o_and", "x && y"), ("o_or", "x || y"), ("o_min", "min(x, y)"), ("o_max", "max(x, y)"), ("o_if", "if(x, x / y, y)"),
            ("o_co", "coalesce(x / y, y)"), ("o_has", "has(x) + has(y) * 2"), ("o_lit", "x - x + -9223372036854775808 / -1"),
            ("o_litmod", "x - x + -9223372036854775808 % -1"), ("o_if0", "if(0, 1/0, 5) + x * 0"), ("o_ifu", "if(1/0, 1, 2) + x * 0"),
            ("o_and0", "(0 && 1/0) + x * 0"), ("o_co9", "coalesce(1/0, 9) + x * 0")]


@pytest.mark.parametrize("compact", [True, False])
def test_every_op_at_the_int64_edges(ctx, compact):
    n = len(EDGE_X)
    tl = _cut({"x": (np.array(EDGE_X, dtype=np.int64), np.array(EDGE_XP, dtype=bool)), "y": (np.array(EDGE_Y, dtype=np.int64), np.array(EDGE_YP, dtype=bool))},
              {}, {}, (1, n - 1))
    t = build(ctx, tl, compact=compact)
    try:
        out, st, ref = _check(t, tl, EVERY_OP, compact)
        cols = D.concat(ref["blocks"])
        assert cols["o_div"][1][:7].tolist() == [-3, -3, -3, -3, I64_MAX, I64_MIN, I64_MIN] and cols["o_mod"][1][:7].tolist() == [1, -1, -1, 1, 0, 0, 0]
        assert cols["o_add"][1][4] == I64_MIN and cols["o_mul"][1][7] == -9223372036709301616 and cols["o_abs"][1][5] == I64_MIN
        assert not cols["o_div"][2][8] and not cols["o_div"][2][9] and cols["o_has"][2].all()
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 4. the limits, chained expressions, has()

def test_eight_columns_64_ops_depth_8_and_chains(main):
    t = main(True)
    exprs = [("c8", "w1 + w2 + w4 + nb + z + min + `a.b` + half"),
             ("ops64", "-(" + "+".join(["w1", "w2"] * 16) + ")"),
             ("deep8", "w1+(w2+(w1+(w2+(w1+(w2+(w1+(w2)))))))"),
             ("lat", "w4 - w2"), ("slow", "lat > 100000000"), ("lat2", "lat * slow + c8 * 0")]
    assert [len(R.compile_expr(e, {c: "int" for c in D.column_types(MAIN)})[0]) for _, e in exprs[:3]] == [15, 64, 15]
    assert R.compile_expr(exprs[2][1], {c: "int" for c in D.column_types(MAIN)})[2] == 8
    out, st, ref = _check(t, MAIN, exprs, True)
    try:
        assert st["exprs"] == 6 and ref["storage"]["slow"] == (1, 0)
    finally:
        out.free()


@pytest.mark.parametrize("compact", [True, False])
def test_has_of_every_column_type(main, compact):
    exprs = [("hs", "has(s)"), ("ht", "has(tags)"), ("hi", "has(nb) + has(`a.b`) * 2 + has(none) * 4 + has(w1) * 8"), ("hh", "has(hs) + hs")]
    out, st, ref = _check(main(compact), MAIN, exprs, compact)
    try:
        assert ref["extrema"] == {"hs": (0, 1), "ht": (0, 1), "hi": (8, 11), "hh": (1, 2)} and st["unpopulated"] == 0
    finally:
        out.free()


# ------------------------------------------------------------------ 5. blocks around the kernel's tile, and one big block

@pytest.mark.parametrize("sizes", [(CX_TILE - 1, CX_TILE, CX_TILE + 1, 1), (CX_TILE + 1, 31, CX_TILE - 1), (65536,)])
def test_blocks_around_the_tile_and_a_65536_row_block(ctx, sizes):
    n = sum(sizes)
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.int64)
    tl = _cut({"start": (1700000000000 + i * 50, None), "end": (1700000000000 + i * 50 + (i * 37) % 500, rng.random(n) > 0.01),
               "status": (np.where(i % 13 == 0, 503, 200), None)}, {}, {}, sizes)
    t = build(ctx, tl, compact=True)
    try:
        out, st, ref = _check(t, tl, [("latency", "end - start"), ("is_error", "status >= 500"), ("hour", "start / 1000 % 86400 / 3600")], True)
        assert ref["storage"]["latency"] == (2, 0) and ref["storage"]["is_error"] == (1, 0) and ref["has_missing"]["latency"]
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 6. a table without rows; t stays as it was

@pytest.mark.parametrize("compact", [True, False])
def test_t_without_rows(ctx, compact):
    tl = [(0, {"k": ("int", np.zeros(0, dtype=np.int64), None), "x": ("int", np.zeros(0, dtype=np.int64), None)})]
    t = build(ctx, tl, compact=compact)
    try:
        out, st, ref = _check(t, tl, [("a", "k + 1"), ("b", "a * has(x)")], compact)
        assert (out.rows, out.blocks, st["range_ms"], st["store_ms"], st["stats_ms"], st["range_bytes"], st["store_bytes"]) == (0, 0, 0, 0, 0, 0, 0)
        assert st["exprs"] == 2 and st["ops"] == 6 and out.samples(limit=5).rows == []
        out.free()
    finally:
        t.free()


def _refused(t, words, exprs):
    """SYBL_E_INVAL with a message that begins `sybl_table_compute: ` and holds `words`; *out stays NULL."""
    import sybil_amd
    from sybil_amd import _native as N
    with pytest.raises(sybil_amd.SyblError) as ei:
        t.compute(exprs)
    msg = str(ei.value)
    assert ei.value.code == E_INVAL and msg.startswith("sybilgpu error -1: sybl_table_compute: "), msg
    assert all(w in msg for w in words), msg
    arr = (N.ComputeCol * max(len(exprs), 1))(*[N.ComputeCol(n.encode(), e.encode()) for n, e in exprs])
    d = N.ComputeDesc(len(exprs), C.cast(arr, C.POINTER(N.ComputeCol)))
    h = C.c_void_p(0xDEAD)
    assert N.lib().sybl_table_compute(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None


def test_every_refusal_names_the_column_and_leaves_t_as_it_was(main):
    from sybil_amd import _native as N
    t = main(True)
    q = t.query(groups=["min"], aggs=["w2"])

    def scan():
        res = q.scan().finalize()
        got = (res.matched, [(r["group_by_key"], r["count"]) for r in res.results])
        res.free()
        return got
    try:
        before = (scan(), t.rows, t.blocks, t.hbm_bytes)
        for words, exprs in ((["'w1'", "already holds"], [("w1", "1")]),                        # a column of t
                             (["'v'", "already holds"], [("v", "1"), ("v", "2")]),              # an earlier computed column
                             (["''", "empty name"], [("", "1")]),
                             (["n_exprs"], []),
                             (["'v'", "unknown column 'nope'", "at byte 5"], [("v", "w1 + nope")]),
                             (["'v'", "unknown column 'v'"], [("v", "v + 1")]),                  # itself
                             (["'u'", "unknown column 'v'"], [("u", "v + 1"), ("v", "1")]),     # a later one
                             (["'v'", "'s'", "str column"], [("v", "s + 1")]),
                             (["'v'", "'tags'", "set column"], [("ok", "has(tags)"), ("v", "tags")]),
                             (["'v'", "at byte 4"], [("v", "w1 +")]),
                             (["'v'", "at byte 3"], [("v", "w1 & 1")]),
                             (["'v'", "argument count"], [("v", "min(w1)")]),
                             (["'v'", "argument count"], [("v", "if(w1, 1)")]),
                             (["'v'", "unknown function 'sum'"], [("v", "sum(w1)")]),
                             (["'v'", "literal above 2^63", "at byte 0"], [("v", "9223372036854775809")]),
                             (["'v'", "8 distinct columns"], [("v", "w1+w2+w4+w8+w8b+nb+z+none+one")]),
                             (["'v'", "64 ops"], [("v", "+".join(["w1"] * 33))]),
                             (["'v'", "stack deeper than 8"], [("v", "1+(1+(1+(1+(1+(1+(1+(1+(1" + ")" * 8)]),
                             (["'v'", "nested deeper than 64"], [("v", "(" * 65 + "1" + ")" * 65)])):
            _refused(t, words, exprs)
        d = N.ComputeDesc()
        h = C.c_void_p(0xDEAD)
        d.n_exprs = 1
        assert N.lib().sybl_table_compute(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None      # exprs NULL
        assert N.lib().sybl_last_error().startswith(b"sybl_table_compute: NULL")
        arr = (N.ComputeCol * 1)(N.ComputeCol(b"v", None))
        d.exprs = C.cast(arr, C.POINTER(N.ComputeCol))
        assert N.lib().sybl_table_compute(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None      # expr NULL
        assert N.lib().sybl_last_error().startswith(b"sybl_table_compute: NULL")
        arr[0] = N.ComputeCol(None, b"1")
        assert N.lib().sybl_table_compute(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None      # name NULL
        assert N.lib().sybl_last_error().startswith(b"sybl_table_compute: NULL")
        assert (scan(), t.rows, t.blocks, t.hbm_bytes) == before         # no version moved: no SYBL_E_STATE
        out = t.compute({"v": "w1 + 1", "u": "v * 2"})                   # a dict, in insertion order; nor by a compute that succeeds
        assert out.samples(limit=1).columns[-2:] == ["v", "u"]
        assert (scan(), t.rows, t.blocks, t.hbm_bytes) == before
        out.free()
    finally:
        q.free()


# ------------------------------------------------------------------ 7. the output is a table like any other

@pytest.mark.parametrize("compact", [True, False])
def test_queries_over_computed_columns_agree_with_the_oracle(ctx, oracle, compact):
    """A group-by on a computed key and a histogram over a computed value: the compute's output against the same rows built by
    hand through append_block, and both against the oracle."""
    rng = np.random.default_rng(4)
    n = N_T
    i = np.arange(n, dtype=np.int64)
    start = 1700000000 + i * 41
    dur = rng.integers(0, 1000, n).astype(np.int64)
    dur[0], dur[1] = 0, 999                                              # (the exact extrema, whatever the draw)
    tl = _cut({"start": (start, None), "end": (start + dur, rng.random(n) > 0.03), "status": (rng.choice([200, 404, 500, 503], n).astype(np.int64), None)},
              {}, {}, T_SIZES)
    tl[0][1]["end"][2][0], tl[1][1]["end"][2][0] = True, True
    t = build(ctx, tl, compact=compact)
    out, hand = None, None
    try:
        out, st, ref = _check(t, tl, [("lat", "end - start"), ("is_error", "status >= 500"), ("hour", "start % 86400 / 3600")], compact)
        hand = build(ctx, ref["blocks"], compact=compact)
        names = [("start", "int"), ("end", "int"), ("status", "int"), ("lat", "int"), ("is_error", "int"), ("hour", "int")]
        got = []
        for tb in (out, hand):
            for q in (dict(groups=["is_error", "hour"], aggs=["lat"], op="hist", want_percentiles=True), dict(groups=["is_error"], aggs=["lat"], op="avg")):
                got.append(_against_oracle(oracle, tb, ref["blocks"], names, {}, q, {"lat": (0, 999)}, full=q["op"] == "hist"))
        assert got == [n] * 4
    finally:
        for tb in (out, hand, t):
            if tb is not None:
                tb.free()


def test_compute_then_select_and_save_and_open(ctx, main, tmp_path):
    t = main(True)
    exprs = [("lat", "w4 - w2"), ("bucket", "if(has(nb), nb / 100, 0 - 9)")]
    out, st, ref = _check(t, MAIN, exprs, True)
    sel, back = None, None
    try:
        sel = out.select(filters=[("bucket", "eq", -9)], columns=["w1", "bucket", "lat"])
        want = [{k: r[k] for k in ("w1", "bucket", "lat") if k in r} for r in D.rows_of(ref["blocks"]) if r.get("bucket") == -9]
        assert 0 < len(want) < N_T and _rows(sel) == want
        out.save(str(tmp_path))
        back = ctx.open_table(str(tmp_path), "events")
        assert back.rows == out.rows and back.blocks == out.blocks and _rows(back) == D.rows_of(ref["blocks"])
    finally:
        for tb in (back, sel, out):
            if tb is not None:
                tb.free()


def test_c_example_runs(ctx, tmp_path):
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    exe = str(tmp_path / "example_compute")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "example_compute.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    text = p.stdout.decode()
    assert text.startswith("3000 rows in 3 blocks, 2 expressions of 6 ops, 33 unpopulated results; latency is stored at 2 byte(s)"), text
