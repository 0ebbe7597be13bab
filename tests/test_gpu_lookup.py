"""GPU: table lookup (Table.lookup / sybl_table_lookup, csrc/lookup.hip) against the restatement in tests/lookup_ref.py.
Tables are built block by block through append_block from the very block lists the restatement reads; the output is read
back whole with samples(limit=N) and read_int.  Every comparison is exact.

Shapes: t has a few thousand rows in blocks of 1, 70, 33, 2049, 31, 64, 777, 32 rows (repeating) -- padding rows, a one-row
first block, blocks on both sides of 32 and of 2048 --, one case has a 65536-row block; dim has 0, 1, 31, 33 or 5000 rows
(and 20000 where the path rule needs 4 x rows > 2^16)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import digest_ref as D
from tests import lookup_ref as L
from tests import sybil_fixture as F
from tests.test_gpu_concat import _against_oracle, _cut, _rows
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_NOMEM = -1, -3
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
T_SIZES = (1, 70, 33, 2049, 31, 64, 777, 32, 1, 70, 33)
N_T = sum(T_SIZES)
DIRECT, HASH, STR = 1, 2, 3
TILE = 2048   # csrc/plan.h: kTileRows, the slack table_reserve / valid_reserve keep behind a table's rows


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
    """Sets the two diagnostic switches for one test (the library reads them at call time)."""
    def set_(path=None, slots=None):
        for name, v in (("SYBL_LOOKUP_PATH", path), ("SYBL_LOOKUP_SLOTS", slots)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    set_()
    return set_


def _phys(blocks):
    sizes = [n for n, _ in blocks if n > 0]
    return sum((n + 31) // 32 * 32 for n in sizes[:-1]) + (sizes[-1] if sizes else 0)


def _wrap(x):
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def _check(t, tl, dim, dl, key, compact, path=None, **kw):
    """t.lookup(dim, key, **kw) against lookup_ref: rows, blocks, counts, every row, storage, dictionaries, column info, the
    stored values of unpopulated rows.  Returns (table, stats, ref)."""
    ref = L.lookup_ref(tl, dl, key, compact=compact, **kw)
    n = sum(b[0] for b in ref["blocks"])
    before = (t.rows, t.blocks, dim.rows, dim.blocks)
    out = t.lookup(dim, key, **kw)
    try:
        st = out.lookup_stats()
        assert (out.rows, out.blocks) == (n, len(ref["blocks"])) and (t.rows, t.blocks, dim.rows, dim.blocks) == before
        assert (st["rows"], st["blocks"], st["columns"], st["dim_rows"]) == (n, len(ref["blocks"]), len(ref["attached"]), sum(b[0] for b in dl)), st
        if path is not None:
            assert st["path"] == path, st
        if st["path"]:
            assert (st["matched"], st["dim_keys"], st["dim_duplicates"]) == (ref["matched"], ref["dim_keys"], ref["dim_duplicates"]), st
        else:
            assert st["matched"] == ref["matched"] == 0
        assert out.samples(limit=1).columns == list(D.column_types(tl)) + [c for c, _ in ref["attached"]]
        assert _rows(out) == D.rows_of(ref["blocks"])
        cols = D.concat(ref["blocks"]) if n else {}
        for name, ty in ref["attached"]:
            info = out.column_info(name)
            assert info["type"] == {"int": 1, "str": 2, "set": 3}[ty] and info["has_missing"] == ref["bitmap"][name], (name, info)
            if ty != "int":
                assert out.column_dict(name) == ref["dicts"][name], name
            if ty == "set":
                continue
            assert out.column_storage(name) == ref["storage"][name], name
            if not n:
                continue
            _, v, p = cols[name]
            if ty == "int":
                base = ref["storage"][name][1]
                # the stored bytes of an unpopulated row are 0: it reads as the column's base
                assert np.array_equal(out.read_int(name, 0, n), np.where(p, v, base)), name
                want = (int(v[p].min()), int(v[p].max())) if p.any() else (I64_MAX, I64_MIN)
            else:
                ids = [ref["dicts"][name].index(s) for s in v if s is not None]
                want = (min(ids), max(ids)) if ids else (I64_MAX, I64_MIN)
            assert (info["exact_min"], info["exact_max"]) == want, (name, info)
    except BaseException:
        out.free()
        raise
    return out, st, ref


def _hbm_of_attached(out_blocks, ref):
    """The HBM bytes the attached int / str columns add to the output: the values, and a bitmap where one has to exist."""
    phys = _phys(out_blocks)
    words = ((phys + TILE + 31) // 32 * 32) // 32 + 1
    return sum((phys + TILE) * ref["storage"][name][0] + (words * 4 if ref["bitmap"][name] else 0) for name, _ in ref["attached"])


# ------------------------------------------------------------------ 1. the three INT paths on one pair of tables

def _main_tables():
    rng = np.random.default_rng(21)
    nd = 5000
    dkeys = rng.permutation(6000)[:nd].astype(np.int64) + 100          # distinct, range 6000 <= 2^16: the default is direct
    i = np.arange(nd, dtype=np.int64)
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[3], w8[nd - 2] = I64_MIN, I64_MAX
    sid = rng.integers(0, 300, nd)
    tlen, tfirst = rng.integers(0, 4, nd), rng.integers(0, 6, nd)
    flat = {"id": (dkeys, rng.random(nd) > 0.02), "w1": (1000 + (i * 37) % 200, None), "w2": (-3 + (i * 7) % 60000, None),
            "w4": (5 + (i * 100003) % (1 << 31), None), "w8": (w8, None), "nb": (rng.integers(-500, 500, nd).astype(np.int64), rng.random(nd) > 0.3),
            "none": (np.full(nd, 77, dtype=np.int64), np.zeros(nd, dtype=bool))}
    strs = {"s": [("user%03d" % s if k % 13 else None) for k, s in enumerate(sid.tolist())]}
    tags = {"tags": [(["tag%d" % (f + k) for k in range(ln)] if k0 % 5 else None) for k0, (f, ln) in enumerate(zip(tfirst.tolist(), tlen.tolist()))]}
    dl = _cut(flat, strs, tags, (1, 70, 33, 2049, 31, 64, 777, 32, 1943))
    tk = rng.integers(0, 6300, N_T).astype(np.int64)                   # some below lo = 100, some above hi, most inside
    tl = _cut({"k": (tk, rng.random(N_T) > 0.05), "x": (np.arange(N_T, dtype=np.int64), None)}, {"name": ["n%d" % (k % 7) for k in range(N_T)]}, {}, T_SIZES)
    return tl, dl


MAIN_T, MAIN_DIM = _main_tables()


@pytest.fixture(scope="module")
def main(ctx):
    made = {}

    def get(which, compact):
        if (which, compact) not in made:
            made[(which, compact)] = build(ctx, MAIN_T if which == "t" else MAIN_DIM, compact=compact, name=which)
        return made[(which, compact)]
    yield get
    for tb in made.values():
        tb.free()


@pytest.mark.parametrize("force,path", [(None, DIRECT), ("direct", DIRECT), ("hash", HASH)])
@pytest.mark.parametrize("t_compact", [True, False])
@pytest.mark.parametrize("dim_compact", [True, False])
def test_int_paths_and_every_kind_of_attached_column(main, env, force, path, t_compact, dim_compact):
    """Source widths 1 / 2 / 4 / 8 (dim compact) and 8 / 4 (dim canonical) into canonical and into compact output, a column
    with a bitmap, a str column, a set column, an all-unpopulated column; unpopulated keys on both sides; keys of t below lo,
    above hi and absent from dim."""
    env(path=force)
    t, dim = main("t", t_compact), main("dim", dim_compact)
    if dim_compact:
        assert [dim.column_storage(c)[0] for c in ("id", "w1", "w2", "w4", "w8", "s", "none")] == [2, 1, 2, 4, 8, 2, 1]
    out, st, ref = _check(t, MAIN_T, dim, MAIN_DIM, "k", t_compact, path=path, dim_key="id", prefix="d.")
    try:
        assert 0 < st["matched"] < N_T and st["dim_duplicates"] == 0 and st["slots"] == (16384 if path == HASH else 0)
        assert st["build_bytes"] > 0 and st["probe_bytes"] > 0 and st["gather_bytes"] > 0
        if t_compact:
            assert [ref["storage"][c] for c in ("d.w1", "d.w2", "d.w4", "d.w8", "d.none")] == [(1, 1000), (2, -3), (4, 5), (8, 0), (1, 0)]
        assert t.lookup_stats() == {k: 0 for k in st}                  # zeros for a table no lookup made
        assert out.concat_stats()["rows"] == 0 and out.select_stats()["rows_in"] == 0
    finally:
        out.free()


# ------------------------------------------------------------------ 2. the default path on both sides of the rule

@pytest.mark.parametrize("rows,span,path", [(31, 1 << 16, DIRECT), (31, (1 << 16) + 1, HASH), (20000, 80000, DIRECT), (20000, 80001, HASH)])
def test_default_path_rule(ctx, env, rows, span, path):
    """direct iff hi - lo + 1 <= max(2^16, 4 x live dim rows)."""
    rng = np.random.default_rng(rows + span)
    lo = -12345
    dk = lo + rng.permutation(span)[:rows].astype(np.int64)
    dk[0], dk[-1] = lo, lo + span - 1
    dl = _cut({"k": (dk, None), "v": (np.arange(rows, dtype=np.int64) * 3, None)}, {}, {}, (rows,))
    tk = np.concatenate([dk[:200], [lo - 1, lo + span, lo + 1]]).astype(np.int64)
    tl = _cut({"k": (tk, None)}, {}, {}, (33, len(tk) - 33))
    t, dim = build(ctx, tl, compact=True), build(ctx, dl, compact=True)
    try:
        out, st, _ = _check(t, tl, dim, dl, "k", True, path=path)
        out.free()
    finally:
        t.free()
        dim.free()


# ------------------------------------------------------------------ 3. dim sizes, the key -1, the int64 edges

@pytest.mark.parametrize("force", ["direct", "hash"])
@pytest.mark.parametrize("rows", [0, 1, 31, 33, 5000])
def test_dim_sizes_with_the_key_minus_one(ctx, main, env, force, rows):
    env(path=force)
    dk = np.arange(rows, dtype=np.int64) * 3 - 1                       # -1, 2, 5, ...
    dl = _cut({"k": (dk, None), "v": (dk * 10, None)}, {}, {}, (rows,))
    tl = [(n, {"k": ("int", c["k"][1] % 97 - 2, c["k"][2]), "x": c["x"]}) for n, c in MAIN_T]          # -2 .. 94: -1 among them
    t, dim = build(ctx, tl), build(ctx, dl)
    try:
        out, st, ref = _check(t, tl, dim, dl, "k", False, path=(0 if rows == 0 else DIRECT if force == "direct" else HASH))
        assert ref["bitmap"]["v"] and (ref["matched"] > 0) == (rows > 0)
        out.free()
    finally:
        t.free()
        dim.free()


EDGE_DIM = [-1, 0, I64_MIN, I64_MAX, 5, 1 << 40, -(1 << 40), 77, I64_MIN + 7]
EDGE_T = [-1, 0, I64_MIN, I64_MAX, 6, -2, 1, I64_MIN + 1, I64_MAX - 1, 1 << 40, -1, 99, I64_MIN, 5, 5]


def test_hash_path_keys_at_the_int64_edges(ctx, env):
    """-1 (the table's free-slot marker as an int64) on both sides, 0, INT64_MIN, INT64_MAX, keys on one side only."""
    dl = _cut({"k": (np.array(EDGE_DIM, dtype=np.int64), None), "v": (np.arange(len(EDGE_DIM), dtype=np.int64) + 100, None)}, {}, {}, (len(EDGE_DIM),))
    tl = _cut({"k": (np.array(EDGE_T, dtype=np.int64), None)}, {}, {}, (1, len(EDGE_T) - 1))
    for compact in (False, True):
        t, dim = build(ctx, tl, compact=compact), build(ctx, dl, compact=compact)
        try:
            env()
            out, st, ref = _check(t, tl, dim, dl, "k", compact, path=HASH)          # the range is 2^64: hash by default
            assert st["slots"] == 64 and ref["matched"] == 9
            rows = D.rows_of(ref["blocks"])
            assert rows[0] == {"k": -1, "v": 100} and rows[10] == {"k": -1, "v": 100} and rows[5] == {"k": -2}
            out.free()
            env(path="direct")                                                       # ... and direct would need 2^64 cells
            _refused(t, dim, ["'k'", "2^27"], key="k")
        finally:
            t.free()
            dim.free()


def test_direct_path_range_test_at_the_int64_edges(ctx, env):
    """Keys of t below lo and above hi of dim, the int64 extremes among them: v - lo wraps as a signed number."""
    for lo in (100, I64_MIN, I64_MAX - 300, -150):
        dk = lo + np.array([0, 300, 7, 150], dtype=object)
        tk = [lo, lo + 300, lo - 1, lo + 301, I64_MIN, I64_MAX, lo + (1 << 63), lo + 7, lo + 8, 0, -1]
        dl = _cut({"k": (np.array([_wrap(x) for x in dk], dtype=np.int64), None), "v": (np.arange(4, dtype=np.int64) + 1, None)}, {}, {}, (4,))
        tl = _cut({"k": (np.array([_wrap(x) for x in tk], dtype=np.int64), None)}, {}, {}, (len(tk),))
        for force in ("direct", None):
            env(path=force)
            for compact in (False, True):
                t, dim = build(ctx, tl, compact=compact), build(ctx, dl, compact=compact)
                try:
                    out, st, ref = _check(t, tl, dim, dl, "k", compact, path=DIRECT)
                    assert ref["matched"] == sum(1 for x in tk if _wrap(x) in [_wrap(y) for y in dk])
                    out.free()
                finally:
                    t.free()
                    dim.free()


# ------------------------------------------------------------------ 4. a small hash table: chains that wrap, a table that fills

def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _keys_hashing_high(n, slots, first_slot):
    """n distinct keys whose home slot (splitmix64(key) >> 32 & mask, csrc/hash_table.h) is >= first_slot: their chains wrap."""
    out, k = [], 1000
    while len(out) < n:
        if (_splitmix64(k) >> 32) & (slots - 1) >= first_slot:
            out.append(k)
        k += 1
    return out


CHAIN_KEYS = _keys_hashing_high(48, 64, 56)       # 48 keys at home in the last 8 of 64 slots


def _chain_tables(ctx):
    dk = np.array(CHAIN_KEYS + CHAIN_KEYS[:10], dtype=np.int64)                      # 10 duplicates behind the first copies
    dl = _cut({"k": (dk, None), "v": (np.arange(len(dk), dtype=np.int64), None)}, {}, {}, (33, len(dk) - 33))
    tk = np.array((CHAIN_KEYS + list(range(990, 1400))) * 2, dtype=np.int64)         # every key, and many that walk to a free slot
    tl = _cut({"k": (tk, None)}, {}, {}, (70, len(tk) - 70))
    return build(ctx, tl), tl, build(ctx, dl), dl


def test_64_slots_for_48_keys_chains_wrap_past_the_last_slot(ctx, env):
    t, tl, dim, dl = _chain_tables(ctx)
    try:
        env(path="hash", slots=64)
        out, st, ref = _check(t, tl, dim, dl, "k", False, path=HASH)
        assert st["slots"] == 64 and (st["dim_keys"], st["dim_duplicates"]) == (48, 10) and ref["matched"] >= 96
        out.free()
    finally:
        t.free()
        dim.free()


def test_32_slots_for_48_keys_is_out_of_memory_and_the_context_lives_on(ctx, env):
    """An error return, not a fault: the build's walk and the probe's are bounded by the slot count (k_lk_build, k_lk_probe)."""
    import sybil_amd
    t, tl, dim, dl = _chain_tables(ctx)
    try:
        env(path="hash", slots=32)
        with pytest.raises(sybil_amd.SyblError) as ei:
            t.lookup(dim, "k")
        assert ei.value.code == E_NOMEM and "sybl_table_lookup: " in str(ei.value) and "32 slots" in str(ei.value)
        for bad in (48, 1, 0, -64, 1 << 28):
            env(path="hash", slots=bad)
            _refused(t, dim, ["SYBL_LOOKUP_SLOTS"], key="k")
        env(path="neither")
        _refused(t, dim, ["SYBL_LOOKUP_PATH"], key="k")
        env(path="hash", slots=64)
        out, st, _ = _check(t, tl, dim, dl, "k", False, path=HASH)                   # the context is usable afterwards
        out.free()
        env()
        out, st, _ = _check(t, tl, dim, dl, "k", False, path=DIRECT)
        out.free()
    finally:
        t.free()
        dim.free()


# ------------------------------------------------------------------ 5. duplicates: the lowest row wins

@pytest.mark.parametrize("force", ["direct", "hash"])
def test_duplicates_spread_over_blocks_the_first_row_wins(ctx, env, force):
    """Every key 1 to 40 times, the copies shuffled over dim blocks of irregular sizes: different workgroups race for a cell."""
    env(path=force)
    rng = np.random.default_rng(8)
    keys = np.repeat(np.arange(200, dtype=np.int64) * 5 - 300, 1 + (np.arange(200) * 7) % 40)
    rng.shuffle(keys)
    n = len(keys)
    sizes, left = [], n
    for s in (1, 70, 33, 2049, 31, 64, 777, 32) * 2:
        if left > s:
            sizes.append(s)
            left -= s
    sizes.append(left)
    dl = _cut({"k": (keys, rng.random(n) > 0.1), "row": (np.arange(n, dtype=np.int64), None)}, {}, {}, tuple(sizes))
    tk = np.arange(-320, 720, dtype=np.int64)
    tl = _cut({"k": (tk, None)}, {}, {}, (70, 33, len(tk) - 103))
    t, dim = build(ctx, tl, compact=True), build(ctx, dl, compact=True)
    try:
        assert len(sizes) > 8 and n > 3000
        out, st, ref = _check(t, tl, dim, dl, "k", True, path=DIRECT if force == "direct" else HASH)
        assert 190 <= st["dim_keys"] <= 200 and st["dim_duplicates"] > 2000 and st["matched"] == st["dim_keys"]
        _, dv, dp = D.concat(dl)["k"]
        for r in D.rows_of(ref["blocks"]):
            if "row" in r:                                             # the lowest populated row that holds the key
                assert r["row"] == int(np.nonzero(dp & (dv == r["k"]))[0][0])
        out.free()
    finally:
        t.free()
        dim.free()


# ------------------------------------------------------------------ 6. stored forms of the key

KEY_RANGES = {1: (1000, 1199), 2: (-30000, 29999), 4: (5, 5 + (1 << 31)), 8: (-(1 << 39), (1 << 39))}


@pytest.mark.parametrize("width", [1, 2, 4, 8])
@pytest.mark.parametrize("compact_side", ["t", "dim"])
def test_stored_forms_of_the_key(ctx, env, width, compact_side):
    """One side compact at 1 / 2 / 4 / 8 bytes from a non-zero base, the other canonical: keys compare as decoded values."""
    lo, hi = KEY_RANGES[width]
    rng = np.random.default_rng(width)
    tk = np.array([lo + int(x) for x in rng.integers(0, hi - lo + 1, N_T)], dtype=np.int64)
    tk[0], tk[-1] = lo, hi
    dk = np.unique(np.concatenate([tk[::2][:1500], [lo + 1, hi - 1]]))
    rng.shuffle(dk)
    tl = _cut({"k": (tk, rng.random(N_T) > 0.03)}, {}, {}, T_SIZES)
    dl = _cut({"k": (dk, None), "v": (np.arange(len(dk), dtype=np.int64), None)}, {}, {}, (33, len(dk) - 33))
    t, dim = build(ctx, tl, compact=compact_side == "t"), build(ctx, dl, compact=compact_side == "dim")
    try:
        packed, plain = (t, dim) if compact_side == "t" else (dim, t)
        assert packed.column_storage("k")[0] == width and plain.column_storage("k") == (8, 0)
        assert width == 8 or packed.column_storage("k")[1] != 0
        out, st, ref = _check(t, tl, dim, dl, "k", compact_side == "t", path=DIRECT if width < 4 else HASH)
        assert ref["matched"] > 1000
        out.free()
    finally:
        t.free()
        dim.free()


# ------------------------------------------------------------------ 7. validity bitmaps

def test_a_bitmap_exists_iff_dim_has_one_or_a_row_missed(ctx, env):
    """`full` has no bitmap in dim: on a lookup where every row matches the output column has none either; with one row of t
    missing it has one.  `holes` has a bitmap in dim and so always.  Seen through sybl_table_hbm_bytes, which counts bitmaps."""
    rng = np.random.default_rng(5)
    dk = np.arange(500, dtype=np.int64) * 2
    dl = _cut({"k": (dk, None), "full": (dk + 7, None), "holes": (dk % 11, rng.random(500) > 0.5)}, {}, {}, (500,))
    tk = dk[rng.integers(0, 500, N_T)]
    tl_all = _cut({"k": (tk, None)}, {}, {}, T_SIZES)
    tk2 = tk.copy()
    tk2[2100] = 1                                                       # one row, in the 2049-row block, finds nothing
    tl_miss = _cut({"k": (tk2, None)}, {}, {}, T_SIZES)
    dim = build(ctx, dl, compact=True)
    try:
        for tl, missed in ((tl_all, False), (tl_miss, True)):
            for compact in (True, False):
                t = build(ctx, tl, compact=compact)
                base = ctx.concat([t])
                try:
                    out, st, ref = _check(t, tl, dim, dl, "k", compact)
                    assert ref["bitmap"] == {"full": missed, "holes": True} and st["matched"] == N_T - missed
                    assert out.hbm_bytes - base.hbm_bytes == _hbm_of_attached(ref["blocks"], ref)
                    out.free()
                finally:
                    base.free()
                    t.free()
    finally:
        dim.free()


# ------------------------------------------------------------------ 8. str keys

@pytest.mark.parametrize("compact", [True, False])
def test_str_keys_compare_as_strings(ctx, env, compact):
    """The two dictionaries hold the strings in different orders and each holds strings the other lacks; unpopulated keys on
    both sides; the empty string is a key like any other."""
    env(path="hash")                                                    # (the switch forces an INT path: a str key ignores it)
    names = ["host%03d" % k for k in range(400)] + [""]
    rng = np.random.default_rng(17)
    t_names = [names[k] for k in rng.permutation(401)[:330]] + ["only_t%d" % k for k in range(20)]
    d_names = [names[k] for k in rng.permutation(401)[:350]] + ["only_dim%d" % k for k in range(20)]
    if "" not in t_names:
        t_names[5] = ""
    if "" not in d_names:
        d_names[9] = ""
    th = [None if k % 17 == 0 else t_names[int(x)] for k, x in enumerate(rng.integers(0, len(t_names), N_T))]
    nd = 1500
    dh = [None if k % 23 == 0 else d_names[int(x)] for k, x in enumerate(rng.integers(0, len(d_names), nd))]
    dh[1], th[3] = "", ""
    dl = _cut({"dcid": (np.arange(nd, dtype=np.int64) % 9 + 40, None)}, {"host": dh, "dc": [None if k % 31 == 0 else "dc%d" % (k % 6) for k in range(nd)]},
              {}, (70, 33, nd - 103))
    tl = _cut({"x": (np.arange(N_T, dtype=np.int64), None)}, {"h": th}, {}, T_SIZES)
    t, dim = build(ctx, tl, compact=compact), build(ctx, dl, compact=compact)
    try:
        assert t.column_dict("h")[:50] != dim.column_dict("host")[:50]
        out, st, ref = _check(t, tl, dim, dl, "h", compact, path=STR, dim_key="host", columns=["dc", "dcid", "host"], prefix="d_")
        assert 0 < st["matched"] < N_T and st["dim_duplicates"] > 0 and st["slots"] == 0
        rows = D.rows_of(ref["blocks"])
        assert rows[3]["h"] == "" and rows[3]["d_host"] == "" and all(r["h"] == r["d_host"] for r in rows if "d_host" in r)
        assert any("d_host" not in r and r.get("h", "").startswith("only_t") for r in rows)
        out.free()
    finally:
        t.free()
        dim.free()


# ------------------------------------------------------------------ 9. dim is t; a 65536-row block; dead blocks; empty t

def test_self_lookup_with_a_prefix(main, env):
    t = main("t", True)
    out, st, ref = _check(t, MAIN_T, t, MAIN_T, "k", True, prefix="first_")
    try:
        assert [c for c, _ in ref["attached"]] == ["first_x", "first_name"]
        rows = D.rows_of(ref["blocks"])
        assert all(("first_x" in r) == ("k" in r) and r.get("first_x", 0) <= r["x"] for r in rows)
        assert st["matched"] == sum(1 for r in rows if "k" in r) and st["dim_duplicates"] > 0
    finally:
        out.free()


def test_a_65536_row_block(ctx, main, env):
    sizes = (1, 65536, 33)
    n = sum(sizes)
    rng = np.random.default_rng(3)
    tl = _cut({"k": (rng.integers(0, 6300, n).astype(np.int64), rng.random(n) > 0.01)}, {}, {}, sizes)
    t = build(ctx, tl, compact=True)
    try:
        for force in ("direct", "hash"):
            env(path=force)
            out, st, _ = _check(t, tl, main("dim", True), MAIN_DIM, "k", True, dim_key="id", columns=["w1", "w4", "s", "nb"], prefix="d.")
            out.free()
    finally:
        t.free()


def test_dead_blocks_of_dim_take_no_part(ctx, env, tmp_path):
    """dim opened from a directory, two of its blocks dropped by refresh: their rows -- which held the first copies of some
    keys -- are gone, the later copies win."""
    blocks = []
    for b, n in enumerate((300, 1000, 77, 450, 33)):
        i = np.arange(n, dtype=np.int64)
        blocks.append((n, {"k": ("int", (i * 3 + b) % 400, (i % 7 != 0)), "row": ("int", i + 10000 * b),
                           "name": ("str", [None if k % 9 == 0 else "user%d" % (k % 50) for k in i.tolist()])}))
    root = str(tmp_path / "db")
    F.write_table(root, "hosts", [cols for _, cols in blocks])
    dim = ctx.open_table(root, "hosts", compact=True)
    tl = _cut({"k": (np.arange(-5, 420, dtype=np.int64), None)}, {}, {}, (70, 355))
    t = build(ctx, tl, compact=True)
    try:
        shutil.rmtree(os.path.join(root, "hosts", "block%09d" % 2))            # (block directories count from 1)
        shutil.rmtree(os.path.join(root, "hosts", "block%09d" % 4))
        assert dim.refresh()[1] == 2 and dim.rows == 300 + 77 + 33
        live = [blocks[0], blocks[2], blocks[4]]
        for force in ("direct", "hash"):
            env(path=force)
            ref = L.lookup_ref(tl, live, "k", compact=True)
            out = t.lookup(dim, "k")
            try:
                st = out.lookup_stats()
                assert (st["dim_rows"], st["matched"], st["dim_keys"], st["dim_duplicates"]) == (410, ref["matched"], ref["dim_keys"], ref["dim_duplicates"])
                rows = _rows(out)
                assert rows == D.rows_of(ref["blocks"])
                assert not any(10000 <= r.get("row", 0) < 20000 or 30000 <= r.get("row", 0) < 40000 for r in rows)
            finally:
                out.free()
    finally:
        t.free()
        dim.free()


@pytest.mark.parametrize("compact", [True, False])
def test_t_without_rows(ctx, main, env, compact):
    tl = [(0, {"k": ("int", np.zeros(0, dtype=np.int64), None), "x": ("int", np.zeros(0, dtype=np.int64), None)})]
    t = build(ctx, tl, compact=compact)
    try:
        out, st, ref = _check(t, tl, main("dim", True), MAIN_DIM, "k", compact, path=0, dim_key="id")
        assert (out.rows, out.blocks, st["matched"], st["build_ms"], st["gather_bytes"]) == (0, 0, 0, 0, 0)
        assert out.samples(limit=5).rows == []
        out.free()
    finally:
        t.free()


# ------------------------------------------------------------------ 10. what the call refuses

def _refused(t, dim, words, **kw):
    """The call returns SYBL_E_INVAL with a message that begins `sybl_table_lookup: ` and holds `words`; *out stays NULL."""
    import sybil_amd
    from sybil_amd import _native as N
    with pytest.raises(sybil_amd.SyblError) as ei:
        t.lookup(dim, **kw)
    msg = str(ei.value)
    assert ei.value.code == E_INVAL and msg.startswith("sybilgpu error -1: sybl_table_lookup: "), msg
    assert all(w in msg for w in words), msg
    d = N.LookupDesc()
    d.dim = dim._h.value
    d.key = kw["key"].encode()
    d.dim_key = kw["dim_key"].encode() if kw.get("dim_key") else None
    names = [c.encode() for c in kw.get("columns") or []]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    d.n_columns, d.columns = len(names), (C.cast(arr, C.POINTER(C.c_char_p)) if names else None)
    d.prefix = kw.get("prefix", "").encode()
    h = C.c_void_p(0xDEAD)
    assert N.lib().sybl_table_lookup(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None


def test_every_refusal_leaves_both_tables_as_they_were(ctx, main, env):
    import sybil_amd
    from sybil_amd import _native as N
    t, dim = main("t", True), main("dim", True)
    clash = build(ctx, [(3, {"id": ("str", ["x", "y", None]), "x": ("int", np.arange(3), None), "tags": ("set", [["a"], None, []])})], name="clash")
    other = sybil_amd.Context(0)
    foreign = build(other, [(2, {"id": ("int", np.array([1, 2]), None)})])
    qt, qd = t.query(groups=["name"], aggs=["x"]), dim.query(groups=["s"], aggs=["w2"], op="hist")

    def scan(q):
        res = q.scan().finalize()
        got = (res.matched, [(r["group_by_key"], r["count"], r["hists"][0]["sum"]) for r in res.results])
        res.free()
        return got
    try:
        before = (scan(qt), scan(qd), t.rows, t.blocks, dim.rows, dim.blocks)
        for d_, words, kw in ((dim, ["'nope'"], dict(key="nope", dim_key="id")),
                              (dim, ["'nope'"], dict(key="k", dim_key="nope")),
                              (dim, ["'k'"], dict(key="k")),                                  # dim has no column k
                              (dim, ["'tags'", "set"], dict(key="k", dim_key="tags")),       # a set key
                              (clash, ["'k'", "'id'", "int", "str"], dict(key="k", dim_key="id")),   # mixed key types
                              (dim, ["'name'", "int", "str"], dict(key="name", dim_key="id")),
                              (dim, ["'zz'"], dict(key="k", dim_key="id", columns=["w1", "zz"])),
                              (clash, ["'x'"], dict(key="name", dim_key="id")),              # x is a column of t
                              (clash, ["'x'"], dict(key="name", dim_key="id", columns=["x"])),
                              (foreign, ["context"], dict(key="k", dim_key="id"))):
            _refused(t, d_, words, **kw)
        _refused(clash, dim, ["'tags'", "set"], key="tags", dim_key="id")                      # a set key on t's side
        # a prefix that makes an attached name collide with a column of t
        tl2 = [(2, {"k": ("int", np.array([1, 2]), None), "d_w1": ("int", np.array([3, 4]), None)})]
        t2 = build(ctx, tl2)
        try:
            _refused(t2, dim, ["'d_w1'"], key="k", dim_key="id", prefix="d_")
            out = t2.lookup(dim, "k", dim_key="id", prefix="e_", columns=["w1", "id", "w1"])          # the key, named; a repeat ignored
            assert out.samples(limit=1).columns == ["k", "d_w1", "e_w1", "e_id"]
            out.free()
        finally:
            t2.free()
        # NULL arguments and a negative column count
        d = N.LookupDesc()
        h = C.c_void_p(0xDEAD)
        assert N.lib().sybl_table_lookup(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None              # dim NULL
        assert N.lib().sybl_last_error().startswith(b"sybl_table_lookup: NULL")
        assert N.lib().sybl_table_lookup(t._h, None, C.byref(h)) == E_INVAL and N.lib().sybl_table_lookup(t._h, C.byref(d), None) == E_INVAL
        d.dim, d.key, d.dim_key, d.n_columns = dim._h.value, b"k", b"id", -1
        assert N.lib().sybl_table_lookup(t._h, C.byref(d), C.byref(h)) == E_INVAL and h.value is None
        assert N.lib().sybl_last_error().startswith(b"sybl_table_lookup: ")
        assert (scan(qt), scan(qd), t.rows, t.blocks, dim.rows, dim.blocks) == before           # no version moved: no SYBL_E_STATE
        out = t.lookup(dim, "k", dim_key="id", columns=["w1"])                                   # ... nor by a lookup that succeeds
        assert (scan(qt), scan(qd), t.rows, t.blocks, dim.rows, dim.blocks) == before
        out.free()
    finally:
        qt.free()
        qd.free()
        foreign.free()
        other.close()
        clash.free()


# ------------------------------------------------------------------ 11. end to end: a query grouped by an attached column

@pytest.mark.parametrize("compact", [True, False])
def test_query_grouped_by_an_attached_str_column_agrees_with_the_oracle(ctx, oracle, env, compact):
    """The lookup's output against the same rows built by hand through append_block, and both against the oracle."""
    rng = np.random.default_rng(2)
    n = N_T
    tl = _cut({"host": (rng.integers(0, 60, n).astype(np.int64), rng.random(n) > 0.02), "lat": (rng.integers(0, 1000, n).astype(np.int64), None)}, {}, {}, T_SIZES)
    tl[0][1]["lat"][1][0], tl[1][1]["lat"][1][0] = 0, 999               # (the exact extrema, whatever the draw)
    dl = _cut({"host": (np.arange(50, dtype=np.int64), None)}, {"dc": [None if k == 13 else "dc%d" % (k % 7) for k in range(50)]}, {}, (50,))
    t, dim = build(ctx, tl, compact=compact), build(ctx, dl, compact=compact)
    out, hand = None, None
    try:
        out, st, ref = _check(t, tl, dim, dl, "host", compact, path=DIRECT)
        hand = build(ctx, ref["blocks"], compact=compact)
        names = [("host", "int"), ("lat", "int"), ("dc", "str")]
        q = dict(groups=["dc"], aggs=["lat"], op="hist", want_percentiles=True)
        got = []
        assert out.column_dict("dc") == ref["dicts"]["dc"] != hand.column_dict("dc")     # dim's order; the rows' first-seen order
        for tb in (out, hand):
            got.append(_against_oracle(oracle, tb, ref["blocks"], names, {"dc": tb.column_dict("dc")}, q, {"lat": (0, 999)}, full=True))
        assert got[0] == got[1] == N_T > ref["matched"] > 0       # no filter: every row is scanned, the unmatched ones in the group without a dc
    finally:
        for tb in (out, hand, t, dim):
            if tb is not None:
                tb.free()


# ------------------------------------------------------------------ 12. the C example

def test_c_example_runs(ctx, tmp_path):
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    exe = str(tmp_path / "example_lookup")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "example_lookup.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    text = p.stdout.decode()
    assert text.startswith("3000 rows in 3 blocks, 2625 matched one of 7 hosts (path 1;")
    assert all(dc in text for dc in ("ams", "fra", "sfo"))
