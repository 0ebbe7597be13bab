"""GPU: table concat (Context.concat / sybl_table_concat, csrc/concat.hip) against the numpy restatement in
tests/concat_ref.py.  Sources are built block by block through append_block with irregular block sizes, so block starts sit
on padded rows; the output is read back whole with samples(limit=N) and read_int.  Every comparison is exact.

Shapes: a 16-byte lane chunk of k_cc_transcode is 2 to 16 rows, a validity word 32 rows, a wave covers 128 to 1024 rows and
the run bisection needs several runs -- block sizes come from (1, 31, 32, 33, 70, 2047, 2049, 8197), one case has a
65536-row block."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import concat_ref as R
from tests import digest_ref as D
from tests import parity
from tests import sybil_fixture as F
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIZES = {"a": (70, 1, 2049, 33, 8197, 31, 32, 2047), "b": (33, 2047, 1, 8197, 31), "c": (2049, 32, 70)}


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


def _cut(flat, strs, tags, sizes):
    blocks, r0 = [], 0
    for s in sizes:
        sl = slice(r0, r0 + s)
        cols = {name: ("int", v[sl], None if p is None else p[sl]) for name, (v, p) in flat.items()}
        for name, v in strs.items():
            cols[name] = ("str", v[sl])
        for name, v in tags.items():
            cols[name] = ("set", v[sl])
        blocks.append((s, cols))
        r0 += s
    return blocks


def _make(kind):
    """Three tables of every column kind whose ranges, bases and dictionaries differ.  a: w1 / w2 / w4 / w8 are stored at 1 / 2 /
    4 / 8 bytes when compact; b: other bases and narrower w4 / w8, the strings of s half overlapping a's in another first-seen
    order; c: lacks w4 and tags, has a column of its own."""
    sizes = SIZES[kind]
    n = sum(sizes)
    rng = np.random.default_rng({"a": 3, "b": 5, "c": 7}[kind])
    i = np.arange(n, dtype=np.int64)
    spop, tpop = rng.random(n) > 0.25, rng.random(n) > 0.25
    tlen, tfirst = rng.integers(0, 4, size=n), rng.integers(0, 6, size=n)
    ni = (rng.integers(-500, 500, size=n).astype(np.int64), rng.random(n) > 0.3)
    if kind == "a":
        w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
        w8[0], w8[n // 2] = I64_MIN, I64_MAX
        flat = {"w1": (1000 + (i * 37) % 200, None), "w2": (-3 + (i * 7) % 60000, None), "w4": (5 + (i * 100003) % (1 << 31), None),
                "w8": (w8, None), "ni": ni}
        sid = rng.integers(0, 50, size=n)
    elif kind == "b":
        flat = {"w1": (1100 + i % 150, None), "w2": (20000 + (i * 11) % 40000, None), "w4": ((1 << 31) + (i * 7) % 1000, None),
                "w8": (i * 3, None), "ni": (ni[0] * 100, None)}
        sid = 74 - rng.integers(0, 50, size=n)
    else:
        flat = {"w1": (900 + i % 50, None), "extra": (i % 7, rng.random(n) > 0.5), "w8": (-i, None), "w2": (i % 300, None), "ni": ni}
        sid = rng.integers(40, 90, size=n)
    strs = {"s": [("user%02d" % s if p else None) for s, p in zip(sid.tolist(), spop.tolist())]}
    tags = {} if kind == "c" else {"tags": [(["tag%d" % (f + k + (3 if kind == "b" else 0)) for k in range(ln)] if p else None)
                                            for f, ln, p in zip(tfirst.tolist(), tlen.tolist(), tpop.tolist())]}
    return _cut(flat, strs, tags, sizes)


BLOCKS = {k: _make(k) for k in "abc"}


@pytest.fixture(scope="module")
def tables(ctx):
    """The source table of (kind, storage), built on first use and kept for the module."""
    made = {}

    def get(kind, storage):
        if (kind, storage) not in made:
            made[(kind, storage)] = build(ctx, BLOCKS[kind], compact=storage == "compact", name="t_" + kind)
        return made[(kind, storage)]
    yield get
    for tb in made.values():
        tb.free()


def _rows(tb, columns=None):
    """Every row of a table in row order (samples returns them newest first)."""
    n = tb.rows
    got = tb.samples(limit=max(n, 1), columns=columns)
    assert got.info["n_rows"] == n and got.row_ids.tolist() == list(range(n - 1, -1, -1))
    return got.rows[::-1]


def _expected_storage(lists, compact, name, ty):
    if not compact:
        return (8, 0) if ty == "int" else (4, 0)
    if ty == "int":
        lo, hi = I64_MAX, I64_MIN
        for blocks in lists:
            c = D.concat(blocks).get(name)
            if c is not None and c[2].any():
                lo, hi = min(lo, int(c[1][c[2]].min())), max(hi, int(c[1][c[2]].max()))
        return R.storage_of(lo, hi, "int")
    holders = [b for b in lists if name in D.column_types(b)]
    return R.storage_of(*R.str_extrema([R.table_dict(b, name) for b in holders],
                                       [[s for s in D.concat(b)[name][1] if s is not None] for b in holders]), "str")


def _check_concat(ctx, srcs, lists, columns=None, rows=True):
    """concat(srcs) against concat_ref(lists): rows, blocks, every row, storage, dictionaries, stats.  Returns the table."""
    ref = R.concat_ref(lists, columns)
    names = R.output_columns(lists, columns)
    n = sum(b[0] for b in ref)
    before = [(t.rows, t.blocks) for t in srcs]
    out = ctx.concat(srcs, columns)
    try:
        assert out.rows == n and out.blocks == len(ref) == sum(1 for bl in lists for b in bl if b[0] > 0)
        assert [(t.rows, t.blocks) for t in srcs] == before
        st = out.concat_stats()
        assert (st["rows"], st["blocks"], st["tables"], st["columns"]) == (n, len(ref), len(srcs), len(names)), st
        assert out.samples(limit=1).columns == [c for c, _ in names]
        cols = D.concat(ref) if ref else {}
        for name, ty in names:
            if ty != "int":
                assert out.column_dict(name) == R.merged_dict([R.table_dict(b, name) for b in lists if name in D.column_types(b)]), name
            elif n:
                _, v, p = cols[name] if name in cols else ("int", np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool))
                assert np.array_equal(out.read_int(name, 0, n)[p], v[p]), name
        if rows:
            assert _rows(out) == D.rows_of(ref)
    except BaseException:
        out.free()
        raise
    return out


def _check_storage(out, lists, compact, columns=None):
    for name, ty in R.output_columns(lists, columns):
        if ty != "set":
            assert out.column_storage(name) == _expected_storage(lists, compact, name, ty), name


# ------------------------------------------------------------------ 1. rows, exactly

@pytest.mark.parametrize("kinds", ["ab", "abc", "ba", "cab"])
@pytest.mark.parametrize("storages", ["canonical+canonical", "compact+compact", "compact+canonical"])
def test_rows_exactly(ctx, tables, kinds, storages):
    first, rest = storages.split("+")
    srcs = [tables(k, first if j == 0 else rest) for j, k in enumerate(kinds)]
    lists = [BLOCKS[k] for k in kinds]
    a = tables("a", "compact")
    assert [a.column_storage(c)[0] for c in ("w1", "w2", "w4", "w8", "s")] == [1, 2, 4, 8, 1]
    out = _check_concat(ctx, srcs, lists)
    try:
        _check_storage(out, lists, storages == "compact+compact")
        st = out.concat_stats()
        assert st["copies"] + st["transcodes"] + st["lut_transcodes"] > 0 and st["copy_bytes"] > 0 and st["runs"] == len(kinds)
        if storages == "compact+compact":
            assert st["lut_transcodes"] >= 1 and st["transcodes"] >= 3      # s through an id table; w1 / w2 / w4 from other bases
    finally:
        out.free()


def test_a_65536_row_block(ctx):
    rng = np.random.default_rng(11)
    lists = []
    for k, sizes in enumerate(((1, 65536, 33), (31, 2049))):
        n = sum(sizes)
        i = np.arange(n, dtype=np.int64)
        sid = rng.integers(0, 30, n) + 20 * k
        lists.append(_cut({"w1": (k * 40 + i % 200, None), "w2": (k * 70000 + (i * 7) % 50000, rng.random(n) > 0.1)},
                          {"s": ["h%02d" % s for s in sid.tolist()]}, {}, sizes))
    srcs = [build(ctx, b, compact=True) for b in lists]
    out = None
    try:
        out = _check_concat(ctx, srcs, lists, rows=False)
        _check_storage(out, lists, True)
        assert out.column_storage("w2")[0] == 4 and out.column_storage("w1") == (1, 0)
        assert _rows(out, ["s", "w2"]) == D.rows_of(R.concat_ref(lists, ["s", "w2"]))
    finally:
        for t in srcs + ([out] if out else []):
            t.free()


# ------------------------------------------------------------------ 2. the width and base matrix

T32 = 1 << 32
MATRIX = {   # name: (range of a, range of b, (stored width of a, of b, of the output))
    "1to1_other_base": ((1000, 1100), (1050, 1250), (1, 1, 1)),
    "1to2_at_the_threshold": ((-5, 250), (100, 251), (1, 1, 2)),
    "1to4_at_the_threshold": ((0, 200), (65400, 65536), (1, 1, 4)),
    "1to8_base_int64_min": ((I64_MIN, I64_MIN + 255), (I64_MAX - 100, I64_MAX), (1, 1, 8)),
    "2to2_negative_base": ((-40000, -40000 + 65535), (-30000, 0), (2, 2, 2)),
    "2to4_at_the_threshold": ((0, 65535), (1, 65536), (2, 2, 4)),
    "2to8": ((0, 300), (T32 - 100, T32 + 200), (2, 2, 8)),
    "1to2_and_2to2": ((7, 9), (-60000, 0), (1, 2, 2)),
    "4to4_other_base": ((0, T32 - 1), (5, 70000), (4, 4, 4)),
    "4to8_at_the_threshold": ((0, T32 - 1), (1, T32), (4, 4, 8)),
    "2to4_and_4to4_base_int64_min": ((I64_MIN + 10, I64_MIN + 1000), (I64_MIN, I64_MIN + T32 - 1), (2, 4, 4)),
    "like_stored": ((-7, 240), (-7, 240), (1, 1, 1)),
    "like_stored_8": ((I64_MIN, I64_MAX), (I64_MIN, 0), (8, 8, 8)),
}


def _range_blocks(lo, hi, sizes, seed):
    n = sum(sizes)
    span = hi - lo
    v = np.array([lo + int(x) for x in np.random.default_rng(seed).integers(0, min(span, (1 << 62)) + 1, n)], dtype=np.int64)
    v[0], v[-1] = lo, hi
    return _cut({"x": (v, None)}, {}, {}, sizes)


@pytest.mark.parametrize("which", sorted(MATRIX))
def test_width_and_base_matrix(ctx, which):
    ra, rb, widths = MATRIX[which]
    lists = [_range_blocks(ra[0], ra[1], (33, 2049), 1), _range_blocks(rb[0], rb[1], (70, 31, 1), 2)]
    srcs = [build(ctx, b, compact=True) for b in lists]
    out = None
    try:
        stored = [t.column_storage("x") for t in srcs]
        assert stored == [R.storage_of(ra[0], ra[1], "int"), R.storage_of(rb[0], rb[1], "int")]
        out = _check_concat(ctx, srcs, lists)
        want = R.storage_of(min(ra[0], rb[0]), max(ra[1], rb[1]), "int")
        assert out.column_storage("x") == want
        assert (stored[0][0], stored[1][0], want[0]) == widths          # the pair this case is there for
        st = out.concat_stats()
        copies = sum(1 for s in stored if s == want)
        assert (st["copies"], st["transcodes"], st["lut_transcodes"]) == (copies, 2 - copies, 0), st
        if which.startswith("like_stored"):
            assert copies == 2
        info = out.column_info("x")
        assert (info["exact_min"], info["exact_max"]) == (min(ra[0], rb[0]), max(ra[1], rb[1]))
    finally:
        for t in srcs + ([out] if out else []):
            t.free()


@pytest.mark.parametrize("n_strings,width", [(40, 1), (300, 2)])
@pytest.mark.parametrize("where", ["first", "second"])
def test_str_ids_narrow_after_set_dict(ctx, n_strings, width, where):
    """sybl_table_set_dict returns a str column of a compact table to int32 ids: the output stores them narrow again --
    4 -> 1 and 4 -> 2, as source 0 (no id table) and as a later source (through one)."""
    vocab = ["k%03d" % k for k in range(n_strings)]
    sizes = (33, 2049, 31)
    n = sum(sizes)
    wide = _cut({}, {"s": [vocab[(k * 7) % n_strings] if k % 7 != 3 else None for k in range(n)]}, {}, sizes)
    other = _cut({}, {"s": [vocab[(n_strings - 1 - k) % 20] for k in range(70)]}, {}, (70,))
    tw, to = build(ctx, wide, compact=True), build(ctx, other, compact=True)
    out = None
    try:
        assert tw.column_storage("s")[0] == width
        tw.set_dict("s", tw.column_dict("s"))
        assert tw.column_storage("s") == (4, 0)
        srcs, lists = ([tw, to], [wide, other]) if where == "first" else ([to, tw], [other, wide])
        out = _check_concat(ctx, srcs, lists)
        assert out.column_storage("s") == (width, 0) == _expected_storage(lists, True, "s", "str")
        st = out.concat_stats()
        # the narrow table goes through an id table when it comes second; the wide one is re-encoded either way
        #   (the narrow one, first, is in the output's form already when that is one byte wide)
        assert (st["copies"], st["transcodes"], st["lut_transcodes"]) == ((0, 1, 1) if where == "first" or width == 2 else (1, 0, 1)), st
    finally:
        for t in [tw, to] + ([out] if out else []):
            t.free()


# ------------------------------------------------------------------ 3. dictionaries

def _ocols(ref, names, dicts):
    """The oracle's columns of a block list; str / set ids are those of dicts[name]."""
    cols = D.concat(ref)
    n = sum(b[0] for b in ref)
    out = []
    for name, ty in names:
        _, v, p = cols.get(name, (ty, np.zeros(n, dtype=np.int64) if ty == "int" else [None] * n, np.zeros(n, dtype=bool)))
        if ty == "int":
            out.append({"type": "int", "data": v, "populated": p})
        elif ty == "str":
            ix = {s: k for k, s in enumerate(dicts[name])}
            out.append({"type": "str", "data": np.array([ix[s] if s is not None else 0 for s in v], dtype=np.int32), "populated": p})
        else:
            ix = {s: k for k, s in enumerate(dicts[name])}
            members = [ix[m] for s in v for m in (s or [])]
            off = np.concatenate([[0], np.cumsum([len(s or []) for s in v])]).astype(np.int64)
            out.append({"type": "set", "data": np.array(members, dtype=np.int32), "offsets": off, "populated": p})
    return out


def _against_oracle(oracle, tb, ref, names, dicts, q, info, okw_filters=None, **cmp):
    okw = parity.oracle_query_kwargs([c for c, _ in names], info, q)
    if okw_filters is not None:
        okw["filters"] = okw_filters
    query = tb.query(**q)
    try:
        gres = query.run()
        ores = oracle.run_query(_ocols(ref, names, dicts), n_threads=4, **okw)
        parity.compare(gres, ores, op=q.get("op", "avg"), n_aggs=len(q.get("aggs", [])), **cmp)
        matched = gres.matched
        gres.free()
        return matched
    finally:
        query.free()


def test_dictionaries_merge_and_str_filters_agree_with_the_oracle(ctx, oracle):
    sizes = (70, 2049, 33)
    n = sum(sizes)
    first = ["s%02d" % k for k in range(20)]
    second = ["s%02d" % k for k in range(29, 9, -1)]            # s29 .. s10: half of them new, another first-seen order
    la = _cut({"v": (np.arange(n, dtype=np.int64) % 97, None)}, {"s": [first[k % 20] for k in range(n)]}, {}, sizes)
    # the second table: rows 0 .. 199 of its first block -- several 32-row words -- are unpopulated, under a remap
    lb = _cut({"v": (np.arange(n, dtype=np.int64) % 89, None)}, {"s": [None if k < 200 or k % 11 == 0 else second[(k * 3) % 20] for k in range(n)]}, {},
              (2049, 70, 33))
    for compact in (True, False):
        ta, tb = build(ctx, la, compact=compact), build(ctx, lb, compact=compact)
        # a string no row uses: it is in table b's dictionary and so in the output's
        tb.append_block(1, {"v": np.array([5]), "s": {"ids": [0], "strings": ["s10", "unused"]}})
        lb2 = lb + [(1, {"v": ("int", np.array([5]), None), "s": ("str", ["s10"])})]
        out = None
        try:
            assert ta.column_dict("s") == first and tb.column_dict("s") == R.table_dict(lb, "s") + ["unused"]
            out = ctx.concat([ta, tb])
            merged = R.merged_dict([first, R.table_dict(lb, "s") + ["unused"]])
            assert merged[:20] == first and merged[-1] == "unused" and sorted(merged[20:-1]) == ["s%02d" % k for k in range(20, 30)]
            assert merged[20:-1] != sorted(merged[20:-1]) and out.column_dict("s") == merged
            ref = R.concat_ref([la, lb2])
            assert _rows(out) == D.rows_of(ref)
            assert out.concat_stats()["lut_transcodes"] == 1
            names = [("v", "int"), ("s", "str")]
            dicts = {"s": merged}
            strs = D.concat(ref)["s"][1]
            for q, of, want in ((dict(filters=[("s", "eq", "s25")], groups=["s"], aggs=["v"]), [(1, "eq", merged.index("s25"))],
                                 sum(1 for s in strs if s == "s25")),
                                (dict(filters=[("s", "re", "^s[12][0-4]$")], groups=["s"], aggs=["v"]),
                                 [(1, "re", 0, np.array([bool(re.search("^s[12][0-4]$", s)) for s in merged], dtype=np.uint8))],
                                 sum(1 for s in strs if s is not None and re.search("^s[12][0-4]$", s)))):
                assert _against_oracle(oracle, out, ref, names, dicts, q, {"v": (0, 96)}, okw_filters=of) == want > 0
        finally:
            for t in [ta, tb] + ([out] if out else []):
                t.free()


# ------------------------------------------------------------------ 4. validity

@pytest.mark.parametrize("compact", [True, False])
def test_validity(ctx, oracle, compact):
    sa, sb = (33, 2049, 31, 70), (31, 1, 2047, 33)
    na, nb = sum(sa), sum(sb)
    rng = np.random.default_rng(9)
    full = _cut({"g": (np.arange(na, dtype=np.int64) % 9, None), "only_a": (np.arange(na, dtype=np.int64), None)}, {}, {}, sa)
    nullable = _cut({"g": (np.arange(nb, dtype=np.int64) % 7 + 3, rng.random(nb) > 0.4)}, {}, {}, sb)
    tf, tn = build(ctx, full, compact=compact), build(ctx, nullable, compact=compact)
    try:
        assert not tf.column_info("g")["has_missing"] and tn.column_info("g")["has_missing"]
        for srcs, lists in (([tf, tn], [full, nullable]), ([tn, tf], [nullable, full]), ([tf, tf], [full, full])):
            out = _check_concat(ctx, srcs, lists)
            try:
                both_full = lists[1] is full and lists[0] is full
                assert out.column_info("g")["has_missing"] == (not both_full)
                assert out.column_info("only_a")["has_missing"] == (not both_full)      # a source with rows lacks it
                ref = R.concat_ref(lists)
                names = R.output_columns(lists)
                pop = D.concat(ref)["g"][2]
                q = dict(groups=["g"], aggs=["only_a"], op="avg")
                assert _against_oracle(oracle, out, ref, names, {}, q, {"only_a": (0, na - 1)}) > 0
                query = out.query(groups=["g"])
                res = query.run()
                counts = sorted(r["count"] for r in res.results)
                res.free()
                query.free()
                vals = D.concat(ref)["g"][1][pop]
                want = sorted(np.bincount(vals).tolist() + ([int((~pop).sum())] if (~pop).any() else []))
                assert counts == [c for c in want if c]
            finally:
                out.free()
    finally:
        tf.free()
        tn.free()


# ------------------------------------------------------------------ 5. schema and errors

def test_schema_and_errors(ctx, tables):
    import sybil_amd
    a, b, c = tables("a", "compact"), tables("b", "compact"), tables("c", "canonical")
    out = _check_concat(ctx, [c, a], [BLOCKS["c"], BLOCKS["a"]], ["tags", "w2", "extra", "s", "w2"])
    out.free()
    out = ctx.concat([c, a, b])
    assert out.samples(limit=1).columns == ["w1", "extra", "w8", "w2", "ni", "s", "w4", "tags"]
    out.free()
    clash = build(ctx, [(3, {"w1": ("str", ["x", "y", None])})], name="clash")
    other = sybil_amd.Context(0)
    foreign = build(other, [(2, {"w1": ("int", np.array([1, 2]), None)})])
    try:
        for call, words in ((lambda: ctx.concat([a, b], ["nope"]), ["nope"]),
                            (lambda: ctx.concat([a, clash]), ["'w1'", "t_a", "clash", "int", "str"]),
                            (lambda: ctx.concat([a, foreign]), ["context"]),
                            (lambda: ctx.concat([]), ["no tables"])):
            with pytest.raises(sybil_amd.SyblError) as ei:
                call()
            assert ei.value.code == E_INVAL and "sybl_table_concat: " in str(ei.value), str(ei.value)
            assert all(w in str(ei.value) for w in words), str(ei.value)
    finally:
        foreign.free()
        other.close()
        clash.free()


@pytest.mark.parametrize("compact", [True, False])
def test_empty_sources(ctx, tables, compact):
    e_blocks = [(0, {"w1": ("int", np.zeros(0, dtype=np.int64), None), "s": ("str", []), "mine": ("int", np.zeros(0, dtype=np.int64), None)})]
    e1, e2 = build(ctx, e_blocks, compact=compact), build(ctx, [], compact=compact)
    storage = "compact" if compact else "canonical"
    a, b = tables("a", storage), tables("b", storage)
    try:
        out = ctx.concat([e1, e2, e1])
        try:
            assert out.rows == 0 and out.blocks == 0 and out.samples(limit=5).columns == ["w1", "s", "mine"] and out.samples(limit=5).rows == []
            st = out.concat_stats()
            assert (st["rows"], st["blocks"], st["tables"], st["columns"], st["copy_bytes"], st["copy_ms"]) == (0, 0, 3, 3, 0, 0)
            assert out.column_info("s")["type"] == 2
        finally:
            out.free()
        lists = [BLOCKS["a"], e_blocks, BLOCKS["b"]]
        out = _check_concat(ctx, [a, e1, b], lists)            # an empty source in the middle: its column, no rows
        try:
            _check_storage(out, lists, compact)
            assert "mine" in out.samples(limit=1).columns and out.column_info("mine")["has_missing"] is True
        finally:
            out.free()
    finally:
        e1.free()
        e2.free()


# ------------------------------------------------------------------ 6. lifetimes

def test_the_same_table_twice_and_a_clone_that_outlives_its_source(ctx):
    blocks = BLOCKS["c"]
    src = build(ctx, blocks, compact=True)
    twice = _check_concat(ctx, [src, src], [blocks, blocks])
    st = twice.concat_stats()
    assert st["transcodes"] == 0 and st["lut_transcodes"] == 0 and st["copies"] == 2 * 6, st      # like-stored: all copies
    twice.free()
    clone = _check_concat(ctx, [src], [blocks])
    src.free()
    filler = build(ctx, [(4096, {"n": ("int", np.zeros(4096, dtype=np.int64), None)})])   # reuses the freed memory
    try:
        assert _rows(clone) == D.rows_of(blocks)
        assert clone.concat_stats()["rows"] == clone.rows and clone.select_stats()["rows_in"] == 0
        q = clone.query(groups=["extra"], aggs=["w2"])
        res = q.run()
        assert res.matched == clone.rows
        res.free()
        q.free()
    finally:
        clone.free()
        filler.free()


def test_prepared_query_on_a_source_survives_the_concat(ctx, tables):
    a, b = tables("a", "compact"), tables("b", "compact")
    q = a.query(groups=["s"], aggs=["ni"], op="hist", want_percentiles=True)

    def scan():
        res = q.scan().finalize()
        out = (res.matched, [(r["group_by_key"], r["count"], r["hists"][0]["sum"]) for r in res.results])
        res.free()
        return out
    try:
        before, shape = scan(), (a.rows, a.blocks, b.rows, b.blocks)
        out = ctx.concat([b, a])
        assert scan() == before and (a.rows, a.blocks, b.rows, b.blocks) == shape      # no version moved: no SYBL_E_STATE
        out.free()
        assert a.concat_stats()["rows"] == 0                                             # zeros for a table no concat made
    finally:
        q.free()


# ------------------------------------------------------------------ 7. queries against the oracle

HOSTS = ["host%02d" % k for k in range(20)]
T0 = 1_700_000_000
Q_NAMES = [("g", "int"), ("v", "int"), ("wt", "int"), ("time", "int"), ("s", "str")]


def _log_table(ctx, n, seed, v_hi, t0, hosts, compact, v_info):
    rng = np.random.default_rng(seed)
    c = {"g": rng.integers(0, 12, n).astype(np.int64), "v": rng.integers(0, v_hi + 1, n).astype(np.int64),
         "wt": rng.integers(1, 6, n).astype(np.int64), "time": (t0 + np.arange(n) // 4).astype(np.int64)}
    c["v"][:2] = (0, v_hi)
    sid = rng.integers(0, len(hosts), n)
    tb = ctx.create_table("q")
    for name in ("g", "wt", "time"):
        tb.add_column(name, "int")
    tb.add_column("v", "int", *(v_info or (1, 0)))
    tb.add_column("s", "str")
    blocks = []
    for r0 in range(0, n, 3000):            # not a multiple of 32: every block is followed by padding rows
        sl = slice(r0, min(n, r0 + 3000))
        m = sl.stop - r0
        tb.append_block(m, {"g": c["g"][sl], "v": c["v"][sl], "wt": c["wt"][sl], "time": c["time"][sl], "s": {"ids": sid[sl], "strings": hosts}})
        cols = {k: ("int", c[k][sl], None) for k in ("g", "v", "wt", "time")}
        cols["s"] = ("str", [hosts[k] for k in sid[sl].tolist()])
        blocks.append((m, cols))
    if compact:
        tb.compact()
    return tb, blocks


QUERIES = {
    "hist_percentiles": (dict(groups=["s"], aggs=["v"], op="hist", want_percentiles=True), dict(full=True)),
    "weighted": (dict(groups=["g"], aggs=["v"], op="avg", weight_col="wt"), {}),
    "time_series": (dict(groups=["g"], aggs=["v"], op="avg", time_col="time", time_bucket=600), dict(time_mode=True)),
}


@pytest.fixture(scope="module")
def log_tables(ctx):
    made = {}
    for mode, compact_b, info_b in (("compact", True, (0, 1499)), ("mixed", False, (0, 1499)), ("info_missing", True, None)):
        a, la = _log_table(ctx, 20000, 1, 999, T0, HOSTS, True, (0, 999))
        b, lb = _log_table(ctx, 14000, 2, 1499, T0 + 5000, HOSTS[::-1][:15] + ["new0", "new1"], compact_b, info_b)
        made[mode] = (ctx.concat([a, b]), R.concat_ref([la, lb]), R.merged_dict([a.column_dict("s"), b.column_dict("s")]))
        a.free()
        b.free()
    yield made
    for out, _, _ in made.values():
        out.free()


@pytest.mark.parametrize("which", sorted(QUERIES))
@pytest.mark.parametrize("mode", ["compact", "mixed", "info_missing"])
def test_queries_agree_with_the_oracle(log_tables, oracle, mode, which):
    out, ref, merged = log_tables[mode]
    q, cmp = QUERIES[which]
    # IntInfo: given in every source -- the minimum of the minima, the maximum of the maxima; not given in one -- the exact extrema
    info = out.column_info("v")
    assert (info["info_min"], info["info_max"]) == (0, 1499)
    assert out.column_storage("v") == ((2, 0) if mode != "mixed" else (8, 0)) and out.column_dict("s") == merged
    assert _against_oracle(oracle, out, ref, Q_NAMES, {"s": merged}, q, {"v": (0, 1499)}, **cmp) == 34000


def test_int_info_is_given_only_when_every_source_gave_it(ctx, oracle):
    """The hist geometry follows the inherited IntInfo: [0, 4999] given by both sources against the exact [3, 1383]."""
    tabs = []
    try:
        for given in ((0, 2999), (100, 4999), None):
            tb = ctx.create_table("i")
            tb.add_column("v", "int", *(given or (1, 0)))
            tb.append_block(70, {"v": 3 + (np.arange(70, dtype=np.int64) * 20) % 1400})
            tabs.append(tb)
        ref = [(70, {"v": ("int", 3 + (np.arange(70, dtype=np.int64) * 20) % 1400, None)})] * 2
        for srcs, want in (((tabs[0], tabs[1]), (0, 4999)), ((tabs[0], tabs[2]), (3, 1383))):
            out = ctx.concat(list(srcs))
            try:
                info = out.column_info("v")
                assert (info["info_min"], info["info_max"]) == want
                q = dict(aggs=["v"], op="hist", want_percentiles=True)
                _against_oracle(oracle, out, ref, [("v", "int")], {}, q, {"v": want}, full=True)
                query = out.query(**q)
                res = query.run()
                assert res.cumulative["hists"][0]["bucket_size"] == oracle.setup_buckets(*want)["bucket_size"]
                res.free()
                query.free()
            finally:
                out.free()
    finally:
        for tb in tabs:
            tb.free()


# ------------------------------------------------------------------ 8. the workflow

def test_digest_of_arrivals_folded_into_a_digested_table(ctx):
    rng = np.random.default_rng(4)

    def table(sizes, t_lo, t_hi, names):
        n = sum(sizes)
        return _cut({"time": (rng.integers(t_lo, t_hi, n).astype(np.int64), rng.random(n) > 0.05), "row": (rng.integers(0, 1 << 20, n).astype(np.int64), None)},
                    {"s": [names[k] for k in rng.integers(0, len(names), n).tolist()]}, {}, sizes)
    la, lb = table((2049, 70, 8197, 33), 1000, 90000, ["a", "b", "c"]), table((31, 2047, 1), 50000, 200000, ["c", "d", "a"])
    a, b = build(ctx, la, compact=True), build(ctx, lb, compact=True)
    made = []
    try:
        made.append(a.digest(block_rows=4096))
        made.append(ctx.concat([made[0], b]))
        assert made[1].blocks == made[0].blocks + 3
        made.append(made[1].digest(block_rows=4096))
        assert _rows(made[2]) == D.rows_of(D.digest_ref(la + lb, block_rows=4096))
        assert made[2].column_dict("s") == ["a", "b", "c", "d"]
    finally:
        for t in [a, b] + made:
            t.free()


def test_save_and_open_round_trip(ctx, tmp_path):
    blocks = [(s, {k: v for k, v in c.items() if k != "tags"}) for s, c in BLOCKS["b"]]
    src = build(ctx, blocks, compact=True, name="events")
    out = ctx.concat([src])
    back = None
    try:
        out.save(str(tmp_path))
        back = ctx.open_table(str(tmp_path), "events")
        assert back.rows == out.rows == src.rows and back.blocks == out.blocks == len(blocks)
        assert _rows(back) == _rows(out) == D.rows_of(blocks)
    finally:
        for t in (back, out, src):
            if t is not None:
                t.free()


# ------------------------------------------------------------------ 9. dead blocks

def test_dead_blocks_contribute_nothing(ctx, tmp_path):
    blocks = []
    for b, n in enumerate((300, 1000, 77, 450, 33)):
        i = np.arange(n)
        blocks.append((n, {"time": ("int", ((i * 7919 + b * 13) % 500 - 100).astype(np.int64), (i % 5 != 0)),
                           "row": ("int", (i + 10000 * b).astype(np.int64)),
                           "name": ("str", [None if k % 9 == 0 else "user%d" % (k % 50) for k in i])}))
    root = str(tmp_path / "db")
    F.write_table(root, "events", [cols for _, cols in blocks])
    tb = ctx.open_table(root, "events", compact=True)
    extra = build(ctx, blocks[:1], compact=True)
    out = None
    try:
        assert tb.blocks == 5
        shutil.rmtree(os.path.join(root, "events", "block%09d" % 2))
        shutil.rmtree(os.path.join(root, "events", "block%09d" % 4))
        assert tb.refresh()[1] == 2 and tb.rows == 300 + 77 + 33
        live = [blocks[0], blocks[2], blocks[4]]
        out = ctx.concat([tb, extra])
        assert out.rows == 300 + 77 + 33 + 300 and out.blocks == 4
        rows = _rows(out)
        assert rows == D.rows_of(live + blocks[:1])
        assert not any(10000 <= r["row"] < 20000 or 30000 <= r["row"] < 40000 for r in rows)
        assert out.concat_stats()["runs"] > 2            # the dead blocks cut the first source into runs
    finally:
        for t in (out, extra, tb):
            if t is not None:
                t.free()


def test_three_runs_between_dead_blocks_are_transcoded(ctx, tmp_path):
    """Live blocks of 33, 1 and 300 rows with a dead block between each pair: three runs of 64, 32 and 320 padded rows.  The second
    source widens `row` and lowers the base of `time`, so k_cc_transcode walks the first source's run list -- both run boundaries
    inside one wave, at 2 and 8 rows per lane -- and k_cc_valid its block list."""
    blocks = []
    for b, n in enumerate((33, 40, 1, 50, 300)):
        i = np.arange(n)
        blocks.append((n, {"time": ("int", ((i * 7919 + b * 13) % 500 - 100).astype(np.int64), (i % 5 != 0) | (n == 1)),
                           "row": ("int", (i + 1000 * b).astype(np.int64)),
                           "name": ("str", [None if k % 9 == 4 else "user%d" % (k % 50) for k in i])}))
    j = np.arange(40)
    wide = [(40, {"time": ("int", (j * 3 - 30000).astype(np.int64), j % 7 != 0),
                  "row": ("int", (j + (1 << 20)).astype(np.int64)),
                  "name": ("str", ["user%d" % (k % 50) for k in j])})]
    root = str(tmp_path / "db")
    F.write_table(root, "events", [cols for _, cols in blocks])
    tb = ctx.open_table(root, "events", compact=True)
    extra = build(ctx, wide, compact=True)
    out = None
    try:
        shutil.rmtree(os.path.join(root, "events", "block%09d" % 2))
        shutil.rmtree(os.path.join(root, "events", "block%09d" % 4))
        assert tb.refresh()[1] == 2 and tb.rows == 334
        live = [blocks[0], blocks[2], blocks[4]]
        out = ctx.concat([tb, extra])
        assert out.rows == 374 and out.blocks == 4
        assert _rows(out) == D.rows_of(R.concat_ref([live, wide]))
        st = out.concat_stats()
        assert st["runs"] == 4 and st["transcodes"] >= 2, st
        for name in ("time", "row"):                     # the first source does not have the output's stored form: it was transcoded
            assert out.column_storage(name) != tb.column_storage(name), name
        assert out.column_storage("row") == (4, 0) and out.column_storage("time")[0] == 2
        n = out.rows
        ref = D.concat(live + wide)
        for name in ("time", "row"):
            _, v, p = ref[name]
            assert np.array_equal(out.read_int(name, 0, n)[p], v[p]), name
    finally:
        for t in (out, extra, tb):
            if t is not None:
                t.free()


# ------------------------------------------------------------------ 10. the C example

def test_c_example_runs(ctx, tmp_path):
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    exe = str(tmp_path / "example_concat")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "example_concat.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()

    def table(sizes, time0, lat0, lat_mod, hosts):
        blocks, t = [], time0
        for n in sizes:
            i = np.arange(n, dtype=np.int64)
            blocks.append((n, {"time": ("int", t + i, None), "latency": ("int", lat0 + (i * 37) % lat_mod, None),
                               "host": ("str", [hosts[k % 3] for k in range(n)])}))
            t += n
        return blocks
    la, lb = table((1000, 1000), T0, 0, 200, ["web1", "web2", "db1"]), table((700,), T0 + 2000, 10000, 60000, ["db1", "cache1", "web1"])
    a, b = build(ctx, la, compact=True), build(ctx, lb, compact=True)
    out = ctx.concat([a, b])
    try:
        st = out.concat_stats()
        assert lines[0] == "concat: 2700 rows in 3 blocks from 2 tables, 3 columns" and (out.rows, out.blocks) == (2700, 3)
        assert lines[1] == "pieces: %d copies, %d transcodes, %d through an id table" % (st["copies"], st["transcodes"], st["lut_transcodes"])
        assert (st["copies"], st["transcodes"], st["lut_transcodes"]) == (2, 3, 1)
        assert lines[2] == "latency: %d bytes from base %d" % out.column_storage("latency") == "latency: 2 bytes from base 0"
        assert lines[3] == "hosts: " + " ".join(out.column_dict("host")) == "hosts: web1 web2 db1 cache1"
        q = out.query(groups=["host"], aggs=["latency"], op="avg")
        res = q.run()
        want = sorted("group %s count %d sum %d" % (r["group_by_key"], r["count"], r["hists"][0]["sum"]) for r in res.results)
        res.free()
        q.free()
        assert sorted(lines[4:]) == want and len(want) == 4
        rows = D.rows_of(R.concat_ref([la, lb]))
        # (a group_by_key ends with the reference's key delimiter, a tab)
        assert [w.replace("\t", "") for w in want] == sorted("group %s count %d sum %d" % (h, sum(1 for r in rows if r["host"] == h), sum(r["latency"] for r in rows if r["host"] == h))
                              for h in ("web1", "web2", "db1", "cache1"))
    finally:
        for t in (out, a, b):
            t.free()
