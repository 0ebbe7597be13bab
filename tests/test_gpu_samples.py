"""GPU: samples queries (`sybil query -samples`: Table.samples / sybl_table_samples, csrc/samples.hip) against the numpy
restatement in tests/samples_ref.py.  Tables are built block by block through append_block from the very arrays the
restatement reads; every comparison is exact: rows, row ids, matched, blocks_visited."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import samples_ref as R
from tests import sybil_fixture as F

pytestmark = pytest.mark.gpu

FIRST_WINDOW = 16  # csrc/samples.hip: kSmpFirstWindow


@pytest.fixture(scope="module")
def ctx():
    import sybil_amd
    c = sybil_amd.Context(0)
    yield c
    c.close()


def _engine_block(cols, nrows):
    """A block of samples_ref's form as Table.append_block takes it (block-local dictionaries)."""
    out = {}
    for name, spec in cols.items():
        if spec[0] == "int":
            pop = spec[2] if len(spec) > 2 else None
            out[name] = np.asarray(spec[1], dtype=np.int64) if pop is None else (np.asarray(spec[1], dtype=np.int64), pop)
        elif spec[0] == "str":
            strings = list(dict.fromkeys(s for s in spec[1] if s is not None))
            ix = {s: i for i, s in enumerate(strings)}
            out[name] = dict(ids=[ix[s] if s is not None else 0 for s in spec[1]], strings=strings,
                             populated=[s is not None for s in spec[1]])
        else:
            strings = list(dict.fromkeys(m for s in spec[1] if s is not None for m in s))
            ix = {s: i for i, s in enumerate(strings)}
            off, ids = [0], []
            for s in spec[1]:
                ids += [ix[m] for m in (s or [])]
                off.append(len(ids))
            out[name] = dict(offsets=off, ids=ids, strings=strings, populated=[s is not None for s in spec[1]])
    return out


def build(ctx, blocks, compact=False, name="t"):
    tb = ctx.create_table(name)
    types = {}
    for _, cols in blocks:
        for cname, spec in cols.items():
            types.setdefault(cname, spec[0])
    for cname, ty in types.items():
        tb.add_column(cname, ty)
    for nrows, cols in blocks:
        tb.append_block(nrows, _engine_block(cols, nrows))
    if compact:
        tb.compact()
    return tb


def check(tb, blocks, **kw):
    got = tb.samples(**kw)
    ref = R.samples_ref(blocks, **kw)
    assert got.info["matched"] == ref["matched"], kw
    assert got.info["blocks_visited"] == ref["blocks_visited"], kw
    assert got.info["blocks_total"] == len(blocks) and got.info["n_rows"] == len(ref["rows"])
    assert got.row_ids.tolist() == ref["row_ids"], kw
    assert got.rows == ref["rows"], kw
    assert json.loads(got.json()) == ref["rows"], kw
    return got


# ------------------------------------------------------------------ 1. block and word edges

EDGE_ROWS = [1, 31, 33, 2047, 2049, 65536, 5]   # 32-row padding, the 2048-row tile, one full reference block
EDGE_BASE5 = sum(EDGE_ROWS[:5])                 # first logical row of the 65536-row block


def _edge_blocks():
    blocks, base = [], 0
    for n in EDGE_ROWS:
        v = np.arange(base, base + n, dtype=np.int64)
        blocks.append((n, {"v": ("int", v, None), "m": ("int", v % 7, None)}))
        base += n
    return blocks


def _rows_of_big_block(first, last):
    """v filters that match exactly the local rows [first, last] of the 65536-row block."""
    return [("v", "gt", EDGE_BASE5 + first - 1), ("v", "lt", EDGE_BASE5 + last + 1)]


EDGE_FILTERS = {
    "none": [],
    "m_eq_3": [("m", "eq", 3)],
    "m_neq_3": [("m", "neq", 3)],
    "word_bits_0_to_31": _rows_of_big_block(0, 31),            # one whole word
    "word_bit_31_to_bit_0": _rows_of_big_block(31, 32),        # the last bit of a word and the first of the next
    "across_wave_step": _rows_of_big_block(2047, 2048),        # words 63 | 64: two waves of the compaction
    "across_workgroup_chunk": _rows_of_big_block(8191, 8192),  # words 255 | 256: two chunks of the block walk
    "bit_0_to_bit_31_far": _rows_of_big_block(32 * 100, 32 * 300 + 31),
    "all_but_the_ends": [("v", "gt", 0), ("v", "lt", sum(EDGE_ROWS) - 1)],
}


@pytest.fixture(scope="module")
def edge_table(ctx):
    blocks = _edge_blocks()
    tb = build(ctx, blocks)
    yield tb, blocks
    tb.free()


@pytest.mark.parametrize("which", sorted(EDGE_FILTERS))
def test_block_and_word_edges(edge_table, which):
    tb, blocks = edge_table
    filters = EDGE_FILTERS[which]
    counts = [int(R.block_matches(b, filters).sum()) for b in blocks]
    total = sum(counts)
    # 0, 1, around the full count, and every value at which the running count EQUALS the limit at a block boundary (strict >)
    limits = {0, 1, total - 1, total, total + 1} | {int(c) for c in np.cumsum(counts)}
    for limit in sorted(x for x in limits if x >= 0):
        check(tb, blocks, filters=filters, columns=["v"], limit=limit)
    check(tb, blocks, filters=filters, limit=3)   # every column


# ------------------------------------------------------------------ 2. storage

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _storage_blocks():
    blocks, base = [], 0
    for n in (100, 2049, 33):
        i = np.arange(base, base + n, dtype=np.int64)
        edge = (i * 7919) % 1000 - 500
        edge[n // 2] = I64_MIN if base == 0 else I64_MAX
        edge[0] = I64_MAX if base == 0 else I64_MIN
        blocks.append((n, {"w1": ("int", 1000 + (i * 37) % 200, None),
                           "w2": ("int", -3 + (i * 7) % 60000, None),
                           "w4": ("int", 5 + (i * 100003) % (1 << 31), None),
                           "w8": ("int", (i * 2654435761) % (1 << 40) - (1 << 39), None),
                           "edge": ("int", edge, None)}))
        base += n
    return blocks


@pytest.fixture(scope="module", params=["canonical", "compact"])
def storage_table(ctx, request):
    blocks = _storage_blocks()
    tb = build(ctx, blocks, compact=request.param == "compact")
    if request.param == "compact":
        assert [tb.column_storage(c)[0] for c in ("w1", "w2", "w4", "w8", "edge")] == [1, 2, 4, 8, 8]
    else:
        assert tb.column_storage("w1") == (8, 0)
    yield tb, blocks
    tb.free()


def test_storage_widths_as_output(storage_table):
    tb, blocks = storage_table
    check(tb, blocks, limit=5000)
    check(tb, blocks, filters=[("w2", "gt", 100), ("w2", "lt", 50000)], limit=150)
    check(tb, blocks, filters=[("w1", "eq", 1037)], limit=1000)
    check(tb, blocks, filters=[("w8", "gt", 0), ("w4", "lt", 1 << 30)], limit=1000)
    check(tb, blocks, filters=[("edge", "eq", I64_MIN)], limit=10)
    check(tb, blocks, filters=[("edge", "gt", I64_MAX - 1)], limit=10)


@pytest.mark.parametrize("col", ["w1", "w2", "w4", "w8", "edge"])
def test_storage_widths_as_order_key(storage_table, col):
    tb, blocks = storage_table
    for asc in (False, True):
        check(tb, blocks, order_by=col, order_asc=asc, limit=40, columns=[col, "w2"])
        check(tb, blocks, filters=[("w2", "lt", 30000)], order_by=col, order_asc=asc, limit=3000)


# ------------------------------------------------------------------ 3. types

def _typed_blocks():
    rng = np.random.default_rng(11)
    blocks = []
    for b, n in enumerate((70, 2100, 45)):
        i = np.arange(n)
        name = [None if k % 5 == 0 else "user%d" % (k % 9) for k in i + b]
        host = ["web%02d" % (k % 4) if k % 3 else "db-%d" % (k % 2) for k in i]
        tags = [None if k % 7 == 0 else ([] if k % 7 == 1 else ["tag%d" % x for x in range(k % 4, k % 4 + 1 + k % 3)]) for k in i + b]
        sparse = rng.integers(-50, 50, size=n).astype(np.int64)
        cols = {"id": ("int", np.arange(n, dtype=np.int64) + 10000 * b, None),
                "sparse": ("int", sparse, rng.random(n) > 0.3),
                "name": ("str", name), "host": ("str", host), "tags": ("set", tags)}
        if b == 1:
            del cols["sparse"], cols["name"]      # columns absent from one block
        blocks.append((n, cols))
    return blocks


@pytest.fixture(scope="module", params=["canonical", "compact"])
def typed_table(ctx, request):
    blocks = _typed_blocks()
    tb = build(ctx, blocks, compact=request.param == "compact")
    yield tb, blocks
    tb.free()


def test_types_every_column(typed_table):
    tb, blocks = typed_table
    got = check(tb, blocks, limit=3000)                 # columns=None: every column
    assert sorted(got.columns) == ["host", "id", "name", "sparse", "tags"]
    assert any("name" not in r for r in got.rows) and any(r.get("tags") == [] for r in got.rows)
    assert any(len(r.get("tags", [])) > 1 for r in got.rows) and any("tags" not in r for r in got.rows)
    check(tb, blocks, columns=["tags", "name"], limit=7)


@pytest.mark.parametrize("filters", [
    [("name", "eq", "user3")],
    [("name", "neq", "user3")],
    [("host", "re", "^web0[12]")],
    [("host", "nre", "web")],
    [("tags", "in", "tag2")],
    [("tags", "nin", "tag2")],
    [("sparse", "gt", 0)],
    [("sparse", "neq", 7), ("tags", "in", "tag1"), ("host", "re", "web.*")],
    [("name", "eq", "nobody")],
], ids=lambda f: "+".join("%s_%s" % (c, o) for c, o, _ in f))
def test_types_filters(typed_table, filters):
    tb, blocks = typed_table
    for limit in (4, 100000):
        check(tb, blocks, filters=filters, limit=limit)
    check(tb, blocks, filters=filters, order_by="sparse", limit=50)


# ------------------------------------------------------------------ 4. sorted

def _sorted_blocks():
    rng = np.random.default_rng(5)
    blocks, base = [], 0
    for n in (40, 2500, 300):
        k = rng.integers(-2, 3, size=n).astype(np.int64)        # a 5-value domain: ties
        blocks.append((n, {"k": ("int", k, rng.random(n) > 0.25), "row": ("int", np.arange(base, base + n, dtype=np.int64), None)}))
        base += n
    return blocks


@pytest.fixture(scope="module", params=["canonical", "compact"])
def sorted_table(ctx, request):
    blocks = _sorted_blocks()
    tb = build(ctx, blocks, compact=request.param == "compact")
    yield tb, blocks
    tb.free()


@pytest.mark.parametrize("asc", [False, True])
def test_sorted_ties_and_missing(sorted_table, asc):
    tb, blocks = sorted_table
    whole = R.samples_ref(blocks, order_by="k", order_asc=asc, limit=100000)
    n_missing = sum(1 for r in whole["rows"] if "k" not in r)
    assert 100 < n_missing < whole["matched"] - 100
    # limits that cut inside the missing group, at its edge, inside a tie group, and beyond everything; a small limit closes
    # the visit after the first block, the larger ones visit further
    for limit in (3, 39, 40, n_missing - 5, n_missing, n_missing + 7, whole["matched"] - n_missing - 3, 100000):
        check(tb, blocks, order_by="k", order_asc=asc, limit=limit)
    check(tb, blocks, order_by="k", order_asc=asc, limit=900, columns=["row"])       # the order column is not returned
    check(tb, blocks, filters=[("k", "neq", 0)], order_by="k", order_asc=asc, limit=500)
    check(tb, blocks, order_by="row", order_asc=asc, limit=50)                       # no missing rows: one sort pass


# ------------------------------------------------------------------ 5. early exit

@pytest.fixture(scope="module")
def many_blocks_table(ctx):
    blocks = [(1024, {"v": ("int", np.arange(b * 1024, (b + 1) * 1024, dtype=np.int64), None)}) for b in range(64)]
    tb = build(ctx, blocks, compact=True)
    yield tb, blocks
    tb.free()


def test_early_exit_follows_the_visited_prefix(many_blocks_table):
    tb, blocks = many_blocks_table
    got = check(tb, blocks, filters=[("v", "gt", -1)], limit=100)
    assert got.info["blocks_visited"] == 1
    assert 1 <= got.info["blocks_filtered"] <= max(FIRST_WINDOW, 4 * got.info["blocks_visited"])
    got = check(tb, blocks, limit=100)                   # no filters: no filter pass at all
    assert got.info["blocks_visited"] == 1 and got.info["blocks_filtered"] == 0
    got = check(tb, blocks, filters=[("v", "gt", 63 * 1024 + 1000)], limit=100)   # matches only in the last block
    assert got.info["blocks_visited"] == 64 and got.info["matched"] == 23 and got.info["blocks_filtered"] == 64
    got = check(tb, blocks, filters=[("v", "gt", 20 * 1024 - 3)], limit=2)   # the second window ends the visit
    assert got.info["blocks_visited"] == 21


# ------------------------------------------------------------------ 6. loader path

@pytest.mark.parametrize("compact", [False, True])
def test_table_opened_from_disk(ctx, tmp_path, compact):
    blocks = []
    for b, n in enumerate((300, 1000, 77)):
        i = np.arange(n)
        tags = [["t0", "t1", "t2", "t3"]] + [None if k % 6 == 0 else ["t%d" % x for x in range(k % 3, k % 3 + 1 + k % 2)] for k in i[1:]]
        cols = {"age": ("int", (10 + i % 20).astype(np.int64), None),
                "big": ("int", ((i * 48271) % 5000 - 2500).astype(np.int64), (i % 4 != 0)),
                "name": ("str", [None if k % 9 == 0 else "user%d" % (k % 50) for k in i]),
                "tags": ("set", tags)}
        if b == 1:
            del cols["big"]           # a block without the column file
        blocks.append((n, cols))
    root = str(tmp_path / "db")
    F.write_table(root, "events", [{c: s for c, s in cols.items()} for _, cols in blocks])
    tb = ctx.open_table(root, "events", compact=compact)
    try:
        assert tb.rows == sum(n for n, _ in blocks) and tb.blocks == 3
        check(tb, blocks, limit=5000)
        check(tb, blocks, filters=[("big", "gt", 0), ("tags", "in", "t2")], order_by="age", limit=200)
        check(tb, blocks, filters=[("name", "re", "user1.")], limit=33)
    finally:
        tb.free()


# ------------------------------------------------------------------ 7. lifetime

def test_result_outlives_its_table(ctx):
    from sybil_amd import _native as N
    blocks = [(3, {"n": ("int", np.array([4, 5, 6], dtype=np.int64), None), "s": ("str", ["a", None, "c"]),
                   "t": ("set", [["x", "y"], [], None])})]
    tb = build(ctx, blocks)
    L = N.lib()
    d = N.SamplesDesc()
    d.order_by, d.limit = b"$COUNT", 10
    h = C.c_void_p()
    N.check(L.sybl_table_samples(tb._h, C.byref(d), C.byref(h)))
    tb.free()
    filler = build(ctx, [(4096, {"n": ("int", np.zeros(4096, dtype=np.int64), None)})])   # reuses the freed memory
    try:
        info = N.SamplesInfo()
        N.check(L.sybl_samples_get_info(h, C.byref(info)))
        assert (info.n_rows, info.matched, info.n_columns) == (3, 3, 3)
        seen = {}
        for c in range(3):
            col = N.SamplesCol()
            N.check(L.sybl_samples_column(h, c, C.byref(col)))
            seen[col.name] = col
        assert [seen[b"n"].ints[i] for i in range(3)] == [6, 5, 4]
        assert [seen[b"s"].strings[i] for i in range(3)] == [b"c", None, b"a"]
        assert [seen[b"s"].str_ids[i] for i in range(3)][1] == -1
        assert [seen[b"t"].set_off[i] for i in range(4)] == [0, 0, 0, 2]
        assert [seen[b"t"].set_strings[i] for i in range(2)] == [b"x", b"y"]
        assert L.sybl_samples_render(h) == b'[{"n":6,"s":"c"},{"n":5,"t":[]},{"n":4,"s":"a","t":["x","y"]}]'
    finally:
        L.sybl_samples_free(h)
        filler.free()


# ------------------------------------------------------------------ 8. JSON bytes

def test_json_bytes(ctx):
    blocks = [(3, {"b": ("int", np.array([1, -5, 7], dtype=np.int64), None), "a": ("str", ["x", "<a&b>", None]),
                   "Z": ("set", [["p", "q\"r"], None, []])})]
    tb = build(ctx, blocks)
    try:
        got = tb.samples(limit=10)
        # keys in bytewise order ("Z" < "a" < "b"), unpopulated columns absent, HTML escaped as encoding/json does
        assert got.json() == '[{"Z":[],"b":7},{"a":"\\u003ca\\u0026b\\u003e","b":-5},{"Z":["p","q\\"r"],"a":"x","b":1}]'
        assert tb.samples(limit=0).json() == "[]"
        assert tb.samples(filters=[("b", "gt", 100)], limit=5).json() == "[]"
    finally:
        tb.free()


# ------------------------------------------------------------------ 9. errors

def test_errors(ctx):
    import sybil_amd
    cols = {"c%d" % k: ("int", np.arange(10, dtype=np.int64), None) for k in range(9)}
    cols["s"] = ("str", ["x"] * 10)
    cols["t"] = ("set", [["x"]] * 10)
    tb = build(ctx, [(10, cols)])
    try:
        for kw, word in ((dict(columns=["nope"]), "nope"), (dict(filters=[("nope", "gt", 1)]), "nope"), (dict(order_by="nope"), "nope"),
                         (dict(order_by="s"), "order_by"), (dict(order_by="t"), "order_by"), (dict(limit=-1), "limit"),
                         (dict(filters=[("c%d" % k, "gt", -1) for k in range(9)]), "8")):
            with pytest.raises(sybil_amd.SyblError) as ei:
                tb.samples(**kw)
            assert ei.value.code == -1 and word in str(ei.value), (kw, str(ei.value))
        # eight filter columns (several filters on one of them) are served
        eight = [("c%d" % k, "gt", 2) for k in range(8)] + [("c0", "lt", 8), ("c0", "neq", 5)]
        check(tb, [(10, cols)], filters=eight, limit=10)
    finally:
        tb.free()


def test_empty_table(ctx):
    tb = ctx.create_table("empty")
    tb.add_column("v", "int")
    try:
        got = tb.samples(limit=5)
        assert got.rows == [] and got.info["matched"] == 0 and got.info["blocks_visited"] == 0 and got.json() == "[]"
    finally:
        tb.free()


# ------------------------------------------------------------------ 10. no interference

def test_aggregate_queries_are_untouched(typed_table):
    tb, blocks = typed_table

    def agg():
        q = tb.query(filters=[("tags", "in", "tag1")], groups=["host"], aggs=["id"], op="hist")
        res = q.run()
        rows = [(r["group_by_key"], r["count"], r["hists"][0]["sum"], r["hists"][0]["percentiles"].tolist()) for r in res.results]
        out = (res.matched, rows, res.render("json"))
        res.free()
        q.free()
        return out

    before = agg()
    check(tb, blocks, filters=[("tags", "in", "tag1")], order_by="sparse", limit=20)
    check(tb, blocks, limit=20)
    assert agg() == before
