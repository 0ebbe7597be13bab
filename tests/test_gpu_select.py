"""GPU: table select (Table.select / sybl_table_select, csrc/select.hip) against the numpy restatement in
tests/select_ref.py.  Tables are built block by block through append_block, with irregular block sizes so that the source has
padding rows; the selected table is read back with samples(limit=N) and read_int.  Every comparison is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import digest_ref as D
from tests import parity
from tests import select_ref as S
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
SMALL = (70, 1, 130, 33, 2049, 31, 64, 5000, 777, 32)
# a one-row block first: the big blocks then start on a padded physical row; 8196 rows cross the 256-word chunk of
# k_sel_rows, 65536 is the reference's block
LARGE = (1, 65536, 70, 33, 130, 2049, 31, 8197, 64, 5000, 777, 32)
EDGES = (31, 32, 2047, 2048, 8191, 8192)
FULL_READBACK = 20000     # selections of more rows are read back whole for one predicate only


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


def _sizes(n):
    pattern = SMALL if n <= 1000 else LARGE
    out, k = [], 0
    while n > 0:
        s = min(n, pattern[k % len(pattern)])
        out.append(s)
        n -= s
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def _blocks(n, seed=3):
    """n rows of every column kind in irregular blocks, made once per n.  `row` is the table-wide row, `par` its parity;
    `edge` marks the rows whose table-wide OR block-local index is one of EDGES, `ends` the first and last row of a block."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    sizes = _sizes(n)
    local = np.concatenate([np.arange(s, dtype=np.int64) for s in sizes])
    last = np.concatenate([np.arange(s, dtype=np.int64) == s - 1 for s in sizes])
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[0] = -(1 << 63)
    if n > 1:
        w8[n // 2] = (1 << 63) - 1
    sid = rng.integers(0, 50, size=n)
    spop = rng.random(n) > 0.25
    tlen = rng.integers(0, 5, size=n)
    tfirst = rng.integers(0, 6, size=n)
    tpop = rng.random(n) > 0.25
    flat = {"w1": (1000 + (i * 37) % 200, None), "w2": (-3 + (i * 7) % 60000, None), "w4": (5 + (i * 100003) % (1 << 31), None),
            "w8": (w8, None), "ni": (rng.integers(-500, 500, size=n).astype(np.int64), rng.random(n) > 0.3),
            "row": (i, None), "par": (i % 2, None), "edge": ((np.isin(i, EDGES) | np.isin(local, EDGES)).astype(np.int64), None),
            "ends": (((local == 0) | last).astype(np.int64), None)}
    strs = [("user%02d" % s if p else None) for s, p in zip(sid.tolist(), spop.tolist())]
    tags = [(["tag%d" % (f + k) for k in range(ln)] if p else None) for f, ln, p in zip(tfirst.tolist(), tlen.tolist(), tpop.tolist())]
    blocks, r0 = [], 0
    for s in sizes:
        sl = slice(r0, r0 + s)
        cols = {name: ("int", v[sl], None if p is None else p[sl]) for name, (v, p) in flat.items()}
        cols["s"] = ("str", strs[sl])
        cols["tags"] = ("set", tags[sl])
        blocks.append((s, cols))
        r0 += s
    return blocks


@pytest.fixture(scope="module")
def tables(ctx):
    """The source table of (n, storage), built on first use and kept for the module."""
    made = {}

    def get(n, storage):
        if (n, storage) not in made:
            made[(n, storage)] = build(ctx, _blocks(n), compact=storage == "compact")
        return made[(n, storage)]
    yield get
    for tb in made.values():
        tb.free()


def _rows(tb):
    """Every row of a table in row order (samples returns them newest first)."""
    n = tb.rows
    got = tb.samples(limit=max(n, 1))
    assert got.info["n_rows"] == n and got.row_ids.tolist() == list(range(n - 1, -1, -1))
    return got.rows[::-1]


def _check_select(src, blocks, filters=(), columns=None, block_rows=0, full=None):
    ref = S.select_ref(blocks, filters, columns, block_rows)
    names = S.output_columns(blocks, columns)
    m = sum(b[0] for b in ref)
    br = block_rows or S.BLOCK_ROWS
    n_src, b_src = src.rows, src.blocks
    sel = src.select(filters, columns, block_rows)
    try:
        assert sel.rows == m and sel.blocks == -(-m // br) == len(ref)
        assert src.rows == n_src and src.blocks == b_src
        st = sel.select_stats()
        assert (st["rows_in"], st["rows_out"], st["blocks_out"]) == (n_src, m, len(ref)), st
        assert sel.samples(limit=1).columns == names
        cols = D.concat(ref)
        for name in names:
            assert sel.column_storage(name) == src.column_storage(name), name
            if D.column_types(blocks)[name] != "int":
                assert sel.column_dict(name) == src.column_dict(name), name
            elif m:
                _, v, p = cols[name]
                assert np.array_equal(sel.read_int(name, 0, m)[p], v[p]), name
        if full if full is not None else m <= FULL_READBACK:
            assert _rows(sel) == D.rows_of(ref)
    finally:
        sel.free()
    return m


# ------------------------------------------------------------------ 1. rows, exactly

def _predicates(n):
    lo, hi = n // 5 + 3, n - n // 5 - 3          # whole interior blocks, the two at its ends cut
    return {
        "everything": [],
        "nothing": [("row", "lt", 0)],
        "every_other_row": [("par", "eq", 0)],
        "only_row_0": [("row", "eq", 0)],
        "only_the_last_row": [("row", "eq", n - 1)],
        "word_wave_chunk_edges": [("edge", "eq", 1)],
        "block_ends": [("ends", "eq", 1)],
        "range": [("row", "gt", lo), ("row", "lt", hi)],
    }


SHAPES = [(1, 0), (33, 32), (257, 100), (1000, 96), (8192 + 5, 100), (65536 + 77, 0), (3 * 65536, 0)]
PREDICATES = sorted(_predicates(10))


@pytest.mark.parametrize("storage", ["canonical", "compact"])
@pytest.mark.parametrize("which", PREDICATES)
@pytest.mark.parametrize("n,block_rows", SHAPES)
def test_rows_exactly(tables, storage, n, block_rows, which):
    blocks = _blocks(n)
    src = tables(n, storage)
    if storage == "compact" and n >= 1000:
        assert [src.column_storage(c)[0] for c in ("w1", "w2", "w4", "w8")] == [1, 2, 4, 8]
    elif storage == "canonical":
        assert src.column_storage("w1") == (8, 0) and src.column_storage("s") == (4, 0)
    filters = _predicates(n)[which]
    m = _check_select(src, blocks, filters, None, block_rows, full=True if which == "every_other_row" else None)
    want = {"everything": n, "nothing": 0, "every_other_row": (n + 1) // 2, "only_row_0": 1, "only_the_last_row": 1,
            "block_ends": sum(1 if s == 1 else 2 for s in _sizes(n))}.get(which)
    assert want is None or m == want
    if which == "word_wave_chunk_edges":
        assert m >= sum(1 for e in EDGES if e < n)


def test_the_shapes_cross_every_boundary():
    """What the shapes above are there for, stated on the source blocks themselves."""
    sizes = _sizes(3 * 65536)
    assert 65536 in sizes and any(8192 < s < 65536 for s in sizes) and any(s % 32 for s in sizes)
    assert max(_sizes(8192 + 5)) > 8192 and max(_sizes(65536 + 77)) == 65536
    for n in (8192 + 5, 65536 + 77):
        local_edges = sum(int(np.isin(np.arange(s), EDGES).sum()) for s in _sizes(n))
        assert local_edges >= len(EDGES)        # a block long enough to hold every edge row block-locally


# ------------------------------------------------------------------ 2. other filter kinds, filter errors

OTHER_FILTERS = {
    "str_eq": [("s", "eq", "user07")],
    "str_regex": [("s", "re", "^user[12]3$")],
    "set_member": [("tags", "in", "tag3")],
    "nullable": [("ni", "lt", 0)],
    "nullable_neq_and_set": [("ni", "neq", 0), ("tags", "nin", "tag0")],
}


@pytest.mark.parametrize("storage", ["canonical", "compact"])
@pytest.mark.parametrize("which", sorted(OTHER_FILTERS))
def test_other_filter_kinds(tables, storage, which):
    n = 8192 + 5
    m = _check_select(tables(n, storage), _blocks(n), OTHER_FILTERS[which], None, 96)
    assert 0 < m < n


def test_nine_distinct_filter_columns_are_refused(tables):
    import sybil_amd
    src = tables(1000, "compact")
    nine = [(c, "gt", -1) for c in ("w1", "w2", "w4", "row", "par", "edge", "ends")] + [("w8", "lt", 1 << 62), ("ni", "lt", 1000)]
    assert len({f[0] for f in nine}) == 9
    with pytest.raises(sybil_amd.SyblError) as ei:
        src.select(nine)
    assert ei.value.code == E_INVAL
    _check_select(src, _blocks(1000), nine[:8], None, 96)     # eight are the limit, not beyond it


# ------------------------------------------------------------------ 3. projection

@pytest.mark.parametrize("storage", ["canonical", "compact"])
def test_projection(tables, storage):
    n = 1000
    src, blocks = tables(n, storage), _blocks(n)
    # not table order; the filter column is not among the outputs; a name given twice counts once
    _check_select(src, blocks, [("par", "eq", 1)], ["tags", "w2", "s", "w8", "w2", "ni"], 96)
    _check_select(src, blocks, [("tags", "in", "tag2")], ["row"], 0)
    _check_select(src, blocks, [], ["s"], 100)


# ------------------------------------------------------------------ 4. lifetime

def test_output_survives_its_source(ctx):
    blocks = _blocks(1000)
    filters = [("par", "eq", 0)]
    want = D.rows_of(S.select_ref(blocks, filters, None, 96))
    src = build(ctx, blocks, compact=True)
    sel = src.select(filters, block_rows=96)
    src.free()
    filler = build(ctx, [(4096, {"n": ("int", np.zeros(4096, dtype=np.int64), None)})])   # reuses the freed memory
    again = None
    try:
        assert _rows(sel) == want
        again = sel.select(block_rows=100)             # a select of a select: the same rows, re-cut
        assert _rows(again) == want and again.blocks == 5
        assert again.select_stats()["rows_in"] == 500 and sel.digest_stats()["rows"] == 0
    finally:
        if again is not None:
            again.free()
        sel.free()
        filler.free()


def test_prepared_query_on_the_source_survives_the_select(tables):
    src = tables(1000, "compact")
    q = src.query(groups=["s"], aggs=["ni"], op="hist", want_percentiles=True)

    def scan():
        res = q.scan().finalize()
        out = (res.matched, [(r["group_by_key"], r["count"], r["hists"][0]["sum"]) for r in res.results])
        res.free()
        return out
    try:
        before = scan()
        sel = src.select([("par", "eq", 0)])
        assert scan() == before                          # the source's version did not move: no SYBL_E_STATE
        sel.free()
        assert src.select_stats()["rows_in"] == 0        # zeros for a table no select made
    finally:
        q.free()


# ------------------------------------------------------------------ 5. queries on the selected table agree with the oracle

N_Q = 100_000
SRC_BLOCK = 10_000            # not a multiple of 32: every source block is followed by padding rows
SEL_BLOCK = 512               # ~4700 rows are kept: ten blocks, time ascending over them
HOSTS = ["host%02d" % k for k in range(20)]
TAGS = ["t%d" % k for k in range(6)]
Q_NAMES = ["g", "v", "u", "time", "s", "tags"]
Q_FILTERS = [("u", "lt", 9000), ("tags", "in", "t2")]
T0 = 1_700_000_000


@pytest.fixture(scope="module")
def query_tables(ctx):
    """A log-like table (time ascending) in compact storage and the oracle's columns of it."""
    rng = np.random.default_rng(17)
    n = N_Q
    c = {"g": rng.integers(0, 12, n).astype(np.int64), "v": rng.integers(0, 1000, n).astype(np.int64),
         "u": rng.integers(0, 30_000, n).astype(np.int64), "time": (T0 + np.arange(n) // 4).astype(np.int64)}
    sid = rng.integers(0, len(HOSTS), n).astype(np.int32)
    tlen = rng.integers(0, 3, n)
    toff = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    tid = rng.integers(0, len(TAGS), int(toff[-1])).astype(np.int32)
    src = ctx.create_table("q")
    for name in ("g", "u", "time"):
        src.add_column(name, "int")
    src.add_column("v", "int", 0, 999)
    src.add_column("s", "str")
    src.add_column("tags", "set")
    for r0 in range(0, n, SRC_BLOCK):
        sl = slice(r0, r0 + SRC_BLOCK)
        o = toff[r0:r0 + SRC_BLOCK + 1]
        # (the whole vocabulary with every block: table-global ids == the ids the oracle is given)
        src.append_block(SRC_BLOCK, {"g": c["g"][sl], "v": c["v"][sl], "u": c["u"][sl], "time": c["time"][sl],
                                     "s": {"ids": sid[sl], "strings": HOSTS},
                                     "tags": {"ids": tid[o[0]:o[-1]], "offsets": o - o[0], "strings": TAGS}})
    src.compact()
    has_t2 = np.array([TAGS.index("t2") in tid[a:b] for a, b in zip(toff[:-1].tolist(), toff[1:].tolist())])
    keep = np.nonzero((c["u"] < 9000) & has_t2)[0]

    def ocols(order):
        lens = tlen[order]
        starts = toff[:-1][order]
        members = np.concatenate([tid[a:a + k] for a, k in zip(starts.tolist(), lens.tolist())])
        return [{"type": "int", "data": c["g"][order]}, {"type": "int", "data": c["v"][order]}, {"type": "int", "data": c["u"][order]},
                {"type": "int", "data": c["time"][order]}, {"type": "str", "data": sid[order]},
                {"type": "set", "data": members.astype(np.int32), "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)}]
    sel = src.select(Q_FILTERS, block_rows=SEL_BLOCK)
    assert sel.rows == len(keep) and 0 < len(keep) < n // 4
    assert [sel.column_storage(x) for x in Q_NAMES] == [src.column_storage(x) for x in Q_NAMES]
    yield src, sel, ocols(np.arange(n)), ocols(keep), c["time"][keep]
    sel.free()
    src.free()


def _oracle_kwargs(q):
    okw = parity.oracle_query_kwargs(Q_NAMES, {"v": (0, 999)}, q)
    okw["filters"] = [(f[0], f[1], TAGS.index(f[2]) if isinstance(f[2], str) else f[2]) for f in okw["filters"]]
    return okw


def _gpu(tb, q):
    query = tb.query(**q)
    try:
        return query.run(), query.stats()
    finally:
        query.free()


@pytest.mark.parametrize("which", ["group_by_avg", "hist_percentiles"])
def test_select_then_query_is_query_with_filters(query_tables, oracle, which):
    src, sel, o_src, o_sel, _ = query_tables
    q = {"group_by_avg": dict(groups=["g"], aggs=["v"], op="avg"),
         "hist_percentiles": dict(groups=["s"], aggs=["v"], op="hist", want_percentiles=True)}[which]
    full = q.get("want_percentiles", False)
    g_sel, _ = _gpu(sel, q)
    g_src, _ = _gpu(src, dict(q, filters=Q_FILTERS))
    try:
        o_of_sel = oracle.run_query(o_sel, block_rows=SEL_BLOCK, n_threads=4, **_oracle_kwargs(q))
        o_of_src = oracle.run_query(o_src, block_rows=SRC_BLOCK, n_threads=4, **_oracle_kwargs(dict(q, filters=Q_FILTERS)))
        assert g_sel.matched == g_src.matched == sel.rows
        # each against its own oracle, and crosswise: the two agree in everything the helper compares
        for g in (g_sel, g_src):
            for o in (o_of_sel, o_of_src):
                parity.compare(g, o, op=q["op"], full=full, n_aggs=1)
    finally:
        g_sel.free()
        g_src.free()


def test_block_statistics_of_the_selected_table(query_tables, oracle):
    """block_skip trusts the per-block min / max: a time filter over the selected table skips blocks, and skips only blocks
    without a matching row."""
    _, sel, _, o_sel, time_kept = query_tables
    cut = int(np.median(time_kept))
    out = {}
    for skip in (True, False):
        q = dict(filters=[("time", "gt", cut)], groups=["g"], aggs=["v"], op="avg", block_skip=skip)
        gres, stats = _gpu(sel, q)
        try:
            ores = oracle.run_query(o_sel, block_rows=SEL_BLOCK, n_threads=4, **_oracle_kwargs(q))
            parity.compare(gres, ores, op="avg", n_aggs=1)
            assert gres.matched == int((time_kept > cut).sum())
            out[skip] = (gres.matched, sorted((r["key"], r["count"], r["hists"][0]["sum"], r["hists"][0]["min"], r["hists"][0]["max"])
                                              for r in gres.results), stats["blocks_skipped"])
        finally:
            gres.free()
    assert out[True][:2] == out[False][:2]
    assert out[True][2] > 0 and out[False][2] == 0


def test_block_statistics_in_canonical_storage(tables):
    """Canonical storage computes the block statistics on first use: the same check on a small table, against numpy."""
    n = 8192 + 5
    src = tables(n, "canonical")
    sel = src.select([("par", "eq", 0)], block_rows=100)
    try:
        cut = n // 2
        want = int((np.arange(0, n, 2) > cut).sum())
        got = {}
        for skip in (True, False):
            query = sel.query(filters=[("row", "gt", cut)], groups=["par"], aggs=["w1"], block_skip=skip)
            res = query.run()
            got[skip] = (res.matched, [(r["count"], r["hists"][0]["sum"]) for r in res.results], query.stats()["blocks_skipped"])
            res.free()
            query.free()
        assert got[True][0] == got[False][0] == want and got[True][1] == got[False][1]
        assert got[True][2] > 0 and got[False][2] == 0
    finally:
        sel.free()


# ------------------------------------------------------------------ 6. round trip

def test_save_and_open_round_trip(ctx, tmp_path):
    blocks = _blocks(1000)
    # (the on-disk format has no empty set: a populated empty set reads back as unpopulated)
    blocks = [(s, dict(c, tags=("set", [t if t else None for t in c["tags"][1]]))) for s, c in blocks]
    src = build(ctx, blocks, compact=True, name="events")
    sel = src.select([("par", "eq", 1)], block_rows=96)
    back = None
    try:
        sel.save(str(tmp_path))
        back = ctx.open_table(str(tmp_path), "events")
        assert back.rows == sel.rows == 500 and back.blocks == sel.blocks == 6
        assert _rows(sel) == D.rows_of(S.select_ref(blocks, [("par", "eq", 1)], None, 96))
        # (the file format keeps a set's members in the order of the block's string table, not the row's: compared sorted)
        norm = lambda rows: [dict(r, tags=sorted(r["tags"])) if "tags" in r else r for r in rows]
        assert norm(_rows(back)) == norm(_rows(sel))
    finally:
        if back is not None:
            back.free()
        sel.free()
        src.free()


# ------------------------------------------------------------------ 7. edges and errors

def test_errors_never_matches_and_the_empty_table(ctx, tables):
    import sybil_amd
    src = tables(33, "canonical")
    for kw, word in ((dict(block_rows=-1), "block_rows"), (dict(block_rows=65537), "block_rows"), (dict(columns=["nope"]), "nope"),
                     (dict(filters=[("nope", "gt", 1)]), "nope")):
        with pytest.raises(sybil_amd.SyblError) as ei:
            src.select(**kw)
        assert ei.value.code == E_INVAL and word in str(ei.value), (kw, str(ei.value))
    assert src.rows == 33 and src.blocks == len(_blocks(33))
    # nothing can match: the columns and no blocks.  The first the planner proves (no kernel runs), the second the kernels find
    for filters, proven in (([("row", "gt", (1 << 63) - 1)], True), ([("row", "gt", 5), ("row", "lt", 3)], False)):
        sel = src.select(filters, ["s", "row"])
        try:
            assert sel.rows == 0 and sel.blocks == 0 and sel.samples(limit=5).columns == ["s", "row"] and sel.samples(limit=5).rows == []
            assert sel.column_dict("s") == src.column_dict("s")
            st = sel.select_stats()
            assert st["rows_in"] == 33 and st["rows_out"] == 0 and st["blocks_out"] == 0 and st["gather_bytes"] == 0
            assert (st["filter_bytes"] == 0 and st["filter_ms"] == 0) == proven
        finally:
            sel.free()
    empty = ctx.create_table("empty")
    empty.add_column("time", "int")
    empty.add_column("s", "str")
    empty.add_column("tags", "set")
    for filters in ([], [("time", "gt", 0)]):
        sel = empty.select(filters)
        try:
            assert sel.rows == 0 and sel.blocks == 0
            assert sel.samples(limit=5).columns == ["time", "s", "tags"] and sel.samples(limit=5).rows == []
            assert sel.column_info("s")["type"] == 2 and sel.column_info("tags")["type"] == 3
        finally:
            sel.free()
    empty.free()


def test_c_example_runs(ctx, tmp_path):
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    exe = str(tmp_path / "example_select")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "example_select.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    out = str(tmp_path / "out")
    p = subprocess.run([exe, out, str(T0 + 1499)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[0] == "source: 3000 rows in 3 blocks"
    assert lines[1].startswith("time > %d: 1500 rows in 3 blocks" % (T0 + 1499))
    back = ctx.open_table(out, "events")
    try:
        assert back.rows == 1500 and back.blocks == 3
        assert back.read_int("time", 0, 1500).tolist() == list(range(T0 + 1500, T0 + 3000))
    finally:
        back.free()
