"""GPU: table digest (Table.digest / sybl_table_digest, csrc/digest.hip) against the numpy restatement in
tests/digest_ref.py.  Tables are built block by block through append_block, with irregular block sizes so that the source has
padding rows; the digest is read back in full with samples(limit=N) and read_int.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from tests import digest_ref as D
from tests import parity
from tests import sybil_fixture as F
from tests.test_gpu_samples import build

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
E_INVAL = -1
IRREGULAR = (70, 1, 130, 33, 2049, 31, 64, 5000, 777, 32)


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


def _sizes(n, pattern=IRREGULAR):
    out, k = [], 0
    while n > 0:
        s = min(n, pattern[k % len(pattern)] * (1 + k // len(pattern)))
        out.append(s)
        n -= s
        k += 1
    return out


def _blocks(n, seed=3, time_of=None):
    """n rows of every column kind in irregular blocks; the time column is nullable, has negative values and ~40 distinct
    values (ties everywhere)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    w8 = (i * 2654435761) % (1 << 40) - (1 << 39)
    w8[0] = I64_MIN
    if n > 1:
        w8[n // 2] = I64_MAX
    time = (rng.integers(-20, 20, size=n) * 1000).astype(np.int64)
    tpop = rng.random(n) > 0.2
    if time_of is not None:
        time, tpop = time_of(n)
    sid = rng.integers(0, 50, size=n)
    spop = rng.random(n) > 0.25
    tlen = rng.integers(0, 5, size=n)
    tfirst = rng.integers(0, 6, size=n)
    tpop2 = rng.random(n) > 0.25
    flat = {"w1": (1000 + (i * 37) % 200, None), "w2": (-3 + (i * 7) % 60000, None), "w4": (5 + (i * 100003) % (1 << 31), None),
            "w8": (w8, None), "ni": (rng.integers(-500, 500, size=n).astype(np.int64), rng.random(n) > 0.3),
            "row": (i, None), "time": (time, tpop)}
    strs = [("user%02d" % s if p else None) for s, p in zip(sid.tolist(), spop.tolist())]
    tags = [(["tag%d" % (f + k) for k in range(ln)] if p else None) for f, ln, p in zip(tfirst.tolist(), tlen.tolist(), tpop2.tolist())]
    blocks, r0 = [], 0
    for s in _sizes(n):
        sl = slice(r0, r0 + s)
        cols = {name: ("int", v[sl], None if p is None else p[sl]) for name, (v, p) in flat.items()}
        cols["s"] = ("str", strs[sl])
        cols["tags"] = ("set", tags[sl])
        blocks.append((s, cols))
        r0 += s
    return blocks


def _rows(tb):
    """Every row of a table in row order (samples returns them newest first)."""
    n = tb.rows
    got = tb.samples(limit=max(n, 1))
    assert got.info["n_rows"] == n and got.row_ids.tolist() == list(range(n - 1, -1, -1))
    return got.rows[::-1]


def _check_digest(src, dg, blocks, block_rows, time_col="time"):
    ref = D.digest_ref(blocks, time_col, block_rows)
    n = sum(b[0] for b in blocks)
    br = block_rows or D.BLOCK_ROWS
    assert dg.rows == n and dg.blocks == -(-n // br) == len(ref)
    assert _rows(dg) == D.rows_of(ref)
    cols = D.concat(ref)
    for name, (ty, v, p) in cols.items():
        if ty == "int":
            got = dg.read_int(name, 0, n)
            assert np.array_equal(got[p], v[p]), name
        else:
            assert dg.column_dict(name) == src.column_dict(name), name
        assert dg.column_storage(name) == src.column_storage(name), name


# ------------------------------------------------------------------ 1. rows, exactly

@pytest.mark.parametrize("storage", ["canonical", "compact"])
@pytest.mark.parametrize("n,block_rows", [(1, 0), (33, 32), (257, 100), (1000, 96), (65536 + 77, 0), (3 * 65536, 0)])
def test_rows_exactly(ctx, storage, n, block_rows):
    blocks = _blocks(n)
    src = build(ctx, blocks, compact=storage == "compact")
    dg = None
    try:
        if storage == "compact" and n >= 1000:
            assert [src.column_storage(c)[0] for c in ("w1", "w2", "w4", "w8")] == [1, 2, 4, 8]
        elif storage == "canonical":
            assert src.column_storage("w1") == (8, 0) and src.column_storage("s") == (4, 0)
        before = _rows(src) if n <= 1000 else None     # (the larger sources are read back once, by the digest's check alone)
        dg = src.digest("time", block_rows)
        _check_digest(src, dg, blocks, block_rows)
        assert (before is None or _rows(src) == before) and src.blocks == len(blocks) and src.rows == n   # the source is untouched
        info = dg.column_info("time")
        tv, tp = D.concat(blocks)["time"][1:]
        assert info["has_missing"] == bool((~tp).any())
        if tp.any():
            assert info["exact_min"] <= tv[tp].min() and info["exact_max"] >= tv[tp].max()
        st = dg.digest_stats()
        assert st["rows"] == n and st["blocks"] == dg.blocks and 1 <= st["key_bits"] <= 32
    finally:
        if dg is not None:
            dg.free()
        src.free()


def test_wide_keys_take_the_64_bit_sort(ctx):
    """A time column whose range does not fit 32 bits (INT64_MIN and INT64_MAX present) with unpopulated rows between."""
    blocks = _blocks(1000, seed=5)
    blocks = [(s, dict(c, time=("int", c["w8"][1], c["ni"][2]))) for s, c in blocks]
    for compact in (False, True):
        src = build(ctx, blocks, compact=compact)
        dg = src.digest(block_rows=96)
        try:
            _check_digest(src, dg, blocks, 96)
            assert dg.digest_stats()["key_bits"] == 64
        finally:
            dg.free()
            src.free()


def test_staged_writer_path_gives_the_same_table(ctx, monkeypatch):
    """SYBL_NO_DIRECT_DECODE=1: the block writer refuses in-place columns, the digest hands its blocks over through the
    staging block instead."""
    blocks = _blocks(1000, seed=9)
    src = build(ctx, blocks, compact=True)
    monkeypatch.setenv("SYBL_NO_DIRECT_DECODE", "1")
    dg = src.digest(block_rows=96)
    monkeypatch.delenv("SYBL_NO_DIRECT_DECODE")
    try:
        _check_digest(src, dg, blocks, 96)
        q = dg.query(filters=[("time", "gt", 0)], groups=["w1"], aggs=["w2"], block_skip=True)
        res = q.run()
        cols = D.concat(blocks)
        hit = cols["time"][2] & (cols["time"][1] > 0)
        assert res.matched == int(hit.sum()) and q.stats()["blocks_skipped"] > 0
        res.free()
        q.free()
    finally:
        dg.free()
        src.free()


def test_other_time_column_and_default_name(ctx):
    blocks = _blocks(257)
    src = build(ctx, blocks, compact=True)
    try:
        for arg, col in ((None, "time"), ("", "time"), ("ni", "ni"), ("w2", "w2")):
            dg = src.digest(arg, 100)
            try:
                _check_digest(src, dg, blocks, 100, time_col=col)
            finally:
                dg.free()
    finally:
        src.free()


# ------------------------------------------------------------------ 2. ties are stable

@pytest.mark.parametrize("compact", [False, True])
def test_ties_are_stable(ctx, compact):
    n = 1000
    same = lambda k: (np.full(k, -7, dtype=np.int64), np.ones(k, dtype=bool))
    none = lambda k: (np.zeros(k, dtype=np.int64), np.zeros(k, dtype=bool))
    for time_of in (same, none):
        blocks = _blocks(n, time_of=time_of)
        src = build(ctx, blocks, compact=compact)
        dg = src.digest(block_rows=96)
        try:
            rows = _rows(dg)
            assert [r["row"] for r in rows] == list(range(n))          # source order, only re-blocked
            assert rows == _rows(src) and dg.blocks == 11
            _check_digest(src, dg, blocks, 96)
        finally:
            dg.free()
            src.free()


# ------------------------------------------------------------------ 3. dead blocks

def test_dead_blocks_contribute_nothing(ctx, tmp_path):
    blocks = []
    for b, n in enumerate((300, 1000, 77, 450)):
        i = np.arange(n)
        cols = {"time": ("int", ((i * 7919 + b * 13) % 500 - 100).astype(np.int64), (i % 5 != 0)),
                "row": ("int", (i + 10000 * b).astype(np.int64)),
                "name": ("str", [None if k % 9 == 0 else "user%d" % (k % 50) for k in i]),
                # (the file format keeps a set's members in the order of the block's string table: the first row fixes it)
                "tags": ("set", [["t0", "t1", "t2", "t3"]] + [None if k % 6 == 0 else ["t%d" % x for x in range(k % 3, k % 3 + 1 + k % 2)] for k in i[1:]])}
        blocks.append((n, cols))
    root = str(tmp_path / "db")
    F.write_table(root, "events", [cols for _, cols in blocks])
    for compact in (False, True):
        tb = ctx.open_table(root, "events", compact=compact)
        dg = None
        try:
            assert tb.blocks == 4
            if not compact:
                dg = tb.digest(block_rows=256)
                _check_digest(tb, dg, blocks, 256)
            else:
                shutil.rmtree(os.path.join(root, "events", "block%09d" % 2))
                assert tb.refresh()[1] == 1 and tb.rows == 300 + 77 + 450
                live = [blocks[0], blocks[2], blocks[3]]
                dg = tb.digest(block_rows=256)
                _check_digest(tb, dg, live, 256)
                rows = _rows(dg)
                assert not any(10000 <= r["row"] < 20000 for r in rows) and len(rows) == 300 + 77 + 450
        finally:
            if dg is not None:
                dg.free()
            tb.free()


# ------------------------------------------------------------------ 4. queries agree with the oracle

N_Q = 200_000
SRC_BLOCK = 10_000            # not a multiple of 32: every source block is followed by padding rows
HOSTS = ["host%02d" % k for k in range(20)]
TAGS = ["t%d" % k for k in range(6)]


@pytest.fixture(scope="module")
def query_tables(ctx):
    rng = np.random.default_rng(17)
    n = N_Q
    c = {"g": rng.integers(0, 12, n).astype(np.int64), "v": rng.integers(0, 1000, n).astype(np.int64),
         "u": rng.integers(0, 30_000, n).astype(np.int64), "time": rng.permutation(1_700_000_000 + (np.arange(n) * 6 * 3600) // n).astype(np.int64)}
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
    dg = src.digest()
    perm = D.permutation([(n, {"time": ("int", c["time"], None)})])

    def ocols(order):
        lens = tlen[order]
        starts = toff[:-1][order]
        members = np.concatenate([tid[a:a + k] for a, k in zip(starts.tolist(), lens.tolist())]) if n else tid
        return [{"type": "int", "data": c["g"][order]}, {"type": "int", "data": c["v"][order]}, {"type": "int", "data": c["u"][order]},
                {"type": "int", "data": c["time"][order]}, {"type": "str", "data": sid[order]},
                {"type": "set", "data": members.astype(np.int32), "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)}]
    yield src, dg, ocols(np.arange(n)), ocols(perm)
    dg.free()
    src.free()


Q_NAMES = ["g", "v", "u", "time", "s", "tags"]
QUERIES = {
    "group_by_avg": dict(groups=["g"], aggs=["v"], op="avg"),
    "hist_percentiles": dict(groups=["g"], aggs=["v"], op="hist", want_percentiles=True),
    "str_group_set_filter": dict(filters=[("tags", "in", "t2")], groups=["s"], aggs=["v"], op="avg"),
    "count_distinct": dict(groups=["g"], distincts=["u"]),
    "time_series": dict(groups=["g"], aggs=["v"], op="avg", time_col="time", time_bucket=3600),
}


@pytest.mark.parametrize("which", sorted(QUERIES))
def test_queries_agree_with_the_oracle(query_tables, oracle, which):
    src, dg, o_src, o_dg = query_tables
    q = QUERIES[which]
    okw = parity.oracle_query_kwargs(Q_NAMES, {"v": (0, 999)}, q)
    okw["filters"] = [(f[0], f[1], TAGS.index(f[2])) for f in okw["filters"]]
    # the digest first, then the source: the source is unchanged by the digest
    for tb, ocols, block_rows in ((dg, o_dg, D.BLOCK_ROWS), (src, o_src, SRC_BLOCK)):
        query = tb.query(**q)
        try:
            gres = query.run()
            if which == "count_distinct":
                from tests.test_gpu_distinct import _compare as compare_distinct
                ores = oracle.run_query(ocols, block_rows=block_rows, n_threads=4, distincts=[Q_NAMES.index("u")], want_registers=True, **okw)
                compare_distinct(gres, ores)
            else:
                ores = oracle.run_query(ocols, block_rows=block_rows, n_threads=4, **okw)
                parity.compare(gres, ores, op=q["op"], full=q.get("want_percentiles", False), n_aggs=1, time_mode="time_col" in q)
            gres.free()
        finally:
            query.free()


# ------------------------------------------------------------------ 5. the digest restores what the order buys

W_ROWS, W_BUCKETS, W_CELLS, W_BUCKET = 8 * 65536, 512, 20, 3600


@pytest.fixture(scope="module")
def window_tables(ctx):
    rng = np.random.default_rng(23)
    n = W_ROWS
    time = rng.permutation((np.arange(n, dtype=np.int64) * W_BUCKETS * W_BUCKET) // n)
    g = rng.integers(0, W_CELLS, n).astype(np.int64)
    v = rng.integers(0, 1000, n).astype(np.int64)
    src = ctx.create_table("w")
    src.add_column("time", "int")
    src.add_column("g", "int")
    src.add_column("v", "int", 0, 999)
    r0 = 0
    for s in _sizes(n, (60000, 70001, 65536, 33333)):
        sl = slice(r0, r0 + s)
        src.append_block(s, {"time": time[sl], "g": g[sl], "v": v[sl]})
        r0 += s
    src.compact()
    dg = src.digest()
    perm = np.argsort(time, kind="stable")
    yield src, dg, [time, g, v], [time[perm], g[perm], v[perm]]
    dg.free()
    src.free()


def _run(tb, oracle, arrays, q, okw, block_rows=D.BLOCK_ROWS):
    query = tb.query(**q)
    try:
        gres = query.run()
        stats = query.stats()
        ores = oracle.run_query([{"type": "int", "data": a} for a in arrays], block_rows=block_rows, n_threads=4, **okw)
        parity.compare(gres, ores, op="avg", n_aggs=1, time_mode=True)
        rows = sorted((r["time_bucket"], r["key"], r["count"], r["hists"][0]["sum"]) for r in gres.time_results)
        gres.free()
        return stats, rows
    finally:
        query.free()


def test_digest_restores_the_windowed_strategy(window_tables, oracle):
    src, dg, a_src, a_dg = window_tables
    q = dict(groups=["g"], aggs=["v"], op="avg", time_col="time", time_bucket=W_BUCKET)
    okw = parity.oracle_query_kwargs(["time", "g", "v"], {"v": (0, 999)}, q)
    s_src, r_src = _run(src, oracle, a_src, q, okw)
    s_dg, r_dg = _run(dg, oracle, a_dg, q, okw)
    print("strategy: source %d, digest %d; lds_bytes %d / %d" % (s_src["strategy"], s_dg["strategy"], s_src["lds_bytes"], s_dg["lds_bytes"]))
    assert s_src["strategy"] not in (3, 4), s_src
    assert s_dg["strategy"] in (3, 4), s_dg
    assert r_src == r_dg


def test_digest_restores_block_skipping(window_tables, oracle):
    src, dg, a_src, a_dg = window_tables
    median = int(np.median(a_src[0]))
    q = dict(filters=[("time", "gt", median)], groups=["g"], aggs=["v"], op="avg", time_col="time", time_bucket=W_BUCKET, block_skip=True)
    okw = parity.oracle_query_kwargs(["time", "g", "v"], {"v": (0, 999)}, q)
    s_src, r_src = _run(src, oracle, a_src, q, okw)
    s_dg, r_dg = _run(dg, oracle, a_dg, q, okw)
    print("blocks skipped: source %d of %d, digest %d of %d" % (s_src["blocks_skipped"], src.blocks, s_dg["blocks_skipped"], dg.blocks))
    assert s_dg["blocks_skipped"] > 0 and s_src["blocks_skipped"] == 0
    assert r_src == r_dg


# ------------------------------------------------------------------ 6. round trip

def test_save_and_open_round_trip(ctx, tmp_path):
    blocks = _blocks(1000)
    # (the on-disk format has no empty set: a populated empty set reads back as unpopulated)
    blocks = [(s, dict(c, tags=("set", [t if t else None for t in c["tags"][1]]))) for s, c in blocks]
    src = build(ctx, blocks, compact=True, name="events")
    dg = src.digest(block_rows=96)
    back = None
    try:
        dg.save(str(tmp_path))
        back = ctx.open_table(str(tmp_path), "events")
        assert back.rows == dg.rows and back.blocks == dg.blocks
        assert _rows(dg) == D.rows_of(D.digest_ref(blocks, block_rows=96))
        # (the file format keeps a set's members in the order of the block's string table, not the row's: compared sorted)
        norm = lambda rows: [dict(r, tags=sorted(r["tags"])) if "tags" in r else r for r in rows]
        assert norm(_rows(back)) == norm(_rows(dg))
    finally:
        if back is not None:
            back.free()
        dg.free()
        src.free()


# ------------------------------------------------------------------ 7. lifetimes and errors

def test_digest_outlives_its_source_and_digests_again(ctx):
    blocks = _blocks(1000)
    want = D.rows_of(D.digest_ref(blocks, block_rows=96))
    src = build(ctx, blocks, compact=True)
    dg = src.digest(block_rows=96)
    src.free()
    filler = build(ctx, [(4096, {"n": ("int", np.zeros(4096, dtype=np.int64), None)})])   # reuses the freed memory
    again = None
    try:
        assert _rows(dg) == want
        q = dg.query(filters=[("tags", "in", "tag3")], groups=["w1"], aggs=["w2"], op="avg")
        res = q.run()
        cols = D.concat(blocks)
        hit = np.array([t is not None and "tag3" in t for t in cols["tags"][1]])
        assert res.matched == int(hit.sum()) and sum(r["count"] for r in res.results) == res.matched
        assert sum(r["hists"][0]["sum"] for r in res.results) == int(cols["w2"][1][hit].sum())
        res.free()
        q.free()
        again = dg.digest(block_rows=96)                 # a digest of a digest is the digest
        assert _rows(again) == want and again.blocks == dg.blocks
        for name in ("w1", "w8", "s"):
            assert again.column_storage(name) == dg.column_storage(name)
    finally:
        if again is not None:
            again.free()
        dg.free()
        filler.free()


def test_prepared_query_on_the_source_survives_the_digest(ctx):
    blocks = _blocks(1000)
    src = build(ctx, blocks, compact=True)
    q = src.query(groups=["s"], aggs=["ni"], op="hist", want_percentiles=True)

    def scan():
        res = q.scan().finalize()
        out = (res.matched, [(r["group_by_key"], r["count"], r["hists"][0]["sum"], r["hists"][0].get("percentiles", np.zeros(0)).tolist()) for r in res.results])
        res.free()
        return out
    try:
        before = scan()
        dg = src.digest(block_rows=96)
        assert scan() == before                          # the source's version did not move: no SYBL_E_STATE
        dg.free()
        assert scan() == before
    finally:
        q.free()
        src.free()


def test_errors_and_the_empty_table(ctx):
    import sybil_amd
    blocks = _blocks(33)
    src = build(ctx, blocks)
    try:
        for args, word in ((("nope", 0), "nope"), (("s", 0), "str"), (("tags", 0), "set"), (("time", -1), "block_rows"),
                           (("time", 65537), "block_rows")):
            with pytest.raises(sybil_amd.SyblError) as ei:
                src.digest(*args)
            assert ei.value.code == E_INVAL and word in str(ei.value), (args, str(ei.value))
        assert src.rows == 33 and src.blocks == len(blocks)
    finally:
        src.free()
    empty = ctx.create_table("empty")
    empty.add_column("time", "int")
    empty.add_column("s", "str")
    empty.add_column("tags", "set")
    dg = empty.digest()
    try:
        assert dg.rows == 0 and dg.blocks == 0
        assert dg.samples(limit=5).columns == ["time", "s", "tags"] and dg.samples(limit=5).rows == []
        assert dg.column_info("s")["type"] == 2 and dg.column_info("tags")["type"] == 3
    finally:
        dg.free()
        empty.free()
