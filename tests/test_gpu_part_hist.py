"""GPU: partitioned histograms (strategy 5: k_count* -> k_emit* -> k_part_hist -> k_part_fix) at their partition, bin, chunk,
batch and bucket edges.

The tables of tests/part_layout.py PLACE what defines the protocol: (workgroup, partition) regions of exactly 0, 1, 15, 16, 17,
..., 1023, 1024, 1025 records, rotated so that one partition's walk meets every size; 64 / 65 / 66 / 130 pairs; 1024 partitions
and the first shapes beyond; ss = 0, 1 and >= 5; a split that does not divide the workgroups; tables that end inside a lane's
rows and workgroups without rows; values at k x BucketSize - 1, + 0, + 1 for bucket sizes from 1 to the largest eligible, with
maxima below and above Info.Max and beyond the last bucket.  tests/test_part_layout.py checks the placement on the CPU.

Every case prepares, scans and finalizes under SYBL_PLAN_TRACE=1 and checks the strategy, the planner's `part hist:` line(s)
against part_layout.geometry / instantiation (partitions, ss, bins, split, the k_part_hist instantiation, k_count_key or not),
every group / bucket / Count / sum / extrema / outlier field / `matched` / Cumulative bit-exact against part_layout.reference
(numpy), and the same against the CPU oracle (parity.compare, full).  Shapes the strategy must leave -- `part hist: rejected
why=pairs | bucket | span | shape` -- are checked for the reason and for the same exact answer from whichever kernel took them.

(aggs, track_max, out): all eight instantiations run.  OUT without TRACK_MAX is reachable -- BucketSize = size / 1000 rounds
down, so 1002 buckets of 49 end below Info.Max = 49999 (column vb / b49) -- and TRACK_MAX runs on canonical storage only: on
compact storage a tracked maximum is the GEN row body's business (planner.cpp: fill_fast_columns), which the emitting kernels
do not have, so such a query is `rejected why=shape` there; the closing test asserts exactly that split.

Rescans: the counting pass is taken once per prepared query of one pass (sybl_run_stats.count_pass_reused 0, 1, 1; 0, 0, 0
under SYBL_NO_COUNT_CACHE=1 and for three aggregations); k_count_key and k_count_packed (SYBL_NO_COUNT16=1) lay out the same
regions -- the emit fills them, and the answers are equal field for field; SYBL_PARTHIST_TAIL=0 counts a region's padding in
field 0 of a partition's first pair, whose carries into that pair's bucket 0 are real and whose own wraps are not.

The last test of the file asserts what ran, from the trace lines, and prints one line per distinct geometry (pytest -s).
"""
import contextlib
import re
import types

import numpy as np
import pytest

import sybil_amd
from tests import parity
from tests import part_layout as PL

pytestmark = pytest.mark.gpu

PART_LINE = re.compile(r"part hist: pass=(\d+) aggs=(\d+) packed=(\d) nf=(\d+) ng=(\d+) parts=(\d+) ss=(\d+) bins=(\d+) n_wg=(\d+) split=(\d+) "
                       r"track_max=(\d) out=(\d) count_key=(\d)")
FIELDS = ("pass_", "aggs", "packed", "nf", "ng", "parts", "ss", "bins", "n_wg", "split", "track_max", "out", "count_key")
REJECTED = re.compile(r"part hist: rejected why=(\w+)")
SEEN = {}            # the fields of a `part hist:` line without its pass number -> the first case that showed it
SYBL_E_STATE = -5
ENV_KEYS = ("SYBL_LATE_PATH", "SYBL_NO_COUNT16", "SYBL_NO_COUNT_CACHE", "SYBL_PARTHIST_TAIL", "SYBL_WG_PER_CU", "SYBL_NO_PARTHIST")


def _q(**kw):
    return dict(dict(op="hist", want_percentiles=True, order_by=None), **kw)


@pytest.fixture(scope="module")
def ctx():
    c = sybil_amd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _env(monkeypatch, **kv):
    with monkeypatch.context() as m:
        for k in ENV_KEYS:
            m.delenv(k, raising=False)
        for k, v in kv.items():
            m.setenv(k, v)
        m.setenv("SYBL_PLAN_TRACE", "1")
        yield


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _build(ctx, layout, compact):
    tb = ctx.create_table(layout.name)
    for c in layout.order:
        tb.add_column(c, "int", *layout.info.get(c, (1, 0)))
    r0 = 0
    for b in layout.blocks:
        tb.append_block(b, {c: layout.cols[c][r0:r0 + b] for c in layout.order})
        r0 += b
    for c, (lo, hi) in layout.keys.items():
        tb.set_bounds(c, lo, hi)
    if compact:
        tb.compact()
    return tb


@pytest.fixture(scope="module")
def world(ctx):
    """The workgroup count of the device (one workgroup per CU: stats()["n_workgroups"] of a first query), then every table,
    canonical and compact."""
    W = types.SimpleNamespace(layouts={}, tb={}, refs={}, oracles={})
    probe = PL.tiny(PL.TINY_ROWS[-1])
    ptb = _build(ctx, probe, True)
    qy = ptb.query(**_q(groups=["g"], aggs=["va"]))
    qy.run().free()
    W.n_wg = qy.stats()["n_workgroups"]
    qy.free()
    ptb.free()
    layouts = [PL.edges(W.n_wg), PL.limit_shapes(W.n_wg), PL.bucket_edges(), PL.padding(W.n_wg)]
    layouts += [PL.few(W.n_wg, r) for r in PL.few_rows(W.n_wg)] + [PL.tiny(r) for r in PL.TINY_ROWS]
    for layout in layouts:
        W.layouts[layout.name] = layout
        for compact in (False, True):
            if layout.name == "padding" and not compact:
                continue
            W.tb[layout.name, compact] = _build(ctx, layout, compact)
    B = W.tb["bucket_edges", True]
    for c, spec in PL.BUCKET_COLS.items():          # the widths the layout promises, as stored
        assert B.column_storage(c)[0] == spec[5], (c, B.column_storage(c))
    assert W.tb["edges", True].column_storage("g")[0] == 2 and W.tb["edges", False].column_storage("g")[0] == 8
    yield W
    for tb in W.tb.values():
        tb.free()


# ---------------------------------------------------------------------------------------------- running and checking
def _traced(tb, q, capfd, monkeypatch, env, scans, on_result):
    """prepare + `scans` x (scan + finalize + on_result(result)) under the plan trace: ([on_result's], [count_pass_reused], stats,
    trace).  A result is freed before the next scan."""
    with _env(monkeypatch, **env):
        capfd.readouterr()
        qy = tb.query(**q)
        out, reused = [], []
        try:
            for _ in range(scans):
                res = qy.run()
                try:
                    reused.append(qy.stats()["count_pass_reused"])
                    out.append(on_result(res))
                finally:
                    res.free()
            st = qy.stats()
        finally:
            qy.free()
        text = capfd.readouterr().err
    lines = [types.SimpleNamespace(**dict(zip(FIELDS, map(int, m)))) for m in PART_LINE.findall(text)]
    return out, reused, st, types.SimpleNamespace(lines=lines, rejected=REJECTED.findall(text), text=text)


def _expected_lines(layout, q, n_wg, compact, env):
    """What `part hist:` must say, pass by pass -- or the reason the strategy must leave the query."""
    hb = q.get("hist_bucket", 0)
    inst = [PL.instantiation(*layout.info[a], hb, layout.data_max(a)) for a in q["aggs"]]
    if compact and any(tm for tm, _ in inst):
        return None, "shape"              # (a tracked maximum over compact storage: the GEN body's, which k_emit_packed has not)
    for a in q["aggs"]:
        ok, why = PL.record_fits(*layout.info[a], hb, layout.data_max(a))
        if not ok:
            return None, why
    nf = len({f[0] for f in q.get("filters", ())})
    out = []
    for p, (a0, na) in enumerate(PL.passes(len(q["aggs"]))):
        parts, ss, bins, split, ok, why = PL.geometry(layout.cells(q), na, layout.n, n_wg)
        if not ok:
            return None, why
        out.append(dict(pass_=p, aggs=na, packed=int(compact), nf=nf, ng=1, parts=parts, ss=ss, bins=bins, n_wg=n_wg, split=split,
                        track_max=int(any(tm for tm, _ in inst[a0:a0 + na])), out=int(any(o for _, o in inst[a0:a0 + na])),
                        count_key=int(compact and nf == 0 and ss == 0 and "SYBL_NO_COUNT16" not in env)))
    return out, "ok"


def _check_numpy(res, ref, layout, q, what):
    """Every group of the reference and no other; Count; per aggregation count, sum, Min / Max, bucket geometry, EVERY bucket,
    the outliers' number, values and sum; `matched`; Cumulative."""
    hb = q.get("hist_bucket", 0)
    got = {tuple(_signed(v) for v in r["key_vals"]): r for r in res.rows(0)}
    assert ref["overflow"] == 0 and res.matched == ref["matched"], (what, res.matched, ref["matched"])
    assert set(got) == set(ref["groups"]), (what, len(got), len(ref["groups"]), sorted(set(got) ^ set(ref["groups"]))[:8])
    bad = []
    for key, (count, aggs) in list(ref["groups"].items()) + [("cumulative", ref["cumulative"])]:
        g = res.cumulative if key == "cumulative" else got[key]
        if g["count"] != count:
            bad.append((key, "count", g["count"], count))
        for name, a, h in zip(q["aggs"], aggs, g["hists"]):
            bs, nv = PL.buckets(*layout.info[name], hb)
            if not h["present"] or (h["count"], h["sum"], h["min"], h["max"]) != (count, a["sum"], a["min"], a["max"]):
                bad.append((key, name, "fields", h["present"], h["count"], h["sum"], h["min"], h["max"], count, a["sum"], a["min"], a["max"]))
            if (h["bucket_size"], h["n_values"]) != (bs, nv) or not np.array_equal(h["values"], a["values"]):
                diff = np.flatnonzero(np.asarray(h["values"]) != a["values"])[:6] if h["n_values"] == nv else []
                bad.append((key, name, "buckets", h["bucket_size"], h["n_values"], [(int(k), int(h["values"][k]), int(a["values"][k])) for k in diff]))
            if h["n_outliers"] != a["n_outliers"]:
                bad.append((key, name, "n_outliers", h["n_outliers"], a["n_outliers"]))
            if key != "cumulative" and h["n_outlier_values"] >= 0:
                ov = h.get("outlier_values", np.zeros(0, dtype=np.int64))
                if not np.array_equal(ov, a["outlier_values"]) or int(ov.sum()) != a["outlier_sum"]:
                    bad.append((key, name, "outlier values", ov[:4], a["outlier_values"][:4]))
    assert not bad, (what, len(bad), bad[:5])


def _snapshot(res):
    """Everything a result says, in the order it says it, floats bit for bit: what two runs must agree on."""
    def row(r):
        return (r["key"], r["count"], r["samples"],
                tuple(tuple((k, v.hex() if isinstance(v, float) else (v.tobytes() if isinstance(v, np.ndarray) else v)) for k, v in h.items())
                      for h in r["hists"]))
    return (res.matched, [[row(r) for r in res.rows(w)] for w in (0, 2)])


def _answers(W, oracle, table, q):
    """(numpy reference, oracle result) of a query on a table: computed once."""
    key = (table, repr(sorted(q.items())))
    if key not in W.refs:
        L = W.layouts[table]
        W.refs[key] = PL.reference(L, q)
        names = list(dict.fromkeys(list(q["groups"]) + list(q["aggs"]) + [f[0] for f in q.get("filters", [])]))
        ocols = [{"type": "int", "data": L.cols[c]} for c in names]
        W.oracles[key] = oracle.run_query(ocols, n_threads=16, **parity.oracle_query_kwargs(names, L.info, q))
    return W.refs[key], W.oracles[key]


def _case(W, oracle, capfd, monkeypatch, table, compact, q, env=None, scans=1, n_wg=None, reused=None):
    """One query on one table: the trace against part_layout, every scan's result against the reference and the oracle.
    Returns (snapshot of the last result, trace, expected reason)."""
    env = env or {}
    L = W.layouts[table]
    n_wg = n_wg or W.n_wg
    what = (table, "compact" if compact else "canonical", q["groups"], q["aggs"], q.get("hist_bucket", 0), q.get("filters"), env)
    ref, ores = _answers(W, oracle, table, q)
    want, why = _expected_lines(L, q, n_wg, compact, env)

    def on_result(res):
        _check_numpy(res, ref, L, q, what)
        parity.compare(res, ores, op="hist", full=True, n_aggs=len(q["aggs"]))
        return _snapshot(res)

    snaps, seen_reused, st, tr = _traced(W.tb[table, compact], q, capfd, monkeypatch, env, scans, on_result)
    assert st["n_workgroups"] == n_wg, (what, st)
    if want is None:
        assert st["strategy"] != 5 and tr.rejected == [why] and not tr.lines, (what, why, st["strategy"], tr.text)
    else:
        assert st["strategy"] == 5 and not tr.rejected, (what, st["strategy"], tr.text)
        assert [vars(l) for l in tr.lines] == want, (what, tr.text, want)
        assert st["packed_kernel"] == int(compact), (what, st)
        for l in tr.lines:
            SEEN.setdefault(tuple(v for k, v in sorted(vars(l).items()) if k != "pass_"), "%s %s %s" % (table, q["groups"][0], "+".join(q["aggs"])))
        if reused is not None:
            assert seen_reused == reused, (what, seen_reused)
    assert all(s == snaps[0] for s in snaps), what          # (every scan of a prepared query says the same)
    return snaps[-1], tr, why


STORAGE = pytest.mark.parametrize("compact", [True, False], ids=["compact", "canonical"])


# ---------------------------------------------------------------------------------------------- edges: exact region sizes
@STORAGE
@pytest.mark.parametrize("agg", ["va", "vb"])
def test_every_region_size_in_every_share(world, oracle, capfd, monkeypatch, compact, agg):
    """Regions of 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1023, 1024 and 1025 records in every workgroup's output, rotated over
    fourteen partitions (first, last, either side of 256 / 512 / 768): the chunk padding and rotation of emit_finish, the
    piece count and the masked last batch of k_part_hist, empty regions skipped by open_region.  vb: outliers (OUT) as well."""
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "edges", compact, _q(groups=["g"], aggs=[agg]))
    assert why == "ok" and (tr.lines[0].parts, tr.lines[0].ss, tr.lines[0].split) == (1024, 0, 1)
    assert tr.lines[0].count_key == int(compact) and tr.lines[0].out == int(agg == "vb") and tr.lines[0].track_max == 0


def test_count_key_and_count_packed_lay_out_the_same_regions(world, oracle, capfd, monkeypatch):
    """k_count_key (eight 2-byte keys per lane and load) against k_count_packed (k_emit_packed's row -> lane mapping) on the placed
    table: both exact -- the emit fills what the count sized -- and equal field for field."""
    q = _q(groups=["g"], aggs=["va"])
    a, ta, _ = _case(world, oracle, capfd, monkeypatch, "edges", True, q)
    b, tb, _ = _case(world, oracle, capfd, monkeypatch, "edges", True, q, env={"SYBL_NO_COUNT16": "1"})
    assert (ta.lines[0].count_key, tb.lines[0].count_key) == (1, 0)
    assert a == b


@pytest.mark.parametrize("late", ["0", "1"])
def test_filtered_regions_keep_their_placed_sizes(world, oracle, capfd, monkeypatch, late):
    """f > 0 passes exactly the placed rows: the same region sizes through the filtered count / emit kernels, plain and LATE."""
    q = _q(groups=["g"], aggs=["va"], filters=PL.EDGE_FILTER)
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "edges", True, q, env={"SYBL_LATE_PATH": late})
    assert why == "ok" and (tr.lines[0].nf, tr.lines[0].count_key) == (1, 0)
    assert ("late path: kernel=count_emit late=%s" % late) in tr.text, tr.text
    ref, _ = _answers(world, oracle, "edges", q)
    assert ref["matched"] == world.n_wg * sum(PL.EDGE_COUNTS)


def test_filtered_regions_canonical(world, oracle, capfd, monkeypatch):
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "edges", False, _q(groups=["g"], aggs=["vb"], filters=PL.EDGE_FILTER))
    assert why == "ok" and (tr.lines[0].nf, tr.lines[0].packed) == (1, 0)


# ---------------------------------------------------------------------------------------------- tiny and few
@STORAGE
@pytest.mark.parametrize("rows", PL.TINY_ROWS)
def test_tiny_tables(world, oracle, capfd, monkeypatch, rows, compact):
    """1, 15, 16, 17 rows (below, at and above a chunk), 2047 / 2049 and 4095 / 4097 (either side of a canonical and a compact tile):
    one workgroup with rows, every other without."""
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "tiny%d" % rows, compact, _q(groups=["g"], aggs=["va"]))
    assert why == "ok" and tr.lines[0].parts == 1024


@STORAGE
@pytest.mark.parametrize("rows", ["r0", "r1", "r2"])
@pytest.mark.parametrize("key,na", PL.FEW_SHAPES)
def test_few_partitions(world, oracle, capfd, monkeypatch, key, na, rows, compact):
    """64 x 1 and 32 x 2 (one full partition), 65 x 1 and 33 x 2 (a last partition of one pair / one cell: `pair >= total_pairs` ends
    the epilogue), 130 x 1 (three partitions: split = 85 at 256 workgroups, regions 4 / 3 / 3) at three row counts: sub-bins by
    lane number (ss up to 6), the step-down of ss, shares of a partition combined with atomics, workgroups without rows."""
    q = _q(groups=[key], aggs=["va", "vb"][:na])
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "few_" + rows, compact, q)
    assert why == "ok" and tr.lines[0].split == max(1, world.n_wg // tr.lines[0].parts) and tr.lines[0].aggs == na


@STORAGE
def test_three_workgroups_per_cu(world, oracle, capfd, monkeypatch, compact):
    """SYBL_WG_PER_CU=3: three times the scanning workgroups (and regions per partition) over the same rows."""
    q = _q(groups=["k130"], aggs=["va"])
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "few_r2", compact, q, env={"SYBL_WG_PER_CU": "3"}, n_wg=3 * world.n_wg)
    assert why == "ok" and tr.lines[0].n_wg == 3 * world.n_wg


# ---------------------------------------------------------------------------------------------- the partition limit
@STORAGE
def test_1024_partitions_of_two_aggregations(world, oracle, capfd, monkeypatch, compact):
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "limits", compact, _q(groups=["k32768"], aggs=["va", "vc"]))
    assert why == "ok" and (tr.lines[0].parts, tr.lines[0].aggs, tr.lines[0].split) == (1024, 2, 1)


@STORAGE
def test_three_aggregations_run_two_passes_of_different_geometry(world, oracle, capfd, monkeypatch, compact):
    """32768 cells x 3: pass 0 over 1024 partitions of two aggregations, pass 1 over 512 of one -- one record buffer, one table of
    counts, taken again by every pass of every scan (count_pass_reused 0, 0, 0); the second pass's Count is the first's."""
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "limits", compact, _q(groups=["k32768"], aggs=["va", "vb", "vc"]), scans=3, reused=[0, 0, 0])
    assert why == "ok" and [(l.pass_, l.aggs, l.parts) for l in tr.lines] == [(0, 2, 1024), (1, 1, 512)]


@STORAGE
@pytest.mark.parametrize("key,aggs", [("k65537", ["va"]), ("k32769", ["va", "vc"])])
def test_the_first_shapes_beyond_1024_partitions(world, oracle, capfd, monkeypatch, key, aggs, compact):
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "limits", compact, _q(groups=[key], aggs=aggs))
    assert why == "pairs"


# ---------------------------------------------------------------------------------------------- the bucket divide
@STORAGE
@pytest.mark.parametrize("col", list(PL.BUCKET_COLS))
def test_bucket_edges_one_column(world, oracle, capfd, monkeypatch, col, compact):
    """Values at k x BucketSize - 1, + 0, + 1 (the shaved reciprocal comes out one short at every exact multiple: field_of's
    correction), first, middle and last buckets, bucket sizes 1 ... 66908; 66909 and the span beyond 2^26 - 2 leave the strategy."""
    q = _q(groups=["g"], aggs=[col], hist_bucket=PL.BUCKET_COLS[col][2])
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "bucket_edges", compact, q)
    role = PL.BUCKET_COLS[col][3]
    expect = "shape" if compact and role != "plain" else {"b66909": "bucket", "outl_far": "span"}.get(col, "ok")
    assert why == expect, (col, why)
    if why == "ok":
        assert (tr.lines[0].track_max, tr.lines[0].out) == (int(role != "plain"), int(role == "outl" or col == "b49")), vars(tr.lines[0])
    assert compact or why == {"b66909": "bucket", "outl_far": "span"}.get(col, "ok")


PAIRS = {"plain-tmax": ["b999", "b66908t"], "outl-plain": ["outl", "b999"], "nv3-nv1002": ["b1odd", "b999"], "plain-out": ["b1000", "b49"],
         "nv1002-nv4": ["b66908", "b1even"]}


@STORAGE
@pytest.mark.parametrize("pair", list(PAIRS))
def test_bucket_edges_two_columns(world, oracle, capfd, monkeypatch, pair, compact):
    """Two aggregations of different geometry in one pass: the words per pair come from the larger len(Values), the epilogue reads
    each aggregation's own; a tracked maximum / outliers beside a column without."""
    snap, tr, why = _case(world, oracle, capfd, monkeypatch, "bucket_edges", compact, _q(groups=["h"], aggs=PAIRS[pair]))
    tracked = pair in ("plain-tmax", "outl-plain")
    assert why == ("shape" if compact and tracked else "ok")
    if why == "ok":
        assert (tr.lines[0].aggs, tr.lines[0].parts, tr.lines[0].track_max) == (2, 1024, int(tracked))
        assert tr.lines[0].out == int(pair in ("outl-plain", "plain-out"))


# ---------------------------------------------------------------------------------------------- padding counted in field 0
def test_padding_counted_in_field_0(world, oracle, capfd, monkeypatch):
    """SYBL_PARTHIST_TAIL=0: the lanes past a region's end add their zero records -- about a thousand per region, all in field 0 of
    the partition's first pair: it wraps, its carries land in that pair's bucket 0 (logged as -1 each), its own wraps mean
    nothing (part_log_wrap).  One real record per region in partition 0; bucket 0 of every partition's first cell is populated."""
    q = _q(groups=["g"], aggs=["va"])
    assert world.n_wg * (PL.BATCH - 1) > 65536                # field 0 of partition 0's first pair wraps
    a, ta, _ = _case(world, oracle, capfd, monkeypatch, "padding", True, q, env={"SYBL_PARTHIST_TAIL": "0"})
    b, tb, _ = _case(world, oracle, capfd, monkeypatch, "padding", True, q)
    assert a == b and ta.lines[0].split == 1
    ref, _ = _answers(world, oracle, "padding", q)
    count, (agg,) = ref["groups"][(0,)]
    assert count == (world.n_wg + 1) // 2 == int(agg["values"][0])


# ---------------------------------------------------------------------------------------------- the cached count pass
@STORAGE
@pytest.mark.parametrize("aggs", [["va"], ["va", "vb"]])
def test_rescans_reuse_the_count_pass(world, oracle, capfd, monkeypatch, aggs, compact):
    """count_pass_reused reads 0, 1, 1 over three scans of one prepared query (every scan exact), 0, 0, 0 under
    SYBL_NO_COUNT_CACHE=1 -- and the answers are the same."""
    q = _q(groups=["k130"], aggs=aggs)
    a, _, _ = _case(world, oracle, capfd, monkeypatch, "few_r2", compact, q, scans=3, reused=[0, 1, 1])
    b, _, _ = _case(world, oracle, capfd, monkeypatch, "few_r2", compact, q, env={"SYBL_NO_COUNT_CACHE": "1"}, scans=3, reused=[0, 0, 0])
    assert a == b


def test_a_grown_table_counts_again(ctx, world, oracle, capfd, monkeypatch):
    """append_block makes the prepared query stale (its cached counts with it); a fresh query counts again, over the grown table."""
    base, extra = PL.tiny(4097), PL.tiny(2049)
    tb = _build(ctx, base, True)
    q = _q(groups=["g"], aggs=["va"])
    try:
        with _env(monkeypatch):
            qy = tb.query(**q)
            for want in (0, 1):
                qy.run().free()
                assert qy.stats()["count_pass_reused"] == want
            tb.append_block(extra.n, {c: extra.cols[c] for c in base.order})
            with pytest.raises(sybil_amd.SyblError) as ei:
                qy.run()
            assert ei.value.code == SYBL_E_STATE
            qy.free()
        grown = PL.Layout("grown", base.n + extra.n, {c: np.concatenate([base.cols[c], extra.cols[c]]) for c in base.order}, base.keys, base.info)
        world.layouts["grown"], world.tb["grown", True] = grown, tb
        snap, tr, why = _case(world, oracle, capfd, monkeypatch, "grown", True, q, scans=2, reused=[0, 1])
        assert why == "ok"
        assert PL.reference(grown, q)["matched"] == 4097 + 2049
    finally:
        world.tb.pop(("grown", True), None)
        tb.free()


# ---------------------------------------------------------------------------------------------- last in the file
def test_what_ran(world, capfd):
    """The cases above must not collapse onto one instantiation or one geometry (needs the rest of the file to have run)."""
    idx = {k: i for i, k in enumerate(sorted(f for f in FIELDS if f != "pass_"))}
    with capfd.disabled():
        print()
        for key in sorted(SEEN):
            print("  part hist: " + " ".join("%s=%d" % (f, key[idx[f]]) for f in FIELDS if f != "pass_") + "   [%s]" % SEEN[key])
    col = lambda f: {k[idx[f]] for k in SEEN}
    inst = {(k[idx["aggs"]], k[idx["track_max"]], k[idx["out"]], k[idx["packed"]]) for k in SEEN}
    # every k_part_hist<aggs, TRACK_MAX, OUT> on canonical storage; on compact storage the four without a tracked maximum
    assert {i[:3] for i in inst if i[3] == 0} == {(a, t, o) for a in (1, 2) for t in (0, 1) for o in (0, 1)}, sorted(inst)
    assert {i[:3] for i in inst if i[3] == 1} == {(a, 0, o) for a in (1, 2) for o in (0, 1)}, sorted(inst)
    assert col("count_key") == {0, 1} and col("packed") == {0, 1}
    assert {0, 1} <= col("ss") and max(col("ss")) >= 5
    assert 1 in col("split") and any(k[idx["n_wg"]] % k[idx["split"]] for k in SEEN)
    assert {1, 2, 3, 1024} <= col("parts") and 512 in col("parts")
