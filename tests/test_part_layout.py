"""CPU: the claims tests/part_layout.py makes about its tables and about strategy 5's geometry, from the arrays (no GPU; the
oracle for setup_buckets and for reference())."""
import numpy as np
import pytest

from tests import parity
from tests import part_layout as PL

N_WGS = (256, 304, 768)
Q1 = dict(groups=["g"], aggs=["va"])


@pytest.fixture(scope="module", params=N_WGS)
def n_wg(request):
    return request.param


@pytest.fixture(scope="module")
def edges(n_wg):
    return PL.edges(n_wg)


# ---------------------------------------------------------------------------------------------- geometry, by hand
def test_geometry_at_the_partition_limits():
    rows = 256 * PL.UNIT + 7
    assert PL.geometry(64, 1, rows, 256)[0] == 1 and PL.geometry(65, 1, rows, 256)[0] == 2 and PL.geometry(33, 2, rows, 256)[0] == 2
    assert PL.geometry(65536, 1, rows, 256) == (1024, 0, 1024, 1, True, "ok")
    assert PL.geometry(32768, 2, rows, 256) == (1024, 0, 1024, 1, True, "ok")
    assert PL.geometry(32768, 1, rows, 256) == (512, 0, 512, 1, True, "ok")         # the second pass of 32768 x 3
    assert PL.passes(3) == [(0, 2), (2, 1)] and PL.passes(2) == [(0, 2)] and PL.passes(1) == [(0, 1)]
    assert PL.geometry(65537, 1, rows, 256)[0::4] == (1025, False) and PL.geometry(65537, 1, rows, 256)[5] == "pairs"
    assert PL.geometry(32769, 2, rows, 256)[0::4] == (1025, False) and PL.geometry(32769, 2, rows, 256)[5] == "pairs"
    assert PL.geometry(64, 1, rows, 2049)[4:] == (False, "n_wg")
    assert PL.geometry(64, 1, 1 << 32, 256)[4:] == (False, "cap")


def test_geometry_of_three_partitions_at_256_workgroups():
    """130 cells: three partitions, the last of two pairs; 256 / 3 = 85 shares a partition, and 256 = 3 x 85 + 1 workgroups'
    regions fall to them as 4 / 3 / 3 / ..."""
    parts, ss, bins, split, ok, why = PL.geometry(130, 1, PL.few_rows(256)["r2"], 256)
    assert (parts, split, ok) == (3, 85, True) and 256 % split == 1
    reg = PL.regions(256, split)
    assert reg[:3] == [4, 3, 3] and set(reg[1:]) == {3} and sum(reg) == 256 and len(reg) == 85
    assert PL.nondividing_cells(256) == 130 and PL.nondividing_cells(304) == 130 and PL.nondividing_cells(768) == 4 * PL.PART + 2


def test_sub_shift_of_the_few_shapes(n_wg):
    """ss by hand for one partition and one aggregation -- the most bins is 1024 (ss = 10), so every value below is a step-down:
    rows / (n_wg x 2^ss) >= 64 -- and over the set: 0, 1 and >= 5, a split that does not divide n_wg, split = n_wg."""
    rows = PL.few_rows(n_wg)
    assert [PL.geometry(64, 1, rows[r], n_wg)[1] for r in ("r0", "r1", "r2")] == [0, 1, 5]
    assert [PL.geometry(32, 2, rows[r], n_wg)[1] for r in ("r0", "r1", "r2")] == [1, 2, 6]
    assert all(r % 4 not in (0,) and r % 2 == 1 for r in rows.values())             # a table's end inside a lane's 2 / 4 rows
    seen_ss, seen_split = set(), set()
    for key, na in PL.FEW_SHAPES:
        cells = PL.FEW_KEYS.get(key) or PL.nondividing_cells(n_wg)
        for r in rows.values():
            parts, ss, bins, split, ok, why = PL.geometry(cells, na, r, n_wg)
            assert ok and parts == (cells * na + 63) // 64 and bins == parts << ss <= 1024 and ss < 10 - (parts > 1), (key, na, r)
            seen_ss.add(ss)
            seen_split.add(split)
    assert {0, 1} <= seen_ss and max(seen_ss) >= 5
    assert n_wg in seen_split and any(n_wg % s for s in seen_split)
    if n_wg in (256, 304):
        assert n_wg % PL.geometry(130, 1, rows["r2"], n_wg)[3] != 0


def test_the_record_limits():
    """(nv + 1) x BucketSize < 2^26: 1003 x 66908 = 67 108 724 fits, 1003 x 66909 = 67 109 727 does not; the outlier span."""
    assert 1003 * 66908 < 1 << 26 < 1003 * 66909
    assert PL.record_fits(0, 66_908_000, 0, 66_908_000) == (True, "ok") and PL.record_fits(0, 66_909_000, 0, 66_909_000) == (False, "bucket")
    assert PL.record_fits(0, 5000, 1 << 24, 5000) == (False, "bucket") and PL.record_fits(0, 5000, 1 << 16, 5000) == (True, "ok")
    bs = PL.buckets(*PL.OUT_INFO)[0]
    assert bs == 8000 and PL.OUT_MAX - PL.OUT_INFO[0] + bs == (1 << 26) - 2 and PL.OUT_MAX <= 10 * PL.OUT_INFO[1]
    assert PL.record_fits(*PL.OUT_INFO, 0, PL.OUT_MAX) == (True, "ok") and PL.record_fits(*PL.OUT_INFO, 0, PL.OUT_MAX + 1) == (False, "span")
    assert PL.record_fits(0, 1 << 27, 4, 1 << 27) == (False, "span")                 # span / BucketSize >= 2^24
    # (track_max, out): all four occur
    assert PL.instantiation(0, 999_999, 0, 999_999) == (False, False) and PL.instantiation(0, 999_999, 0, 1_000_000) == (True, False)
    assert PL.instantiation(0, 49_999, 0, 49_999) == (False, True) and PL.instantiation(*PL.OUT_INFO, 0, PL.OUT_MAX) == (True, True)


def test_buckets_equal_the_oracles(oracle):
    infos = [PL.INFO_A + (0,), PL.INFO_B + (0,), PL.OUT_INFO + (0,)] + [v[:3] for v in PL.BUCKET_COLS.values()]
    infos += [(0, s, 0) for s in (0, 1, 2, 98, 99, 100, 101, 299, 999, 1000, 1001, 1999, 2000)] + [(-7, 7, 0), (0, 10**6, 990), (5, 5, 3)]
    for lo, hi, hb in infos:
        o = oracle.setup_buckets(lo, hi, hb)
        assert PL.buckets(lo, hi, hb) == (o["bucket_size"], o["n_values"]), (lo, hi, hb, o)
    sizes = {PL.buckets(*v[:3]) for v in PL.BUCKET_COLS.values()}
    assert {(1, 3), (1, 4), (3, 102), (7, 1002), (999, 1002), (1000, 1002), (4096, 1002), (65535, 1002), (65536, 1002), (66908, 1002), (66909, 1002)} <= sizes


def test_lane_to_sub_bin():
    """Canonical: 2 rows per lane, 2048-row tile; compact: 4 rows per lane, 4096-row tile; the sub-bin is tid & mask."""
    r = np.arange(3 * PL.TILE)
    for ss in (0, 1, 5, 9):
        mask = (1 << ss) - 1
        assert np.array_equal(PL.sub_bin(r, ss, False), ((r % 2048) // 2) & mask) and np.array_equal(PL.sub_bin(r, ss, True), ((r % 4096) // 4) & mask)
        assert PL.sub_bin(r, ss, True).max() == mask == PL.sub_bin(r, ss, False).max()
    assert PL.sub_bin([0, 1, 2, 3, 4, 2047, 2048, 4095, 4096], 3, False).tolist() == [0, 0, 1, 1, 2, 7, 0, 7, 0]
    assert PL.sub_bin([0, 3, 4, 7, 8, 4095, 4096], 3, True).tolist() == [0, 0, 1, 1, 2, 7, 0]


# ---------------------------------------------------------------------------------------------- edges
def test_edges_places_every_region_size_in_every_share(n_wg, edges):
    assert edges.n == n_wg * PL.SHARE and [len(s) for s in PL.shares(edges, n_wg)] == [1] * n_wg
    assert [s[0] for s in PL.shares(edges, n_wg)] == [(w * PL.SHARE, PL.SHARE) for w in range(n_wg)]
    assert PL.geometry(65536, 1, edges.n, n_wg)[:4] == (1024, 0, 1024, 1)
    k = len(PL.EDGE_COUNTS)
    for compact in (False, True):
        rr = PL.region_records(edges, Q1, n_wg, compact)
        assert rr.shape == (n_wg, 1024) and rr.sum() == edges.n
        for w in range(n_wg):
            assert [int(rr[w, PL.EDGE_PARTS[(i + w) % k]]) for i in range(k)] == list(PL.EDGE_COUNTS), w
        # the walk of one partition meets every size, empty regions included, next to one another
        for p in PL.EDGE_PARTS:
            assert set(rr[:k, p].tolist()) == set(PL.EDGE_COUNTS)
        other = np.setdiff1d(np.arange(1024), PL.EDGE_PARTS + PL.BG_PARTS)
        assert (rr[:, other] == 0).all() and (rr[:, list(PL.BG_PARTS)] > 0).all()
        # under the filter the placed regions are what they were and nothing else is left
        fr = PL.region_records(edges, dict(Q1, filters=PL.EDGE_FILTER), n_wg, compact)
        assert np.array_equal(fr[:, list(PL.EDGE_PARTS)], rr[:, list(PL.EDGE_PARTS)]) and fr.sum() == n_wg * sum(PL.EDGE_COUNTS)
    # around the chunk (16) and the wave batch (1024): every count, one less and one more
    assert all({c - 1, c, c + 1} <= set(PL.EDGE_COUNTS) for c in (16, 32, 48, PL.BATCH)) and {0, 1} <= set(PL.EDGE_COUNTS)
    g = edges.cols["g"]
    assert int(g.min()) == 0 and int(g.max()) == 65535 and np.unique(g).size == 3 * k + 2 * len(PL.BG_PARTS)
    assert set((np.unique(g[edges.cols["f"] == 1]) % PL.PART).tolist()) == set(PL.EDGE_LOCALS)


# ---------------------------------------------------------------------------------------------- few, limits, tiny, padding
def test_few_tables(n_wg):
    for name, rows in PL.few_rows(n_wg).items():
        L = PL.few(n_wg, name)
        assert L.n == rows
        for key, cells in dict(PL.FEW_KEYS, kx=PL.nondividing_cells(n_wg)).items():
            assert L.keys[key] == (0, cells - 1) and np.unique(L.cols[key]).size == cells          # every declared cell, the last pair too
        sh = PL.shares(L, n_wg)
        with_rows = sum(1 for s in sh if s)
        assert sum(n for s in sh for _, n in s) == rows and (with_rows < n_wg // 4 if name != "r2" else with_rows == n_wg)
        if name != "r2":
            assert sh[-1] and not sh[0]           # workgroups without rows before workgroups with rows
        # sub-bins: every bin of a partition takes records where ss > 0 (compact and canonical differ in which)
        q = dict(groups=["k33"], aggs=["va", "vb"])
        parts, ss, bins, split, ok, why = PL.geometry(33, 2, rows, n_wg)
        for compact in (False, True):
            rr = PL.region_records(L, q, n_wg, compact)
            assert rr.shape == (n_wg, bins) and rr.sum() == 2 * rows and (rr.sum(axis=0) > 0).all()
        assert ss == 0 or not np.array_equal(PL.region_records(L, q, n_wg, False), PL.region_records(L, q, n_wg, True))


def test_limit_tiny_and_padding_tables(n_wg):
    L = PL.limit_shapes(n_wg)
    for key, cells in PL.LIMIT_KEYS.items():
        assert L.keys[key] == (0, cells - 1) and int(L.cols[key].min()) == 0 and int(L.cols[key].max()) == cells - 1
    assert L.n % 2 == 1 and PL.geometry(32768, 2, L.n, n_wg)[4] and not PL.geometry(32769, 2, L.n, n_wg)[4]
    for rows in PL.TINY_ROWS:
        T = PL.tiny(rows)
        assert T.n == rows and PL.geometry(65536, 1, rows, n_wg)[:5] == (1024, 0, 1024, 1, True)
    assert {r % PL.UNIT for r in PL.TINY_ROWS} >= {1, 15, 16, 17, 2047} and {r % PL.TILE for r in PL.TINY_ROWS} >= {4095, 1}
    P = PL.padding(n_wg)
    assert PL.geometry(65536, 1, P.n, n_wg)[:4] == (1024, 0, 1024, 1)
    rr = PL.region_records(P, Q1, n_wg, True)
    assert rr[:, 0].tolist() == [1] * n_wg                     # one record and fifteen padding records in partition 0's regions
    wg, _ = PL.row_owner(P, n_wg)
    zero = P.cols["g"] < PL.PART
    assert P.cols["g"][zero][np.argsort(wg[zero])].tolist() == [w % 2 for w in range(n_wg)]
    bs = PL.buckets(*PL.INFO_A)[0]
    first = P.cols["g"] % PL.PART == 0
    assert (P.cols["va"][first] < bs).all() and first.sum() > n_wg          # a partition's first pair: populated, in bucket 0
    assert (P.cols["va"][P.cols["g"] == 1] >= bs).all()
    assert not PL.hist_fits_lds(64, [1002]) and not PL.hist_fits_lds(32, [1002, 1002]) and not PL.hist_fits_lds(32768, [3, 1002])
    assert not PL.hist_fits_lds(65536, [3])


# ---------------------------------------------------------------------------------------------- bucket edges
def test_bucket_edge_columns_hold_their_edges():
    B = PL.bucket_edges()
    widths = set()
    for name, (lo, hi, hb, role, bs, width) in PL.BUCKET_COLS.items():
        v = B.cols[name]
        assert (bs, ) == PL.buckets(lo, hi, hb)[:1]
        nv = PL.buckets(lo, hi, hb)[1]
        end = lo + nv * bs                     # the first value beyond the last bucket
        top = int(v.max())
        assert int(v.min()) == lo and top <= hi * 10
        if role == "plain":
            assert top == hi
        elif role == "tmax":
            assert hi < top == end - 1
        else:
            assert top == PL.OUT_MAX + (role == "outl_far") and {end - 1, end, end + 1} <= set(v.tolist())
        assert PL.instantiation(lo, hi, hb, top) == (role != "plain", top >= end)
        # every exact multiple of BucketSize the range holds, with its neighbours, for k in 0, 1, 2, nv / 2, nv - 2, nv - 1
        want = {lo + k * bs + d for k in (0, 1, 2, nv // 2, nv - 2, nv - 1) for d in (-1, 0, 1)}
        want = {x for x in want if lo <= x <= min(top, hi if role == "plain" else top)}
        for gkey in PL.BUCKET_GROUPS:
            assert want <= set(v[B.cols["h"] == gkey].tolist()), (name, gkey)
        assert len(want) >= (2 if nv < 10 else 12), (name, sorted(want))
        span = top - int(v.min())
        assert width == (1 if span < 256 else 2 if span < 65536 else 4)
        widths.add(width)
        assert PL.record_fits(lo, hi, hb, top) == {"b66909": (False, "bucket"), "outl_far": (False, "span")}.get(name, (True, "ok"))
    assert widths == {1, 2, 4}
    assert {v[0] for v in PL.BUCKET_COLS.values()} >= {-1, 0, 1 << 40} and any(v[0] < -1000 for v in PL.BUCKET_COLS.values())
    assert int(B.cols["g"].max()) == 65535 and int(B.cols["h"].max()) == 32767


# ---------------------------------------------------------------------------------------------- reference() against the oracle
def _oracle(oracle, L, q):
    names = list(q["groups"]) + list(q["aggs"])
    ocols = [{"type": "int", "data": L.cols[c]} for c in names]
    return oracle.run_query(ocols, n_threads=4, **parity.oracle_query_kwargs(names, L.info, dict(q, op="hist")))


def check_reference_against_oracle(ref, o, q):
    """reference() and oracle.run_query say the same: groups, Count, buckets, sum, extrema, outliers; Cumulative."""
    assert ref["overflow"] == 0 and ref["matched"] == o["matched"]
    assert {r["key_vals"] for r in o["results"]} == {tuple(k % (1 << 64) for k in key) for key in ref["groups"]}
    rows = [(ref["groups"][tuple(k - (1 << 64) if k >= 1 << 63 else k for k in r["key_vals"])], r) for r in o["results"]]
    for (count, aggs), r in rows + [(ref["cumulative"], o["cumulative"])]:
        assert r["count"] == count
        for a, h in zip(aggs, r["hists"]):
            assert h["present"] and (h["count"], h["sum_exact"], h["min"], h["max"]) == (count, a["sum"], a["min"], a["max"]), (r["key_vals"], h)
            assert np.array_equal(h["values"], a["values"]) and h["n_outliers"] == a["n_outliers"] and h["n_underliers"] == 0
            assert np.array_equal(np.sort(h["outlier_values"]), a["outlier_values"]) and a["outlier_sum"] == int(a["outlier_values"].sum())


BUCKET_QUERIES = [dict(groups=["g"], aggs=[c], hist_bucket=v[2]) for c, v in PL.BUCKET_COLS.items()] + \
                 [dict(groups=["h"], aggs=["b999", "b66908t"]), dict(groups=["h"], aggs=["outl", "b999"]), dict(groups=["h"], aggs=["b1odd", "b999"])]


@pytest.mark.parametrize("q", BUCKET_QUERIES, ids=lambda q: "-".join(q["aggs"]))
def test_reference_equals_the_oracle_on_bucket_edges(oracle, q):
    B = PL.bucket_edges()
    ref = PL.reference(B, q)
    check_reference_against_oracle(ref, _oracle(oracle, B, q), q)
    assert len(ref["groups"]) == PL.BUCKET_GROUPS.size + (q["groups"] == ["g"])
    for a, name in zip(ref["cumulative"][1], q["aggs"]):
        lo, hi, hb, role, bs, _ = PL.BUCKET_COLS[name]
        assert (a["n_outliers"] > 0) == PL.instantiation(lo, hi, hb, B.data_max(name))[1] and (a["max"] > hi) == (role != "plain")
        # bucket k holds exactly the rows at Info.Min + k x BucketSize and + 1, bucket k - 1 the rows one below
        v = B.cols[name]
        for k in (1, 2):
            if lo + (k + 1) * bs <= int(v.max()) and bs > 1:
                assert a["values"][k] >= int(((v == lo + k * bs) | (v == lo + k * bs + 1)).sum()) > 0
                assert a["values"][k - 1] >= int((v == lo + k * bs - 1).sum()) > 0


def test_reference_equals_the_oracle_on_a_few_table(oracle):
    L = PL.few(256, "r1")
    for q in (dict(groups=["k33"], aggs=["va", "vb"]), dict(groups=["k130"], aggs=["vb"]), dict(groups=["k65"], aggs=["va"], hist_bucket=990)):
        ref = PL.reference(L, q)
        check_reference_against_oracle(ref, _oracle(oracle, L, q), q)
        assert len(ref["groups"]) == PL.FEW_KEYS[q["groups"][0]]
    E = PL.tiny(4097)
    q = dict(groups=["g"], aggs=["va"], filters=[("va", "gt", 500_000)])
    ref = PL.reference(E, q)
    assert 0 < ref["matched"] < 4097
    names = ["g", "va"]
    o = oracle.run_query([{"type": "int", "data": E.cols[c]} for c in names], **parity.oracle_query_kwargs(names, E.info, dict(q, op="hist")))
    check_reference_against_oracle(ref, o, q)
