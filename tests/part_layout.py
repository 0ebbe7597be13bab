"""Placed tables behind tests/test_gpu_part_hist.py, and their exact references; checked on the CPU by tests/test_part_layout.py.

Strategy 5 (partitioned histograms: k_count* -> k_emit* -> k_part_hist -> k_part_fix; csrc/scan_fast.h, scan_packed.h, kernels.hip)
is a counting sort whose geometry is exact: what can go wrong is where a partition, a staging bin, a 16-record chunk, a
1024-record wave batch or a bucket begins and ends.  These tables PLACE rows there.

Geometry, the code's (planner.cpp: plan_part_pass, bind_part_pass, setup_buckets, deal_tiles):
  * a pass takes one or two aggregations (a query of three or four runs two passes over the one record buffer); its pairs are
    (cell, agg), cell x aggs + agg; a partition is PART = 64 pairs, at most MAX_PARTS = 1024 of them (`why=pairs` beyond);
  * a partition is spread over 1 << ss staging bins: ss is the largest with parts << ss <= 1024, stepped down while
    rows x aggs / (n_wg x bins) < 64; a lane's sub-bin is tid & ((1 << ss) - 1), tid = (row in segment % tile) / rows per lane
    -- canonical storage: 2 rows per lane, 2048-row tile; compact: 4 rows per lane, 4096-row tile;
  * a workgroup's rows are deal_tiles' (window_layout.shares); k_count sizes a region per (workgroup, bin) as whole chunks of
    CHUNK = 16 records, k_emit fills it and pads the last chunk with the all-zero record;
  * k_part_hist: split = max(1, n_wg / parts) workgroups share a partition, share `sub` walking the regions of the workgroups
    sub, sub + split, ...: (n_wg - sub + split - 1) / split of them (`regions`); a wave takes BATCH = 1024 records of a region
    at a time and masks the lanes of the last batch;
  * a record is local pair << 26 | (v - Info.Min + BucketSize): (len(Values) + 1) x BucketSize < 2^26, BucketSize < 2^24,
    len(Values) <= 1024 (`why=bucket`); where a value may lie beyond the last bucket, every accepted value must fit as well:
    span = min(max, Info.Max x 10) - Info.Min + BucketSize < 2^26 - 1 and span / BucketSize < 2^24 (`why=span`);
  * k_part_hist<aggs, TRACK_MAX, OUT>: TRACK_MAX when some column's maximum lies above its Info.Max, OUT when some column's
    accepted maximum lies beyond its last bucket -- which ends above Info.Max, or below it: BucketSize = size / 1000 rounds
    down, and 1002 buckets of 49 end at 49098 under Info = [0, 49999] (`instantiation`).

Tests use geometry / region_records only to check that a table has the shape its case claims and to predict the `part hist:`
trace line; every expected RESULT comes from reference().

Every table honours its contract -- keys inside their declared bounds, values inside [Info.Min, Info.Max x 10], which is what
the reference accepts (hist_basic.go:104) -- and Layout asserts it: the plain row bodies take those bounds on trust.

Cases:
  * edges(n_wg): key g (2 stored bytes, 65536 declared cells), one aggregation: 1024 partitions, ss = 0, a bin is a partition.
    n_wg x 8192 rows, a share of two 4096-row tiles per workgroup.  In every share the EDGE_PARTS receive exactly EDGE_COUNTS
    records (0, 1, 15, 16, 17, ..., 1023, 1024, 1025), rotated by one partition from workgroup to workgroup: the walk of one
    partition meets regions of every size, empty ones included.  The other rows go to BG_PARTS.  Column f is 1 on the placed
    rows and 0 on the others: under f > 0 the region sizes are still the placed ones (and BG_PARTS' regions are all empty).
  * few(n_wg): keys of 64, 65, 32, 33 and 130 declared cells (FEW_KEYS; with one or two aggregations: one partition exactly, a
    last partition of one pair or of one cell, three partitions) at three row counts (FEW_ROWS) that end inside a lane's rows:
    ss takes 0, 1 and >= 5, the step-down fires, 130 cells give a split that does not divide 256 or 304 workgroups (kx: a
    key for which it does not divide n_wg, whatever n_wg).  Few rows: most workgroups have none, next to some that do.
  * limit_shapes(n_wg): keys of 32768, 32769 and 65537 declared cells: 32768 x 2 is the last eligible shape (1024 partitions),
    32769 x 2 and 65537 x 1 the first that are not, 32768 x 3 two passes of 1024 and 512 partitions.
  * tiny(rows): TINY_ROWS = 1, 15, 16, 17, 2047, 2049, 4095, 4097 rows under key g.
  * bucket_edges(): per value column (BUCKET_COLS) rows at Info.Min + k x BucketSize + {-1, 0, +1} for k in {0, 1, 2, nv / 2,
    nv - 2, nv - 1}, clipped to the column's range, in every group; roles plain (max <= Info.Max), tmax (Info.Max < max <
    Info.Min + nv x BucketSize), outl (a maximum beyond the last bucket at the largest eligible span) and outl_far (one more:
    `why=span`); BucketSize 1 (odd and even nv), 3, 7 (-int-bucket), 49, 999, 1000, 4096, 65535, 65536, 66908 (the largest
    eligible with 1002 values) and 66909 (`why=bucket`); Info.Min negative, 0 and 2^40; stored widths 1, 2 and 4 bytes.  Keys g
    (65536 cells) and h (32768 cells, for two aggregations).
  * padding(n_wg): n_wg x 2048 rows under key g (split = 1): every share holds exactly ONE row of partition 0 -- cell 0 in
    bucket 0, or cell 1, by turns -- so its region there is one record and fifteen padding records; every background
    partition's first cell is populated in bucket 0 as well (padding counts in field 0 of a partition's first pair, whose
    carry goes into that pair's bucket 0).
"""
import numpy as np

from tests import window_layout as WL

PART = 64              # kPartCells
MAX_PARTS = 1024       # kMaxParts
MAX_BINS = 1024        # kEmitMaxBins
CHUNK = 16             # kEmitChunk
BATCH = 1024           # k_part_hist: kBatch = 256 pieces of four records
REC_BITS = 26          # kRecValueBits
MAX_VALUES = 1024      # 1 << kBucketBits
LDS_BUDGET = WL.LDS_BUDGET
UNIT, TILE = WL.UNIT, WL.TILE
SHARE = 2 * TILE
BLOCK = 65536          # rows of an appended block (a multiple of 32: the blocks touch and physical rows are logical rows)
ROWS_PER_LANE = {False: 2, True: 4}          # by `compact`
TILE_ROWS = {False: UNIT, True: TILE}


# ---------------------------------------------------------------------------------------------- the planner, restated
def buckets(info_min, info_max, hist_bucket=0):
    """setup_buckets (hist_basic.go:34-70): (BucketSize, len(Values))."""
    size = info_max - info_min
    nb = 1000
    bs = size // nb
    if hist_bucket > 0:
        bs = hist_bucket
    if bs == 0:
        if size < 100:
            bs, nb = 1, size
        else:
            bs = size // 100
            nb = size // bs
    return bs, nb + 2


def geometry(n_cells, na, rows, n_wg, wg_rows_max=None):
    """plan_part_pass / bind_part_pass for one pass of `na` aggregations over `rows` scanned rows:
    (parts, ss, bins, split, eligible, why).  wg_rows_max: the largest share (default: rows dealt evenly in 2048-row units)."""
    pairs = n_cells * na
    parts = (pairs + PART - 1) // PART
    if parts > MAX_PARTS:
        return parts, 0, 0, 0, False, "pairs"
    if n_wg > 2048:
        return parts, 0, 0, 0, False, "n_wg"
    recs = rows * na
    ss = 0
    while (parts << (ss + 1)) <= MAX_BINS:
        ss += 1
    while ss > 0 and recs // (n_wg * (parts << ss)) < 64:
        ss -= 1
    bins = parts << ss
    split = max(1, n_wg // parts)
    if wg_rows_max is None:
        units = (rows + UNIT - 1) // UNIT
        wg_rows_max = (units + n_wg - 1) // n_wg * UNIT
    if recs + n_wg * bins * CHUNK + CHUNK >= (1 << 32) - (1 << 22) or (wg_rows_max * na + bins * CHUNK) * 4 >= 1 << 31:
        return parts, ss, bins, split, False, "cap"
    return parts, ss, bins, split, True, "ok"


def passes(n_aggs):
    """[(first aggregation, aggregations)] of a query: k_emit / k_part_hist take two."""
    return [(a0, min(2, n_aggs - a0)) for a0 in range(0, n_aggs, 2)]


def regions(n_wg, split):
    """Regions (scanning workgroups) every share of a partition walks."""
    return [(n_wg - sub + split - 1) // split if n_wg > sub else 0 for sub in range(split)]


def record_fits(info_min, info_max, hist_bucket, data_max):
    """The 2^26 / 2^24 limits of plan_part_pass for one column: (fits, why)."""
    bs, nv = buckets(info_min, info_max, hist_bucket)
    if nv > MAX_VALUES or bs >= 1 << 24 or (nv + 1) * bs >= 1 << REC_BITS:
        return False, "bucket"
    if instantiation(info_min, info_max, hist_bucket, data_max)[1]:
        hi = min(data_max, info_max * 10)
        span = hi - info_min + bs
        if span >= (1 << REC_BITS) - 1 or span // bs >= 1 << 24:
            return False, "span"
    return True, "ok"


def instantiation(info_min, info_max, hist_bucket, data_max):
    """(track_max, out) of a column (Planner::aggregations: m_max, f_out), data inside [Info.Min, Info.Max x 10]."""
    bs, nv = buckets(info_min, info_max, hist_bucket)
    vhi = min(data_max, info_max * 10)
    return data_max > info_max, (max(vhi - info_min, 0) // bs >= nv)


def hist_fits_lds(n_cells, nvs):
    """select_fast_path keeps the bucket arrays of few cells in LDS (strategy 2, not 5): a lower bound of what it needs."""
    return n_cells * sum(nvs) * 4 + (1 + len(nvs)) * n_cells * 8 <= LDS_BUDGET


def sub_bin(row_in_segment, ss, compact):
    """The sub-bin of a row: its lane's number, masked."""
    tid = (np.asarray(row_in_segment) % TILE_ROWS[compact]) // ROWS_PER_LANE[compact]
    return tid & ((1 << ss) - 1)


def nondividing_cells(n_wg):
    """The fewest cells (one aggregation) whose split = n_wg / parts > 1 does not divide n_wg: a last pair past whole partitions."""
    for parts in range(2, n_wg // 2 + 1):
        if n_wg % (n_wg // parts):
            return PART * (parts - 1) + 2
    raise AssertionError(n_wg)


# ---------------------------------------------------------------------------------------------- layouts
class Layout:
    """cols: name -> int64 array; keys: name -> declared (lo, hi); info: name -> (Info.Min, Info.Max) of the value columns."""

    def __init__(self, name, n, cols, keys, info, other=None, hist_bucket=None):
        self.name, self.n = name, int(n)
        self.blocks = [BLOCK] * (self.n // BLOCK) + ([self.n % BLOCK] if self.n % BLOCK else [])
        self.cols, self.keys, self.info, self.other = cols, dict(keys), dict(info), dict(other or {})
        self.hist_bucket = dict(hist_bucket or {})           # column -> the -int-bucket its edges were placed for
        self.order = tuple(cols)
        for c, a in cols.items():
            assert a.dtype == np.int64 and a.shape == (self.n,), (name, c)
        for c, (lo, hi) in list(self.keys.items()) + list(self.other.items()):
            assert lo <= int(cols[c].min()) and int(cols[c].max()) <= hi, (name, c)
        for c, (lo, hi) in self.info.items():
            assert lo <= int(cols[c].min()) and int(cols[c].max()) <= hi * 10, (name, c, int(cols[c].min()), int(cols[c].max()))
        assert set(cols) == set(self.keys) | set(self.info) | set(self.other), name

    def declared(self, c):
        return self.keys.get(c) or self.info.get(c) or self.other[c]

    def data_max(self, c):
        return int(self.cols[c].max())

    def cells(self, q):
        n = 1
        for g in q["groups"]:
            n *= self.keys[g][1] - self.keys[g][0] + 1
        return n


def shares(layout, n_wg):
    return WL.shares(layout.blocks, n_wg)


def row_owner(layout, n_wg):
    """(workgroup, row offset inside its segment) of every row."""
    wg = np.full(layout.n, -1, dtype=np.int64)
    off = np.zeros(layout.n, dtype=np.int64)
    for w, segs in enumerate(shares(layout, n_wg)):
        for s0, sn in segs:
            assert wg[s0:s0 + sn].max(initial=-1) == -1
            wg[s0:s0 + sn] = w
            off[s0:s0 + sn] = np.arange(sn)
    assert (wg >= 0).all()          # (blocks of BLOCK rows: physical rows are logical rows, and every one is dealt)
    return wg, off


def keep(layout, filters):
    m = np.ones(layout.n, dtype=bool)
    for c, op, v in filters or ():
        m &= {"gt": layout.cols[c] > v, "lt": layout.cols[c] < v, "eq": layout.cols[c] == v}[op]
    return m


def region_records(layout, q, n_wg, compact, a0=0, na=None):
    """[n_wg][bins] records of the pass [a0, a0 + na) of q: what k_count must count (a region is this, rounded up to chunks)."""
    na = na or passes(len(q["aggs"]))[0][1]
    parts, ss, bins, split, ok, why = geometry(layout.cells(q), na, layout.n, n_wg)
    assert ok, why
    (g,) = q["groups"]
    wg, off = row_owner(layout, n_wg)
    m = keep(layout, q.get("filters"))
    cell = layout.cols[g] - layout.keys[g][0]
    b = (((cell * na) // PART) << ss) | sub_bin(off, ss, compact)
    out = np.bincount(wg[m] * bins + b[m], minlength=n_wg * bins).reshape(n_wg, bins)
    return out * na


INFO_A, INFO_B, INFO_C = (0, 999_999), (0, 49_999), (0, 999_999)


def _values(rng, n, info):
    v = rng.integers(info[0], info[1] + 1, n, dtype=np.int64)
    if n >= 2:
        v[0], v[n - 1] = info[0] + 1, info[1]        # (the stored width is the same in every table; the maximum is Info.Max)
    return v


# ---- edges
G_KEY = (0, 65535)
EDGE_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1023, 1024, 1025)
EDGE_PARTS = (0, 1, 2, 3, 255, 256, 511, 512, 513, 767, 768, 1021, 1022, 1023)
EDGE_LOCALS = (0, 1, 63)                       # the cells of a placed partition that take its rows, by turns
BG_PARTS = tuple(range(5, 1021, 43))           # 24 partitions, none of them placed
BG_LOCALS = (7, 40)
assert len(EDGE_COUNTS) == len(EDGE_PARTS) and not set(EDGE_PARTS) & set(BG_PARTS) and sum(EDGE_COUNTS) < SHARE


def edges(n_wg, seed=11):
    rng = np.random.default_rng(seed)
    n = n_wg * SHARE
    g = np.empty(n, dtype=np.int64)
    f = np.empty(n, dtype=np.int64)
    k = len(EDGE_COUNTS)
    n_placed = sum(EDGE_COUNTS)
    bg_cells = np.array([PART * p + l for p in BG_PARTS for l in BG_LOCALS], dtype=np.int64)
    for w in range(n_wg):
        placed = np.concatenate([PART * EDGE_PARTS[(i + w) % k] + np.array(EDGE_LOCALS, dtype=np.int64)[np.arange(c) % len(EDGE_LOCALS)]
                                 for i, c in enumerate(EDGE_COUNTS)])
        keys = np.concatenate([placed, bg_cells[rng.integers(0, bg_cells.size, SHARE - n_placed)]])
        flag = np.concatenate([np.ones(n_placed, dtype=np.int64), np.zeros(SHARE - n_placed, dtype=np.int64)])
        p = rng.permutation(SHARE)
        g[w * SHARE:(w + 1) * SHARE] = keys[p]
        f[w * SHARE:(w + 1) * SHARE] = flag[p]
    cols = {"f": f, "g": g, "va": _values(rng, n, INFO_A), "vb": _values(rng, n, INFO_B)}
    return Layout("edges", n, cols, {"g": G_KEY}, {"va": INFO_A, "vb": INFO_B}, {"f": (0, 1)})


EDGE_FILTER = [("f", "gt", 0)]


# ---- few
FEW_KEYS = {"k64": 64, "k65": 65, "k32": 32, "k33": 33, "k130": 130}
FEW_SHAPES = (("k64", 1), ("k65", 1), ("k32", 2), ("k33", 2), ("k130", 1), ("kx", 1))      # (key, aggregations): what the issue lists, and kx


def few_rows(n_wg):
    """Three row counts, each ending inside a lane's 2 or 4 rows: ss of one partition and one aggregation is 0, 1 and 5."""
    return {"r0": n_wg * 64 + 3, "r1": n_wg * 192 + 1, "r2": n_wg * 2048 + 5}


def few(n_wg, rows_name, seed=12):
    rng = np.random.default_rng(seed + len(rows_name) + ord(rows_name[-1]))
    n = few_rows(n_wg)[rows_name]
    keys = dict({k: (0, c - 1) for k, c in FEW_KEYS.items()}, kx=(0, nondividing_cells(n_wg) - 1))
    cols = {}
    for k, (lo, hi) in keys.items():
        cols[k] = rng.integers(lo, hi + 1, n, dtype=np.int64)
        cols[k][1], cols[k][n - 2] = lo, hi
    cols["va"], cols["vb"] = _values(rng, n, INFO_A), _values(rng, n, INFO_B)
    return Layout("few_" + rows_name, n, cols, keys, {"va": INFO_A, "vb": INFO_B})


# ---- limit shapes
LIMIT_KEYS = {"k32768": 32768, "k32769": 32769, "k65537": 65537}


def limit_shapes(n_wg, seed=13):
    rng = np.random.default_rng(seed)
    n = n_wg * UNIT + 7
    keys = {k: (0, c - 1) for k, c in LIMIT_KEYS.items()}
    cols = {}
    for k, (lo, hi) in keys.items():
        some = np.array(sorted({0, 1, 31, 32, 63, 64, 65, hi // 2, hi - 64, hi - 63, hi - 32, hi - 1, hi}), dtype=np.int64)
        cols[k] = some[rng.integers(0, some.size, n)]
        cols[k][1], cols[k][n - 2] = lo, hi
    cols["va"], cols["vb"], cols["vc"] = _values(rng, n, INFO_A), _values(rng, n, INFO_B), _values(rng, n, INFO_C)
    return Layout("limits", n, cols, keys, {"va": INFO_A, "vb": INFO_B, "vc": INFO_C})


# ---- tiny
TINY_ROWS = (1, 15, 16, 17, 2047, 2049, 4095, 4097)
TINY_CELLS = np.array([0, 1, 63, 64, 32767, 32768, 65472, 65535], dtype=np.int64)


def tiny(rows, seed=14):
    rng = np.random.default_rng(seed + rows)
    cols = {"g": TINY_CELLS[rng.integers(0, TINY_CELLS.size, rows)], "va": rng.integers(1, INFO_A[1] + 1, rows, dtype=np.int64)}
    return Layout("tiny%d" % rows, rows, cols, {"g": G_KEY}, {"va": INFO_A})


# ---- bucket edges
H_KEY = (0, 32767)
OUT_INFO = (0, 8_000_000)
OUT_MAX = OUT_INFO[0] + (1 << REC_BITS) - 2 - buckets(*OUT_INFO)[0]      # span = 2^26 - 2: the largest eligible
# column -> (Info.Min, Info.Max, -int-bucket or 0, role, BucketSize, stored bytes after compact())
BUCKET_COLS = {
    "b1odd": (0, 1, 0, "plain", 1, 1),                        # size < 100: nv = 3
    "b1even": (-1, 1, 0, "plain", 1, 1),                      # nv = 4, a negative Info.Min
    "b3": (0, 300, 0, "plain", 3, 2),                         # size 100...999
    "b3t": (0, 300, 0, "tmax", 3, 2),
    "b7": (0, 7010, 7, "plain", 7, 2),                        # -int-bucket
    "b7t": (0, 7010, 7, "tmax", 7, 2),
    "b49": (0, 49_999, 0, "plain", 49, 2),                    # 1002 x 49 < Info.Max: outliers without a tracked maximum
    "b999": (0, 999_999, 0, "plain", 999, 4),
    "b1000": (-500_000, 500_000, 0, "plain", 1000, 4),
    "b4096": (1 << 40, (1 << 40) + 4_096_000, 0, "plain", 4096, 4),
    "b65535": (0, 65_535_000, 0, "plain", 65535, 4),
    "b65536": (0, 65_536_000, 0, "plain", 65536, 4),
    "b66908": (0, 66_908_000, 0, "plain", 66908, 4),          # 1003 x 66908 < 2^26: the largest eligible BucketSize at 1002 values
    "b66908t": (0, 66_908_000, 0, "tmax", 66908, 4),
    "b66909": (0, 66_909_000, 0, "plain", 66909, 4),          # 1003 x 66909 > 2^26
    "outl": OUT_INFO + (0, "outl", 8000, 4),
    "outl_far": OUT_INFO + (0, "outl_far", 8000, 4),
}
BUCKET_GROUPS = np.array([0, 1, 63, 64, 65, 127, 128, 32767], dtype=np.int64)      # cells under g and h alike
BUCKET_ROWS = 3 * UNIT + 1


def bucket_column(name):
    """The column's edge values, sorted: Info.Min + k x BucketSize + {-1, 0, +1}, clipped to its role's range."""
    lo, hi, hb, role, bs_claim, _ = BUCKET_COLS[name]
    bs, nv = buckets(lo, hi, hb)
    assert bs == bs_claim, (name, bs)
    top = {"plain": hi, "tmax": lo + nv * bs - 1, "outl": OUT_MAX, "outl_far": OUT_MAX + 1}[role]
    assert top <= hi * 10 and (role == "plain" or top > hi)
    # (k = nv: the first value beyond the last bucket -- within Info.Max where 1002 buckets of size / 1000 end below it: b49)
    vals = {lo + k * bs + d for k in (0, 1, 2, nv // 2, nv - 2, nv - 1, nv) for d in (-1, 0, 1)} | {top}
    return np.array(sorted(v for v in vals if lo <= v <= top), dtype=np.int64)


def bucket_edges(seed=15):
    rng = np.random.default_rng(seed)
    n = BUCKET_ROWS
    g = BUCKET_GROUPS[np.arange(n) % BUCKET_GROUPS.size]
    cols = {"g": g.copy(), "h": g.copy()}
    cols["g"][n - 1] = G_KEY[1]                      # (a group of one row in the last cell of the last partition)
    info, hb = {}, {}
    for name, (lo, hi, b, role, _, _) in BUCKET_COLS.items():
        e = bucket_column(name)
        # every group takes every edge value: group of row i is i % 8, value number (i // 8) % len -- and a shuffled tail
        v = e[(np.arange(n) // BUCKET_GROUPS.size) % e.size]
        assert n // BUCKET_GROUPS.size >= 2 * e.size
        tail = n // 2 + rng.permutation(n - n // 2)
        v[n // 2:] = v[tail]
        cols[name], info[name] = v, (lo, hi)
        if b:
            hb[name] = b
    return Layout("bucket_edges", n, cols, {"g": G_KEY, "h": H_KEY}, info, hist_bucket=hb)


# ---- padding
def padding(n_wg, seed=16):
    rng = np.random.default_rng(seed)
    n = n_wg * UNIT
    bs = buckets(*INFO_A)[0]
    bg_first = np.array([PART * p for p in BG_PARTS], dtype=np.int64)
    bg_cells = np.array([PART * p + l for p in BG_PARTS for l in (0,) + BG_LOCALS], dtype=np.int64)
    g = bg_cells[rng.integers(0, bg_cells.size, n)]
    va = rng.integers(1, INFO_A[1] + 1, n, dtype=np.int64)
    va[np.isin(g, bg_first)] = rng.integers(0, bs, int(np.isin(g, bg_first).sum()))       # bucket 0 of a partition's first pair
    at = np.arange(n_wg) * UNIT + rng.integers(0, UNIT, n_wg)                           # one row of every share
    g[at] = np.arange(n_wg) % 2                                                         # cell 0, cell 1, cell 0, ...
    va[at] = np.where(g[at] == 0, rng.integers(0, bs, n_wg), rng.integers(bs, INFO_A[1], n_wg))
    return Layout("padding", n, {"g": g, "va": va}, {"g": G_KEY}, {"va": INFO_A})


# ---------------------------------------------------------------------------------------------- the exact answer
def reference(layout, q):
    """numpy group-by of a full-histogram query: {"matched", "overflow", "groups": {key tuple: (Count, [per aggregation
    {"values", "sum", "min", "max", "n_outliers", "outlier_sum", "outlier_values"}])}, "cumulative": (Count, [the same])}.
    hist_basic.go:101-151 on tables that honour their contract: every value is accepted; bucket (v - Info.Min) / BucketSize, a
    value beyond the last bucket clipped into it and remembered; Min / Max start at Info.Min / Info.Max."""
    cols = layout.cols
    m = keep(layout, q.get("filters"))
    inb = np.ones(layout.n, dtype=bool)
    for g in q["groups"]:
        lo, hi = layout.keys[g]
        inb &= (cols[g] >= lo) & (cols[g] <= hi)
    matched, overflow = int(m.sum()), int((m & ~inb).sum())
    m &= inb
    cell = np.zeros(int(m.sum()), dtype=np.int64)             # the key columns as digits of one number, first column highest
    for g in q["groups"]:
        lo, hi = layout.keys[g]
        cell = cell * (hi - lo + 1) + (cols[g][m] - lo)
    ucell, inv = np.unique(cell, return_inverse=True)
    G = ucell.size
    uniq = np.zeros((G, len(q["groups"])), dtype=np.int64)
    for k, g in reversed(list(enumerate(q["groups"]))):
        lo, hi = layout.keys[g]
        uniq[:, k], ucell = ucell % (hi - lo + 1) + lo, ucell // (hi - lo + 1)
    count = np.bincount(inv, minlength=G)
    by_group = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[by_group], np.arange(G))          # (every group of `uniq` has a row)
    per_agg = []
    for a in q["aggs"]:
        lo, hi = layout.info[a]
        bs, nv = buckets(lo, hi, q.get("hist_bucket", 0))
        v = cols[a][m]
        assert v.size == 0 or (int(v.min()) >= lo and int(v.max()) <= hi * 10), a
        b = (v - lo) // bs
        out = b >= nv
        values = np.bincount(inv * nv + np.minimum(b, nv - 1), minlength=G * nv).reshape(G, nv)
        total = np.add.reduceat(v[by_group], starts) if G else np.zeros(0, dtype=np.int64)
        vmax = np.maximum(np.maximum.reduceat(v[by_group], starts), hi) if G else np.zeros(0, dtype=np.int64)
        order = np.lexsort((v[out], inv[out]))
        per_agg.append(dict(nv=nv, bs=bs, lo=lo, hi=hi, values=values, total=total, vmax=vmax, out_inv=inv[out][order], out_v=v[out][order], v=v))

    def agg_of(A, sel_values, total, vmax, out_v):
        return {"values": sel_values, "sum": int(total), "min": A["lo"], "max": int(vmax), "n_outliers": int(out_v.size),
                "outlier_sum": int(out_v.sum()), "outlier_values": np.sort(out_v)}

    groups = {}
    for i in range(G):
        aggs = []
        for A in per_agg:
            s0, s1 = np.searchsorted(A["out_inv"], [i, i + 1])
            aggs.append(agg_of(A, A["values"][i], A["total"][i], A["vmax"][i], A["out_v"][s0:s1]))
        groups[tuple(int(x) for x in uniq[i])] = (int(count[i]), aggs)
    cum = [agg_of(A, A["values"].sum(axis=0), A["total"].sum(), A["vmax"].max(initial=A["hi"]), A["out_v"]) for A in per_agg]
    return {"matched": matched, "overflow": overflow, "groups": groups, "cumulative": (int(m.sum()), cum)}
