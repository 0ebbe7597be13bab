"""Placed tables behind tests/test_gpu_time_window.py, and their exact references; checked on the CPU by tests/test_window_layout.py.

The lds-window strategies (3: k_scan<.., USE_LDS>, 4: k_scan_fast / k_scan_packed / k_scan_hash_packed<.., HASH = false>) give
every workgroup a window [wg_cell_base, + lds_cells) of the [time bucket][group] table (planner.cpp: Planner::window), accumulate
at lcell = cell - cell_base and flush the touched cells into the global table.  What can go wrong is where a window begins and
ends; these tables PLACE rows there.

Geometry, the code's:
  * append_block puts a block at the next 32-row boundary of the physical rows (table.cpp: block_begin); Planner::work joins
    scanned blocks that touch into runs, and deal_tiles (planner.cpp) hands out units of kTileRows = 2048 rows, per run,
    total * (w + 1) / n_wg - total * w / n_wg units to workgroup w.  `shares` restates exactly that.
  * a packed tile is kWgThreads x kPackedRows = 4096 rows (plan.h, scan_packed.h); the kernels launch one workgroup per CU.
  * SHARE = 8192 rows per workgroup (two packed tiles, four units): a table has n_wg x 8192 rows unless its case says otherwise.
  * Planner::window takes, per workgroup, the extrema of the time column over every block that overlaps one of its segments
    (blocks without a time value left out), truncating division by the bucket, and the widest window wmax; the query is
    windowed when wmax x cells x (sum fields + max fields) x 8 bytes <= kLdsBudgetBytes = 152 KiB (plan.h).  `windows`
    restates that.  A workgroup without a populated block keeps base 0.
  * fill_packed (planner.cpp) leaves k_scan_packed at n_cells >= 2^24.

Tests use shares / windows only to check that a table has the shape its case claims and to predict windowed or not; every
expected RESULT comes from reference().

Every table declares its time bounds N_DECL buckets wide (sybl_table_set_bounds: declared bounds size the cell table), so that
the whole [time bucket][group] table exceeds LDS at any workgroup count while a window of a few buckets fits.

Cases (functions of n_wg; the time column is sorted unless stated):
  * spike(n_wg, W=3): blocks equal shares; shares pair up -- 2j and 2j + 1 are the first and second half of one bucket, so two
    workgroups flush sums and maxima into the same cells -- but workgroup n_wg // 2, whose share holds its first row at
    k * TB - 1, its next rows at k * TB and k * TB + 1, one row in each bucket between and the rest in bucket k + W - 2, which
    the next share continues: W consecutive buckets, wmax == W.  budget(n_wg, W) is spike with W chosen by the test.
  * straddle: blocks of 12288 rows and a ragged last block (n % 2048 != 0); share g lies in bucket g, its window comes from
    two blocks and holds buckets the workgroup has no row in.
  * small_blocks: blocks of 1000 rows, each a run of its own (1000 % 32 != 0), eight or nine to a share, buckets of 8000 rows.
  * idle: 5 x 2048 + 7 rows in blocks of 2048, two buckets to a block: most workgroups have no segment.
  * nullable: blocks of 2048 rows; rows without a time value scattered, one block in the middle of share n_wg // 3 without
    any (blk_pop == 0), share 2 * n_wg // 3 made of such blocks only (no window: base 0), and a nullable group column kn.
  * signed: times from -3 * TB - 1 to 3 * TB + 1, every second of it present: bucket 0 is double width under truncation.
  * skips: blocks of 4096 rows; column s is 0 throughout every other block of a stretch (block_skip drops them under s > 0:
    the runs have gaps and a share is made of segments of blocks that are not neighbours), 0 in every fourth row elsewhere.
  * wide_declared(n_tb): 3 x 2048 + 5 rows in the LAST three of n_tb declared buckets: wg_cell_base near n_tb x 256 under the
    256-cell key kb; n_tb = 65535 and 65536 give n_cells = 2^24 - 256 and 2^24.

Columns (columns_for): keys k1 (1 stored byte, 0..5), k2 (2 bytes, a quarter of 0..299), k3, k4 (0..1), kb (1 byte, 0..255), kn (0..3, missing
rows in `nullable`); aggregation columns a1 (1 byte), a2 (2 bytes), a4 (4 bytes), sg (2 bytes, both signs), never 0; weight w
(1..5); filter columns f1 (0..999, a range filter) and f2..f5 (0..99); s (see skips).  All inside the declared bounds; a failing
row carries in-range keys and non-zero values, so a leak changes a count.
"""
import numpy as np

from tests.int64_edges import trunc_div

UNIT = 2048             # kTileRows: what deal_tiles counts
TILE = 4096             # kWgThreads x kPackedRows
SHARE = 2 * TILE        # rows of one workgroup
LDS_BUDGET = 152 * 1024  # kLdsBudgetBytes (plan.h)
PACKED_CELL_LIMIT = 1 << 24  # fill_packed: n_cells below it
TB = 3600
T0 = 1_700_000_000 - 1_700_000_000 % TB
N_DECL = 2048           # declared time buckets of every table but `signed` and `wide_declared`

KEYS = {"k1": (0, 5), "k2": (0, 299), "k3": (0, 1), "k4": (0, 1), "kb": (0, 255), "kn": (0, 3)}
INFO = {"a1": (0, 200), "a2": (0, 40_000), "a4": (0, 1_000_000), "sg": (-20_000, 30_000)}
OTHER = {"w": (1, 5), "f1": (0, 999), "f2": (0, 99), "f3": (0, 99), "f4": (0, 99), "f5": (0, 99), "s": (0, 9)}
STORED_BYTES = {"k1": 1, "k2": 2, "k3": 1, "k4": 1, "kb": 1, "kn": 1, "a1": 1, "a2": 2, "a4": 4, "sg": 2}
COLUMN_ORDER = ("f1", "f2", "f3", "f4", "f5", "s", "k1", "k2", "k3", "k4", "kb", "kn", "a1", "a2", "a4", "sg", "w", "t")
# k2 takes a quarter of its 300 declared values -- every fifth, and those around the powers of two and at both ends of a bucket's
# cells: the windows are 300 cells a bucket wide, the results (and the seconds a test spends reading them) a quarter of that
K2_VALUES = np.array(sorted(set(range(0, 300, 5)) | {1, 31, 32, 33, 63, 64, 127, 128, 129, 254, 256, 257, 297, 298, 299}), dtype=np.int64)
MISSING = -1            # a row's key where its group column has no value (MISSING_VALUE, all ones, read as int64)

F_RANGE = [("f1", "gt", 99), ("f1", "lt", 900)]
F_FIVE = F_RANGE + [("f2", "gt", 4), ("f3", "gt", 4), ("f4", "gt", 4), ("f5", "gt", 4)]


TIME = dict(time_col="t", time_bucket=TB)


def _q(**kw):
    return dict(dict(op="avg", want_percentiles=False, **TIME), **kw)


# the GPU matrix (tests/test_gpu_time_window.py); spike and straddle run all of it, the other cases FIRST_TWO unless they say otherwise
QUERIES = {
    "avg": _q(groups=["k2"], aggs=["a4"]),
    "signed_agg": _q(groups=["k2"], aggs=["sg"]),                                  # the tracked minimum: max(-v)
    "lean1": _q(groups=["k2"], aggs=["a4"], op="hist"),
    "lean2": _q(groups=["k2"], aggs=["a2", "a4"], op="hist"),
    "full": _q(groups=["k1"], aggs=["a1"], op="hist", want_percentiles=True),
    "weighted": _q(groups=["k2"], aggs=["a4"], weight_col="w"),
    "keys3": _q(groups=["k1", "k3", "k4"], aggs=["a4"]),
    "aggs3": _q(groups=["k2"], aggs=["a1", "a2", "a4"]),
    "range": _q(filters=F_RANGE, groups=["k2"], aggs=["a4"]),
    "five": _q(filters=F_FIVE, groups=["k2"], aggs=["a4"]),
    "nullable_key": _q(groups=["k1", "kn"], aggs=["a4"]),                          # `nullable` only: the MISSING digit
    "nullable_key_signed": _q(groups=["k1", "kn"], aggs=["sg"]),
    "wide": _q(groups=["kb"], aggs=["a4"]),                                        # `wide_declared` only: 256 cells
    "skip_s": _q(filters=[("s", "gt", 0)], groups=["k2"], aggs=["a4"], block_skip=True),   # `skips` only
}
FIRST_TWO = ("avg", "signed_agg")
# sum fields + max fields per cell, from Planner::aggregations: Count, per aggregation its sum (+ count and samples when
# weighted, + two moments in hist mode without percentiles), Samples when weighted; a maximum per aggregation whose values
# can beat the start value (avg mode: above 0), a minimum (as max(-v)) where they can go below it (avg mode: below 0)
FIELDS = {"avg": 3, "signed_agg": 4, "lean1": 4, "lean2": 7, "full": 2, "weighted": 6, "keys3": 3, "aggs3": 7, "range": 3, "five": 3,
          "nullable_key": 3, "nullable_key_signed": 4, "wide": 3, "skip_s": 3}


def cells_of(q, layout=None):
    """Group cells of a query: the product of the declared key ranges, one more digit (MISSING) for a column with missing rows."""
    n = 1
    for g in q["groups"]:
        lo, hi = KEYS[g]
        n *= hi - lo + 1 + (1 if layout is not None and g in layout.pop else 0)
    return n


class Layout:
    def __init__(self, name, blocks, t, seed, t_bounds=None, t_pop=None, kn_pop=None, s=None):
        self.name, self.blocks = name, [int(b) for b in blocks]
        self.n = int(t.size)
        assert sum(self.blocks) == self.n and t.dtype == np.int64
        self.cols = columns_for(self.n, seed)
        self.cols["t"] = t
        if s is not None:
            self.cols["s"] = s
        self.pop = {}
        if t_pop is not None:
            self.pop["t"] = t_pop.astype(np.uint8)
        if kn_pop is not None:
            self.pop["kn"] = kn_pop.astype(np.uint8)
        lo = int(t[self.pop["t"] != 0].min()) if "t" in self.pop else int(t.min())
        lo -= lo % TB
        self.t_bounds = t_bounds if t_bounds is not None else (lo, lo + N_DECL * TB - 1)
        self.block_rows = self.blocks[0]        # the oracle's block size (its blocks are equal but for the last)
        assert all(b == self.block_rows for b in self.blocks[:-1]) and self.blocks[-1] <= self.block_rows

    def declared(self, col):
        return self.t_bounds if col == "t" else KEYS.get(col) or INFO.get(col) or OTHER[col]


def columns_for(n, seed):
    rng = np.random.default_rng(seed)
    r = lambda lo, hi: rng.integers(lo, hi + 1, n, dtype=np.int64)
    c = {}
    for name in ("f1", "f2", "f3", "f4", "f5"):
        c[name] = r(*OTHER[name])
    c["s"] = r(1, 9)
    for name in KEYS:
        c[name] = r(*KEYS[name])
    c["k2"] = K2_VALUES[rng.integers(0, K2_VALUES.size, n)]
    c["a1"], c["a2"], c["a4"] = r(1, 200), r(1, 40_000), r(1, 1_000_000)
    sg = r(-20_000, 29_999)
    c["sg"] = np.where(sg >= 0, sg + 1, sg)
    c["w"] = r(1, 5)
    # the declared extrema occur (first and last row): stored widths and bases are the same in every table
    for name in c:
        lo, hi = KEYS.get(name) or INFO.get(name) or OTHER[name]
        if n >= 2 and name != "s":
            c[name][0], c[name][n - 1] = (lo if lo != 0 or name not in INFO else 1), hi
    return c


# ---------------------------------------------------------------------------------------------- deal_tiles and window, restated
def block_starts(block_rows):
    """Physical first row of every block: each begins at the next multiple of 32."""
    out, p = [], 0
    for b in block_rows:
        s = (p + 31) // 32 * 32
        out.append(s)
        p = s + b
    return out


def shares(block_rows, n_wg, scanned=None):
    """[[(first physical row, rows), ...] per workgroup]: Planner::work's runs dealt by deal_tiles."""
    starts = block_starts(block_rows)
    runs = []
    for b, n in enumerate(block_rows):
        if n == 0 or (scanned is not None and not scanned[b]):
            continue
        if runs and runs[-1][0] + runs[-1][1] == starts[b]:
            runs[-1][1] += n
        else:
            runs.append([starts[b], n])
    tiles = lambda n: (n + UNIT - 1) // UNIT
    total = sum(tiles(n) for _, n in runs)
    out, ri, used = [], 0, 0
    for w in range(n_wg):
        want = total * (w + 1) // n_wg - total * w // n_wg
        mine = []
        while want > 0 and ri < len(runs):
            r0, rn = runs[ri]
            take = min(want, tiles(rn) - used)
            start = r0 + used * UNIT
            mine.append((start, min(r0 + rn, start + take * UNIT) - start))
            used += take
            want -= take
            if used == tiles(rn):
                ri, used = ri + 1, 0
        out.append(mine)
    return out


def block_extrema(block_rows, values, pop=None):
    """(min, max, populated rows) of every block, as the table keeps them."""
    mn, mx, cnt, r0 = [], [], [], 0
    for b in block_rows:
        v = values[r0:r0 + b]
        if pop is not None:
            v = v[pop[r0:r0 + b] != 0]
        cnt.append(int(v.size))
        mn.append(int(v.min()) if v.size else 0)
        mx.append(int(v.max()) if v.size else 0)
        r0 += b
    return mn, mx, cnt


def windows(block_rows, n_wg, blk_min, blk_max, blk_pop, time_bucket, t_bounds, scanned=None):
    """Planner::window: ([(first bucket, last bucket) or None per workgroup], wmax, inside) -- buckets as trunc(t / bucket);
    None: no segment, or no populated block under one (base 0); inside: no window leaves the declared bounds."""
    starts = block_starts(block_rows)
    tb_min, tb_max = trunc_div(t_bounds[0], time_bucket), trunc_div(t_bounds[1], time_bucket)
    out, wmax, inside = [], 1, True
    for segs in shares(block_rows, n_wg, scanned):
        lo = hi = None
        for s0, sn in segs:
            for b, n in enumerate(block_rows):
                if starts[b] + n > s0 and starts[b] < s0 + sn and blk_pop[b] > 0:
                    lo = blk_min[b] if lo is None else min(lo, blk_min[b])
                    hi = blk_max[b] if hi is None else max(hi, blk_max[b])
        if lo is None:
            out.append(None)
            continue
        first, last = trunc_div(lo, time_bucket), trunc_div(hi, time_bucket)
        if first < tb_min or last > tb_max:
            inside = False
        out.append((first, last))
        wmax = max(wmax, last - first + 1)
    return out, wmax, inside


def layout_windows(layout, n_wg, scanned=None):
    mn, mx, cnt = block_extrema(layout.blocks, layout.cols["t"], layout.pop.get("t"))
    return windows(layout.blocks, n_wg, mn, mx, cnt, TB, layout.t_bounds, scanned)


def window_bytes(wmax, cells, fields):
    return wmax * cells * fields * 8


def fit(cells, fields):
    """The widest window the budget holds."""
    return LDS_BUDGET // (cells * fields * 8)


# ---------------------------------------------------------------------------------------------- cases
def _spread(lo, hi, n):
    """n sorted times from lo to hi inclusive, both present."""
    if n == 1:
        return np.array([lo], dtype=np.int64)
    return lo + np.arange(n, dtype=np.int64) * (hi - lo) // (n - 1)


def _check_n_wg(n_wg):
    assert 16 <= n_wg <= 512, "n_workgroups = %d: sized for one workgroup per CU of a 16..512-CU device" % n_wg


def spike(n_wg, W=3, name="spike"):
    _check_n_wg(n_wg)
    assert 2 <= W <= 64
    s = n_wg // 2
    k = T0 // TB + (s - 1) // 2 + 1              # the spike's first row closes bucket k - 1, where share s - 1 lies
    last = k + W - 2
    half = TB // 2
    parts = []
    for g in range(n_wg):
        if g < s:
            b = T0 // TB + g // 2
            first_half = g % 2 == 0
        elif g > s:
            b = last + (g - s) // 2
            first_half = (g - s) % 2 == 0
        if g == s:
            t = np.empty(SHARE, dtype=np.int64)
            t[0], t[1], t[2] = k * TB - 1, k * TB, k * TB + 1
            mid = [(k + j) * TB for j in range(1, W - 2)]          # one row in each bucket between
            t[3:3 + len(mid)] = mid
            rest = SHARE - 3 - len(mid)
            t[3 + len(mid):] = _spread(last * TB if W > 2 else k * TB + 2, last * TB + half - 1, rest)
            parts.append(t)
        elif g == s - 1 and s % 2 == 1:
            parts.append(_spread(b * TB, b * TB + TB - 2, SHARE))       # a pair's first half alone: up to the spike's first row
        else:
            parts.append(_spread(b * TB, b * TB + half - 1, SHARE) if first_half else _spread(b * TB + half, b * TB + TB - 1, SHARE))
    t = np.concatenate(parts)
    return Layout(name, [SHARE] * n_wg, t, seed=11)


def budget(n_wg, W):
    return spike(n_wg, W, name="budget%d" % W)


def straddle(n_wg):
    _check_n_wg(n_wg)
    n = n_wg * SHARE + 777
    i = np.arange(n, dtype=np.int64)
    t = T0 + (i // SHARE) * TB + (i % SHARE) * TB // SHARE
    blocks = [12288] * (n // 12288) + ([n % 12288] if n % 12288 else [])
    return Layout("straddle", blocks, t, seed=12)


def small_blocks(n_wg):
    _check_n_wg(n_wg)
    nb = 8 * n_wg + 3
    i = np.arange(nb * 1000, dtype=np.int64)
    t = T0 + (i // 8000) * TB + (i % 8000) * TB // 8000
    return Layout("small_blocks", [1000] * nb, t, seed=13)


def idle(n_wg):
    _check_n_wg(n_wg)
    n = 5 * UNIT + 7
    i = np.arange(n, dtype=np.int64)
    t = T0 + (i // 1024) * TB + (i % 1024) * TB // 1024
    return Layout("idle", [UNIT] * 5 + [7], t, seed=14)


def nullable(n_wg):
    _check_n_wg(n_wg)
    n = n_wg * SHARE
    rng = np.random.default_rng(150)
    i = np.arange(n, dtype=np.int64)
    t = T0 + (i // SHARE) * TB + (i % SHARE) * TB // SHARE
    t_pop = rng.random(n) >= 0.1
    a, b = n_wg // 3, 2 * n_wg // 3
    t_pop[a * SHARE + UNIT:a * SHARE + 2 * UNIT] = False          # the second of share a's four blocks
    t_pop[b * SHARE:(b + 1) * SHARE] = False                       # every block of share b
    t_pop[0] = t_pop[n - 1] = True
    t = np.where(t_pop, t, 0)                                      # what a row without a value stores is nobody's business
    kn_pop = rng.random(n) >= 0.15
    return Layout("nullable", [UNIT] * (n // UNIT), t, seed=15, t_pop=t_pop, kn_pop=kn_pop)


SIGNED_PLACED = (-TB - 1, -TB, -TB + 1, -1, 0, 1)


def signed(n_wg):
    _check_n_wg(n_wg)
    n = n_wg * SHARE
    t = _spread(-3 * TB - 1, 3 * TB + 1, n)
    return Layout("signed", [SHARE] * n_wg, t, seed=16, t_bounds=(-(N_DECL // 2) * TB, (N_DECL // 2) * TB - 1))


def skips(n_wg):
    _check_n_wg(n_wg)
    n = n_wg * SHARE
    nb = n // TILE
    i = np.arange(n, dtype=np.int64)
    t = T0 + (i // SHARE) * TB + (i % SHARE) * TB // SHARE
    s = 1 + i % 9
    s[i % 4 == 3] = 0
    blk = i // TILE
    s[(blk >= nb // 4) & (blk < nb // 2) & (blk % 2 == 1)] = 0
    return Layout("skips", [TILE] * nb, t, seed=17, s=s)


def skips_scanned(layout, filters):
    """[bool per block]: what block_skip keeps under gt / lt / eq filters (planner.cpp: should_scan_block)."""
    keep = [True] * len(layout.blocks)
    for col, op, v in filters:
        mn, mx, cnt = block_extrema(layout.blocks, layout.cols[col], layout.pop.get(col))
        for b in range(len(keep)):
            if cnt[b] == 0 or (op == "gt" and not mx[b] > v) or (op == "lt" and not mn[b] < v) or (op == "eq" and (mn[b] > v or mx[b] < v)):
                keep[b] = False
    return keep


def wide_declared(n_tb):
    n = 3 * UNIT + 5
    i = np.arange(n, dtype=np.int64)
    first = T0 // TB + n_tb - 3
    t = (first + i // UNIT).clip(max=first + 2) * TB + (i % UNIT) * TB // UNIT
    t[n - 1] = (first + 3) * TB - 1                               # the last second of the declared range
    t.sort()
    return Layout("wide%d" % n_tb, [UNIT] * 3 + [5], t, seed=18, t_bounds=(T0, T0 + n_tb * TB - 1))


# ---------------------------------------------------------------------------------------------- the reference
_OPS = {"gt": np.greater, "lt": np.less, "eq": np.equal, "neq": np.not_equal}


def keep(layout, filters):
    """bool[n]: the rows that pass every filter; a row without a value in a filter column fails (filter.go:171)."""
    m = np.ones(layout.n, dtype=bool)
    for col, op, val in filters:
        m &= _OPS[op](layout.cols[col], val)
        if col in layout.pop:
            m &= layout.pop[col] != 0
    return m


def time_buckets(t, bucket):
    """trunc(t / bucket) * bucket over an int64 array (aggregate.go:174: Go's division truncates)."""
    q = np.abs(t) // bucket
    return np.where(t < 0, -q, q) * bucket


def reference(layout, q, bucket_size=None):
    """The exact answer to query kwargs q over the whole columns of `layout`:
    {"matched": rows passing the filters (rows without a time value count, then drop out: aggregate.go:147-153),
     "groups": {(time bucket, key...): (count, samples, ((sum, min, max, buckets or None) per aggregation))}}.
    A key is MISSING where its column has no value.  A weight multiplies count and sum; samples counts rows.  op="hist":
    buckets[(v - Info.Min) // BucketSize] per aggregation, with bucket_size = [BucketSize per aggregation] from the oracle's
    result.  int64 throughout, shown not to wrap."""
    cols = layout.cols
    m = keep(layout, q.get("filters", ()))
    out = {"matched": int(m.sum()), "groups": {}}
    if "t" in layout.pop:
        m = m & (layout.pop["t"] != 0)
    idx = np.flatnonzero(m)
    if idx.size == 0:
        return out
    tbv = time_buckets(cols[q["time_col"]][idx], q["time_bucket"])
    assert all(trunc_div(int(a), q["time_bucket"]) * q["time_bucket"] == int(b) for a, b in zip(cols[q["time_col"]][idx][:64], tbv[:64]))
    parts = [tbv]
    for g in q.get("groups", ()):
        v = cols[g][idx]
        if g in layout.pop:
            v = np.where(layout.pop[g][idx] != 0, v, MISSING)
        parts.append(v)
    order = np.lexsort(tuple(reversed(parts)))
    parts = [p[order] for p in parts]
    new = np.zeros(idx.size, dtype=bool)
    new[0] = True
    for p in parts:
        new[1:] |= p[1:] != p[:-1]
    starts = np.flatnonzero(new)
    w = cols[q["weight_col"]][idx][order] if q.get("weight_col") else np.ones(idx.size, dtype=np.int64)
    counts = np.add.reduceat(w, starts)
    samples = np.diff(np.r_[starts, idx.size])
    per_agg = []
    for a, name in enumerate(q.get("aggs", ())):
        v = cols[name][idx][order]
        assert idx.size * int(w.max()) * max(abs(int(v.min())), abs(int(v.max())), 1) < 1 << 62        # no sum can wrap
        lo, hi = INFO[name]
        assert int(v.min()) >= lo and int(v.max()) <= hi                                             # no value is rejected
        buckets = None
        if q.get("op") == "hist" and q.get("want_percentiles", True):
            bs = bucket_size[a]
            gid = np.cumsum(new) - 1
            bk = (v - lo) // bs
            nv = int(bk.max()) + 1
            assert q.get("weight_col") is None and starts.size * nv < 1 << 26
            buckets = np.bincount(gid * nv + bk, minlength=starts.size * nv).reshape(starts.size, nv)
        per_agg.append((np.add.reduceat(v * w, starts), np.minimum.reduceat(v, starts), np.maximum.reduceat(v, starts), buckets))
    for j, s in enumerate(starts):
        key = tuple(int(p[s]) for p in parts)
        out["groups"][key] = (int(counts[j]), int(samples[j]),
                              tuple((int(sm[j]), int(lo[j]), int(hi[j]), None if bk is None else bk[j]) for sm, lo, hi, bk in per_agg))
    assert sum(g[1] for g in out["groups"].values()) == idx.size
    return out


def appended(layout, t_new, seed):
    """`layout` with one more block of rows at times t_new: (the grown layout, the new block's columns)."""
    assert not layout.pop and t_new.size <= layout.block_rows == layout.blocks[-1]
    extra = columns_for(int(t_new.size), seed)
    extra["t"] = t_new
    g = Layout.__new__(Layout)
    g.__dict__.update(layout.__dict__)
    g.cols = {c: np.concatenate([layout.cols[c], extra[c]]) for c in layout.cols}
    g.blocks = layout.blocks + [int(t_new.size)]
    g.n = layout.n + int(t_new.size)
    return g, extra
