"""Placed tables behind tests/test_gpu_late_path.py, and their exact references; checked on the CPU by tests/test_late_layout.py.

The LATE kernels (k_scan_hash_packed<.., LATE>, k_count_packed / k_emit_packed<.., LATE>, k_scan_packed's late loop) read the
filter columns one tile ahead and request the key, value and time columns of a tile only when some row of the wave's window
passed.  The geometry is the code's: a packed tile is kWgThreads x kPackedRows = 4096 rows (plan.h, scan_packed.h), a wave's
window 64 lanes x 4 rows = 256 consecutive rows of it, deal_tiles (planner.cpp) hands out units of kTileRows = 2048 rows, and
the kernels launch one workgroup per CU.

* main(n_wg): n_wg x 16384 rows in 65536-row blocks -- every workgroup's share is four packed tiles of one block, as long as
  n % (n_wg x 2048) == 0 (asserted; the only thing restated of deal_tiles).  Window `it` of wave w of workgroup g holds a passing
  row iff bit `it` of (w + g) mod 16 is set: the sixteen waves of every workgroup run the sixteen pass / skip sequences of four
  tiles, and the assignment rotates from workgroup to workgroup.  Inside a passing window the passing rows are one of five
  position classes (CLASSES), cycling with w + it + g.
* ragged(n_wg): unequal blocks (RAGGED_BLOCKS, repeated until there are 2 x n_wg units); the first and the last two rows of a
  block pass, every other row with probability 0.002.  Claims partial tiles, partial windows and tiles past n in the
  look-ahead -- nothing about which wave sees what.
* tiny(rows): one block, exactly the last row passes.

Every table has the same columns (columns_for): filter columns f1 / f2 / f4 that each carry the pattern alone (FILTERS: stored
at 1, 2 and 4 bytes once compact) and as the conjunction of two thresholds neither of which empties a window; group columns
ga, gb, gx (1 byte), gc (2 bytes), gh (2 bytes, high cardinality: strategy 5); aggregation columns a1 (1 byte), a2 (2 bytes,
both signs), a2b (2 bytes), a4 (4 bytes) inside their declared bounds and never 0; a sorted time column.  A row that fails
carries keys inside every key range and non-zero values -- accumulated by mistake it changes a count and a sum -- and in gx a
key outside the declared range (DECLARED): through a query that groups by gx a leaked row is an overflow, which fails the query.

reference(): count, sum, min, max per group as a numpy int64 group-by over the whole columns.
"""
import numpy as np

WINDOW = 256            # rows of a wave's window: 64 lanes x kPackedRows
LANE_ROWS = 4           # kPackedRows
TILE = 4096             # kWgThreads x kPackedRows
UNIT = 2048             # kTileRows: what deal_tiles counts
SHARE = 4 * TILE        # rows of one workgroup in `main`
BLOCK = 65536
WAVES = TILE // WINDOW  # 16
CLASSES = ("row0", "row255", "k3", "two_lanes", "all")
# the rows of a window that pass, per class (None: all 256): k3 is row 3 of lane 37, two_lanes row 1 of lane 5 and row 2 of lane 60
POSITIONS = {"row0": (0,), "row255": (255,), "k3": (4 * 37 + 3,), "two_lanes": (4 * 5 + 1, 4 * 60 + 2), "all": None}
RAGGED_BLOCKS = (65536, 3 * 4096 + 5, 1, 2048 + 255, 40961, 4095, 4097)
TINY_ROWS = (1, 255, 257, 4097)
RAGGED_P = 0.002

T0, TB, N_TB = 1_700_000_000 - 1_700_000_000 % 3600, 3600, 4
# declared key ranges (sybl_table_set_bounds) and aggregation bounds (IntInfo): the data of passing rows lies inside all of them
DECLARED = {"ga": (0, 3), "gb": (0, 1), "gc": (0, 259), "gx": (0, 1), "gh": (0, 2499)}
GX_LEAK = 200           # gx of every failing row: outside DECLARED["gx"], inside one stored byte
# (ranges of 200, 50 000, 40 000 and 1 000 000: span / BucketSize stays below the bucket count, hist_basic.go:34-70 -- no outliers)
INFO = {"a1": (0, 200), "a2": (-20_000, 30_000), "a2b": (0, 40_000), "a4": (0, 1_000_000)}
STORED_BYTES = {"f1": 1, "f2": 2, "f4": 4, "ga": 1, "gb": 1, "gx": 1, "gc": 2, "gh": 2, "a1": 1, "a2": 2, "a2b": 2, "a4": 4}
# the pattern through one column of each width, and as a conjunction: a failing row passes f1 > 99 or f2 > 29999, never both
FILTERS = {
    "f1": [("f1", "gt", 199)],
    "f2": [("f2", "gt", 59_999)],
    "f4": [("f4", "gt", 2_999_999)],
    "and": [("f1", "gt", 99), ("f2", "gt", 29_999)],
}
ALL3 = [("f1", "gt", 199), ("f2", "gt", 59_999), ("f4", "gt", 2_999_999)]   # config 3's three filters, each the pattern
# ... and three whose stored offsets fit one 32-bit filter word and are worth one (8 + 9 + 12 bits of 1 + 2 + 2 stored bytes;
# f2's 16 and f4's 22 bits leave no room for a third column): the second and third pass every row
WORD3 = [("f1", "gt", 199), ("gc", "gt", -1), ("gh", "gt", -1)]
NOTHING = [("f1", "gt", 1000)]          # beyond every stored value of the column: plo > phi
EVERYTHING = [("f1", "gt", -1)]
COLUMN_ORDER = ("f1", "f2", "f4", "ga", "gb", "gc", "gx", "gh", "a1", "a2", "a2b", "a4", "t")


class Layout:
    def __init__(self, name, blocks, passing, seed):
        self.name, self.blocks, self.passing = name, list(blocks), passing
        self.n = int(passing.size)
        assert sum(self.blocks) == self.n
        self.cols = columns_for(passing, seed)


def main_geometry(n_wg):
    """(g, it, w, p) of every row of main(n_wg): workgroup, tile of its share, wave, row of the wave's window."""
    n = n_wg * SHARE
    i = np.arange(n, dtype=np.int64)
    return i // SHARE, (i % SHARE) // TILE, (i % TILE) // WINDOW, i % WINDOW


def main_passing(n_wg):
    # the guard the other sized files use, and what makes a share four whole tiles of one block
    assert 16 <= n_wg <= 512, "n_workgroups = %d: sized for one workgroup per CU of a 16..512-CU device" % n_wg
    n = n_wg * SHARE
    assert n % (n_wg * UNIT) == 0 and SHARE % TILE == 0 and BLOCK % SHARE == 0
    g, it, w, p = main_geometry(n_wg)
    needed = (((w + g) % WAVES) >> it) & 1 == 1
    ok = np.zeros((len(CLASSES), WINDOW), dtype=bool)
    for c, name in enumerate(CLASSES):
        if POSITIONS[name] is None:
            ok[c, :] = True
        else:
            ok[c, list(POSITIONS[name])] = True
    return needed & ok[(w + it + g) % len(CLASSES), p]


def main_blocks(n_wg):
    n = n_wg * SHARE
    return [min(BLOCK, n - r0) for r0 in range(0, n, BLOCK)]


def main(n_wg):
    return Layout("main", main_blocks(n_wg), main_passing(n_wg), seed=1)


def ragged_blocks(n_wg):
    blocks, units = [], 0
    while units < 2 * n_wg:
        for b in RAGGED_BLOCKS:
            blocks.append(b)
            units += (b + UNIT - 1) // UNIT
    return blocks


def ragged(n_wg):
    blocks = ragged_blocks(n_wg)
    n = sum(blocks)
    rng = np.random.default_rng(77)
    passing = rng.random(n) < RAGGED_P
    r0 = 0
    for b in blocks:
        passing[r0] = True
        passing[max(r0, r0 + b - 2):r0 + b] = True
        r0 += b
    return Layout("ragged", blocks, passing, seed=2)


def tiny(rows):
    passing = np.zeros(rows, dtype=bool)
    passing[-1] = True
    return Layout("tiny%d" % rows, [rows], passing, seed=3 + rows)


def columns_for(passing, seed):
    """{name: int64[n]} of every column, from the pass mask alone."""
    rng = np.random.default_rng(seed)
    n = passing.size
    i = np.arange(n, dtype=np.int64)
    even = i % 2 == 0
    r = lambda lo, hi: rng.integers(lo, hi, n, dtype=np.int64)     # [lo, hi)
    c = {}
    c["f1"] = np.where(passing, 200 + r(0, 50), np.where(even, 100 + r(0, 100), r(0, 100)))
    c["f2"] = np.where(passing, 60_000 + r(0, 1000), np.where(even, r(0, 30_000), 30_000 + r(0, 30_000)))
    c["f4"] = np.where(passing, 3_000_000 + r(0, 100_000), r(0, 3_000_000))
    c["ga"], c["gb"], c["gc"], c["gh"] = r(0, 4), r(0, 2), r(0, 260), r(0, 2500)
    c["gx"] = np.where(passing, r(0, 2), GX_LEAK)
    c["a1"] = r(1, 201)
    a2 = r(-20_000, 30_000)
    c["a2"] = np.where(a2 >= 0, a2 + 1, a2)
    c["a2b"] = r(1, 40_001)
    c["a4"] = r(1, 1_000_001)
    c["t"] = T0 + i * (N_TB * TB) // n
    return c


_OPS = {"gt": np.greater, "lt": np.less, "eq": np.equal, "neq": np.not_equal}


def keep(cols, filters):
    """bool[n]: the rows that pass every filter (all of them without one)."""
    n = next(iter(cols.values())).size
    m = np.ones(n, dtype=bool)
    for col, op, val in filters:
        m &= _OPS[op](cols[col], val)
    return m


def reference(cols, q, declared=DECLARED):
    """The exact answer to query kwargs q (filters, groups, aggs, time_col / time_bucket) over cols:
    {"matched": rows passing the filters, "overflow": those of them with a group key outside its declared range (the engine
    fails such a query and says how many), "groups": {key: (count, ((sum, min, max) per aggregation))}} over the others, key =
    the group columns' values, in time mode preceded by the time bucket (t // bucket * bucket).  int64 throughout, shown not to
    wrap."""
    m = keep(cols, q.get("filters", ()))
    matched = int(m.sum())
    inb = m.copy()
    for gcol in q.get("groups", ()):
        lo, hi = declared[gcol]
        inb &= (cols[gcol] >= lo) & (cols[gcol] <= hi)
    idx = np.flatnonzero(inb)
    out = {"matched": matched, "overflow": matched - int(idx.size), "groups": {}}
    if idx.size == 0:
        return out
    digits = []          # (values, cardinality, back to a key part)
    if q.get("time_col"):
        tb = cols[q["time_col"]][idx] // q["time_bucket"]
        t_lo = int(tb.min())
        digits.append((tb - t_lo, int(tb.max()) - t_lo + 1, lambda d, t_lo=t_lo: (d + t_lo) * q["time_bucket"]))
    for gcol in q.get("groups", ()):
        lo, hi = declared[gcol]
        digits.append((cols[gcol][idx] - lo, hi - lo + 1, lambda d, lo=lo: d + lo))
    comp = np.zeros(idx.size, dtype=np.int64)
    space = 1
    for vals, card, _ in digits:
        comp = comp * card + vals
        space *= card
    assert space < 1 << 62
    order = np.argsort(comp, kind="stable")
    cs = comp[order]
    starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    counts = np.diff(np.r_[starts, cs.size])
    per_agg = []
    for a in q.get("aggs", ()):
        v = cols[a][idx][order]
        assert int(counts.max()) * max(abs(int(v.min())), abs(int(v.max())), 1) < 1 << 63    # no per-group sum can wrap
        per_agg.append((np.add.reduceat(v, starts), np.minimum.reduceat(v, starts), np.maximum.reduceat(v, starts)))
    for j, s in enumerate(starts):
        rest, key = int(cs[s]), []
        for _, card, back in reversed(digits):
            rest, d = divmod(rest, card)
            key.append(int(back(d)))
        out["groups"][tuple(reversed(key))] = (int(counts[j]), tuple((int(sm[j]), int(lo[j]), int(hi[j])) for sm, lo, hi in per_agg))
    assert sum(c for c, _ in out["groups"].values()) == idx.size
    return out
