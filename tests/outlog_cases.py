"""Placed tables behind tests/test_gpu_outlier_log.py, and a model of one wave's appends to the outlier log; both are checked
on the CPU by tests/test_outlog_cases.py.

The log (csrc/plan.h, csrc/outlog.h): kOutStripes = 64 staging stripes of per = cap / 64 records, each behind a cursor.  A wave
hashes (workgroup, wave) to its home stripe; the lanes that hold an outlier at the same point of the row body reserve their
places with ONE fetch-add on the cursor; the lanes whose place lies beyond the stripe's share go on to the next stripe, up to
kOutSpill = 8 of them; a lane that found no place in all eight raises the home stripe's `dropped` flag.  k_outlog_gather
(csrc/kernels.hip) clamps the cursors that ran past their share and closes the stripes up.

The tables
* Columns g (GROUPS groups) and v with Info INFO = [0, 60000]; QUERY is `-op hist -hist-bucket 3` with bucket arrays, so a
  value from FIRST_OUTLIER up lies beyond the last bucket (hist_basic.go:34-70, 132-142: NumBuckets stays 1000).  Every row that
  is no outlier holds a value below IN_RANGE; outlier number k of a table (in row order) holds OUTLIER_BASE + k -- every outlier
  value of a table is distinct and inside Info, so a lost, duplicated or misattributed record changes the answer.
* one_wave(n): ONE_WAVE_BLOCKS blocks of ONE_WAVE_BLOCK rows, exactly n outliers, all among the first 64 rows of the first
  block (WAVE_ROWS[:n], a fixed shuffle of 0..63).  Why that is ONE wave: the first block starts the table's only run of rows,
  deal_tiles (planner.cpp) cuts runs into segments at multiples of kTileRows = 2048 rows from the run's start, and every scan
  kernel maps a segment's rows to lanes in order --
      k_scan            kernels.hip     `row = seg.start + tid * kRowsPerThread`        (2 rows per lane)
      k_scan_hash       hashgroup.hip   `row = seg.start + tid * kRowsPerThread`
      k_scan_fast       scan_fast.h     `row = seg.start + tid * kRowsPerThread`
      k_scan_hash_fast  hashfast.hip    `row = seg.start + tid * kRowsPerThread`
      k_scan_packed     scan_packed.h   `r = tid * kPackedRows` from `first = seg.start + c0` (4 rows per lane)
  -- so rows 0..63 belong to lanes 0..31 (0..15 packed) of wave 0 of the workgroup that owns the first segment, whichever
  that is, and `home` (outlog.h: a hash of blockIdx.x and threadIdx.x >> 6) is the same at every call.
* time_wave(n): one_wave(n) with a time column -- the outlier rows alternate between two time buckets and two groups.
* many_waves(): MANY_ROWS rows in MANY_BLOCK-row blocks, MANY_SHARE of them outliers, spread over all blocks and groups.

The model
* one_wave_outcome(n, per): what the issue's prose says -- stripes home .. home + 7, each filled to exactly `per` before the
  next is tried, a drop once all eight are full.  (placed, dropped).
* replay(calls, per): log_outlier and k_outlog_gather word for word, for the calls of one wave: cursors that run past `per`,
  the flag, the clamp, the header word.  calls_of(rows, rows_per_lane) gives the sizes of a wave's calls under a kernel's row
  mapping (the lanes that hold an outlier in their j-th row meet in one call), on the assumption that the compiler keeps them
  converged there; the OUTCOME does not depend on it (test_outlog_cases: every split of the lanes gives the same answer).
With cap = 64 * per and nobody else logging, the n outliers of one wave are all kept iff n <= 8 * per.
"""
import numpy as np

STRIPES = 64              # kOutStripes (plan.h)
SPILL = 8                 # kOutSpill (outlog.h)
DEFAULT_CAP = 1 << 20     # kOutLogDefaultCap (plan.h)

GROUPS = 5
INFO = (0, 60_000)
BUCKET = 3
QUERY = dict(groups=["g"], aggs=["v"], op="hist", hist_bucket=BUCKET, want_percentiles=True)
FIRST_OUTLIER = 3006      # len(Values) = 1002 buckets of 3 from Info.Min = 0 (checked through the oracle)
IN_RANGE = 3000           # every other value lies in [0, IN_RANGE)
OUTLIER_BASE = 50_000

ONE_WAVE_BLOCK, ONE_WAVE_BLOCKS = 4096, 3
WAVE_ROWS = tuple(int(x) for x in np.random.default_rng(20_251).permutation(64))
MANY_ROWS, MANY_BLOCK, MANY_SHARE = 200_000, 40_000, 0.02
T0, TB = 1_700_000_000 - 1_700_000_000 % 3600, 3600


def wave_ns(per):
    """The outlier counts the one-wave tests use at stripes of `per`: the home stripe alone, the first spill, the exact fit of
    all eight stripes, the first record without a place."""
    return (per, per + 1, SPILL * per, SPILL * per + 1)


def rounded_cap(cap):
    """SYBL_OUTLIER_LOG_CAP as the planner takes it (planner.cpp: `max(1, cap)`, then `(cap + 63) / 64 * 64` -- equal stripes)."""
    return (max(1, int(cap)) + STRIPES - 1) // STRIPES * STRIPES


def per_of(cap):
    return rounded_cap(cap) // STRIPES


class Case:
    def __init__(self, name, block, cols, outlier_rows):
        self.name, self.block, self.cols = name, block, cols
        self.n = int(cols["v"].size)
        self.outlier_rows = np.asarray(outlier_rows, dtype=np.int64)
        self.n_outliers = int(self.outlier_rows.size)
        self.blocks = [min(block, self.n - r0) for r0 in range(0, self.n, block)]


def _fill(n, outlier_rows, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, GROUPS, n, dtype=np.int64)
    v = rng.integers(0, IN_RANGE, n, dtype=np.int64)
    rows = np.sort(np.asarray(outlier_rows, dtype=np.int64))
    v[rows] = OUTLIER_BASE + np.arange(rows.size, dtype=np.int64)
    return {"g": g, "v": v}, rows


def one_wave(n_outliers):
    assert 0 <= n_outliers <= 64
    n = ONE_WAVE_BLOCK * ONE_WAVE_BLOCKS
    cols, rows = _fill(n, WAVE_ROWS[:n_outliers], seed=100 + n_outliers)
    cols["g"][:64] = np.arange(64) % GROUPS          # the outliers of a wave go to every group
    return Case("wave%d" % n_outliers, ONE_WAVE_BLOCK, cols, rows)


def time_wave(n_outliers):
    c = one_wave(n_outliers)
    rng = np.random.default_rng(7)
    r = np.arange(64)
    c.cols["g"][:64] = (r // 2) % 2 * 2 + 1          # groups 1 and 3 ...
    c.cols["t"] = T0 + rng.integers(0, 2 * TB, c.n, dtype=np.int64)
    c.cols["t"][:64] = T0 + (r % 2) * TB + r         # ... in both time buckets
    c.name = "time%d" % n_outliers
    return c


def many_waves():
    rng = np.random.default_rng(4242)
    rows = np.flatnonzero(rng.random(MANY_ROWS) < MANY_SHARE)
    cols, rows = _fill(MANY_ROWS, rows, seed=4243)
    return Case("many", MANY_BLOCK, cols, rows)


def oracle_result(orc, case, time=False):
    """QUERY over the case's columns through the CPU oracle (time: as a time series over `t`)."""
    names = ["g", "v"] + (["t"] if time else [])
    cols = [{"type": "int", "data": case.cols[c]} for c in names]
    kw = dict(groups=[0], aggs=[(1,) + INFO], op="hist", hist_bucket=BUCKET, block_rows=case.block, n_threads=2)
    if time:
        kw.update(time_col=2, time_bucket=TB)
    return orc.run_query(cols, **kw)


def claimed_outliers(case, time=False):
    """{(time bucket or 0, group): ascending outlier values} from the arrays alone."""
    out = {}
    for r in case.outlier_rows.tolist():
        tb = int(case.cols["t"][r]) // TB * TB if time else 0
        out.setdefault((tb, int(case.cols["g"][r])), []).append(int(case.cols["v"][r]))
    return {k: sorted(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------- the model
def one_wave_outcome(n_outliers, per, home=0):
    """(placed, dropped) of one wave's n outliers against stripes of `per` records, nobody else logging."""
    fill = [0] * STRIPES
    placed = dropped = 0
    for _ in range(n_outliers):
        for t in range(SPILL):
            s = (home + t) % STRIPES
            if fill[s] < per:
                fill[s] += 1
                placed += 1
                break
        else:
            dropped += 1
    return placed, dropped


def calls_of(rows, rows_per_lane):
    """Sizes of the calls of log_outlier a wave makes for outliers in `rows` (< 64) when a lane owns rows_per_lane consecutive
    rows and the row body takes a lane's rows one after the other."""
    rows = [int(r) for r in rows]
    assert all(0 <= r < 64 for r in rows)
    return [k for k in (sum(1 for r in rows if r % rows_per_lane == j) for j in range(rows_per_lane)) if k]


def replay(calls, per, home=0):
    """log_outlier (outlog.h) for the calls of ONE wave, each by `calls[i]` lanes together, then k_outlog_gather (kernels.hip).
    Returns a dict: cursors, flag, placed, straddles (reservations of which a part fitted), overrun (stripes whose cursor
    stands beyond `per`), kept (the gather's clamped sum), unclamped (the sum without the clamp), header (kHdrOutLog)."""
    cursor = [0] * STRIPES
    flag = placed = straddles = 0
    for lanes in calls:
        if flag:                                         # `if (load(dropped) != 0) return`
            continue
        pending = lanes
        for t in range(SPILL):
            s = (home + t) % STRIPES
            if cursor[s] >= per:                         # `if (load(cursor) >= per) continue`
                continue
            b = cursor[s]
            cursor[s] += pending                         # one fetch-add for the lanes still looking
            fit = min(pending, per - b)                  # ranks with b + rank < per
            straddles += 1 if fit < pending else 0
            placed += fit
            pending -= fit
            if not pending:
                break
        if pending:
            flag = 1
    kept = sum(min(c, per) for c in cursor)
    cap = per * STRIPES
    return dict(cursor=cursor, flag=flag, placed=placed, straddles=straddles, overrun=sum(1 for c in cursor if c > per),
                kept=kept, unclamped=sum(cursor), header=cap + 1 if flag else kept)
