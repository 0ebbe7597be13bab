"""Inputs for the device histogram summaries (k_hist_summary / k_hist_total / k_hist_gather in sybil_amd/csrc/kernels.hip)
and a plain Python big-integer reference of BasicHist, shared by tests/test_oracle_hist_summary.py (oracle vs this
reference, CPU) and tests/test_gpu_hist_summary.py (engine vs oracle and vs this reference).  No GPU code, no oracle code.

A case is a dict: name, cols {name: int64 array}, pop {agg column: uint8 array} (optional: 0 = the row leaves the column
unpopulated), info {agg column: (Info.Min, Info.Max)}, block_rows, q (sybil_amd query kwargs).  reference(case) returns
{"matched", "groups": {key tuple: group}, "total": group}; a group holds rows / row_samples and, per aggregation, a dict
restating hist_basic.go:34-70 (SetupBuckets) and :101-219 (AddWeightedValue with its reject gate and the clamping of
outliers and underliers, GetPercentiles, GetStdDev around the exact mean), plus sb / sb2: the bucket moments
sum(b * x) and sum(b^2 * x) mod 2^64 as int64 (Query.debug_cells) next to their true values (sb_true / sb2_true).

Summary-path cases give the group column 2048 or more cells by a row at key 0 and one at a far key; the live groups sit at
the cells of KEYS(far): 0, 1, 3, 4, ..., one in the middle, the last.  FAR (2050) makes 2051 cells: k_hist_summary's last
workgroup of four (cell, aggregation) pairs is partial and so is k_hist_total's last block of 128 cells (3 cells: the
remainder loop only); FAR_TOTAL (2188) makes 2189 = 17 * 128 + 13, a last block with one unrolled-by-8 step and 5 left.

An underlier cannot be made through a query: h.Min starts at Info.Min (hist_basic.go:39) and the gate (:104) rejects
every value below Info.Min, so `bucket_value < 0` (:139) is dead code there.  The reference restates it all the same."""
import math
from fractions import Fraction

import numpy as np

from tests import int64_edges as E
from tests.int64_edges import M64, i64, trunc_div, wrap64

NUM_BUCKETS = 1000  # config.go
FAR, FAR_TOTAL = 2050, 2188
N_PATTERNS = 13


# ---------------------------------------------------------------- the reference
def setup_buckets(imin, imax, hist_bucket=0):
    """SetupBuckets, hist_basic.go:34-70: (BucketSize, NumBuckets, len(Values))."""
    size = imax - imin
    nb = NUM_BUCKETS
    bs = trunc_div(size, nb)
    if hist_bucket > 0:
        bs = hist_bucket
    if bs == 0:
        if size < 100:
            bs, nb = 1, size
        else:
            bs = trunc_div(size, 100)
            nb = trunc_div(size, bs)
    nb += 1
    return bs, nb, nb + 1


class RefHist:
    """BasicHist in percentile mode on unbounded ints (Avg kept as the exact sum)."""

    def __init__(self, imin, imax, hist_bucket, weight_col):
        self.imin, self.imax, self.wc = imin, imax, weight_col
        self.min, self.max = imin, imax  # :39-40
        self.bs, self.nb, nv = setup_buckets(imin, imax, hist_bucket)
        self.values = [0] * nv
        self.count = self.samples = self.sum = self.pop = 0
        self.true_min = self.true_max = None
        self.outliers, self.underliers = [], []

    def add(self, v, w):
        self.pop += 1
        if v > wrap64(self.imax * 10) or v < self.imin:  # :104, Info.Max*10 wrapping like Go's int64
            return
        if self.wc or w > 1:  # :111-116
            self.samples += 1
            self.count += w
        else:
            self.count += 1
        self.sum += v * w
        self.max = max(self.max, v)
        self.min = min(self.min, v)
        self.true_min = v if self.true_min is None else min(self.true_min, v)
        self.true_max = v if self.true_max is None else max(self.true_max, v)
        b = trunc_div(v - self.min, self.bs)  # :132
        if b >= len(self.values):
            self.outliers.append(v)
            b = len(self.values) - 1
        if b < 0:
            self.underliers.append(v)
            b = 0
        self.values[b] += w  # :147

    def percentiles(self):
        """GetPercentiles, :153-183."""
        if self.count == 0:
            return []
        p = [0] * 101
        p[0] = self.min
        c = prev = 0
        for k, n in enumerate(self.values):
            c += n
            q = trunc_div(100 * c, self.count)
            for ip in range(prev, q + 1):
                p[ip] = k * self.bs + self.min
            p[q] = k
            prev = q
        return p[:100]

    def stddev(self):
        """GetStdDev, :192-219, with h.Avg the exact mean: every bucket at its lower edge, every outlier and underlier once
        more under its own value with ratio 1 / Count."""
        if self.count == 0:
            return None
        mean = Fraction(self.sum, self.count)
        var = sum((Fraction(b * self.bs + self.min) - mean) ** 2 * Fraction(c, self.count) for b, c in enumerate(self.values) if c)
        var += sum((Fraction(o) - mean) ** 2 / self.count for o in self.outliers + self.underliers)
        return math.sqrt(var)

    def result(self):
        sb = sum(b * c for b, c in enumerate(self.values))
        sb2 = sum(b * b * c for b, c in enumerate(self.values))
        return {"present": self.pop > 0, "count": self.count, "samples": self.samples, "sum": self.sum, "sum64": wrap64(self.sum),
                "mean": Fraction(self.sum, self.count) if self.count else None, "min": self.min, "max": self.max,
                "true_min": self.true_min, "true_max": self.true_max, "bucket_size": self.bs, "num_buckets": self.nb,
                "n_values": len(self.values), "values": i64(self.values), "n_outliers": len(self.outliers),
                "n_underliers": len(self.underliers), "outliers": sorted(self.outliers + self.underliers),
                "percentiles": self.percentiles(), "stddev": self.stddev(),
                "sb_true": sb, "sb2_true": sb2, "sb": wrap64(sb), "sb2": wrap64(sb2)}


class _RefGroup:
    def __init__(self, case):
        q = case["q"]
        self.rows = self.row_samples = 0
        self.hists = [RefHist(case["info"][a][0], case["info"][a][1], q.get("hist_bucket", 0), bool(q.get("weight_col"))) for a in q["aggs"]]

    def result(self):
        return {"rows": self.rows, "row_samples": self.row_samples, "hists": [h.result() for h in self.hists]}


def reference(case):
    q, cols, pop = case["q"], case["cols"], case.get("pop", {})
    assert q["op"] == "hist" and not q.get("filters") and not q.get("time_col")
    n = len(next(iter(cols.values())))
    groups, total = {}, _RefGroup(case)
    for i in range(n):
        key = tuple(int(cols[g][i]) & (M64 - 1) for g in q["groups"])
        w = int(cols[q["weight_col"]][i]) if q.get("weight_col") else 1
        if key not in groups:
            groups[key] = _RefGroup(case)
        for g in (groups[key], total):
            g.rows += w
            g.row_samples += 1
            for a, h in zip(q["aggs"], g.hists):
                if a not in pop or pop[a][i]:
                    h.add(int(cols[a][i]), w)
    return {"matched": n, "groups": {k: g.result() for k, g in groups.items()}, "total": total.result()}


# ---------------------------------------------------------------- the patterns of a bucket array
def keys(far):
    """The cells of the N_PATTERNS live groups: 0, 1, 3, 4 and on, one in the middle, the last."""
    return [0, 1, 3, 4, 5, 6, 8, 9, 10, 11, 13, far // 2, far]


def pattern_values(p, imin, imax, hist_bucket=0):
    """The values of pattern p, the group at keys(far)[p], for one column: the same number of rows whatever the geometry, so
    that several aggregation columns line up.  Returns (values, populated)."""
    bs, nb, nv = setup_buckets(imin, imax, hist_bucket)
    top = wrap64(imax * 10)
    at = lambda b: imin + b * bs  # the lower edge of bucket b
    last = nv - 1
    assert at(last) <= top, "the last bucket has to be reachable by an accepted value"
    tail0 = last // 64 * 64  # the chunk of the wave scan that holds the last bucket
    spread = lambda n: [at(i * last // (n - 1)) if nv >= n else at(i % nv) for i in range(n)]  # n rows, distinct buckets while they last
    if p == 0:    # one row in bucket 0 (the anchor at key 0)
        v = [at(0)]
    elif p == 1:  # one row in the last bucket
        v = [at(last)]
    elif p == 2:  # one row each in buckets 63 and 64 -- either side of the first chunk boundary -- or the last bucket there is
        v = [at(min(63, last)), at(min(64, last))]
    elif p == 3:  # Counts of 3, 7 and 200 (patterns 3, 4, 5): 100 * c / Count lands on and just under integers
        v = [at(0), at(last // 2), at(last)]
    elif p == 4:
        v = [at((i * i) % nv) for i in range(7)]
    elif p == 5:
        v = [at((i * 37) % nv) for i in range(200)]
    elif p == 6:  # 101 rows: a bucket adds less than one percent, so some leave p unchanged
        v = spread(101)
    elif p == 7:  # 199 rows
        v = spread(199)
    elif p == 8:  # every value rejected by the gate: the hist is present, Count is 0, no percentiles
        v = [imin - 1, top + 1, imin - 2]
    elif p == 9:  # only unpopulated values: no hist
        return [at(0), at(last)], [0, 0]
    elif p == 10:  # outliers: accepted values past the last bucket (clamped into it), next to values inside
        first_out = at(nv)
        v = [at(0), at(last), at(last) + bs - 1] + ([first_out, min(first_out + 7 * bs + 1, top), top, top] if first_out <= top else [at(1 % nv)] * 4)
    elif p == 11:  # all rows in the tail after the last multiple of 64 (the middle cell)
        v = [at(tail0 + (i * 5) % (nv - tail0)) for i in range(9)]
    elif p == 12:  # 100 rows in 100 distinct buckets (the last cell)
        v = spread(100)
    else:
        raise KeyError(p)
    return v, [1] * len(v)


def _pattern_table(far, infos, hist_bucket=0, weights=False, dense=False):
    """One table: pattern p lives at keys(far)[p] (dense: at p) and fills every column of `infos` by that column's geometry."""
    g, w = [], []
    cols = {a: [] for a in infos}
    pop = {a: [] for a in infos}
    for p, key in enumerate(keys(far)):
        n = None
        for a, (imin, imax) in infos.items():
            v, m = pattern_values(p, imin, imax, hist_bucket)
            assert n in (None, len(v))
            n = len(v)
            cols[a] += v
            pop[a] += m
        g += [p if dense else key] * n
    w = [i % 4 + 1 for i in range(len(g))]
    # interleave the groups (the table's row order is not the groups' order)
    order = np.random.default_rng(len(g)).permutation(len(g))
    out = {"g": i64(g)[order]}
    if weights:
        out["w"] = i64(w)[order]
    for a in infos:
        out[a] = i64(cols[a])[order]
    return out, {a: np.array(pop[a], dtype=np.uint8)[order] for a in infos}


# ---------------------------------------------------------------- G: geometry
# Info ranges by the n_values SetupBuckets makes of them (asserted below); both signs of Info.Min, a bucket size above 1
G_INFO = {2: (7, 7), 3: (4, 5), 63: (-3, 58), 64: (100, 162), 65: (0, 63), 128: (-50, 76), 129: (1, 128), 1002: (-500, 4511)}
G_N_VALUES = tuple(G_INFO)
G_HIST_BUCKETS = (2, 3)  # -hist-bucket: 1002 buckets whatever the range, outliers past Min + 1001 * bucket
G_HB_INFO = {2: (0, 5000), 3: (-40, 9000)}
for _nv, (_lo, _hi) in G_INFO.items():
    assert setup_buckets(_lo, _hi)[2] == _nv, (_nv, setup_buckets(_lo, _hi))
assert setup_buckets(*G_INFO[1002])[0] == 5


def case_g(nv, far=None):
    far = far or (FAR_TOTAL if nv in (129, 1002) else FAR)
    cols, pop = _pattern_table(far, {"v": G_INFO[nv]})
    return {"name": "G-%d" % nv, "cols": cols, "pop": pop, "info": {"v": G_INFO[nv]}, "block_rows": 256, "far": far,
            "q": dict(groups=["g"], aggs=["v"], op="hist")}


def case_g_hist_bucket(hb):
    cols, pop = _pattern_table(FAR, {"v": G_HB_INFO[hb]}, hist_bucket=hb)
    return {"name": "G-hb%d" % hb, "cols": cols, "pop": pop, "info": {"v": G_HB_INFO[hb]}, "block_rows": 256, "far": FAR,
            "q": dict(groups=["g"], aggs=["v"], op="hist", hist_bucket=hb)}


# ---------------------------------------------------------------- M: several aggregations of different geometry
M_AGGS = {2: ["a2", "a1002"], 3: ["a65", "a129", "a2"], 4: ["a1002", "a2", "a65", "a129"]}


def case_m(n_aggs):
    aggs = M_AGGS[n_aggs]
    infos = {a: G_INFO[int(a[1:])] for a in aggs}
    far = FAR_TOTAL if n_aggs == 3 else FAR
    cols, pop = _pattern_table(far, infos)
    return {"name": "M-%d" % n_aggs, "cols": cols, "pop": pop, "info": infos, "block_rows": 300, "far": far,
            "q": dict(groups=["g"], aggs=aggs, op="hist")}


# ---------------------------------------------------------------- E: the int64 edges through the device path
E_SPANS = ((1 << 51) + 1, 1 << 61)


def cases_e():
    out = []
    for span in E_SPANS:
        for bs in E.c_bucket_sizes(span):
            for negative in (False, True):
                c = E.case_c(span, bs, E.c_min(span, negative))
                imin = c["info"]["v"][0]
                # the anchor at the far key (key 0 is one of case_c's groups): one row, at the top of the range
                c["cols"] = {"g": np.concatenate([c["cols"]["g"], i64([FAR])]), "v": np.concatenate([c["cols"]["v"], i64([imin + span])])}
                c["name"] = "E-" + c["name"]
                c["far"] = FAR
                out.append(c)
    return out


# ---------------------------------------------------------------- W: weights
W_INFO = (0, 1000)
assert setup_buckets(*W_INFO) == (1, 1001, 1002)
W_BIG = 1 << 33
# rows of weight 2^33, all at value 1000 (bucket 1000), whose true sum(b^2 * w) = 10^6 * 2^33 * rows lies ...
W_ROWS = (1073, 1500, 2148)
assert 10 ** 6 * W_BIG * W_ROWS[0] < 1 << 63 <= 10 ** 6 * W_BIG * (W_ROWS[0] + 1)  # ... just below 2^63,
assert 1 << 63 < 10 ** 6 * W_BIG * W_ROWS[1] < 1 << 64                             # between 2^63 and 2^64,
assert 10 ** 6 * W_BIG * (W_ROWS[2] - 1) < 1 << 64 < 10 ** 6 * W_BIG * W_ROWS[2]   # just above 2^64;
# a fourth group of the largest Count spread evenly over buckets 0..1000.
# Those three have a true stddev of 0, which is also what a variance gone negative is reported as: two more groups alternate
# between 1000 and 900 (stddev 50), with sum(b^2 * w) = (10^6 + 810 000) / 2 * 2^33 * rows ...
W_SPLIT_ROWS = (1400, 2600)
assert 1 << 63 < 905_000 * W_BIG * W_SPLIT_ROWS[0] < 1 << 64 < 905_000 * W_BIG * W_SPLIT_ROWS[1]  # ... past 2^63 and past 2^64.
# Everywhere Count * (hi - lo) < 2^64: sum and avg are inside the bound of include/sybilgpu.h at `sum`, and so is Cumulative
assert sum(W_ROWS + W_ROWS[2:] + W_SPLIT_ROWS) * W_BIG * (W_INFO[1] - W_INFO[0]) < 1 << 64
# (and inside the bound of the bucket moments, same place: (n_values - 1) * sb - sb^2 / Count < 2^64 for each of the six)
W_KEYS = (0, 1, 3, FAR)
W_SPLIT_KEYS = (4, FAR // 2)


def case_w_patterns(summary):
    """Weights 1-4 on the G patterns (n_values 1002, bucket size 1)."""
    cols, pop = _pattern_table(FAR, {"v": W_INFO}, weights=True, dense=not summary)
    return {"name": "W-patterns-" + ("summary" if summary else "moments"), "cols": cols, "pop": pop, "info": {"v": W_INFO}, "block_rows": 256,
            "far": FAR if summary else None, "q": dict(groups=["g"], aggs=["v"], op="hist", weight_col="w", want_percentiles=summary)}


def case_w_big(summary):
    g, v = [], []
    for k, rows in enumerate(W_ROWS):
        g += [W_KEYS[k] if summary else k] * rows
        v += [1000] * rows
    g += [W_KEYS[3] if summary else 3] * W_ROWS[2]
    v += [i % 1001 for i in range(W_ROWS[2])]
    for k, rows in enumerate(W_SPLIT_ROWS):
        g += [W_SPLIT_KEYS[k] if summary else 4 + k] * rows
        v += [1000 - i % 2 * 100 for i in range(rows)]
    order = np.random.default_rng(33).permutation(len(g))
    cols = {"g": i64(g)[order], "w": i64([W_BIG] * len(g)), "v": i64(v)[order]}
    return {"name": "W-big-" + ("summary" if summary else "moments"), "cols": cols, "info": {"v": W_INFO}, "block_rows": 1000,
            "far": FAR if summary else None, "q": dict(groups=["g"], aggs=["v"], op="hist", weight_col="w", want_percentiles=summary)}


def summary_cases():
    """Every case that takes the device summary path: G, M, E and the summary form of W."""
    return ([case_g(nv) for nv in G_N_VALUES] + [case_g_hist_bucket(hb) for hb in G_HIST_BUCKETS] + [case_m(n) for n in M_AGGS] +
            cases_e() + [case_w_patterns(True), case_w_big(True)])


def moments_cases():
    """The W cases as moments queries: want_percentiles=False, few groups."""
    return [case_w_patterns(False), case_w_big(False)]


# ---------------------------------------------------------------- the printers' tables
def printer_table(n_aggs):
    """About 700 live groups among FAR_TOTAL + 1 cells, 1 to 100 rows each (ties in Count: rows are compared by key)."""
    rng = np.random.default_rng(700 + n_aggs)
    aggs = ["v"] if n_aggs == 1 else M_AGGS[4]
    infos = {"v": G_INFO[1002]} if n_aggs == 1 else {a: G_INFO[int(a[1:])] for a in aggs}
    live = np.sort(rng.choice(np.arange(1, FAR_TOTAL), size=698, replace=False))
    live = np.concatenate([[0], live, [FAR_TOTAL]])
    g = np.repeat(live, 1 + np.arange(live.size) * 37 % 100)
    rng.shuffle(g)
    cols = {"g": i64(g)}
    for a, (lo, hi) in infos.items():
        bs, nb, nv = setup_buckets(lo, hi)
        v = lo + rng.integers(0, nv * bs, size=g.size)
        far_out = rng.random(g.size) < 0.02  # some outliers where the gate lets them through
        v[far_out] = min(lo + nv * bs + 3, hi * 10)
        cols[a] = i64(np.minimum(v, hi * 10))
    return {"name": "P-%d" % n_aggs, "cols": cols, "info": infos, "block_rows": 8192, "far": FAR_TOTAL,
            "q": dict(groups=["g"], aggs=aggs, op="hist")}
