"""Inputs at the int64 edges and a plain Python big-integer reference of the aggregation, shared by
tests/test_oracle_int64_edges.py (oracle vs this reference, CPU) and tests/test_gpu_int64_edges.py (engine vs oracle).

A case is a dict: cols {name: int64 array}, info {agg column: (Info.Min, Info.Max)}, q (sybil_amd query kwargs),
block_rows.  reference(case) returns {(time_bucket, key tuple): group} and the cumulative group, each group a dict of
count, samples, sum64 (sum mod 2^64 as int64), mean (fractions.Fraction or None), min / max over the accepted values,
values (bucket counts, hist mode) and stddev (GetStdDev's formula, hist_basic.go:192-219, around the exact mean)."""
import math
from fractions import Fraction

import numpy as np

MIN, MAX = -(1 << 63), (1 << 63) - 1
M64 = 1 << 64


def wrap64(x):
    """Go's int64 arithmetic: x mod 2^64 as a signed value."""
    x &= M64 - 1
    return x - M64 if x >> 63 else x


def trunc_div(a, b):
    """Go's integer division (truncates toward zero) on Python ints."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def i64(values):
    return np.array([int(v) for v in values], dtype=np.int64)


# ---------------------------------------------------------------- the reference
def _passes(v, op, c):
    return {"gt": v > c, "lt": v < c, "eq": v == c, "neq": v != c}[op]


def _new_group():
    return {"rows": 0, "row_samples": 0, "count": 0, "samples": 0, "sum": 0, "min": None, "max": None, "pop": 0, "vals": {}}


def _add(g, v, w, weighted, info, geo):
    g["pop"] += 1
    imin, imax = info
    if v > wrap64(imax * 10) or v < imin:  # hist_basic.go:104, Info.Max*10 wrapping like Go's int64
        return
    if weighted or w > 1:
        g["samples"] += 1
        g["count"] += w
        g["sum"] += v * w
    else:
        g["count"] += 1
        g["sum"] += v
        w = 1
    g["min"] = v if g["min"] is None else min(g["min"], v)
    g["max"] = v if g["max"] is None else max(g["max"], v)
    if geo:
        bs, nv = geo
        b = trunc_div(v - imin, bs)  # hist_basic.go:130
        assert 0 <= b < nv, "the cases of this file keep every accepted value inside the bucket array"
        g["vals"][b] = g["vals"].get(b, 0) + w


def _finish(g, info, geo):
    n = g["count"]
    g["sum64"] = wrap64(g["sum"])
    g["mean"] = Fraction(g["sum"], n) if n else None
    if geo and n:
        bs, nv = geo
        var = sum((Fraction(b * bs + info[0]) - g["mean"]) ** 2 * c for b, c in g["vals"].items()) / n
        g["stddev"] = math.sqrt(var)
        g["values"] = np.zeros(nv, dtype=np.int64)
        for b, c in g["vals"].items():
            g["values"][b] = c
    return g


def reference(case, geo=None):
    """geo: (BucketSize, len(Values)) in hist mode (SetupBuckets' geometry is not what this file is about: the callers pass
    the oracle's, which tests/test_oracle_kat.py pins)."""
    q, cols = case["q"], case["cols"]
    n = len(next(iter(cols.values())))
    agg = q["aggs"][0]
    info = case["info"][agg]
    weighted = bool(q.get("weight_col"))
    groups, total = {}, _new_group()
    matched = 0
    for i in range(n):
        if not all(_passes(int(cols[f[0]][i]), f[1], int(f[2])) for f in q.get("filters", [])):
            continue
        matched += 1
        key = tuple(int(cols[g][i]) & (M64 - 1) for g in q.get("groups", []))
        tb = 0
        if q.get("time_col"):
            tb = trunc_div(int(cols[q["time_col"]][i]), q["time_bucket"]) * q["time_bucket"]  # aggregate.go:174
        w = int(cols[q["weight_col"]][i]) if weighted else 1
        for g in (groups.setdefault((tb, key), _new_group()), total):
            g["rows"] += w
            g["row_samples"] += 1
            _add(g, int(cols[agg][i]), w, weighted, info, geo)
    for g in groups.values():
        _finish(g, info, geo)
    return {"matched": matched, "groups": groups, "total": _finish(total, info, geo)}


# ---------------------------------------------------------------- A: sums that leave int64
def _a1(negate=False):
    rng = np.random.default_rng(101)
    n = 20_000
    v = 1_700_000_000_000_000 + rng.integers(0, 86_400_000_000, size=n)
    g = rng.integers(0, 3, size=n)
    if negate:
        v = -v
    v = v.astype(np.int64)
    # Info exact -- but for the negated column Info.Max = 0: with a negative Info.Max the gate `value > Info.Max*10`
    # (hist_basic.go:104) rejects every value near it, and the case is about sums, not about the gate (B2 is)
    info = (int(v.min()), 0 if negate else int(v.max()))
    return {"cols": {"g": g.astype(np.int64), "v": v}, "info": {"v": info}, "block_rows": 4096}


def case_a(name, op):
    if name in ("A1", "A2"):
        c = _a1(negate=name == "A2")
        c["q"] = dict(groups=["g"], aggs=["v"], op=op)
    elif name == "A3":
        rng = np.random.default_rng(103)
        v = 900_000_000_000_000_000 - rng.integers(0, 1_000_000, size=64)
        v[0], v[1] = 900_000_000_000_000_000, 900_000_000_000_000_000 - 999_999
        c = {"cols": {"g": i64(np.arange(64) % 2 * 5), "w": i64(np.arange(64) % 4 + 1), "v": i64(v)},
             "info": {"v": (900_000_000_000_000_000 - 999_999, 900_000_000_000_000_000)}, "block_rows": 24,
             "q": dict(groups=["g"], aggs=["v"], op=op, weight_col="w")}
    elif name == "A4":
        c = {"cols": {"g": i64([3] * 11), "v": i64([900_000_000_000_000_000] * 11)},
             "info": {"v": (900_000_000_000_000_000 - 1000, 900_000_000_000_000_000)}, "block_rows": 65536,
             "q": dict(groups=["g"], aggs=["v"], op=op)}
    elif name == "A5":
        c = {"cols": {"g": i64([1] * 5), "v": i64([9 * 10 ** 18] * 4 + [-4 * 10 ** 18])},
             "info": {"v": (-(1 << 62), 900_000_000_000_000_000)}, "block_rows": 65536,
             "q": dict(groups=["g"], aggs=["v"], op=op)}
    else:
        raise KeyError(name)
    c["name"] = "%s-%s" % (name, op)
    return c


# ---------------------------------------------------------------- B: the extremes themselves
B_INFO = (MIN, MAX // 10)


def case_b1(two_groups=False):
    cols = {"k": i64([MIN, MAX, 0, MIN, MAX, 7, 7]), "g_small": i64([0, 1, 2, 0, 1, 2, 2]),
            "v": i64([MIN, MIN, -1, 0, 5, MIN, MIN])}
    return {"name": "B1" + ("x2" if two_groups else ""), "cols": cols, "info": {"v": B_INFO}, "block_rows": 4,
            "q": dict(groups=["g_small", "k"] if two_groups else ["k"], aggs=["v"], op="avg")}


def case_b2(which):
    """The reject gate, one value per group (plus two groups that mix an accepted and a rejected value)."""
    if which == "edges":
        imin, imax = -5, MAX // 10
        max10 = imax * 10
        v = [max10, max10 + 1, imin, imin - 1, 0, max10, max10 + 1, imin - 1, imin, MAX, MIN]
        g = [0, 1, 2, 3, 4, 5, 5, 6, 6, 7, 8]
    else:  # Info.Max*10 wraps negative: every value is above it
        imin, imax = -5, 10 ** 18
        assert wrap64(imax * 10) < imin
        v = [0, 1, -5, 10 ** 18, MIN, wrap64(imax * 10), 7]
        g = [0, 0, 1, 1, 2, 2, 3]
    return {"name": "B2-" + which, "cols": {"g": i64(g), "v": i64(v)}, "info": {"v": (imin, imax)}, "block_rows": 4,
            "q": dict(groups=["g"], aggs=["v"], op="avg")}


B3_CONSTANTS = (MIN, MIN + 1, MAX - 1, MAX)


def case_b3(col, op, const):
    base = MAX - 200
    cols = {"wide": i64([MIN, MIN + 1, 0, MAX - 1, MAX, MIN, MAX, 0, MAX - 1, MIN + 1]),
            "near": i64([base, base + 199, base + 200, base + 1, base + 200, base, base + 199, base + 100, base + 200, base + 7]),
            "g": i64([0, 1, 2, 0, 1, 2, 0, 1, 2, 0]), "v": i64([1, 2, 3, 4, 5, 6, 7, 8, 9, 10])}
    return {"name": "B3-%s-%s-%d" % (col, op, const), "cols": cols, "info": {"v": (1, 10)}, "block_rows": 4,
            "q": dict(filters=[(col, op, const)], groups=["g"], aggs=["v"], op="avg")}


def cols_b4():
    return {"g": i64([0, 1, 0, 1, 0, 1, 0, 1, 2, 2]), "d": i64([MIN, MIN, MAX, 0, MIN, MAX, 0, 0, MIN, MIN])}


# ---------------------------------------------------------------- C: the divide switch
C_SPANS = ((1 << 51) - 1, 1 << 51, (1 << 51) + 1, (1 << 53) + 12345, 1 << 61)


def c_bucket_sizes(span):
    """Two bucket sizes that keep every value inside the 1002 buckets SetupBuckets makes whatever -int-bucket says:
    ceil(span / 1000) (no power of two for any span of C_SPANS) and the power of two above it."""
    bs = -(-span // 1000)
    assert bs & (bs - 1)
    return bs, 1 << bs.bit_length()


def c_min(span, negative):
    """Info.Min of a C column: 0, or so far below zero that Info.Max is 1000 (a negative Min whose Info.Max*10 neither wraps nor
    turns negative: either would reject the whole column)."""
    return 1000 - span if negative else 0


def case_c(span, bs, imin, loghist=False):
    """The rows go round-robin over as many groups as keep rows-per-group * span below 2^64 (3, or 100 for the 2^61 span): the
    bound up to which avg is exact (include/sybilgpu.h at `sum`), so that parity.compare holds on every field."""
    n_groups = 3 if 250 * span < M64 else 100
    rng = np.random.default_rng(span % 1000 + 7)
    ks = rng.integers(1, span // bs, size=200)
    v = [imin, imin + span]
    for k in ks:
        v += [imin + int(k) * bs - 1, imin + int(k) * bs, imin + int(k) * bs + 1]
    v = [x for x in v if imin <= x <= imin + span]
    g = [i % n_groups for i in range(len(v))]
    assert (len(v) // n_groups + 1) * span < M64
    q = dict(groups=["g"], aggs=["v"], op="hist", loghist=True) if loghist else dict(groups=["g"], aggs=["v"], op="hist", hist_bucket=bs)
    return {"name": "C-%d-%d-%d%s" % (span, bs, imin, "-loghist" if loghist else ""), "cols": {"g": i64(g), "v": i64(v)},
            "info": {"v": (imin, imin + span)}, "block_rows": 256, "q": q}


def case_c_time(which):
    rng = np.random.default_rng(211)
    n = 300
    if which == "big":  # either side of 2^51: the exact-division branch of the time bucket
        tbk = 1 << 44
        t = (1 << 51) + rng.integers(-(1 << 47), 1 << 47, size=n)
        t[:4] = [(1 << 51) - 1, 1 << 51, (1 << 51) + 1, (1 << 51) - tbk]
    elif which == "usec":  # microsecond timestamps by the hour
        tbk = 3_600_000_000
        t = 1_700_000_000_000_000 + rng.integers(0, 40 * tbk, size=n)
        t[:3] = [1_700_000_000_000_000 // tbk * tbk + tbk - 1, 1_700_000_000_000_000 // tbk * tbk + tbk, 1_700_000_000_000_000]
    else:  # negative times: truncation and floor differ
        tbk = 3600
        t = rng.integers(-20 * tbk, 20 * tbk, size=n)
        t[:6] = [-1, 0, 1, -tbk, -tbk + 1, -tbk - 1]
    cols = {"g": i64(np.arange(n) % 3), "t": i64(t), "v": i64(rng.integers(0, 1000, size=n))}
    return {"name": "Ct-" + which, "cols": cols, "info": {"v": (0, 999)}, "block_rows": 128,
            "q": dict(groups=["g"], aggs=["v"], op="hist", time_col="t", time_bucket=tbk)}
