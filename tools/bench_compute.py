#!/usr/bin/env python3
"""Measures sybl_table_compute pass by pass.

Table t: --rows rows (default 1e8), compact, appended in 65536-row blocks: `a` / `b` and `c2` .. `c7` (1 stored byte each),
`status` (2), `x` (4, uniform in [0, 2^31)), `start` / `end` (8: millisecond timestamps an hour apart at most, `end` with 1% of
its rows unpopulated).  Then, in one process, one expression per call:
    a + b,  end - start,  x / 1024,  x % 86400 / 3600,  if(status >= 500, 1, 0),  the sum of 8 columns,
and, for the per-row cost of the software division,  x * 1024  and  x - 1024  beside  x / 1024  (same source, same op count).
Per expression: --warmup calls, then --runs timed ones; hipEvent time of the range pass, the store pass and the block statistics
(sybl_table_compute_stats), minimum and median, beside the bytes each pass moves (computed from the shapes, not measured) and
the GB/s they make.  For comparison, in the same run: sybl_table_select without filters (a sequential copy of every column).

    python tools/bench_compute.py [--rows N] [--runs 3] [--warmup 1] [--out profiles/compute.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXPRS = [("a + b", "a + b"), ("end - start", "end - start"), ("x / 1024", "x / 1024"), ("x % 86400 / 3600", "x % 86400 / 3600"),
         ("if(status >= 500, 1, 0)", "if(status >= 500, 1, 0)"), ("8-column sum", "a + b + c2 + c3 + c4 + c5 + c6 + c7"),
         ("x * 1024 (no division)", "x * 1024"), ("x - 1024 (no division)", "x - 1024")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 1 and args.warmup >= 0
    import sybil_amd

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    ctx = sybil_amd.Context(0)
    n = args.rows
    rng = np.random.default_rng(20240611)
    t0 = time.time()
    start = 1_700_000_000_000 + (np.arange(n, dtype=np.int64) * 86_400_000) // n
    cols = {"a": rng.integers(0, 100, n, dtype=np.int64), "b": rng.integers(0, 100, n, dtype=np.int64),
            "status": rng.choice(np.array([200, 204, 301, 404, 500, 503], dtype=np.int64), n), "x": rng.integers(0, 1 << 31, n, dtype=np.int64),
            "start": start, "end": start + rng.integers(0, 3_600_000, n, dtype=np.int64)}
    for k in range(2, 8):
        cols["c%d" % k] = (cols["x"] >> (3 * k)) % 200
    end_pop = rng.random(n) > 0.01
    t = ctx.create_table("compute_bench")
    for name in cols:
        t.add_column(name, "int")
    t.compact()
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        t.append_block(r1 - r0, {c: ((cols[c][r0:r1], end_pop[r0:r1]) if c == "end" else cols[c][r0:r1]) for c in cols})
    t.compact()
    del cols, start, end_pop
    say("# tools/bench_compute.py --rows %d --runs %d --warmup %d on %s" % (n, args.runs, args.warmup, ctx.device_info()["name"]))
    say("# one process on one device; times are hipEvent times, bytes are computed from the shapes (not measured)")
    names = ["a", "b", "status", "x", "start", "end"] + ["c%d" % k for k in range(2, 8)]
    widths = {c: t.column_storage(c)[0] for c in names}
    say("table t: %d rows, %d blocks, compact storage %s, %.1f MB resident; built in %.1f s (host)" % (t.rows, t.blocks, widths, t.hbm_bytes / 1e6, time.time() - t0))
    say()
    say("%-26s %4s %6s %9s %9s %9s %9s %9s %9s %9s %10s" % ("expression", "ops", "stored", "range ms", "(median)", "GB/s", "store ms", "(median)", "GB/s", "stats ms", "ps/row r+s"))
    per_row = {}
    for label, expr in EXPRS:
        runs, out = [], None
        for k in range(args.warmup + args.runs):
            if out is not None:
                out.free()
            w0 = time.time()
            out = t.compute([("v", expr)])
            wall = (time.time() - w0) * 1e3
            st = out.compute_stats()
            st["wall_ms"] = wall
            if k >= args.warmup:
                runs.append(st)
        w = out.column_storage("v")[0]
        out.free()
        st = runs[0]
        rm, sm, tm = [r["range_ms"] for r in runs], [r["store_ms"] for r in runs], [r["stats_ms"] for r in runs]
        per_row[label] = (min(rm) + min(sm)) * 1e9 / n
        say("%-26s %4d %6d %9.3f %9.3f %9.1f %9.3f %9.3f %9.1f %9.3f %10.1f" % (
            label, st["ops"], w, min(rm), statistics.median(rm), st["range_bytes"] / min(rm) / 1e6, min(sm), statistics.median(sm),
            st["store_bytes"] / min(sm) / 1e6, min(tm), per_row[label]))
        say("%-26s      unpopulated %d; range %d bytes, store %d bytes; the whole call %.1f ms of host wall time (the concat of t, allocation, readbacks, frees)" % (
            "", st["unpopulated"], st["range_bytes"], st["store_bytes"], min(r["wall_ms"] for r in runs)))
        flush()
    say()
    say("the software division, per row (range + store): x / 1024 %.1f ps, x * 1024 %.1f ps, x - 1024 %.1f ps" % (
        per_row["x / 1024"], per_row["x * 1024 (no division)"], per_row["x - 1024 (no division)"]))

    # ---- the yardstick over the same t: select without filters (a sequential copy of every column)
    runs, out = [], None
    for k in range(args.warmup + args.runs):
        if out is not None:
            out.free()
        out = t.select()
        if k >= args.warmup:
            runs.append(out.select_stats())
    out.free()
    ms = [r["gather_ms"] for r in runs]
    say("select without filters (sequential copy of every column): gather min %.3f ms, median %.3f ms, %d bytes, %.1f GB/s at the min" % (
        min(ms), statistics.median(ms), runs[0]["gather_bytes"], runs[0]["gather_bytes"] / min(ms) / 1e6))
    t.free()
    ctx.close()
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
