#!/usr/bin/env python3
"""Measures sybl_table_select phase by phase.

Input: --rows rows (default 1e8) of three int columns -- `time` (4 stored bytes, SHUFFLED), `k` (2 stored bytes, uniform in
[0, 60000)), `v` (4 stored bytes) -- appended in 65536-row blocks, compact storage.  Then, in one process, for each cut that
keeps roughly 0.1 %, 10 %, 50 % and 100 % of the rows:
  select   `k < cut`: --warmup selects, then --runs timed ones: hipEvent time of the filter pass, the row list (count +
           k_sel_rows) and the gather (sybl_table_select_stats), minimum and median, beside the bytes each phase moves
           (computed from the shapes, not measured).
For comparison, digest's gather_ms on the same table (a random permutation of every row) and on its own digest (the identity
permutation: what the select that keeps 100 % gathers).

    python tools/bench_select.py [--rows N] [--runs 3] [--warmup 1] [--out profiles/select.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_RANGE = 60000
CUTS = (60, 6000, 30000, 60000)


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

    ctx = sybil_amd.Context(0)
    n = args.rows
    rng = np.random.default_rng(20240229)
    t0 = time.time()
    cols = {"time": rng.permutation(1_700_000_000 + (np.arange(n, dtype=np.int64) * 86400) // n),
            "k": rng.integers(0, K_RANGE, n, dtype=np.int64), "v": rng.integers(0, 1_000_000, n, dtype=np.int64)}
    src = ctx.create_table("select_bench")
    for name in cols:
        src.add_column(name, "int")
    src.compact()  # (an empty table: switches compact mode on, blocks are packed as they arrive)
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        src.append_block(r1 - r0, {c: cols[c][r0:r1] for c in cols})
    src.compact()
    counts = {cut: int((cols["k"] < cut).sum()) for cut in CUTS}
    del cols
    say("# tools/bench_select.py --rows %d --runs %d --warmup %d on %s" % (n, args.runs, args.warmup, ctx.device_info()["name"]))
    say("# one process on one device; times are hipEvent times, bytes are computed from the shapes (not measured)")
    say("table: %d rows, %d blocks, compact storage %s, %.1f MB resident; built in %.1f s (host)" % (
        src.rows, src.blocks, {c: src.column_storage(c)[0] for c in ("time", "k", "v")}, src.hbm_bytes / 1e6, time.time() - t0))

    ok = True
    for cut in CUTS:
        runs, sel = [], None
        for k in range(args.warmup + args.runs):
            if sel is not None:
                sel.free()
            w0 = time.time()
            sel = src.select([("k", "lt", cut)])
            wall = (time.time() - w0) * 1e3
            st = sel.select_stats()
            st["wall_ms"] = wall
            if k >= args.warmup:
                runs.append(st)
        st = runs[0]
        ok = ok and st["rows_out"] == counts[cut] == sel.rows
        sel.free()
        say("select k < %d: %d of %d rows (%.2f %%) -> %d blocks; %d warm-up + %d timed runs" % (
            cut, st["rows_out"], st["rows_in"], 100.0 * st["rows_out"] / max(st["rows_in"], 1), st["blocks_out"], args.warmup, args.runs))
        say("%-8s %10s %10s %14s %18s" % ("phase", "min ms", "median ms", "bytes moved", "GB/s at the min"))
        for ph in ("filter", "rows", "gather"):
            ms = [r[ph + "_ms"] for r in runs]
            by = st[ph + "_bytes"]
            say("%-8s %10.3f %10.3f %14d %18.1f" % (ph, min(ms), statistics.median(ms), by, by / max(min(ms), 1e-9) / 1e6))
        wall = [r["wall_ms"] for r in runs]
        say("%-8s %10.3f %10.3f   (host wall time of the whole call: allocation, readback, block writer and frees included)" % (
            "call", min(wall), statistics.median(wall)))

    # ---- digest's gather over the same table: a random permutation, and the identity
    dg = None
    for label in ("digest of the table (random permutation)", "digest of that digest (identity permutation)"):
        runs = []
        base = src if dg is None else dg
        out = None
        for k in range(args.warmup + args.runs):
            if out is not None:
                out.free()
            out = base.digest("time")
            if k >= args.warmup:
                runs.append(out.digest_stats())
        ms = [r["gather_ms"] for r in runs]
        by = runs[0]["gather_bytes"]
        say("%s: gather min %.3f ms, median %.3f ms, %d bytes, %.1f GB/s at the min" % (label, min(ms), statistics.median(ms), by, by / min(ms) / 1e6))
        if dg is None:
            dg = out
        else:
            out.free()
    dg.free()
    src.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
