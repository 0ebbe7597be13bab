#!/usr/bin/env python3
"""Measures sybl_table_digest and what it buys a time-series query ("Digest").

Input: --rows rows (default 1e8) of config 5's columns (c00 time, c09 group, c07 aggregate; sybil_amd/synth.py) with the
time column SHUFFLED, appended in 65536-row blocks, compact storage.  Then, in one process:
  digest   --warmup digests, then --runs timed ones: hipEvent time of key extraction, sort and gather
           (sybl_table_digest_stats), minimum and median, beside the bytes each phase moves (computed from the shapes);
  query    config 5's query prepared on the shuffled table and on its digest, scanned back to back, alternating between
           the two tables: strategy and scan time of each.

    python tools/bench_digest.py [--rows N] [--runs 5] [--warmup 2] [--out profiles/digest.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 1 and args.warmup >= 0
    import sybil_amd
    from sybil_amd import synth

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = sybil_amd.Context(0)
    n = args.rows
    wl = synth.WORKLOADS["cfg5_time_rollup"]
    rng = np.random.default_rng(synth.SEED)
    _, _, a, b, _, _ = synth.COLUMNS["c00"]
    t0 = time.time()
    cols = {"c00": rng.permutation(a + (np.arange(n, dtype=np.int64) * b) // n),
            "c09": rng.integers(0, 500, n, dtype=np.int64), "c07": rng.integers(0, 1_000_000, n, dtype=np.int64)}
    src = ctx.create_table("digest_bench")
    for name in wl["columns"]:
        src.add_column(name, "int", synth.COLUMNS[name][4], synth.COLUMNS[name][5])
    src.compact()  # (an empty table: switches compact mode on, blocks are packed as they arrive)
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        src.append_block(r1 - r0, {c: cols[c][r0:r1] for c in wl["columns"]})
    src.compact()
    del cols
    say("# tools/bench_digest.py --rows %d --runs %d --warmup %d on %s" % (n, args.runs, args.warmup, ctx.device_info()["name"]))
    say("table: %d rows, %d blocks, shuffled time column, compact storage %s, %.1f MB resident; built in %.1f s (host)" % (
        src.rows, src.blocks, {c: src.column_storage(c)[0] for c in wl["columns"]}, src.hbm_bytes / 1e6, time.time() - t0))

    # ---- digest
    runs, dg = [], None
    for k in range(args.warmup + args.runs):
        if dg is not None:
            dg.free()
        w0 = time.time()
        dg = src.digest("c00")
        wall = (time.time() - w0) * 1e3
        st = dg.digest_stats()
        st["wall_ms"] = wall
        if k >= args.warmup:
            runs.append(st)
    st = runs[0]
    say("digest: %d rows -> %d blocks, %d key bits; %d warm-up + %d timed runs in one process" % (st["rows"], st["blocks"], st["key_bits"], args.warmup, args.runs))
    say("%-8s %10s %10s %14s %18s" % ("phase", "min ms", "median ms", "bytes moved", "GB/s at the min"))
    for ph in ("keys", "sort", "gather"):
        ms = [r[ph + "_ms"] for r in runs]
        by = st[ph + "_bytes"]
        say("%-8s %10.3f %10.3f %14d %18.1f" % (ph, min(ms), statistics.median(ms), by, by / min(ms) / 1e6))
    wall = [r["wall_ms"] for r in runs]
    say("%-8s %10.3f %10.3f   (host wall time of the whole call: allocation, block writer and frees included)" % ("call", min(wall), statistics.median(wall)))

    # ---- the time-series query on both tables, alternating
    q_src, q_dg = src.query(**wl["query"]), dg.query(**wl["query"])
    times = {"shuffled": [], "digest": []}
    for k in range(args.warmup + args.runs):
        for name, q in (("shuffled", q_src), ("digest", q_dg)):
            q.scan()
            ctx.sync()
            if k >= args.warmup:
                times[name].append(q.stats()["scan_ms"])
    r_src, r_dg = q_src.finalize(), q_dg.finalize()
    same = sorted((r["time_bucket"], r["key"], r["count"], r["hists"][0]["sum"]) for r in r_src.time_results) == \
        sorted((r["time_bucket"], r["key"], r["count"], r["hists"][0]["sum"]) for r in r_dg.time_results)
    say("query (config 5: %s), back-to-back scans alternating between the tables:" % wl["flags"])
    for name, q in (("shuffled", q_src), ("digest", q_dg)):
        s = q.stats()
        say("%-9s strategy %d, %d cells, lds %d B, scan min %.3f ms, median %.3f ms" % (
            name, s["strategy"], s["n_cells"], s["lds_bytes"], min(times[name]), statistics.median(times[name])))
    say("results of the two tables equal: %s" % same)
    for x in (r_src, r_dg, q_src, q_dg, dg, src):
        x.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
