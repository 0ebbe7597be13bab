#!/usr/bin/env python3
"""Measures sybl_table_concat.

Input: tools/bench_select.py's table -- --rows rows (default 1e8) of `time` (4 stored bytes), `k` (2 stored bytes) and `v`
(4 stored bytes), 65536-row blocks, compact storage -- cut into two sources of rows / 2.  Four cases, in one process:
  (a) copies      the halves are stored alike (same widths, same bases): every piece is a device-to-device copy
  (b) transcode   the second half's `time` and `v` are shifted, so its bases differ: 4 -> 4 transcodes without an id table
  (c) id table    both halves carry a str column `s` (2 stored bytes) whose dictionaries overlap by half: the second half's
                  ids go through an id table
  (d) widening    the second half in canonical storage, so the output is canonical: the first half's columns go 4 -> 8 and
                  2 -> 8, the second half's are copies
For each: --warmup concats, then --runs timed ones: hipEvent time of all copies and transcodes (sybl_table_concat_stats:
copy_ms), minimum and median, beside the bytes they move (computed from the shapes, not measured) and the host wall time of the
call.  The yardstick, in the same process: select without filters over the concatenated table of (a) -- until concat the only
way to copy a table in HBM.

    python tools/bench_concat.py [--rows N] [--runs 3] [--warmup 1] [--out profiles/concat.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_RANGE = 60000
N_STRINGS = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 1 and args.warmup >= 0 and args.rows >= 4
    import sybil_amd

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = sybil_amd.Context(0)
    n = args.rows
    half = n // 2
    rng = np.random.default_rng(20240229)
    t0 = time.time()
    cols = {"time": rng.permutation(1_700_000_000 + (np.arange(n, dtype=np.int64) * 86400) // n),
            "k": rng.integers(0, K_RANGE, n, dtype=np.int64), "v": rng.integers(0, 1_000_000, n, dtype=np.int64)}
    for name, (lo, hi) in (("time", (1_700_000_000, 1_700_086_399)), ("k", (0, K_RANGE - 1)), ("v", (0, 999_999))):
        for r0 in (0, half):  # (both halves span the whole range: stored alike)
            cols[name][r0], cols[name][r0 + 1] = lo, hi
    sid = rng.integers(0, N_STRINGS, n).astype(np.int32)
    vocab = [["s%04d" % k for k in range(N_STRINGS)], ["s%04d" % k for k in range(N_STRINGS // 2, N_STRINGS + N_STRINGS // 2)]]

    def table(r0, r1, shift, strings, compact=True):
        tb = ctx.create_table("concat_bench")
        for name in cols:
            tb.add_column(name, "int")
        if strings is not None:
            tb.add_column("s", "str")
        if compact:
            tb.compact()  # (an empty table: switches compact mode on, blocks are packed as they arrive)
        for b0 in range(r0, r1, 65536):
            b1 = min(r1, b0 + 65536)
            blk = {"time": cols["time"][b0:b1] + shift, "k": cols["k"][b0:b1], "v": cols["v"][b0:b1] + 2 * shift}
            if strings is not None:
                blk["s"] = {"ids": sid[b0:b1], "strings": strings}
            tb.append_block(b1 - b0, blk)
        return tb.compact() if compact else tb

    first, second = table(0, half, 0, vocab[0]), table(half, 2 * half, 0, vocab[1])
    shifted = table(half, 2 * half, 7, None)
    canonical = table(half, 2 * half, 0, None, compact=False)
    del cols, sid
    say("# tools/bench_concat.py --rows %d --runs %d --warmup %d on %s" % (n, args.runs, args.warmup, ctx.device_info()["name"]))
    say("# one process on one device; times are hipEvent times, bytes are computed from the shapes (not measured)")
    for label, tb in (("first half", first), ("second half", second), ("second half, shifted", shifted), ("second half, canonical", canonical)):
        say("%s: %d rows, %d blocks, compact storage %s, %.1f MB resident" % (
            label, tb.rows, tb.blocks, {c: tb.column_storage(c) for c in tb.samples(limit=1).columns}, tb.hbm_bytes / 1e6))
    say("built in %.1f s (host)" % (time.time() - t0))

    ok = True
    plain = ["time", "k", "v"]
    kept = None
    for label, srcs, columns, want in (("(a) like-stored halves", [first, second], plain, (3 * 2, 0, 0)),
                                       ("(b) second half from other bases", [first, shifted], plain, (3 + 1, 2, 0)),
                                       ("(c) with a str column through an id table", [first, second], None, (3 * 2 + 1, 0, 1)),
                                       ("(d) second half canonical: the first widens", [first, canonical], plain, (3, 3, 0))):
        runs, out = [], None
        for k in range(args.warmup + args.runs):
            if out is not None:
                out.free()
            w0 = time.time()
            out = ctx.concat(srcs, columns)
            wall = (time.time() - w0) * 1e3
            st = out.concat_stats()
            st["wall_ms"] = wall
            if k >= args.warmup:
                runs.append(st)
        st = runs[0]
        ok = ok and out.rows == 2 * half == st["rows"] and (st["copies"], st["transcodes"], st["lut_transcodes"]) == want
        say("%s: %d rows in %d blocks, %d columns; pieces: %d copies, %d transcodes, %d through an id table; %d warm-up + %d timed runs" % (
            label, st["rows"], st["blocks"], st["columns"], st["copies"], st["transcodes"], st["lut_transcodes"], args.warmup, args.runs))
        say("    output storage %s" % {c: out.column_storage(c) for c in out.samples(limit=1).columns})
        say("%-8s %10s %10s %14s %18s" % ("phase", "min ms", "median ms", "bytes moved", "GB/s at the min"))
        ms = [r["copy_ms"] for r in runs]
        say("%-8s %10.3f %10.3f %14d %18.1f" % ("copy", min(ms), statistics.median(ms), st["copy_bytes"], st["copy_bytes"] / max(min(ms), 1e-9) / 1e6))
        ms = [r["stats_ms"] for r in runs]
        say("%-8s %10.3f %10.3f   (block statistics recomputed for the remapped str column; zero launches otherwise)" % ("stats", min(ms), statistics.median(ms)))
        wall = [r["wall_ms"] for r in runs]
        say("%-8s %10.3f %10.3f   (host wall time of the whole call: allocation, id tables, readback and frees included)" % (
            "call", min(wall), statistics.median(wall)))
        if kept is None:
            kept = out
        else:
            out.free()

    # ---- the yardstick: select without filters over the same rows
    runs, sel = [], None
    for k in range(args.warmup + args.runs):
        if sel is not None:
            sel.free()
        w0 = time.time()
        sel = kept.select()
        wall = (time.time() - w0) * 1e3
        st = sel.select_stats()
        st["wall_ms"] = wall
        if k >= args.warmup:
            runs.append(st)
    ok = ok and sel.rows == kept.rows
    sel.free()
    ms = [r["gather_ms"] for r in runs]
    by = runs[0]["gather_bytes"]
    say("select without filters over the output of (a): gather min %.3f ms, median %.3f ms, %d bytes, %.1f GB/s at the min; rows "
        "phase %.3f ms; call %.3f ms" % (min(ms), statistics.median(ms), by, by / min(ms) / 1e6, min(r["rows_ms"] for r in runs),
                                         min(r["wall_ms"] for r in runs)))
    for tb in (kept, first, second, shifted, canonical):
        tb.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
