#!/usr/bin/env python3
"""Measures sybl_table_lookup phase by phase.

Table t: --rows rows (default 1e8), compact, appended in 65536-row blocks: `time` (4 stored bytes, SHUFFLED), three key
columns `k4` / `k6` / `k7` uniform in [0, 1e4) / [0, 1e6) / [0, 1e7) (2 / 4 / 4 stored bytes) and `v` (4).  For each dim size D
in --dims (default 1e4, 1e6, 1e7) a table of D rows: the key `id` (a permutation of 0..D-1), `a1` / `a2` / `a4` (1 / 2 / 4
stored bytes), `s` (a str column of 100 strings, 1 stored byte) and `name` (a str key, one string per row, in another order
than t's).  Then, in one process, per D:
  INT direct   t.lookup(dim, k, 'id') -- the range D is dense, so the default path;
  INT hash     the same call under SYBL_LOOKUP_PATH=hash: same keys, same matches;
  STR          (D <= --str-max, default 1e6) t's key column as STRINGS -- made by this very call, t.lookup(names, k, columns =
               ['name']) -- against dim's `name`;
each with one (`a4`) and four (`a1`, `a2`, `a4`, `s`) attached columns: --warmup lookups, then --runs timed ones; hipEvent
time of build, probe and gather (sybl_table_lookup_stats), minimum and median, beside the bytes each phase moves (computed
from the shapes, not measured).
For comparison, in the same run: sybl_table_digest's gather_ms over t (a random gather of every column of t) and
sybl_table_select without filters (a sequential copy of every column of t), both per row and output byte.

    python tools/bench_lookup.py [--rows N] [--dims 10000,1000000,10000000] [--runs 3] [--warmup 1] [--out profiles/lookup.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEY_OF = {10_000: "k4", 1_000_000: "k6", 10_000_000: "k7"}
COLS = {1: ["a4"], 4: ["a1", "a2", "a4", "s"]}


def build_dim(ctx, d, rng, with_names):
    dim = ctx.create_table("dim%d" % d)
    for name in ("id", "a1", "a2", "a4"):
        dim.add_column(name, "int")
    dim.add_column("s", "str")
    if with_names:
        dim.add_column("name", "str")
    dim.compact()
    ids = rng.permutation(d).astype(np.int64)
    cats = ["cat%02d" % k for k in range(100)]
    for r0 in range(0, d, 65536):
        k = ids[r0:min(d, r0 + 65536)]
        cols = {"id": k, "a1": 1000 + k % 200, "a2": -7 + (k * 7) % 60000, "a4": 5 + (k * 100003) % (1 << 31),
                "s": dict(ids=(k % 100).astype(np.int32), strings=cats)}
        if with_names:
            cols["name"] = dict(ids=np.arange(len(k), dtype=np.int32), strings=["key%08d" % x for x in k.tolist()])
        dim.append_block(len(k), cols)
    dim.compact()
    return dim


def build_names(ctx, d):
    """id -> 'key%08d' in id order: t's dictionary, once its key has gone through it, is in another order than dim's."""
    tb = ctx.create_table("names%d" % d)
    tb.add_column("id", "int")
    tb.add_column("name", "str")
    tb.compact()
    for r0 in range(0, d, 65536):
        k = np.arange(r0, min(d, r0 + 65536), dtype=np.int64)
        tb.append_block(len(k), {"id": k, "name": dict(ids=np.arange(len(k), dtype=np.int32), strings=["key%08d" % x for x in k.tolist()])})
    tb.compact()
    return tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--dims", default="10000,1000000,10000000")
    ap.add_argument("--str-max", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 1 and args.warmup >= 0
    dims = [int(x) for x in args.dims.split(",")]
    assert all(d in KEY_OF for d in dims)
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
    rng = np.random.default_rng(20240229)
    t0 = time.time()
    k7 = rng.integers(0, 10_000_000, n, dtype=np.int64)
    cols = {"time": rng.permutation(1_700_000_000 + (np.arange(n, dtype=np.int64) * 86400) // n), "k4": k7 % 10_000, "k6": k7 % 1_000_000, "k7": k7,
            "v": rng.integers(0, 1_000_000, n, dtype=np.int64)}
    t = ctx.create_table("lookup_bench")
    for name in cols:
        t.add_column(name, "int")
    t.compact()
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        t.append_block(r1 - r0, {c: cols[c][r0:r1] for c in cols})
    t.compact()
    del cols, k7
    say("# tools/bench_lookup.py --rows %d --dims %s --runs %d --warmup %d on %s" % (n, args.dims, args.runs, args.warmup, ctx.device_info()["name"]))
    say("# one process on one device; times are hipEvent times, bytes are computed from the shapes (not measured)")
    widths = {c: t.column_storage(c)[0] for c in ("time", "k4", "k6", "k7", "v")}
    say("table t: %d rows, %d blocks, compact storage %s, %.1f MB resident; built in %.1f s (host)" % (t.rows, t.blocks, widths, t.hbm_bytes / 1e6, time.time() - t0))
    row_bytes = sum(widths.values())
    ok = True

    def measure(label, tb, dim, key, dim_key, ncols, force):
        nonlocal ok
        if force:
            os.environ["SYBL_LOOKUP_PATH"] = force
        else:
            os.environ.pop("SYBL_LOOKUP_PATH", None)
        runs, out = [], None
        for k in range(args.warmup + args.runs):
            if out is not None:
                out.free()
            w0 = time.time()
            out = tb.lookup(dim, key, dim_key=dim_key, columns=COLS[ncols], prefix="d_")
            wall = (time.time() - w0) * 1e3
            st = out.lookup_stats()
            st["wall_ms"] = wall
            if k >= args.warmup:
                runs.append(st)
        st = runs[0]
        ok = ok and st["matched"] == st["rows"] == tb.rows and st["dim_keys"] == dim.rows
        ow = [out.column_storage("d_" + c)[0] for c in COLS[ncols]]
        out.free()
        os.environ.pop("SYBL_LOOKUP_PATH", None)
        say("%s, %d attached column(s) %s (stored bytes %s): path %d, %d slots, %d of %d rows matched %d keys" % (
            label, ncols, COLS[ncols], ow, st["path"], st["slots"], st["matched"], st["rows"], st["dim_keys"]))
        say("  %-8s %10s %10s %14s %14s" % ("phase", "min ms", "median ms", "bytes moved", "bytes/ms (min)"))
        for ph in ("build", "probe", "gather"):
            ms = [r[ph + "_ms"] for r in runs]
            by = st[ph + "_bytes"]
            say("  %-8s %10.3f %10.3f %14d %14.3e" % (ph, min(ms), statistics.median(ms), by, by / max(min(ms), 1e-9)))
        g = min(r["gather_ms"] for r in runs)
        say("  gather: %.3f ns per row and column, %.3f ns per row and output byte" % (g * 1e6 / st["rows"] / ncols, g * 1e6 / st["rows"] / sum(ow)))
        wall = [r["wall_ms"] for r in runs]
        say("  %-8s %10.3f %10.3f   (host wall time of the whole call: the concat of t, allocation, readbacks and frees included)" % ("call", min(wall), statistics.median(wall)))
        flush()

    for d in dims:
        t1 = time.time()
        with_names = d <= args.str_max
        dim = build_dim(ctx, d, rng, with_names)
        say()
        say("dim: %d rows, compact storage %s, %.1f MB resident; built in %.1f s (host)" % (
            dim.rows, {c: dim.column_storage(c)[0] for c in ("id", "a1", "a2", "a4", "s")}, dim.hbm_bytes / 1e6, time.time() - t1))
        key = KEY_OF[d]
        for force, label in ((None, "INT direct"), ("hash", "INT hash")):
            for ncols in (1, 4):
                measure("%s, dim %d" % (label, d), t, dim, key, "id", ncols, force)
        if with_names:
            t1 = time.time()
            names = build_names(ctx, d)
            os.environ.pop("SYBL_LOOKUP_PATH", None)
            ts = t.lookup(names, key, dim_key="id", columns=["name"])
            names.free()
            say("t with `name` = the key %s as strings (stored bytes %d, a dictionary of %d strings): made by lookup in %.1f s (host, the dictionary included)" % (
                key, ts.column_storage("name")[0], d, time.time() - t1))
            for ncols in (1, 4):
                measure("STR, dim %d" % d, ts, dim, "name", "name", ncols, None)
            ts.free()
        else:
            say("STR, dim %d: not measured (a dictionary of %d strings through the append path; --str-max)" % (d, d))
        dim.free()
        flush()

    # ---- the two yardsticks over the same t: digest's gather (random) and select without filters (sequential)
    say()
    for label, call, stats, ms_key in (("digest of t (random gather of every column)", lambda: t.digest("time"), "digest_stats", "gather_ms"),
                                       ("select without filters (sequential copy of every column)", lambda: t.select(), "select_stats", "gather_ms")):
        runs, out = [], None
        for k in range(args.warmup + args.runs):
            if out is not None:
                out.free()
            out = call()
            if k >= args.warmup:
                runs.append(getattr(out, stats)())
        out.free()
        ms = [r[ms_key] for r in runs]
        by = runs[0]["gather_bytes"]
        say("%s: gather min %.3f ms, median %.3f ms, %d bytes, %.3e bytes/ms at the min; %d columns of %s stored bytes: %.3f ns per row and column, %.3f ns per row and output byte" % (
            label, min(ms), statistics.median(ms), by, by / min(ms), len(widths), list(widths.values()), min(ms) * 1e6 / n / len(widths), min(ms) * 1e6 / n / row_bytes))
    t.free()
    ctx.close()
    flush()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
