#!/usr/bin/env python3
"""Measures sybl_table_rollup phase by phase.

Table: --rows rows (default 1e8) of config 5's columns generated on the device -- `c00` (time, ascending, here over 15 hours = 16
hourly buckets, so that hourly x 100 keys fits the LDS body), `c09` (500 values), `c07` (10^6 values) --, compact, plus two computed keys: `h100` =
c09 % 100 and `k7` = (c07 * 10 + c09 % 10) * 977 (10^7 values spread over 10^10).  A second table holds the same rows ordered
by c07, i.e. shuffled in time.  Shapes, each --warmup calls then --runs timed ones, hipEvent minima per phase
(sybl_table_rollup_stats), in one process:
  hourly x h100 on the time-ordered table (LDS body), and under SYBL_ROLLUP_PATH=global (the A/B of the LDS body)
  hourly x h100 on the shuffled table, likewise
  c07 alone: 10^6 cells (direct, HBM cells)
  k7 alone: 10^7 sparse values (hash)
  no key: one group, with the wave-uniform merge and under SYBL_ROLLUP_MERGE=0 (the A/B of the merge), HBM cells
  hourly alone on the time-ordered table, HBM cells, with the merge and without
Yardsticks in the same run: sybl_table_select without filters over the same columns (the pace of a copy) and the engine's own
query of the same group-by (Table.query(...).run(), scan time from its stats).

--only pct measures the percentiles instead (p50,p99 of the aggregated column; sybl_table_rollup_pct_stats), same table and
protocol: hourly x h100 (direct-LDS) by default and under each SYBL_ROLLUP_PCT, c07 as key (direct-global), k7 as key (hash),
one group, and hourly x h100 behind a 0.1 % filter.  Beside each shape, from the same run: that shape's rollup without
percentiles, and sort_ms.  The variant the plan chose is then held against the next wider one forced on the same shape: it stays
where it wins by more than the spread of the timed runs.

    python tools/bench_rollup.py [--rows N] [--runs 3] [--warmup 1] [--only plain|pct] [--out profiles/rollup.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("filter_ms", "accumulate_ms", "order_ms", "emit_ms")
PATHS = {0: "-", 1: "direct-LDS", 2: "direct-global", 3: "hash"}


PCT_PHASES = ("keys_ms", "sort_ms", "pick_ms")
VARIANTS = (("variant32", "32"), ("variant64", "64"), ("variant_pairs", "pairs"))


def bench_pct(args, say, base):
    """The percentile shapes: see the module's docstring."""
    say("%-40s %-13s %-7s %4s %10s %9s %8s %8s %8s %9s %8s %10s %10s" % (
        "shape (p50,p99)", "path", "variant", "bits", "items", "groups", "keys", "sort", "pick", "pct total", "spread", "rollup", "no pct"))
    results = {}

    def one(tb, env, **kw):
        for k in ("SYBL_ROLLUP_PATH", "SYBL_ROLLUP_PCT"):
            os.environ.pop(k, None)
        os.environ.update(env or {})
        runs = []
        for r in range(args.warmup + args.runs):
            out = tb.rollup(**kw)
            st, ps = out.rollup_stats(), out.rollup_pct_stats()
            out.free()
            if r >= args.warmup:
                runs.append((st, ps))
        for k in ("SYBL_ROLLUP_PATH", "SYBL_ROLLUP_PCT"):
            os.environ.pop(k, None)
        return runs

    def measure(label, tb, col, env=None, **kw):
        runs = one(tb, env, aggs=[(col, "sum,max,p50,p99")], **kw)
        plain = one(tb, None, aggs=[(col, "sum,max")], **kw)
        st, ps = runs[0]
        best = {k: min(r[1][k] for r in runs) for k in PCT_PHASES}
        totals = [sum(r[1][k] for k in PCT_PHASES) for r in runs]
        rollup = min(sum(r[0][k] for k in PHASES) for r in runs)
        no_pct = min(sum(r[0][k] for k in PHASES) for r in plain)
        variant = "+".join(name for key, name in VARIANTS if ps[key]) or "-"
        say("%-40s %-13s %-7s %4d %10d %9d %8.3f %8.3f %8.3f %9.3f %8.3f %10.3f %10.3f" % (
            label, PATHS[st["path"]], variant, ps["key_bits_max"], ps["items"], st["groups"], best["keys_ms"], best["sort_ms"], best["pick_ms"],
            min(totals), max(totals) - min(totals), rollup, no_pct))
        results[label] = dict(variant=variant, total=min(totals), spread=max(totals) - min(totals), rows_in=st["rows_in"], items=ps["items"])

    hourly = dict(groups=["h100"], time_col="c00", time_bucket=3600)
    measure("hourly x h100", base, "c07", **hourly)
    for v in ("32", "64", "pairs"):
        measure("hourly x h100, PCT=%s" % v, base, "c07", {"SYBL_ROLLUP_PCT": v}, **hourly)
    measure("c07 (10^6 values)", base, "c09", groups=["c07"])
    measure("c07 (10^6 values), PCT=64", base, "c09", {"SYBL_ROLLUP_PCT": "64"}, groups=["c07"])
    measure("k7 (10^7 sparse values)", base, "c09", groups=["k7"])
    measure("k7 (10^7 sparse values), PCT=pairs", base, "c09", {"SYBL_ROLLUP_PCT": "pairs"}, groups=["k7"])
    measure("one group", base, "c07")
    measure("one group, PCT=64", base, "c07", {"SYBL_ROLLUP_PCT": "64"})
    measure("hourly x h100, c07 < 1000 (0.1 %)", base, "c07", filters=[("c07", "lt", 1000)], **hourly)
    say()
    say("# keys / sort / pick: hipEvent minima in ms over the timed runs, summed over the columns; pct total = their sum per run, its")
    say("# minimum, and spread = max - min of it over the timed runs; rollup = filter + accumulate + order + emit of the same calls;")
    say("# no pct = the same shape with aggs sum,max only, same process")
    say()
    for narrow, wide in (("hourly x h100", "hourly x h100, PCT=64"), ("c07 (10^6 values)", "c07 (10^6 values), PCT=64"),
                         ("k7 (10^7 sparse values)", "k7 (10^7 sparse values), PCT=pairs"), ("one group", "one group, PCT=64")):
        a, b = results[narrow], results[wide]
        spread = max(a["spread"], b["spread"])
        say("%s: the plan's variant %s %.3f ms vs %s forced %.3f ms, spread %.3f ms -> %s" % (
            narrow, a["variant"], a["total"], b["variant"], b["total"], spread,
            "the narrower variant stays" if b["total"] - a["total"] > spread else "NO gain beyond the spread"))
    f = results["hourly x h100, c07 < 1000 (0.1 %)"]
    say("0.1 %% filter: %d items of %d rows in" % (f["items"], f["rows_in"]))
    say()
    say("not measured: canonical storage, more than one column with percentiles, 10^9 rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("plain", "pct"), default="plain")
    args = ap.parse_args()
    assert args.runs >= 1 and args.warmup >= 0
    import sybil_amd
    from sybil_amd import synth

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    ctx = sybil_amd.Context(0)
    n = args.rows
    cols = synth.synth_cols(["c00", "c09", "c07"])
    cols[0]["b"] = 15 * 3600                              # 16 hourly buckets: 16 x 100 cells x 5 fields x 8 B fit 64 KiB
    cols[0]["info_max"] = cols[0]["a"] + cols[0]["b"] - 1
    raw = ctx.synth_table("rollup_bench", synth.SEED, n, 0, n, cols).compact()
    base = raw.compute([("h100", "c09 % 100"), ("k7", "(c07 * 10 + c09 % 10) * 977")])
    raw.free()
    shuffled = base.digest("c07") if args.only == "plain" else None
    say("# tools/bench_rollup.py --rows %d --runs %d --warmup %d on %s" % (n, args.runs, args.warmup, ctx.device_info()["name"]))
    say("# one process on one device; times are hipEvent minima in ms, bytes are computed from the shapes (not measured)")
    say("table: %d rows, %d blocks, stored widths %s" % (base.rows, base.blocks, {c: base.column_storage(c)[0] for c in ("c00", "c09", "c07", "h100", "k7")}))
    say()
    if args.only == "pct":
        bench_pct(args, say, base)
        base.free()
        ctx.close()
        return
    say("%-44s %-13s %10s %9s %8s %10s %8s %8s %9s %8s" % ("shape", "path", "cells", "groups", "filter", "accumulate", "order", "emit", "total", "GB/s acc"))
    results = {}

    def measure(label, tb, env=None, **kw):
        for k in ("SYBL_ROLLUP_PATH", "SYBL_ROLLUP_MERGE"):
            os.environ.pop(k, None)
        os.environ.update(env or {})
        best = None
        for r in range(args.warmup + args.runs):
            out = tb.rollup(**kw)
            st = out.rollup_stats()
            out.free()
            if r >= args.warmup:
                best = st if best is None else {k: (min(best[k], v) if k in PHASES else v) for k, v in st.items()}
        for k in ("SYBL_ROLLUP_PATH", "SYBL_ROLLUP_MERGE"):
            os.environ.pop(k, None)
        total = sum(best[k] for k in PHASES)
        say("%-44s %-13s %10d %9d %8.3f %10.3f %8.3f %8.3f %9.3f %8.1f" % (
            label, PATHS[best["path"]], best["cells_or_slots"], best["groups"], best["filter_ms"], best["accumulate_ms"], best["order_ms"],
            best["emit_ms"], total, best["accumulate_bytes"] / best["accumulate_ms"] / 1e6 if best["accumulate_ms"] > 0 else 0.0))
        results[label] = best
        return best

    hourly = dict(groups=["h100"], aggs=[("c07", "sum,max")], time_col="c00", time_bucket=3600)
    measure("hourly x h100, time-ordered", base, **hourly)
    measure("hourly x h100, time-ordered, PATH=global", base, {"SYBL_ROLLUP_PATH": "global"}, **hourly)
    measure("hourly x h100, shuffled", shuffled, **hourly)
    measure("hourly x h100, shuffled, PATH=global", shuffled, {"SYBL_ROLLUP_PATH": "global"}, **hourly)
    measure("c07 (10^6 values)", base, groups=["c07"], aggs=[("c09", "sum,max")])
    measure("k7 (10^7 sparse values)", base, groups=["k7"], aggs=[("c09", "sum,max")])
    measure("one group, PATH=global", base, {"SYBL_ROLLUP_PATH": "global"}, aggs=[("c07", "sum,max")])
    measure("one group, PATH=global, MERGE=0", base, {"SYBL_ROLLUP_PATH": "global", "SYBL_ROLLUP_MERGE": "0"}, aggs=[("c07", "sum,max")])
    measure("one group (LDS)", base, aggs=[("c07", "sum,max")])
    by_hour = dict(aggs=[("c07", "sum,max")], time_col="c00", time_bucket=3600)
    measure("hourly, time-ordered, PATH=global", base, {"SYBL_ROLLUP_PATH": "global"}, **by_hour)
    measure("hourly, time-ordered, PATH=global, MERGE=0", base, {"SYBL_ROLLUP_PATH": "global", "SYBL_ROLLUP_MERGE": "0"}, **by_hour)
    say()

    def ratio(a, b):
        return results[b]["accumulate_ms"] / results[a]["accumulate_ms"] if results[a]["accumulate_ms"] > 0 else 0.0
    say("LDS body vs HBM cells, accumulate: time-ordered x%.2f, shuffled x%.2f" % (
        ratio("hourly x h100, time-ordered", "hourly x h100, time-ordered, PATH=global"), ratio("hourly x h100, shuffled", "hourly x h100, shuffled, PATH=global")))
    say("wave-uniform merge vs none, accumulate (HBM cells): one group x%.2f, hourly time-ordered x%.2f" % (
        ratio("one group, PATH=global", "one group, PATH=global, MERGE=0"), ratio("hourly, time-ordered, PATH=global", "hourly, time-ordered, PATH=global, MERGE=0")))
    say()

    # ---- yardsticks
    best = None
    for r in range(args.warmup + args.runs):
        out = base.select(columns=["c00", "h100", "c07"])
        st = out.select_stats()
        out.free()
        if r >= args.warmup:
            best = st if best is None else {k: (min(best[k], v) if k.endswith("_ms") else v) for k, v in st.items()}
    say("select without filters of c00, h100, c07 (a copy): rows %.3f ms + gather %.3f ms, %.1f GB/s gathered" % (
        best["rows_ms"], best["gather_ms"], best["gather_bytes"] / best["gather_ms"] / 1e6 if best["gather_ms"] > 0 else 0.0))
    q = base.query(groups=["h100"], aggs=["c07"], op="avg", time_col="c00", time_bucket=3600)
    scans = []
    for r in range(args.warmup + args.runs):
        res = q.run()
        res.free()
        if r >= args.warmup:
            scans.append(q.stats()["scan_ms"])
    q.free()
    say("the engine's query of hourly x h100 (avg of c07): scan %.3f ms" % min(scans))
    say()
    say("not measured: canonical storage, STR keys at scale, 10^9 rows")
    shuffled.free()
    base.free()
    ctx.close()


if __name__ == "__main__":
    main()
