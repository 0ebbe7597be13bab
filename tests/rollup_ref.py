"""Python restatement of a table rollup (Table.rollup / sybl_table_rollup), written from the definition in
include/sybilgpu.h ("rollup") and not from the library: the checker of tests/test_gpu_rollup.py, itself checked by
tests/test_rollup_ref.py.

A table is a list of blocks in the form tests/samples_ref.py and tests/digest_ref.py use: (nrows, {column: spec}).  The
predicate is samples_ref.block_matches; arithmetic is Python's (exact), sums wrap to int64 at the end.
"""
import numpy as np

from tests import concat_ref as C
from tests import digest_ref as D
from tests import samples_ref as R

BLOCK_ROWS = D.BLOCK_ROWS
LDS, GLOBAL, HASH = 1, 2, 3
MAX_CELLS = 1 << 27
OPS = ("n", "sum", "min", "max")


def wrap(x):
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def trunc_div(v, b):
    """Go's integer division: toward zero."""
    q = abs(int(v)) // int(b)
    return -q if v < 0 else q


def parse_ops(ops):
    got = ops.split(",") if ops else []
    if not got or any(o not in OPS for o in got) or len(set(got)) != len(got):
        raise ValueError("ops '%s'" % ops)
    return [o for o in OPS if o in got]


def agg_pairs(aggs):
    return list(aggs.items()) if isinstance(aggs, dict) else [tuple(a) for a in aggs]


def choose_path(product, live_rows, fields, force=None):
    """direct iff product <= max(2^16, 4 x live rows) and <= 2^27; the LDS body iff cells x fields x 8 B <= 64 KiB."""
    fits = product <= MAX_CELLS
    lds = fits and product * fields * 8 <= 64 * 1024
    if force == "direct":
        return None if not fits else LDS if lds else GLOBAL
    if force == "global":
        return None if not fits else GLOBAL
    if force == "hash":
        return HASH
    if not fits or product > max(1 << 16, 4 * live_rows):
        return HASH
    return LDS if lds else GLOBAL


def slots_for(live_rows, product, asked=0):
    def pow2(x):
        s = 1
        while s < x and s < MAX_CELLS:
            s <<= 1
        return s
    if asked > 0:
        return pow2(asked)
    return max(64, pow2(2 * min(live_rows, product)))


def rollup_ref(blocks, groups=(), aggs=(), filters=(), time_col=None, time_bucket=0, count_name="count", block_rows=0,
               compact=False, force=None, slots=0):
    """{"columns": [(name, type)], "blocks": the output as blocks of the same form, "storage": {new column: (width, base)},
    "bitmap": {column: bool}, "dicts": {str key: dictionary}, "stats": the counts of sybl_rollup_stats}."""
    assert 0 <= block_rows <= BLOCK_ROWS and time_bucket >= 0
    br = block_rows or BLOCK_ROWS
    live = [b for b in blocks if b[0] > 0]
    types = D.column_types(blocks)
    cols = D.concat(live)
    N = sum(b[0] for b in live)
    groups = list(groups)
    pairs = [(c, parse_ops(o)) for c, o in agg_pairs(aggs)]
    assert len(groups) <= 4 and len(set(groups)) == len(groups) and len(pairs) <= 8
    tname = (time_col or "time") if time_bucket > 0 else None
    if tname is not None:
        assert types[tname] == "int"
    for g in groups:
        assert types[g] in ("int", "str"), g
    for c, _ in pairs:
        assert types[c] == "int", c

    # ---- the output's columns
    names = ([(tname, "int")] if tname else []) + [(g, types[g]) for g in groups] + [(count_name or "count", "int")]
    for c, ops in pairs:
        names += [("%s_%s" % (c, o), "int") for o in ops]
    assert len(set(n for n, _ in names)) == len(names), "a name collides"
    dicts = {g: C.table_dict(blocks, g) for g in groups if types[g] == "str"}

    # ---- every key column as integers (dictionary ids for str) and its populated bits, over the live rows
    def ints_of(name):
        ty, v, p = cols[name] if N else (types[name], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool))
        if ty == "int":
            return [int(x) for x in v.tolist()], p.tolist()
        ix = {s: i for i, s in enumerate(dicts[name])}
        return [ix[s] if s is not None else 0 for s in v], p.tolist()

    # ---- the plan: radices from the extrema of the WHOLE table, the composite's size, the path
    fields = 1 + 4 * len(pairs)
    product = 1
    keys = []
    if tname:
        v, p = ints_of(tname)
        pv = [x for x, ok in zip(v, p) if ok]
        product *= max(1, trunc_div(max(pv), time_bucket) - trunc_div(min(pv), time_bucket) + 1 if pv else 0)
        keys.append((v, p))
    for g in groups:
        v, p = ints_of(g)
        pv = [x for x, ok in zip(v, p) if ok]
        # the MISSING digit: where the column has a bitmap.  A table built block by block has one iff a row is unpopulated; a
        # derived table says which of its columns have one (tests/chain_ref.py: Blocks.bitmap), unpopulated rows or not
        digit = getattr(blocks, "bitmap", {}).get(g, not (all(p) and N))
        product *= max(1, (max(pv) - min(pv) + 1 if pv else 0) + (1 if digit else 0))
        keys.append((v, p))
    stats = dict(rows_in=N, rows_matched=0, rows_no_time=0, groups=0, blocks_out=0, path=0, fields=fields, cells_or_slots=0)
    out = dict(columns=names, blocks=[], storage={}, bitmap={n: False for n, _ in names}, dicts=dicts, stats=stats, product=product)
    new_cols = [n for n, _ in names if n not in groups]
    for n in new_cols:
        out["storage"][n] = (1, 0) if compact else (8, 0)
    if product > (1 << 62):
        raise OverflowError("the composite key exceeds 2^62")
    if N == 0:
        return out

    match = np.concatenate([R.block_matches(b, filters) for b in live]).tolist()
    stats["rows_matched"] = sum(match)
    path = choose_path(product, N, fields, force)
    assert path is not None, "direct forced beyond 2^27 cells"
    stats["path"] = path
    stats["cells_or_slots"] = slots_for(N, product, slots) if path == HASH else product

    # ---- accumulate: key -> [count, per aggregated column [n, sum, min, max]].  A key part is (0, 0) when unpopulated -- before
    # every value -- and (1, value) otherwise.
    avals = [ints_of(c) for c, _ in pairs]
    cells = {}
    for r in range(N):
        if not match[r]:
            continue
        key = []
        k0 = 0
        if tname:
            if not keys[0][1][r]:
                stats["rows_no_time"] += 1
                continue
            key.append((1, trunc_div(keys[0][0][r], time_bucket) * time_bucket))
            k0 = 1
        for v, p in keys[k0:]:
            key.append((1, v[r]) if p[r] else (0, 0))
        cell = cells.setdefault(tuple(key), [0] + [[0, 0, None, None] for _ in pairs])
        cell[0] += 1
        for a, (v, p) in enumerate(avals):
            if p[r]:
                f = cell[1 + a]
                f[0] += 1
                f[1] += v[r]
                f[2] = v[r] if f[2] is None else min(f[2], v[r])
                f[3] = v[r] if f[3] is None else max(f[3], v[r])
    order = sorted(cells)
    G = len(order)
    stats["groups"] = G
    if path == HASH and not slots:
        assert G <= stats["cells_or_slots"]
    if G == 0:
        return out

    # ---- the output's values: (values, populated) per column
    table = {}
    k = 0
    if tname:
        table[tname] = ([key[0][1] for key in order], [True] * G)
        k = 1
    for i, g in enumerate(groups):
        table[g] = ([key[k + i][1] for key in order], [bool(key[k + i][0]) for key in order])
    table[count_name or "count"] = ([cells[key][0] for key in order], [True] * G)
    for a, (c, ops) in enumerate(pairs):
        for o in ops:
            f = OPS.index(o)
            if o == "n":
                table["%s_n" % c] = ([cells[key][1 + a][0] for key in order], [True] * G)
            else:
                pop = [cells[key][1 + a][0] > 0 for key in order]
                vals = [wrap(cells[key][1 + a][f]) if ok else 0 for key, ok in zip(order, pop)]
                table["%s_%s" % (c, o)] = (vals, pop)
    for n, _ in names:
        v, p = table[n]
        out["bitmap"][n] = not all(p)
        if n in new_cols:
            pv = [x for x, ok in zip(v, p) if ok]
            out["storage"][n] = (C.storage_of(min(pv), max(pv), "int") if pv else (1, 0)) if compact else (8, 0)
    for r0 in range(0, G, br):
        n = min(br, G - r0)
        bc = {}
        for name, ty in names:
            v, p = table[name]
            if ty == "int":
                bc[name] = ("int", np.array(v[r0:r0 + n], dtype=np.int64), np.array(p[r0:r0 + n], dtype=bool))
            else:
                bc[name] = ("str", [dicts[name][x] if ok else None for x, ok in zip(v[r0:r0 + n], p[r0:r0 + n])])
        out["blocks"].append((n, bc))
    stats["blocks_out"] = len(out["blocks"])
    return out
