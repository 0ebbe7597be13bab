"""Python restatement of a table rollup with percentiles (the p<k> tokens of sybl_rollup_agg.ops), written from the
definition in include/sybilgpu.h ("rollup", "percentiles") and not from the library: the checker of
tests/test_gpu_rollup_pct.py, itself checked by tests/test_rollup_pct_ref.py.

It strips the percentile tokens, lets tests/rollup_ref.py restate everything else, and splices brute-force columns (Python
`sorted`, nearest rank) into that output at the places the definition gives them: after the column's _n, _sum, _min, _max, in
ascending k.  It also restates the host plan of the sort (csrc/rollup_plan.h): the bits of the cell and of the value span, and
the variant they select.
"""
import re

import numpy as np

from tests import concat_ref as C
from tests import digest_ref as D
from tests import rollup_ref as U
from tests import samples_ref as R

MAX_PCTS = 8
V32, V64, PAIRS = 1, 2, 3
FORCE = {None: 0, "32": V32, "64": V64, "pairs": PAIRS}


def split_ops(ops):
    """(the tokens among n, sum, min, max as given, the percentile ks ascending).  ValueError for anything the header refuses."""
    toks = ops.split(",") if ops else []
    base, ks = [], []
    for tok in toks:
        if tok in U.OPS:
            base.append(tok)
            continue
        m = re.fullmatch(r"p([1-9][0-9]?)", tok)
        if not m or int(m.group(1)) in ks:
            raise ValueError("ops '%s'" % ops)
        ks.append(int(m.group(1)))
    if not toks or len(ks) > MAX_PCTS or len(set(base)) != len(base):
        raise ValueError("ops '%s'" % ops)
    return base, sorted(ks)


def nearest_rank(values, k):
    """p<k> of a non-empty list: the element of 1-based rank ceil(k * n / 100) in ascending order."""
    s = sorted(values)
    return s[(k * len(s) + 99) // 100 - 1]


def plan(n_cells, lo, hi, force=None):
    """(cbits, vbits, variant) of a column whose populated values span [lo, hi]; variant None: the forced one does not fit."""
    cbits = (n_cells - 1).bit_length()
    vbits = (hi - lo).bit_length()
    fit = V32 if cbits + vbits <= 32 else V64 if cbits + vbits <= 64 else PAIRS
    f = FORCE[force]
    return cbits, vbits, (fit if f == 0 else f if f >= fit else None)


def rollup_pct_ref(blocks, groups=(), aggs=(), filters=(), time_col=None, time_bucket=0, count_name="count", block_rows=0,
                   compact=False, force=None, slots=0, pct_force=None):
    """rollup_ref's dictionary with the percentile columns spliced in, and "pct_stats": the counts of sybl_rollup_pct_stats."""
    pairs = [(c, split_ops(o)) for c, o in U.agg_pairs(aggs)]
    groups = list(groups)
    # a column with percentile tokens only still has its four fields in every cell: rollup_ref is asked for its _n, taken out below
    only = [c for c, (base, ks) in pairs if not base]
    base_aggs = [(c, ",".join(base) if base else "n") for c, (base, ks) in pairs]
    tname = (time_col or "time") if time_bucket > 0 else None
    final = ([tname] if tname else []) + groups + [count_name or "count"]
    for c, (base, ks) in pairs:
        final += ["%s_%s" % (c, o) for o in U.OPS if o in base] + ["%s_p%d" % (c, k) for k in ks]
    assert len(set(final)) == len(final), "a name collides"
    for c in only:
        assert final.count("%s_n" % c) == 0
    out = U.rollup_ref(blocks, groups=groups, aggs=base_aggs, filters=filters, time_col=time_col, time_bucket=time_bucket,
                       count_name=count_name, block_rows=block_rows, compact=compact, force=force, slots=slots)
    stats = dict(columns=sum(1 for _, (_, ks) in pairs if ks), percentiles=sum(len(ks) for _, (_, ks) in pairs), variant32=0,
                 variant64=0, variant_pairs=0, key_bits_max=0, items=0)
    out["pct_stats"] = stats
    G = out["stats"]["groups"]

    # ---- the groups' values, by the key rollup_ref orders by
    live = [b for b in blocks if b[0] > 0]
    N = sum(b[0] for b in live)
    cols = D.concat(live) if N else {}
    values = {c: {} for c, (_, ks) in pairs if ks}
    order = []
    if G:
        match = np.concatenate([R.block_matches(b, filters) for b in live]).tolist()

        def ints_of(name):
            ty, v, p = cols[name]
            if ty == "int":
                return [int(x) for x in v.tolist()], p.tolist()
            ix = {s: i for i, s in enumerate(C.table_dict(blocks, name))}
            return [ix[s] if s is not None else 0 for s in v], p.tolist()
        tk = ints_of(tname) if tname else None
        gk = [ints_of(g) for g in groups]
        av = {c: ints_of(c) for c in values}
        seen = set()
        for r in range(N):
            if not match[r] or (tk and not tk[1][r]):
                continue
            key = ([(1, U.trunc_div(tk[0][r], time_bucket) * time_bucket)] if tk else []) + [(1, v[r]) if p[r] else (0, 0) for v, p in gk]
            key = tuple(key)
            seen.add(key)
            for c, (v, p) in av.items():
                if p[r]:
                    values[c].setdefault(key, []).append(v[r])
        order = sorted(seen)
        assert len(order) == G

    # ---- splice: names, storage, bitmaps, blocks
    ty_of = dict(out["columns"])
    names = [(n, ty_of.get(n, "int")) for n in final]
    table = {}
    for c, (base, ks) in pairs:
        for k in ks:
            name = "%s_p%d" % (c, k)
            pop = [key in values[c] for key in order]
            vals = [nearest_rank(values[c][key], k) if ok else 0 for key, ok in zip(order, pop)]
            table[name] = (vals, pop)
            out["bitmap"][name] = not all(pop)
            pv = [x for x, ok in zip(vals, pop) if ok]
            out["storage"][name] = ((C.storage_of(min(pv), max(pv), "int") if pv else (1, 0)) if compact else (8, 0))
    for c in only:
        out["bitmap"].pop("%s_n" % c, None)
        out["storage"].pop("%s_n" % c, None)
    out["columns"] = names
    br = block_rows or U.BLOCK_ROWS
    spliced = []
    for j, (n, bc) in enumerate(out["blocks"]):
        r0 = j * br
        nb = {}
        for name, _ in names:
            if name in table:
                v, p = table[name]
                nb[name] = ("int", np.array(v[r0:r0 + n], dtype=np.int64), np.array(p[r0:r0 + n], dtype=bool))
            else:
                nb[name] = bc[name]
        spliced.append((n, nb))
    out["blocks"] = spliced

    # ---- the plan of the sorts that run: a column is sorted iff one of its values passed
    if G:
        n_cells = out["stats"]["cells_or_slots"]
        for c in values:
            items = sum(len(v) for v in values[c].values())
            ty, v, p = cols[c]
            if not p.any():
                continue
            cbits, vbits, variant = plan(n_cells, int(v[p].min()), int(v[p].max()), pct_force)
            assert variant is not None, "the forced variant does not hold the bits"
            if items == 0:
                continue
            stats["items"] += items
            stats["key_bits_max"] = max(stats["key_bits_max"], cbits + vbits)
            stats[{V32: "variant32", V64: "variant64", PAIRS: "variant_pairs"}[variant]] += 1
    return out
