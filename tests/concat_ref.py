"""numpy restatement of a table concat (Context.concat / sybl_table_concat), written from the definition in
include/sybilgpu.h ("concat") and not from the library: the checker of tests/test_gpu_concat.py, itself checked by
tests/test_concat_ref.py.  The reference has no such call; the semantics are this project's.

A table is a list of blocks in the form of tests/digest_ref.py: (nrows, {column: spec}).  A table's columns are the columns
its blocks name, in first-seen order (what tests.test_gpu_samples.build declares).
"""
from tests import digest_ref as D

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def output_columns(tables, columns=None):
    """[(name, type)] of the output: the named columns in the order named, each once; None = the union of the tables'
    columns in first-seen order.  KeyError for a name no table holds, ValueError for one name with two types."""
    seen = {}
    for k, blocks in enumerate(tables):
        for name, ty in D.column_types(blocks).items():
            if name in seen and seen[name][0] != ty:
                raise ValueError("column %r is %s in table %d and %s in table %d" % (name, seen[name][0], seen[name][1], ty, k))
            seen.setdefault(name, (ty, k))
    if columns is None:
        return [(name, ty) for name, (ty, _) in seen.items()]
    out = []
    for name in columns:
        if name not in seen:
            raise KeyError(name)
        if name not in [n for n, _ in out]:
            out.append((name, seen[name][0]))
    return out


def concat_ref(tables, columns=None):
    """The output's block list: every table's non-empty blocks in order, holding the output columns the block has (a column
    a block lacks is unpopulated for the block, as everywhere in this form)."""
    names = [n for n, _ in output_columns(tables, columns)]
    out = []
    for blocks in tables:
        for nrows, cols in blocks:
            if nrows > 0:
                out.append((nrows, {n: cols[n] for n in names if n in cols}))
    return out


def merged_dict(dicts):
    """The output dictionary of one str / set column: the first table's id for id, then each later table's strings in its
    id order where they are new.  dicts: the dictionaries of the tables that hold the column, in table order."""
    out, ix = [], set()
    for d in dicts:
        for s in d:
            if s not in ix:
                ix.add(s)
                out.append(s)
    return out


def table_dict(blocks, name):
    """The dictionary a table built block by block holds for a str / set column: its strings in first-seen order.  A block list
    that stands for a DERIVED table (tests/chain_ref.py: Blocks) carries the dictionaries its table inherited id for id, which
    need not be in the first-seen order of its own rows; those win."""
    carried = getattr(blocks, "dicts", None)
    if carried is not None and name in carried:
        return list(carried[name])
    out = []
    for _, cols in blocks:
        spec = cols.get(name)
        for v in (spec[1] if spec else []):
            for s in ([] if v is None else [v] if spec[0] == "str" else v):
                if s not in out:
                    out.append(s)
    return out


def storage_of(lo, hi, kind):
    """(width, base) of a compact column whose values lie in [lo, hi] (lo > hi: no populated row): the narrowest of 1 / 2 / 4 /
    8 bytes that holds hi - lo, offsets from lo; the canonical width (8 for "int", 4 for "str") has base 0."""
    canon = 8 if kind == "int" else 4
    if lo > hi:
        return 1, 0
    r = hi - lo
    fit = 1 if r < 256 else 2 if r < 65536 else 4 if r < (1 << 32) else 8
    return (fit, lo) if fit < canon else (canon, 0)


def str_extrema(dicts, used):
    """(lo, hi) of a str column's ids in the output.  dicts[k]: table k's dictionary; used[k]: the strings its populated rows
    hold.  A table tracks the extrema [a, b] of its own ids; through its id table T they become min / max of T[a..b]."""
    merged = merged_dict(dicts)
    lo, hi = INT64_MAX, INT64_MIN
    for d, u in zip(dicts, used):
        ids = [d.index(s) for s in set(u)]
        if not ids:
            continue
        table = [merged.index(s) for s in d]
        span = table[min(ids):max(ids) + 1]
        lo, hi = min(lo, min(span)), max(hi, max(span))
    return lo, hi
