"""numpy / Python restatement of a table lookup (Table.lookup / sybl_table_lookup), written from the definition in
include/sybilgpu.h ("lookup") and not from the library: the checker of tests/test_gpu_lookup.py, itself checked by
tests/test_lookup_ref.py.  The reference has no join; the semantics are this project's.

A table is a list of blocks in the form of tests/digest_ref.py -- (nrows, {column: spec}), what tests.test_gpu_samples.build
takes.  A table's columns are the columns its blocks name, in first-seen order; a block of zero rows declares columns and
holds nothing.
"""
import numpy as np

from tests import concat_ref as R
from tests import digest_ref as D


class LookupError_(ValueError):
    """What the library refuses with SYBL_E_INVAL; .column is the name the message has to carry."""

    def __init__(self, msg, column):
        super().__init__(msg)
        self.column = column


def attached_columns(t_blocks, dim_blocks, key, dim_key=None, columns=None, prefix=""):
    """[(dim column, output name, type)] of the attached columns; raises LookupError_ for everything the call refuses."""
    tt, dt = D.column_types(t_blocks), D.column_types(dim_blocks)
    dkey = dim_key if dim_key else key
    if key not in tt:
        raise LookupError_("unknown key column", key)
    if dkey not in dt:
        raise LookupError_("unknown key column of dim", dkey)
    if tt[key] == "set":
        raise LookupError_("a set key", key)
    if dt[dkey] == "set":
        raise LookupError_("a set key", dkey)
    if tt[key] != dt[dkey]:
        raise LookupError_("mixed key types", key)
    if columns:
        src = []
        for name in columns:
            if name not in dt:
                raise LookupError_("unknown dim column", name)
            if name not in src:
                src.append(name)
    else:
        src = [name for name in dt if name != dkey]
    out = []
    for name in src:
        full = (prefix or "") + name
        if full in tt or full in [o for _, o, _ in out]:
            raise LookupError_("the output already holds the name", full)
        out.append((name, full, dt[name]))
    return out


def match_rows(t_blocks, dim_blocks, key, dim_key=None):
    """(match, dim_keys, dim_duplicates): match[r] = the index, among dim's rows in resident order, of the FIRST dim row
    whose populated key equals row r's populated key, or -1."""
    dkey = dim_key if dim_key else key
    n = sum(b[0] for b in t_blocks)
    first, populated = {}, 0
    if sum(b[0] for b in dim_blocks):
        _, dv, dp = D.concat(dim_blocks)[dkey]
        dvals = dv.tolist() if isinstance(dv, np.ndarray) else dv
        for i in np.nonzero(dp)[0].tolist():
            populated += 1
            first.setdefault(dvals[i], i)
    match = np.full(n, -1, dtype=np.int64)
    if n:
        _, tv, tp = D.concat(t_blocks)[key]
        tvals = tv.tolist() if isinstance(tv, np.ndarray) else tv
        for r in np.nonzero(tp)[0].tolist():
            match[r] = first.get(tvals[r], -1)
    return match, len(first), populated - len(first)


def lookup_ref(t_blocks, dim_blocks, key, dim_key=None, columns=None, prefix="", compact=False):
    """dict(blocks=, attached=, matched=, dim_keys=, dim_duplicates=, storage=, bitmap=, dicts=):
    blocks    the output's block list: t's non-empty blocks, each with t's columns and the attached ones
    attached  [(output name, type)] in output order
    storage   {output name: (width, base)} of the attached int / str columns (compact: the output is in compact mode)
    bitmap    {output name: bool}: the attached column has a validity bitmap
    dicts     {output name: dictionary} of the attached str / set columns: dim's, id for id"""
    att = attached_columns(t_blocks, dim_blocks, key, dim_key, columns, prefix)
    match, dim_keys, dups = match_rows(t_blocks, dim_blocks, key, dim_key)
    n, n_dim = len(match), sum(b[0] for b in dim_blocks)
    hit = match >= 0
    matched = int(hit.sum())
    dcols = D.concat(dim_blocks)
    out_cols, storage, bitmap, dicts = {}, {}, {}, {}
    for name, full, ty in att:
        _, dv, dp = dcols[name]
        dp = np.asarray(dp, dtype=bool)
        m = np.where(hit, match, 0)
        pop = hit & (dp[m] if n_dim else np.zeros(n, dtype=bool))
        if ty == "int":
            vals = np.where(pop, dv[m] if n_dim else 0, 0).astype(np.int64)
            out_cols[full] = ("int", vals, pop)
            lo, hi = (int(dv[dp].min()), int(dv[dp].max())) if dp.any() else (1, 0)
        else:
            out_cols[full] = (ty, [dv[i] if p else None for i, p in zip(m.tolist(), pop.tolist())])
            dicts[full] = R.table_dict(dim_blocks, name)
            ids = [dicts[full].index(s) for s in set(x for x, p in zip(dv, dp.tolist()) if p)] if ty == "str" else []
            lo, hi = (min(ids), max(ids)) if ids else (1, 0)
        if ty != "set":
            storage[full] = R.storage_of(lo, hi, ty) if compact else ((8, 0) if ty == "int" else (4, 0))
        bitmap[full] = bool((not dp.all()) or matched < n)
    blocks, r0 = [], 0
    for nrows, cols in t_blocks:
        if nrows <= 0:
            continue
        bc = dict(cols)
        for full, spec in out_cols.items():
            if spec[0] == "int":
                bc[full] = ("int", spec[1][r0:r0 + nrows], spec[2][r0:r0 + nrows])
            else:
                bc[full] = (spec[0], spec[1][r0:r0 + nrows])
        blocks.append((nrows, bc))
        r0 += nrows
    return dict(blocks=blocks, attached=[(full, ty) for _, full, ty in att], matched=matched, dim_keys=dim_keys,
                dim_duplicates=dups, storage=storage, bitmap=bitmap, dicts=dicts)
