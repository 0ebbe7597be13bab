"""numpy restatement of a table select (Table.select / sybl_table_select), written from the definition in
include/sybilgpu.h ("select") and not from the library: the checker of tests/test_gpu_select.py, itself checked by
tests/test_select_ref.py.

A table is a list of blocks in the form tests/samples_ref.py and tests/digest_ref.py use: (nrows, {column: spec}).  The
predicate is samples_ref.block_matches; the rows are concatenated and cut into blocks with digest_ref's helpers.
"""
import numpy as np

from tests import digest_ref as D
from tests import samples_ref as R

BLOCK_ROWS = D.BLOCK_ROWS


def matching_rows(blocks, filters=()):
    """The source rows (index among the rows of all blocks) that pass every filter, ascending."""
    live = [b for b in blocks if b[0] > 0]
    if not live:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(np.concatenate([R.block_matches(b, filters) for b in live]))[0].astype(np.int64)


def output_columns(blocks, columns=None):
    """The output's column names: the named ones in the order named, each once; None = every column in table order."""
    have = list(D.column_types(blocks))
    if columns is None:
        return have
    out = []
    for name in columns:
        if name not in have:
            raise KeyError(name)
        if name not in out:
            out.append(name)
    return out


def select_ref(blocks, filters=(), columns=None, block_rows=0):
    """The selected table as a list of blocks of the same form (every output column in every block)."""
    assert 0 <= block_rows <= BLOCK_ROWS
    br = block_rows or BLOCK_ROWS
    names = output_columns(blocks, columns)
    rows = matching_rows(blocks, filters)
    cols = D.concat(blocks)
    out = []
    for r0 in range(0, len(rows), br):
        idx = rows[r0:r0 + br]
        bc = {}
        for name in names:
            ty, v, p = cols[name]
            if ty == "int":
                bc[name] = ("int", v[idx], p[idx])
            else:
                bc[name] = (ty, [v[i] for i in idx.tolist()])
        out.append((len(idx), bc))
    return out
