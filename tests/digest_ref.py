"""numpy restatement of a table digest (Table.digest / sybl_table_digest), written from the definition in
include/sybilgpu.h ("digest") and not from the library: the checker of tests/test_gpu_digest.py, itself checked by
tests/test_digest_ref.py.

A table is a list of blocks in the form tests/samples_ref.py uses: (nrows, {column: spec}) with spec one of
    ("int", values[nrows], populated[nrows] or None)
    ("str", [str or None] * nrows)
    ("set", [list of str or None] * nrows)
A column missing from a block's dict is unpopulated for the whole block.  Blocks of zero rows contribute nothing.
"""
import numpy as np

BLOCK_ROWS = 65536  # CHUNK_SIZE, table.go:44


def column_types(blocks):
    types = {}
    for _, cols in blocks:
        for name, spec in cols.items():
            types.setdefault(name, spec[0])
    return types


def concat(blocks):
    """{column: (type, values, populated)} over the rows of every block in order.  int: int64 array (0 where unpopulated);
    str / set: a list with None where unpopulated."""
    types = column_types(blocks)
    out = {}
    for name, ty in types.items():
        vals, pops = [], []
        for nrows, cols in blocks:
            spec = cols.get(name)
            if ty == "int":
                if spec is None:
                    v, p = np.zeros(nrows, dtype=np.int64), np.zeros(nrows, dtype=bool)
                else:
                    v = np.asarray(spec[1], dtype=np.int64).reshape(nrows)
                    p = np.ones(nrows, dtype=bool) if len(spec) < 3 or spec[2] is None else np.asarray(spec[2], dtype=bool).reshape(nrows)
                vals.append(np.where(p, v, 0))
                pops.append(p)
            else:
                v = [None] * nrows if spec is None else list(spec[1])
                assert len(v) == nrows
                vals.append(v)
                pops.append(np.array([x is not None for x in v], dtype=bool).reshape(nrows))
        if ty == "int":
            out[name] = (ty, np.concatenate(vals) if vals else np.zeros(0, dtype=np.int64),
                         np.concatenate(pops) if pops else np.zeros(0, dtype=bool))
        else:
            out[name] = (ty, [x for v in vals for x in v], np.concatenate(pops) if pops else np.zeros(0, dtype=bool))
    return out


def permutation(blocks, time_col="time"):
    """perm[i] = the source row (index among the rows of all blocks) of sorted row i: ascending key, stable; the key is the
    time value where populated, else 0."""
    n = sum(b[0] for b in blocks)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    cols = concat(blocks)
    if time_col not in cols:
        raise KeyError(time_col)
    ty, v, p = cols[time_col]
    assert ty == "int", "rows are ordered by an int column"
    key = np.where(p, v, 0).astype(np.int64)
    assert key.shape == (n,)
    return np.argsort(key, kind="stable")


def digest_ref(blocks, time_col="time", block_rows=0):
    """The digested table as a list of blocks of the same form (every column in every block)."""
    assert 0 <= block_rows <= BLOCK_ROWS
    br = block_rows or BLOCK_ROWS
    perm = permutation(blocks, time_col)
    cols = concat(blocks)
    n = len(perm)
    out = []
    for r0 in range(0, n, br):
        idx = perm[r0:r0 + br]
        bc = {}
        for name, (ty, v, p) in cols.items():
            if ty == "int":
                bc[name] = ("int", v[idx], p[idx])
            else:
                bc[name] = (ty, [v[i] for i in idx.tolist()])
        out.append((len(idx), bc))
    return out


def rows_of(blocks):
    """The rows of a table in order, as Table.samples shows them: {column: int | str | [str]}, unpopulated columns absent."""
    cols = concat(blocks)
    n = sum(b[0] for b in blocks)
    rows = [{} for _ in range(n)]
    for name, (ty, v, p) in cols.items():
        vv = v.tolist() if ty == "int" else v
        for i in np.nonzero(p)[0].tolist():
            rows[i][name] = vv[i] if ty != "set" else list(vv[i])
    return rows
