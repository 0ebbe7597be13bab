"""numpy restatement of a samples query (`sybil query -samples`), written from the definition in include/sybilgpu.h
("samples") and not from the library: the checker of tests/test_gpu_samples.py, itself checked by tests/test_samples_ref.py.

A table is a list of blocks in resident order; a block is (nrows, {column: spec}) with spec one of
    ("int", values[nrows], populated[nrows] or None)
    ("str", [str or None] * nrows)                       None = unpopulated
    ("set", [list of str or None] * nrows)               None = unpopulated, [] = populated and empty
A column missing from a block's dict is unpopulated for the whole block.  Filters are (column, op, value) with the ops of
sybil_amd.engine: gt lt eq neq (int), eq neq re nre (str), in nin (set); they are ANDed and an unpopulated row fails.
"""
import re

import numpy as np


def _column(block, name):
    nrows, cols = block
    spec = cols.get(name)
    if spec is None:
        return None, np.zeros(nrows, dtype=bool)
    if spec[0] == "int":
        pop = np.ones(nrows, dtype=bool) if len(spec) < 3 or spec[2] is None else np.asarray(spec[2], dtype=bool)
        return spec, pop
    return spec, np.array([v is not None for v in spec[1]], dtype=bool).reshape(nrows)


def block_matches(block, filters):
    """bool[nrows]: the rows of the block that pass every filter."""
    nrows = block[0]
    ok = np.ones(nrows, dtype=bool)
    for col, op, val in filters:
        spec, pop = _column(block, col)
        if spec is None:
            ok[:] = False
            continue
        if spec[0] == "int":
            v = np.asarray(spec[1], dtype=np.int64)
            hit = {"gt": v > val, "lt": v < val, "eq": v == val, "neq": v != val}[op]
        elif spec[0] == "str":
            if op in ("eq", "neq"):
                hit = np.array([(s == val) == (op == "eq") for s in spec[1]], dtype=bool)
            else:
                rx = re.compile(val)
                hit = np.array([s is not None and (rx.search(s) is not None) == (op == "re") for s in spec[1]], dtype=bool)
        else:
            hit = np.array([s is not None and (val in s) == (op == "in") for s in spec[1]], dtype=bool)
        ok &= pop & hit.reshape(nrows)
    return ok


def visited_prefix(counts, limit):
    """(P, M): the smallest p >= 1 with counts[0] + .. + counts[p-1] > limit (else all blocks), and the matches in it."""
    total = 0
    for p, m in enumerate(counts):
        total += int(m)
        if total > limit:
            return p + 1, total
    return len(counts), total


def _row(blocks, b, r, columns):
    out = {}
    for name in columns:
        spec, pop = _column(blocks[b], name)
        if spec is None or not pop[r]:
            continue
        v = spec[1][r]
        out[name] = int(v) if spec[0] == "int" else (str(v) if spec[0] == "str" else [str(x) for x in v])
    return out


def all_columns(blocks):
    names = []
    for _, cols in blocks:
        for n in cols:
            if n not in names:
                names.append(n)
    return names


def samples_ref(blocks, filters=(), columns=None, order_by="$COUNT", order_asc=False, limit=100):
    assert limit >= 0
    if columns is None:
        columns = all_columns(blocks)
    match = [block_matches(b, filters) for b in blocks]
    P, M = visited_prefix([int(m.sum()) for m in match], limit)
    base = np.concatenate([[0], np.cumsum([b[0] for b in blocks])]).astype(np.int64)
    # candidates in ascending logical row order: (block, row in block, logical row)
    cand = [(b, int(r), int(base[b] + r)) for b in range(P) for r in np.nonzero(match[b])[0]]
    assert len(cand) == M
    L = min(limit, M)
    if order_by in (None, "", "$COUNT"):
        picked = cand[::-1][:L]
    else:
        def key(c):
            spec, pop = _column(blocks[c[0]], order_by)
            assert spec is None or spec[0] == "int", "only int columns order samples"
            has = spec is not None and bool(pop[c[1]])
            # rows without the column first; then value descending; ties (and the rows without it) by descending row
            return (1, -int(spec[1][c[1]]), -c[2]) if has else (0, 0, -c[2])
        D = sorted(cand, key=key)
        picked = (D[::-1] if order_asc else D)[:L]
    return {"rows": [_row(blocks, b, r, columns) for b, r, _ in picked], "row_ids": [g for _, _, g in picked],
            "matched": M, "blocks_visited": P}
