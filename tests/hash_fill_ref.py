"""numpy restatements behind tests/test_gpu_hash_fill.py, written from the definitions (csrc/scan_generic.h: splitmix64,
csrc/hash_table.h: the slot of a key and linear probing) and not from the library; themselves checked by
tests/test_hash_fill_ref.py on a machine without a GPU.

* splitmix64 / home_slots / occupied_slots / longest_run / wraps: where the keys of a linear-probing table end up.  The SET
  of occupied slots does not depend on the order the keys were inserted in (only who sits where does), so the length of
  the longest walk any insertion order can take is a property of the key set: the longest run of occupied slots.
* key_values / cyclic_column: key columns in which every window of S rows holds each of K keys at least S // K times.
* group_ref: an exact group-by (count, sum, min, max) in int64, shown not to wrap.
"""
import numpy as np

MASK64 = (1 << 64) - 1


def splitmix64(x):
    """The finalizer of SplitMix64 (Steele, Lea, Flood 2014; Vigna's splitmix64.c: next() with the state x), elementwise
    on uint64, arithmetic mod 2^64."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def home_slots(keys, slots):
    """The slot a key's probe sequence starts at in a table of `slots` (a power of two) slots: the high half of the hash."""
    assert slots > 0 and slots & (slots - 1) == 0
    return ((splitmix64(keys) >> np.uint64(32)) & np.uint64(slots - 1)).astype(np.int64)


def occupied_slots(keys, slots):
    """bool[slots]: the slots taken once every one of the DISTINCT keys is in the table (h, h + 1, ... mod slots until a free
    one), whatever the insertion order.  Slot s is taken iff keys are waiting there: those whose home it is and those pushed
    on from s - 1.  carry(s + 1) = max(carry(s) + homes(s) - 1, 0); two rounds, the second starting from the carry that
    comes round the table end (exact once a free slot has been passed, and there is one while keys < slots)."""
    keys = np.asarray(keys, dtype=np.uint64)
    assert np.unique(keys).size == keys.size <= slots
    homes = np.bincount(home_slots(keys, slots), minlength=slots).tolist()
    occ = np.zeros(slots, dtype=bool)
    carry = 0
    for rnd in range(2):
        for s in range(slots):
            waiting = carry + homes[s]
            occ[s] = waiting > 0
            carry = max(waiting - 1, 0)
    assert int(occ.sum()) == keys.size
    return occ


def longest_run(occ):
    """The longest cyclic run of True in occ (len(occ) when every slot is taken)."""
    occ = np.asarray(occ, dtype=bool)
    if occ.all():
        return occ.size
    first_free = int(np.flatnonzero(~occ)[0])
    o = np.roll(occ, -first_free)          # starts at a free slot: no run crosses the end any more
    edges = np.flatnonzero(np.diff(np.r_[False, o, False].astype(np.int8)))
    return int((edges[1::2] - edges[0::2]).max()) if edges.size else 0


def wraps(occ):
    """A run of occupied slots crosses slot len(occ) - 1 -> 0: some key's walk went through (h + 1) & mask == 0."""
    return bool(occ[-1] and occ[0])


def key_values(k, seed, space=65536):
    """k distinct key values out of [0, space), 0 and space - 1 among them, in a seeded random order."""
    assert 2 <= k <= space
    rng = np.random.default_rng(seed)
    inner = 1 + rng.choice(space - 2, k - 2, replace=False)
    return rng.permutation(np.r_[0, space - 1, inner]).astype(np.int64)


def cyclic_column(values, n):
    """column[i] = values[i mod K]: any window of S consecutive rows holds every one of the K values at least S // K times."""
    values = np.asarray(values, dtype=np.int64)
    return values[np.arange(n, dtype=np.int64) % values.size]


def group_ref(key, val=None, keep=None):
    """{key: (count, sum, min, max)} of val per key over the rows where keep (all of them if None), exact: counts with
    bincount, the rest over a stable sort by key with reduceat -- int64 throughout, and shown not to wrap.  Without val:
    {key: (count, 0, 0, 0)}.  Keys in [0, 2^31)."""
    key = np.asarray(key, dtype=np.int64)
    val = np.zeros(key.size, dtype=np.int64) if val is None else np.asarray(val, dtype=np.int64)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        key, val = key[keep], val[keep]
    if key.size == 0:
        return {}
    assert 0 <= int(key.min()) and int(key.max()) < 1 << 31
    cnt = np.bincount(key, minlength=int(key.max()) + 1)
    assert int(cnt.max()) * max(abs(int(val.min())), abs(int(val.max())), 1) < 1 << 63   # no per-group sum can wrap int64
    # (a stable sort of 16-bit keys is a radix sort: several times faster on the millions of rows of the GPU tests)
    order = np.argsort(key.astype(np.uint16) if int(key.max()) < 65536 else key, kind="stable")
    ks, vs = key[order], val[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    sums, mins, maxs = np.add.reduceat(vs, starts), np.minimum.reduceat(vs, starts), np.maximum.reduceat(vs, starts)
    ref = {int(k): (int(cnt[k]), int(s), int(lo), int(hi)) for k, s, lo, hi in zip(ks[starts], sums, mins, maxs)}
    assert sum(c for c, _, _, _ in ref.values()) == key.size
    return ref
