"""The checker of tests/test_gpu_hash_fill.py (tests/hash_fill_ref.py) against definitions that do not share its code: the
published SplitMix64 sequence, a literal insertion loop, brute-force window counts and a dict loop.  No GPU."""
import numpy as np
import pytest

from tests import hash_fill_ref as H

GAMMA = 0x9E3779B97F4A7C15


def test_splitmix64_is_the_published_generator():
    """Vigna's splitmix64.c seeded with 1234567 (the sequence quoted with the algorithm, e.g. Rosetta Code "Pseudo-random
    numbers/Splitmix64"): output n is the finalizer of seed + (n - 1) * gamma, the increment being the function's first
    step.  And a Python-int restatement on random inputs, the all-ones key among them."""
    states = [(1234567 + n * GAMMA) & H.MASK64 for n in range(5)]
    assert H.splitmix64(np.array(states, dtype=np.uint64)).tolist() == [
        6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]

    def py(x):
        x = (x + GAMMA) & H.MASK64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & H.MASK64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & H.MASK64
        return x ^ (x >> 31)

    xs = [0, 1, H.MASK64, 1 << 63, (1 << 62) - 1] + np.random.default_rng(1).integers(0, 1 << 63, 200).tolist()
    assert H.splitmix64(np.array(xs, dtype=np.uint64)).tolist() == [py(x) for x in xs]
    assert H.home_slots(np.array(xs, dtype=np.uint64), 4096).tolist() == [(py(x) >> 32) & 4095 for x in xs]


def _insert_all(keys, slots):
    """hash_find_or_insert as a loop: every key walks from its home slot to the first free one.  (table, longest walk)"""
    table = [None] * slots
    longest = 0
    for k in keys:
        h = int(H.home_slots(np.array([k], dtype=np.uint64), slots)[0])
        steps = 0
        while table[h] is not None:
            h = (h + 1) & (slots - 1)
            steps += 1
            assert steps < slots
        table[h] = k
        longest = max(longest, steps + 1)
    return table, longest


def _longest_run_literal(occ):
    n = len(occ)
    if all(occ):
        return n
    best = 0
    for s in range(n):
        run = 0
        while occ[(s + run) % n]:
            run += 1
        best = max(best, run)
    return best


@pytest.mark.parametrize("n_keys", [0, 1, 20, 48, 58, 63, 64])
def test_occupied_slots_do_not_depend_on_insertion_order(n_keys):
    """A 64-slot table at loads up to 100 %, keys inserted ascending and in a shuffled order: the same slots are taken, they are
    what occupied_slots says, no walk is longer than the longest run, and longest_run / wraps agree with literal loops."""
    wrapped = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 * n_keys + seed)
        keys = np.sort(rng.choice(1 << 20, n_keys, replace=False))
        t1, walk1 = _insert_all(keys.tolist(), 64)
        t2, walk2 = _insert_all(rng.permutation(keys).tolist(), 64)
        occ1, occ2 = [x is not None for x in t1], [x is not None for x in t2]
        occ = H.occupied_slots(keys, 64)
        assert occ1 == occ2 == occ.tolist()
        run = H.longest_run(occ)
        assert run == _longest_run_literal(occ1)
        assert max(walk1, walk2) <= max(run, 1)
        assert H.wraps(occ) == (occ1[63] and occ1[0])
        wrapped += H.wraps(occ)
    if n_keys >= 48:
        assert wrapped > 0          # (the cases where a run crosses the table end are among those compared)


def test_longest_run_of_runs_that_cross_the_end():
    occ = np.zeros(16, dtype=bool)
    assert H.longest_run(occ) == 0 and not H.wraps(occ)
    occ[[14, 15, 0, 1, 2, 7, 8]] = True
    assert H.longest_run(occ) == 5 and H.wraps(occ)
    occ[:] = True
    assert H.longest_run(occ) == 16 and H.wraps(occ)
    occ[15] = False
    assert H.longest_run(occ) == 15 and not H.wraps(occ)


@pytest.mark.parametrize("k,s", [(2, 4), (7, 14), (7, 30), (64, 128), (96, 200), (100, 1000)])
def test_every_window_holds_every_key(k, s):
    """cyclic_column: every window of s rows, at every offset, holds each of the k keys at least s // k times (counted with a
    sliding bincount, not with the modulus the generator uses); key_values are k distinct values with both ends."""
    vals = H.key_values(k, seed=k, space=4096)
    assert np.unique(vals).size == k and vals.min() == 0 and vals.max() == 4095
    assert not np.array_equal(vals, np.sort(vals)) or k == 2
    n = 5 * s + 3
    col = H.cyclic_column(vals, n)
    assert col.size == n
    rank = {int(v): i for i, v in enumerate(np.sort(vals).tolist())}
    ids = np.array([rank[int(v)] for v in col.tolist()])
    counts = np.bincount(ids[:s], minlength=k)
    least = int(counts.min())
    for off in range(1, n - s + 1):
        counts[ids[off - 1]] -= 1
        counts[ids[off + s - 1]] += 1
        least = min(least, int(counts.min()))
    assert least >= s // k >= 2


def test_group_ref_is_a_dict_loop():
    rng = np.random.default_rng(5)
    n = 20_000
    key = rng.choice(np.array([0, 3, 4, 70, 65535, 1 << 20]), n)
    val = rng.integers(-(1 << 40), 1 << 40, n)
    keep = rng.random(n) < 0.5
    for key, sel in ((key, None), (key, keep), (key & 0xFFFF, keep)):     # (keys beyond 16 bits and within: both sorts)
        want = {}
        for i in range(n):
            if sel is not None and not sel[i]:
                continue
            k, v = int(key[i]), int(val[i])
            c, s, lo, hi = want.get(k, (0, 0, v, v))
            want[k] = (c + 1, s + v, min(lo, v), max(hi, v))
        assert H.group_ref(key, val, sel) == want
        assert H.group_ref(key, None, sel) == {k: (c, 0, 0, 0) for k, (c, _, _, _) in want.items()}
    assert H.group_ref(key, val, np.zeros(n, dtype=bool)) == {}
    with pytest.raises(AssertionError):          # a sum that could wrap is refused, not returned
        H.group_ref(np.zeros(4, dtype=np.int64), np.full(4, 1 << 62))
