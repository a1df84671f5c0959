"""hipHeadMerge (the shard merge of the first n rows of every group; pure host code, no GPU) through ctypes: the shards'
ascending (bin, [best,] word) lists against a sort of their union cut to n per bin."""
import numpy as np
import pytest

import qpelib as q

pq = q.pq
U64 = (1 << 64) - 1


def split(entries, n_shards, limit, how, seed=0):
    """entries: [(bin, best_or_None, word)], all different.  -> per shard the list a shard would hand: its entries in
    order, cut to `limit` per bin."""
    rng = np.random.default_rng([0x3E46E, seed, len(entries), n_shards])
    if how == "random":
        where = rng.integers(0, n_shards, len(entries))
    elif how == "last":
        where = np.full(len(entries), n_shards - 1)
    else:                                                        # "round": consecutive entries of a bin on different shards
        where = np.arange(len(entries)) % n_shards
    shards = []
    for s in range(n_shards):
        mine, kept, count = sorted(e for e, w in zip(entries, where) if w == s), [], {}
        for e in mine:
            count[e[0]] = count.get(e[0], 0) + 1
            if count[e[0]] <= limit:
                kept.append(e)
        shards.append(kept)
    return shards


def expected(entries, limit):
    out, count = [], {}
    for e in sorted(entries):
        count[e[0]] = count.get(e[0], 0) + 1
        if count[e[0]] <= limit:
            out.append(e)
    return out


def merge(shards, limit, wide):
    arg = [([e[0] for e in s], [e[2] for e in s], [e[1] for e in s] if wide else None) for s in shards]
    bins, words, best = pq.head_merge(arg, limit)
    return list(zip(bins, best if wide else [None] * len(bins), words))


def narrow_entries(seed, n_bins, n_entries):
    """Few distinct key images, so that many entries of a bin differ in the row alone."""
    rng = np.random.default_rng([7, seed])
    rows = rng.permutation(1 << 20)[:n_entries]
    return [(int(b), None, (int(k) << 32) | int(r)) for b, k, r in zip(rng.integers(0, n_bins, n_entries), rng.integers(0, 3, n_entries), rows)]


def wide_entries(seed, n_bins, n_entries):
    rng = np.random.default_rng([8, seed])
    pool = [0, 1, (1 << 63) - 1, 1 << 63, U64 - 1, U64]
    rows = rng.permutation(1 << 20)[:n_entries]
    return [(int(b), pool[int(k)], int(r)) for b, k, r in zip(rng.integers(0, n_bins, n_entries), rng.integers(0, len(pool), n_entries), rows)]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n_shards", [1, 2, 5])
@pytest.mark.parametrize("limit", [1, 2, 3, 17])
def test_merge_is_the_sorted_union_cut_per_bin(limit, n_shards, wide):
    entries = (wide_entries if wide else narrow_entries)(limit * 10 + n_shards, 9, 400) + \
              (wide_entries if wide else narrow_entries)(99, 3, 5)          # bins 0 .. 2 get a few more: below n in total elsewhere
    entries = sorted(set(entries))
    for how in ("random", "last", "round"):
        shards = split(entries, n_shards, limit, how)
        assert merge(shards, limit, wide) == expected(entries, limit), (how,)


def test_a_bin_on_one_shard_only_and_bins_below_n():
    entries = [(0, None, 5), (0, None, 9), (4, None, 1), (7, None, 3), (7, None, 2)]
    shards = [[(0, None, 5)], [(4, None, 1)], [(0, None, 9), (7, None, 2), (7, None, 3)]]
    assert merge(shards, 17, False) == sorted(entries)                      # every bin has fewer than n rows: all kept
    assert merge(shards, 1, False) == [(0, None, 5), (4, None, 1), (7, None, 2)]
    assert merge([[], [], shards[2]], 2, False) == shards[2]                # every entry on the last shard


def test_equal_keys_across_shards_are_decided_by_row():
    word = lambda key, row: (key << 32) | row
    shards = [[(3, None, word(7, 900)), (3, None, word(7, 950))], [(3, None, word(7, 10)), (3, None, word(8, 1))], [(3, None, word(7, 500))]]
    assert merge(shards, 3, False) == [(3, None, word(7, 10)), (3, None, word(7, 500)), (3, None, word(7, 900))]
    assert merge(shards, 1, False) == [(3, None, word(7, 10))]


def test_command_id_compares_best_then_row():
    """A lower row does not beat a lower key image; images at and above 2^63 compare unsigned."""
    shards = [[(0, 1 << 63, 5), (0, U64, 1)], [(0, (1 << 63) - 1, 800), (0, 1 << 63, 2)], [(1, 0, 7)]]
    assert merge(shards, 3, True) == [(0, (1 << 63) - 1, 800), (0, 1 << 63, 2), (0, 1 << 63, 5), (1, 0, 7)]
    assert merge(shards, 1, True) == [(0, (1 << 63) - 1, 800), (1, 0, 7)]


def test_nothing_to_merge_and_refusals():
    assert merge([], 3, False) == []
    assert merge([[], []], 3, False) == []
    with pytest.raises(ValueError):
        merge([[(0, None, 1)]], 0, False)
    with pytest.raises(ValueError):                                         # lists with and without best mixed
        pq.head_merge([([0], [1], None), ([0], [2], [3])], 2)
