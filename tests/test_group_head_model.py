"""tests/group_head_model.py against a row-by-row Python loop: random inputs with repeated rows, n below, at and above the
groups' sizes, both directions; n = 1 equals group_first_model's first_rows_fast; the [round][bin] word tables of the
device, narrow and wide, row by row."""
import numpy as np
import pytest

import group_first_model as m
import group_head_model as hm

NS = (1, 2, 3, 17)


def candidates(seed, n_rows, n_groups, n_keys, wide=False):
    """Random candidates with every fifth row listed twice (shuffled); group sizes from 1 to far above 17."""
    rng = np.random.default_rng([0x4EAD, seed, n_rows])
    keys_of = rng.integers(0, 1 << 64, n_rows, dtype=np.uint64) if wide else rng.integers(-n_keys, n_keys, n_rows)
    if wide and n_rows >= 4:
        keys_of[:4] = np.array([0, (1 << 63) - 1, 1 << 63, m.U64], np.uint64)
    groups_of = np.minimum(rng.integers(0, n_groups, n_rows), rng.integers(0, n_groups, n_rows))
    groups_of[: min(3, n_rows)] = np.arange(n_groups, n_groups + min(3, n_rows))          # groups of one row
    rows = rng.permutation(np.r_[np.arange(n_rows), np.arange(0, n_rows, 5)])
    return rows, keys_of[rows], groups_of[rows]


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (40, 3, 2), (500, 12, 5), (500, 60, 1000), (2000, 4, 3)])
def test_model_matches_the_loop(shape, n, descending):
    n_rows, n_groups, n_keys = shape
    for grouped in (True, False):
        rows, keys, groups = candidates(n, n_rows, n_groups, n_keys)
        g = groups if grouped else None
        values, offsets, r, k = hm.head_rows(rows, keys, g, descending, n)
        got, want = hm.as_dict(values, offsets, r, k), hm.head_rows_slow(rows, keys, g, descending, n)
        assert got == want
        assert list(got) == sorted(got)                                                  # groups in key order
        sizes = {}
        for row, grp_ in set(zip(rows.tolist(), (g if grouped else np.zeros(len(rows), int)).tolist())):
            sizes[grp_] = sizes.get(grp_, 0) + 1
        assert {grp_: len(v) for grp_, v in got.items()} == {grp_: min(n, c) for grp_, c in sizes.items()}
        assert len(set(r.tolist())) == len(r)                                            # each row at most once


def test_groups_smaller_than_n_occur():
    rows, keys, groups = candidates(17, 500, 60, 1000)
    values, offsets, _, _ = hm.head_rows(rows, keys, groups, False, 17)
    sizes = np.diff(offsets)
    assert (sizes == 1).any() and (sizes < 17).any() and (sizes == 17).any()


@pytest.mark.parametrize("descending", [False, True])
def test_one_row_is_the_first_row(descending):
    for wide in (False, True):
        rows, keys, groups = candidates(1, 3000, 40, 6, wide)
        for g in (groups, None):
            values, offsets, r, k = hm.head_rows(rows, keys, g, descending, 1)
            fv, fr, fk = m.first_rows_fast(rows, keys, g, descending)
            assert np.array_equal(values, fv) and np.array_equal(r, fr) and np.array_equal(k, fk)
            assert np.array_equal(offsets, np.arange(len(fv) + 1))


@pytest.mark.parametrize("descending", [False, True])
def test_round_words(descending):
    """Round r of bin b holds the (r + 1)-th row's word; bins past n_bins left out; round 0 = the first-row words."""
    rows, keys, groups = candidates(3, 700, 9, 4)
    n_bins, base = 7, 1000
    want = hm.head_rows_slow(rows, keys, groups, descending, 5)
    out = hm.expected_round_words(n_bins, 5, m.KIND_I32, descending, rows, keys, groups, base)
    assert out.shape == (5, n_bins)
    for b in range(n_bins):
        words = [m.pack_word(m.KIND_I32, descending, k, r + base) for r, k in want.get(b, [])]
        assert out[:, b].tolist() == words + [m.EMPTY] * (5 - len(words))
        assert words == sorted(words)                                                    # ascending words are the order
    assert np.array_equal(out[0], m.expected_words(n_bins, m.KIND_I32, descending, rows, keys, groups, base))
    rows, keys, groups = candidates(4, 700, 9, 4, wide=True)
    want = hm.head_rows_slow(rows, keys, groups, descending, 3)
    out, best = hm.expected_round_wide(n_bins, 3, descending, rows, keys, groups, base)
    for b in range(n_bins):
        have = want.get(b, [])
        assert out[:, b].tolist() == [r + base for r, _ in have] + [m.EMPTY] * (3 - len(have))
        assert best[:len(have), b].tolist() == [k ^ (m.U64 if descending else 0) for _, k in have]
    o1, b1 = m.expected_wide(n_bins, descending, rows, keys, groups, base)
    assert np.array_equal(out[0], o1) and np.array_equal(best[0][o1 != m.EMPTY], b1[o1 != m.EMPTY])


def test_run_flags():
    """keep[i] = i < limit or keys[i - limit] != keys[i] marks exactly the first `limit` of every run."""
    rng = np.random.default_rng(5)
    for limit in (1, 2, 3, 17, 5000):
        lengths = np.r_[rng.integers(1, 40, 60), [limit, limit + 1, max(limit - 1, 1), 1]]
        keys = np.repeat(np.arange(len(lengths)) * 3, lengths).astype(np.uint64)
        rank = np.concatenate([np.arange(c) for c in lengths])
        assert np.array_equal(hm.runs_head_flags(keys, limit), (rank < limit).astype(np.uint8))
    assert hm.runs_head_flags(np.zeros(0, np.uint64), 3).tolist() == []
