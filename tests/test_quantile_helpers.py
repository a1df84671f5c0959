"""The host half of exact percentiles (hipQuantileRank, hipQuantileDigitBits, hipQuantilePick; pure host code, no GPU)
through ctypes, and tests/quantile_model.py itself: the model against a row-by-row loop, the rank against Fraction arithmetic,
the pick against a cumulative sum, and the whole radix select -- numpy histograms standing in for the kernel -- against the
model."""
import math
from fractions import Fraction

import numpy as np
import pytest

import quantile_model as m

pq = m.pq
PPMS = (0, 1, 70_000, 499_999, 500_000, 500_001, 999_999, 1_000_000)


def test_model_against_a_row_by_row_loop():
    rng = np.random.default_rng(0x9A47)
    values = rng.integers(-40, 40, size=1025)
    ppm = list(PPMS) + [950_000, 333_333]
    assert [int(v) for v in m.pick(values, ppm)] == m.pick_slow(values, ppm)
    assert m.pick(values, [0])[0] == values.min() and m.pick(values, [1_000_000])[0] == values.max()
    assert m.pick(values, [500_000])[0] == np.sort(values)[512]             # the lower median of 1025
    assert m.pick(np.array([7, 3]), [500_000]) == [3] and m.pick([], [500_000]) == []
    groups = rng.integers(0, 7, size=1025)
    for a, n, at in m.grouped_positions(values, groups, ppm):
        mine = values[groups == groups[a]]
        assert n == len(mine) and [int(values[i]) for i in at] == m.pick_slow(mine, ppm)


@pytest.mark.parametrize("n", [1, 2, 3, 99, 100, 101, (1 << 32) - 2])
def test_rank_against_fractions(n):
    for p in PPMS:
        want = max(math.ceil(Fraction(p, 1_000_000) * n) - 1, 0)
        assert pq.quantile_rank(n, p) == want == m.rank(n, p), (n, p)
        assert 0 <= want < n


def test_rank_takes_no_floating_point():
    assert math.ceil(0.07 * 100) == 8                                   # what a double would have picked: rank 7
    assert pq.quantile_rank(100, 70_000) == 6
    assert pq.quantile_rank(0, 500_000) == 0 and pq.quantile_rank(5, 2_000_000) == 4


def test_fractions_as_parts_per_million():
    assert [pq.quantile_ppm(x) for x in (0, 1, 500_000, 1_000_000, 0.5, 0.07, 0.95, 1.0, 0.0, Fraction(1, 8), np.int64(7))] == \
        [0, 1, 500_000, 1_000_000, 500_000, 70_000, 950_000, 1_000_000, 0, 125_000, 7]
    for bad in (-1, 1_000_001, 1.5, -0.1, 0.12345678, Fraction(1, 3), True):
        with pytest.raises(ValueError):
            pq.quantile_ppm(bad)


def test_digit_bits_plan():
    bits = pq.quantile_digit_bits
    assert [bits(b, b, 70_000) for b in (1, 3, 11)] == [1, 3, 11]       # at most 2048 values: one pass whatever the tables
    assert [bits(12, 12, t) for t in (1, 8, 9, 64, 65, 1 << 20)] == [11, 11, 8, 8, 8, 8]
    assert bits(1, 12, 1) == 1 and bits(4, 12, 9) == 4 and bits(0, 12, 1) == 0
    assert [bits(left, 64, 1) for left in (64, 53, 42, 31, 20, 9)] == [11, 11, 11, 11, 11, 9]
    assert bits(11, 32, 9) == 8                                         # a later pass: the one-pass rule is pass 0's


def cumulative_pick(table, r):
    below = 0
    for digit, c in enumerate(table):
        if r < below + c:
            return digit, r - below
        below += c
    raise AssertionError("rank past the table")


def check_pick(tables, d, prefixes, entries):
    digits, ranks_in, nxt, slots = pq.quantile_pick(tables, d, prefixes, entries)
    want = [cumulative_pick(tables[s], r) for r, s in entries]
    assert list(zip(digits, ranks_in)) == want
    full = [((prefixes[s] if prefixes else 0) << d) | dg for (r, s), (dg, _) in zip(entries, want)]
    assert nxt == sorted(set(full)) and [nxt[i] for i in slots] == full
    return nxt


def test_pick_random_tables():
    rng = np.random.default_rng(0x91C4)
    for case in range(60):
        d, n_slots = int(rng.integers(1, 12)), int(rng.integers(1, 17))
        tables = rng.integers(0, 50, size=(n_slots, 1 << d)) * (rng.random((n_slots, 1 << d)) < 0.3)
        tables[:, int(rng.integers(0, 1 << d))] += 1                    # no empty table
        prefixes = sorted(rng.choice(1 << 20, size=n_slots, replace=False).tolist()) if case % 3 else None
        if prefixes is None:
            tables, n_slots = tables[:1], 1
        entries = []
        for _ in range(int(rng.integers(1, 17))):
            s = int(rng.integers(0, n_slots))
            entries.append((int(rng.integers(0, int(tables[s].sum()))), s))
        check_pick(tables.tolist(), d, prefixes, entries)


def test_pick_degenerate_tables():
    one = [0] * 256
    one[137] = 1000                                                     # all the mass in one digit
    assert check_pick([one], 8, None, [(0, 0), (999, 0), (500, 0)]) == [137]
    edges = [0, 5, 0, 0, 3, 0, 0, 2]                                    # first and last count of a bucket, empty ones between
    digits, ranks_in, nxt, _ = pq.quantile_pick([edges], 3, None, [(0, 0), (4, 0), (5, 0), (7, 0), (8, 0), (9, 0)])
    assert digits == [1, 1, 4, 4, 7, 7] and ranks_in == [0, 4, 0, 2, 0, 1] and nxt == [1, 4, 7]
    assert check_pick([one], 8, [3], [(k, 0) for k in range(16)]) == [(3 << 8) | 137]          # 16 fractions, one bucket
    spread = [0] * 2048
    for k in range(16):
        spread[100 * k + 7] = 2
    got = check_pick([spread], 11, [5], [(2 * (15 - k) + 1, 0) for k in range(16)])            # 16 buckets, unsorted order
    assert got == [(5 << 11) | (100 * k + 7) for k in range(16)]
    top = (1 << 53) - 1                                                 # the prefix of a 64-bit key before its last digit
    assert check_pick([[1] * 2048], 11, [top], [(2047, 0)]) == [(1 << 64) - 1]


def test_pick_refuses():
    for tables, d, prefixes, entries in (([[1, 1]], 1, None, [(2, 0)]), ([[1, 1]], 1, None, [(0, 1)]), ([[1, 1]], 0, None, [(0, 0)]),
                                         ([[1, 1]], 1, None, [(0, 0)] * 17), ([[1, 1, 1]], 1, None, [(0, 0)])):
        with pytest.raises(ValueError):
            pq.quantile_pick(tables, d, prefixes, entries)


@pytest.mark.parametrize("bits", [1, 11, 12, 22, 23, 32, 64])
def test_host_radix_select_against_the_model(bits):
    rng = np.random.default_rng([0x5E1EC7, bits])
    top = (1 << bits) - 1
    ppm = [0, 1, 500_000, 950_000, 999_999, 1_000_000, 500_000, 70_000, 333_333]
    draws = {
        "uniform": [int(x) for x in rng.integers(0, 1 << min(bits, 62), size=700)] + [0, top, top >> 1, (top >> 1) + 1 if bits > 1 else 1],
        "equal": [top] * 300,
        "two": [0] * 150 + [top] * 151,
        "one": [top >> 1],
        "clustered": [min(top, (top >> 1) + int(x)) for x in rng.integers(0, 5, size=400)],
    }
    for name, images in draws.items():
        for tables in (1, 9):
            n, got, passes = m.radix_select(images, bits, ppm, tables)
            assert n == len(images) and got == [int(v) for v in m.pick(np.array(images, dtype=object), ppm)], (bits, name, tables)
            # at most 2048 values: ONE pass; otherwise digits of 11 bits at the most, of 8 at the least (but the last)
            assert passes == 1 if bits <= 11 else math.ceil(bits / 11) <= passes <= math.ceil(bits / 8), (bits, name, tables, passes)
    assert m.radix_select([], bits, ppm) == (0, [], 0)
