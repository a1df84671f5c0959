"""hipGroupTopOrder (the ORDER BY aggregate [DESC] LIMIT n rule of the top-N groups; pure host code, no GPU) against
numpy.lexsort: every order, both directions, limits around the number of groups, ties (which go to the ascending key in both
directions), negative i32 sums, command_id images at and above 2^63, no groups at all."""
import numpy as np
import pytest

import group_top_model as gtm
import qpelib as q

pq = q.pq
U64, I32 = pq.HIPKIND_U64, pq.HIPKIND_I32
SIGN = np.uint64(1 << 63)


def groups(n, kind, seed, ties=True):
    """n groups in shuffled bin order: the arrays hipGroupTopOrder reads, and the same aggregates as plain numbers."""
    rng = np.random.default_rng([0x70B, n, seed])
    bins = rng.permutation(np.arange(3, 3 + 5 * n, 5, dtype=np.uint64))
    counts = rng.integers(1, 4 if ties else 1 << 40, n).astype(np.uint64)
    if kind == I32:
        sums = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
        lo = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64)
        hi = np.maximum(lo, rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64))
        if ties and n:
            sums[: n // 2], lo[: n // 2], hi[: n // 2] = -7, -(1 << 31), (1 << 31) - 1
        plain = {"key": bins, "count": counts, "sum": sums, "min": lo, "max": hi}
        images = (sums.view(np.uint64), lo.view(np.uint64) ^ SIGN, hi.view(np.uint64) ^ SIGN)
    else:
        sums = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        lo = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        hi = np.maximum(lo, rng.integers(0, 1 << 64, n, dtype=np.uint64))
        if n >= 4:
            sums[:4] = lo[:4] = hi[:4] = np.array([(1 << 63) - 1, 1 << 63, (1 << 64) - 1, 0], dtype=np.uint64)
        plain = {"key": bins, "count": counts, "sum": sums, "min": lo, "max": hi}
        images = (sums, lo, hi)
    return bins, counts, images, plain


def check(bins, counts, images, plain, kind, n):
    for by in gtm.BY:
        for descending in (False, True):
            for limit in sorted({1, n - 1, n, n + 1, 0, -5}):
                got = pq.group_top_order(bins, counts, *images, value_kind=kind, by=by, descending=descending, limit=limit)
                want = gtm.order(bins, plain[by], descending, limit).tolist()
                assert got == want, (by, descending, limit, n)


@pytest.mark.parametrize("kind", [I32, U64])
@pytest.mark.parametrize("n", [1, 2, 7, 200, 5000])
def test_order_matches_lexsort(kind, n):
    for ties in (True, False):
        bins, counts, images, plain = groups(n, kind, int(ties), ties)
        check(bins, counts, images, plain, kind, n)


@pytest.mark.parametrize("kind", [I32, U64])
def test_all_equal_aggregates_are_key_order_in_both_directions(kind):
    n = 300
    bins, counts, images, plain = groups(n, kind, 9)
    counts[:] = 5
    for a in images:
        a[:] = 12345
    key_order = np.argsort(bins).tolist()
    for by in ("count", "sum", "min", "max"):
        for descending in (False, True):
            for limit in (0, 1, 17, n, n + 1):
                got = pq.group_top_order(bins, counts, *images, value_kind=kind, by=by, descending=descending, limit=limit)
                assert got == key_order[: limit or n], (by, descending, limit)
    assert pq.group_top_order(bins, counts, by="key", descending=True, limit=0) == key_order[::-1]


def test_negative_sums_compare_signed_and_command_id_unsigned():
    bins = np.array([10, 11, 12, 13], dtype=np.uint64)
    counts = np.ones(4, dtype=np.uint64)
    bits = np.array([-5, 3, -(1 << 62), 0], dtype=np.int64).view(np.uint64)       # as i32 sums: 12 < 10 < 13 < 11
    assert pq.group_top_order(bins, counts, bits, value_kind=I32, by="sum", descending=False, limit=0) == [2, 0, 3, 1]
    assert pq.group_top_order(bins, counts, bits, value_kind=I32, by="sum", descending=True, limit=2) == [1, 3]
    # the same bits as command_id sums: 0 < 3 < 2^63 + 2^62 < 2^64 - 5
    assert pq.group_top_order(bins, counts, bits, value_kind=U64, by="sum", descending=False, limit=0) == [3, 1, 2, 0]
    big = np.array([1 << 63, (1 << 63) - 1, (1 << 64) - 1, 1 << 63], dtype=np.uint64)
    assert pq.group_top_order(bins, counts, None, big, big, value_kind=U64, by="max", descending=True, limit=3) == [2, 0, 3]
    assert pq.group_top_order(bins, counts, None, big, big, value_kind=U64, by="min", descending=False, limit=0) == [1, 0, 3, 2]
    # counts compare unsigned too
    counts = np.array([1 << 63, 1, (1 << 64) - 1, 2], dtype=np.uint64)
    assert pq.group_top_order(bins, counts, by="count", descending=True, limit=0) == [2, 0, 3, 1]


def test_zero_groups_and_refusals():
    empty = np.zeros(0, dtype=np.uint64)
    for by in gtm.BY:
        for limit in (0, 1, 10):
            assert pq.group_top_order(empty, empty, empty, empty, empty, value_kind=I32, by=by, limit=limit) == []
    bins = np.arange(4, dtype=np.uint64)
    for bad in (-1, 5, 99):
        with pytest.raises(pq.PqpsError):
            pq.group_top_order(bins, bins, by=bad)
    with pytest.raises(pq.PqpsError):
        pq.group_top_order(bins, bins, None, None, None, value_kind=I32, by="sum")      # the sums it orders by are missing
    with pytest.raises(pq.PqpsError):
        pq.group_top_order(bins, bins, bins, value_kind=pq.HIPKIND_DICT, by="sum")      # sums of a column that is no number
