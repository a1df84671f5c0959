"""CPU model of exact percentiles (executeQueryQuantilesHIP / HipEngine.quantiles; SQL's PERCENTILE_DISC): the selection's
values sorted with numpy and indexed at the rank k = max(ceil(p n / 10^6) - 1, 0), p in parts per million, per group.  The
rank is Python integer arithmetic.  radix_select is the host half of the engine's algorithm with numpy histograms standing
in for the kernel (it calls only the pure helpers hipQuantileDigitBits and hipQuantilePick).  Nothing here calls the engine."""
import numpy as np

import qpelib as q
import test_gpu_order_by as order

pq = q.pq
PPM = 1_000_000


def rank(n, ppm):
    """0-based rank of the fraction ppm / 10^6 among n sorted values."""
    return max(-((-ppm * n) // PPM) - 1, 0)


def pick(values, ppm_list):
    """The elements of `values` (any order) at the ranks of ppm_list in their ascending sort; [] for no values."""
    s = np.sort(np.asarray(values), kind="stable")
    return [s[rank(len(s), p)] for p in ppm_list] if len(s) else []


def pick_slow(values, ppm_list):
    """The same by a row-by-row loop: for every fraction the smallest value v with #(values <= v) > k."""
    vals, out = [int(v) for v in values], []
    for p in ppm_list:
        k, best = rank(len(vals), p), None
        for v in vals:
            below_or_equal = sum(1 for w in vals if w <= v)
            if below_or_equal > k and (best is None or v < best):
                best = v
        out.append(best)
    return out if vals else []


def grouped_positions(vkeys, gkeys, ppm_list):
    """vkeys[i] / gkeys[i]: the order-preserving integers of candidate i's value and group (gkeys None: one group).
    -> [(a candidate of the group, n, [the candidate at each rank]), ...] in ascending group order: positions into the input."""
    vkeys = np.asarray(vkeys)
    n = len(vkeys)
    if n == 0:
        return []
    g = np.zeros(n, np.int64) if gkeys is None else np.asarray(gkeys).astype(np.int64)
    by = np.lexsort((vkeys, g))                                  # group, then value; stable
    starts = np.flatnonzero(np.r_[True, g[by][1:] != g[by][:-1]])
    ends = np.r_[starts[1:], n]
    return [(int(by[a]), int(b - a), [int(by[a + rank(int(b - a), p)]) for p in ppm_list]) for a, b in zip(starts, ends)]


def render(column, cell):
    """A cell's text as HipEngine.quantiles returns the value."""
    kind = pq.COLUMN_KIND[pq.COL[column]]
    if kind == pq.KIND_DICT:
        return cell
    return cell == "true" if column == "sudo_used" else int(cell)


def column_expected(cm, ids, value_column, ppm_list, group_column=None):
    """HipEngine.quantiles over a ColumnModel and the rows select_ids gave (duplicates counted)."""
    rows = np.asarray(ids, dtype=np.int64)
    pos = grouped_positions(cm.codes(value_column)[rows], cm.codes(group_column)[rows] if group_column else None, ppm_list)
    return [(cm.cell(int(rows[a]), group_column) if group_column else None, n, [render(value_column, cm.cell(int(rows[i]), value_column)) for i in at])
            for a, n, at in pos]


def synth_expected(host, ids, value_column, ppm_list, group_column=None):
    """The same for a HostSynth table."""
    rows = np.asarray(ids, dtype=np.int64)
    pos = grouped_positions(order.synth_keys(host, value_column)[rows], order.synth_keys(host, group_column)[rows] if group_column else None, ppm_list)
    return [(host.cell(int(rows[a]), group_column) if group_column else None, n, [render(value_column, host.cell(int(rows[i]), value_column)) for i in at])
            for a, n, at in pos]


def digit_tables(images, tables_of, n_tables, shift, d):
    """What pqps_filter_digit_hist counts: images[i] (Python ints or uint64) into table tables_of[i] (-1: left out)."""
    out = np.zeros((n_tables, 1 << d), dtype=np.uint64)
    for img, t in zip(images, tables_of):
        if t >= 0:
            out[t, (int(img) >> shift) & ((1 << d) - 1)] += 1
    return out


def radix_select(images, key_bits, ppm_list, tables=1):
    """The engine's select over ONE group of key images below 2^key_bits (Python ints): -> (n, [image per fraction], passes).
    `tables`: what the launch would count beside this group (moves the digit width as a group column does)."""
    images = [int(x) for x in images]
    n = len(images)
    assert all(0 <= x < (1 << key_bits) for x in images)
    if n == 0:
        return 0, [], 0
    ranks, slots, prefixes, left, passes = [rank(n, p) for p in ppm_list], [0] * len(ppm_list), None, key_bits, 0
    while left:
        n_slots = len(prefixes) if prefixes is not None else 1
        d = pq.quantile_digit_bits(left, key_bits, tables * n_slots)
        assert 1 <= d <= min(left, 11)
        shift = left - d
        where = {p: j for j, p in enumerate(prefixes)} if prefixes is not None else None
        of = [0 if where is None else where.get(x >> (shift + d), -1) for x in images]
        t = digit_tables(images, of, n_slots, shift, d)
        digits, ranks, prefixes, slots = pq.quantile_pick(t.tolist(), d, prefixes, list(zip(ranks, slots)))
        assert prefixes == sorted(set(prefixes)) and len(digits) == len(ppm_list)
        left, passes = shift, passes + 1
    return n, [prefixes[s] for s in slots], passes
