"""CPU model of "the first row of every group" (executeQueryGroupFirstHIP / pqps_filter_group_first): among candidate rows,
per group, the row that comes first by (key ascending or descending, row ascending).  numpy lexsort((row, key image)) inside
every group; a brute-force loop of the same rule for the self-test; the device's word layout packed and unpacked in plain
Python ints.  Nothing here calls the engine."""
import numpy as np

import qpelib as q
import test_gpu_group_count as grp
import test_gpu_order_by as order

U32 = 0xFFFFFFFF
U64 = (1 << 64) - 1
EMPTY = U64                                               # the word of a bin without rows
KIND_U64, KIND_I32, KIND_BOOL, KIND_DICT = 0, 1, 2, 3       # HIPKIND_* of include/hipPredicate.h


def key_image(keys, descending):
    """An array whose ASCENDING order is the wanted key order: uint64 keys are complemented, everything else negated."""
    k = np.asarray(keys)
    if not descending:
        return k
    return ~k if k.dtype == np.uint64 else -k.astype(np.int64)


def first_rows(rows, keys, groups, descending):
    """rows[i] a candidate table row (the same row may be listed more than once), keys[i] its order key (integers whose
    numeric order is the column's), groups[i] its group (integers in key order; None: one group).
    -> (group values ascending, the first row of each, that row's key), three arrays."""
    rows = np.asarray(rows, dtype=np.int64)
    keys = np.asarray(keys)
    g = np.zeros(len(rows), np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    if len(rows) == 0:
        return g[:0], rows[:0], keys[:0]
    pick = []
    for value in np.unique(g):
        members = np.flatnonzero(g == value)
        img = key_image(keys[members], descending)
        pick.append(members[np.lexsort((rows[members], img))[0]])
    pick = np.array(pick)
    return g[pick], rows[pick], keys[pick]


def first_rows_fast(rows, keys, groups, descending):
    """first_rows with one lexsort over (group, key image, row): for the tables of a million rows."""
    rows = np.asarray(rows, dtype=np.int64)
    keys = np.asarray(keys)
    g = np.zeros(len(rows), np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    if len(rows) == 0:
        return g[:0], rows[:0], keys[:0]
    by = np.lexsort((rows, key_image(keys, descending), g))
    head = by[np.r_[True, g[by][1:] != g[by][:-1]]]
    return g[head], rows[head], keys[head]


def first_rows_slow(rows, keys, groups, descending):
    """The same rule, row by row in Python ints: {group: (row, key)}."""
    best = {}
    for i, (r, k) in enumerate(zip(rows, keys)):
        r, k = int(r), int(k)
        grp_ = 0 if groups is None else int(groups[i])
        if grp_ not in best:
            best[grp_] = (r, k)
            continue
        br, bk = best[grp_]
        better = (k > bk) if descending else (k < bk)
        if better or (k == bk and r < br):
            best[grp_] = (r, k)
    return best


# ---- the device's words ------------------------------------------------------------------------------------------------
def pack_word(kind, descending, key, row):
    """(img ^ x) << 32 | row of include/pqps_hip.h for a narrow key: i32 signed, otherwise the code or the bool."""
    img = (int(key) ^ 0x80000000) & U32 if kind == KIND_I32 else int(key) & U32
    if descending:
        img ^= U32
    return (img << 32) | int(row)


def unpack_word(kind, descending, word):
    """None for the empty word, else (key, row)."""
    if word == EMPTY:
        return None
    img = word >> 32
    if descending:
        img ^= U32
    if kind == KIND_I32:
        img ^= 0x80000000
        img = img - (1 << 32) if img >= 1 << 31 else img
    return img, word & U32


def expected_words(n_bins, kind, descending, rows, keys, bins, row_base=0):
    """out[0 .. n_bins) of pqps_filter_group_first for narrow keys (uint64 array); candidates with a bin >= n_bins left out."""
    out = np.full(n_bins, EMPTY, dtype=np.uint64)
    rows, keys = np.asarray(rows, np.int64), np.asarray(keys)
    bins = np.zeros(len(rows), np.int64) if bins is None else np.asarray(bins).astype(np.int64)
    keep = bins < n_bins
    g, r, k = first_rows_fast(rows[keep], keys[keep], bins[keep], descending)
    for b, row, key in zip(g.tolist(), r.tolist(), k.tolist()):
        out[b] = pack_word(kind, descending, key, row + row_base)
    return out


def expected_wide(n_bins, descending, rows, keys, bins, row_base=0):
    """(out, best) of the two-pass form for u64 keys: out[b] = the row, best[b] = key ^ x; best means nothing where out is empty."""
    out = np.full(n_bins, EMPTY, dtype=np.uint64)
    best = np.full(n_bins, EMPTY, dtype=np.uint64)
    rows, keys = np.asarray(rows, np.int64), np.asarray(keys, np.uint64)
    bins = np.zeros(len(rows), np.int64) if bins is None else np.asarray(bins).astype(np.int64)
    keep = bins < n_bins
    g, r, k = first_rows_fast(rows[keep], keys[keep], bins[keep], descending)
    for b, row, key in zip(g.tolist(), r.tolist(), k.tolist()):
        out[b] = row + row_base
        best[b] = int(key) ^ (U64 if descending else 0)
    return out, best


# ---- engine-level expectations -------------------------------------------------------------------------------------------
def ranks(values, key):
    """values (any hashable) -> int64 ranks in the order of key(value)."""
    table = {v: i for i, v in enumerate(sorted(set(values), key=key))}
    return np.array([table[v] for v in values], dtype=np.int64)


class CsvModel:
    """The cells of a CSV through the oracle, once per column: texts, and integer ranks in the engine's key order."""

    def __init__(self, orc):
        self.orc, self.text, self.rank = orc, {}, {}

    def column(self, name):
        if name not in self.text:
            self.text[name] = [self.orc.cell(r, name) for r in range(self.orc.n)]
            self.rank[name] = ranks(self.text[name], lambda t: order.cell_key(name, t))
        return self.text[name], self.rank[name]

    def expected(self, ids, group_column, order_column, descending):
        """group_first()'s `groups` for the candidate rows `ids` (select_ids' answer, duplicates and all)."""
        ids = np.asarray(ids, dtype=np.int64)
        otext, orank = self.column(order_column)
        gtext, grank = self.column(group_column) if group_column else (None, None)
        _, rows, _ = first_rows(ids, orank[ids], grank[ids] if group_column else None, descending)
        return [(gtext[r] if group_column else None, r, otext[r]) for r in rows.tolist()]


def synth_expected(host, ids, group_column, order_column, descending):
    """The same for a HostSynth table (dictionary codes turned into ranks of their words)."""
    ids = np.asarray(ids, dtype=np.int64)
    okeys = order.synth_keys(host, order_column)[ids]
    gkeys = order.synth_keys(host, group_column)[ids] if group_column else None
    _, rows, _ = first_rows_fast(ids, okeys, gkeys, descending)
    return [(host.cell(r, group_column) if group_column else None, r, host.cell(r, order_column)) for r in rows.tolist()]


__all__ = ["q", "grp", "order", "first_rows", "first_rows_fast", "first_rows_slow", "pack_word", "unpack_word", "expected_words",
           "expected_wide", "CsvModel", "synth_expected", "ranks", "EMPTY"]
