"""CPU model of "the first n rows of every group" (executeQueryGroupHeadHIP / pqps_filter_group_head): among candidate rows,
each counted once however often it is listed, per group the first n by (key ascending or descending, row ascending).  One
numpy lexsort over (group, key image, row); a row-by-row loop of the same rule for the self-test; the device's [round][bin]
word tables built on group_first_model's pack_word.  Nothing here calls the engine."""
import numpy as np

import group_first_model as m

EMPTY, U64 = m.EMPTY, m.U64


def head_rows(rows, keys, groups, descending, n):
    """rows[i] a candidate table row (the same row may be listed more than once: it counts once), keys[i] its order key
    (integers whose numeric order is the column's), groups[i] its group (integers in key order; None: one group).
    -> (group values ascending, offsets (len + 1), rows, keys): group j's rows are rows[offsets[j]:offsets[j + 1]], in order."""
    rows = np.asarray(rows, dtype=np.int64)
    keys = np.asarray(keys)
    g = np.zeros(len(rows), np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    if len(rows) == 0:
        return g[:0], np.zeros(1, np.int64), rows[:0], keys[:0]
    _, once = np.unique(rows, return_index=True)                    # repeated rows are removed first
    rows, keys, g = rows[once], keys[once], g[once]
    by = np.lexsort((rows, m.key_image(keys, descending), g))
    gs = g[by]
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    rank = np.arange(len(by)) - np.repeat(starts, np.diff(np.r_[starts, len(by)]))
    keep = by[rank < n]
    values, counts = np.unique(g[keep], return_counts=True)
    return values, np.r_[0, np.cumsum(counts)].astype(np.int64), rows[keep], keys[keep]


def head_rows_slow(rows, keys, groups, descending, n):
    """The same rule, row by row in Python ints: {group: [(row, key), ...]}."""
    seen, per = set(), {}
    for i, (r, k) in enumerate(zip(rows, keys)):
        r, k = int(r), int(k)
        if r in seen:
            continue
        seen.add(r)
        per.setdefault(0 if groups is None else int(groups[i]), []).append((r, k))
    out = {}
    for grp_, members in per.items():
        taken = []
        while members and len(taken) < n:
            best = members[0]
            for cand in members[1:]:
                better = (cand[1] > best[1]) if descending else (cand[1] < best[1])
                if better or (cand[1] == best[1] and cand[0] < best[0]):
                    best = cand
            members.remove(best)
            taken.append(best)
        out[grp_] = taken
    return out


def as_dict(values, offsets, rows, keys):
    """head_rows' answer in head_rows_slow's shape."""
    return {int(v): list(zip(rows[offsets[j]:offsets[j + 1]].tolist(), [int(k) for k in keys[offsets[j]:offsets[j + 1]]]))
            for j, v in enumerate(values.tolist())}


# ---- the device's words ------------------------------------------------------------------------------------------------
def _rounds(n_bins, n_rounds, rows, keys, bins, descending):
    """-> (bin, round, row, key) of every entry of the tables, as arrays."""
    rows, keys = np.asarray(rows, np.int64), np.asarray(keys)
    bins = np.zeros(len(rows), np.int64) if bins is None else np.asarray(bins).astype(np.int64)
    keep = bins < n_bins
    values, offsets, r, k = head_rows(rows[keep], keys[keep], bins[keep], descending, n_rounds)
    counts = np.diff(offsets)
    return np.repeat(values, counts), np.arange(len(r)) - np.repeat(offsets[:-1], counts), r, k


def pack_words(kind, descending, keys, rows):
    """group_first_model's pack_word over arrays (uint64)."""
    img = np.asarray(keys).astype(np.int64).astype(np.uint64) & np.uint64(m.U32)
    if kind == m.KIND_I32:
        img ^= np.uint64(0x80000000)
    if descending:
        img ^= np.uint64(m.U32)
    return (img << np.uint64(32)) | np.asarray(rows).astype(np.uint64)


def expected_round_words(n_bins, n_rounds, kind, descending, rows, keys, bins, row_base=0):
    """out[n_rounds][n_bins] of pqps_filter_group_head for narrow keys (uint64): candidates with a bin >= n_bins left out,
    all ones where a bin has fewer than round + 1 rows."""
    out = np.full((n_rounds, n_bins), EMPTY, dtype=np.uint64)
    b, rnd, r, k = _rounds(n_bins, n_rounds, rows, keys, bins, descending)
    out[rnd, b] = pack_words(kind, descending, k, r + row_base)
    return out


def expected_round_wide(n_bins, n_rounds, descending, rows, keys, bins, row_base=0):
    """(out, best), [n_rounds][n_bins] each, of the two-pass form for u64 keys: out = the row, best = key ^ x (best means
    nothing where out is all ones)."""
    out = np.full((n_rounds, n_bins), EMPTY, dtype=np.uint64)
    best = np.full((n_rounds, n_bins), EMPTY, dtype=np.uint64)
    b, rnd, r, k = _rounds(n_bins, n_rounds, rows, np.asarray(keys, np.uint64), bins, descending)
    out[rnd, b] = (r + row_base).astype(np.uint64)
    best[rnd, b] = k.astype(np.uint64) ^ np.uint64(U64 if descending else 0)
    return out, best


def runs_head_flags(sorted_keys, limit):
    """keep[i] = i < limit or keys[i - limit] != keys[i]: pqps_runs_head_flags as one numpy expression."""
    k = np.asarray(sorted_keys)
    i = np.arange(len(k))
    return ((i < limit) | (k[np.maximum(i - limit, 0)] != k)).astype(np.uint8)


# ---- engine-level expectations -------------------------------------------------------------------------------------------
def groups_of(values, offsets, rows, group_text, order_text):
    """group_head()'s `groups`: group_text(row) / order_text(row) give the cells (group_text None: one group)."""
    return [(group_text(int(rows[offsets[j]])) if group_text else None,
             [(int(r), order_text(int(r))) for r in rows[offsets[j]:offsets[j + 1]]]) for j in range(len(values))]


def csv_expected(model, ids, group_column, order_column, descending, n):
    """group_head()'s `groups` for the candidate rows `ids` (select_ids' answer, duplicates and all); model: a CsvModel."""
    ids = np.asarray(ids, dtype=np.int64)
    otext, orank = model.column(order_column)
    gtext, grank = model.column(group_column) if group_column else (None, None)
    values, offsets, rows, _ = head_rows(ids, orank[ids], grank[ids] if group_column else None, descending, n)
    return groups_of(values, offsets, rows, (lambda r: gtext[r]) if group_column else None, lambda r: otext[r])


def synth_expected(host, ids, group_column, order_column, descending, n):
    """The same for a HostSynth table."""
    ids = np.asarray(ids, dtype=np.int64)
    okeys = m.order.synth_keys(host, order_column)[ids]
    gkeys = m.order.synth_keys(host, group_column)[ids] if group_column else None
    values, offsets, rows, _ = head_rows(ids, okeys, gkeys, descending, n)
    return groups_of(values, offsets, rows, (lambda r: host.cell(r, group_column)) if group_column else None,
                     lambda r: host.cell(r, order_column))
