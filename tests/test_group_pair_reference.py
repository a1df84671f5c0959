"""The numpy reference of GROUP BY two columns that tests/test_gpu_group_pair.py compares the engine with, and its own check
(CPU, no GPU): numpy_group_pair groups the selected rows by a stable sort on (A, B) and reduces every run with reduceat;
here it is compared, on tests/golden/commands_2k.csv, with a plain-Python dict fold over OracleTable.select_ids and cell --
scan mode and index mode (rows that several probes return count as often as they occur), pairs with A == B and a swapped
pair, no value column, an i32 one and command_id."""
import numpy as np

import qpelib as q
import test_gpu_group_count as grp

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
M64 = (1 << 64) - 1
PAIRS = (("user_name", "risk_level"), ("risk_level", "user_name"), ("sudo_used", "base_command"), ("risk_level", "risk_level"),
         ("base_command", "exit_code"), ("exit_code", "sudo_used"), ("user_name", "user_name"))
VALUES = (None, "risk_level", "command_id")


def key_text(column, words=None):
    """key -> key text of a group column: the dictionary word, true / false, or the decimal number."""
    if words is not None:
        return lambda k: words[k] if isinstance(words[k], str) else words[k].decode("latin-1")
    if column == "sudo_used":
        return lambda k: "true" if k else "false"
    return lambda k: str(int(k))


def numpy_group_pair(a_keys, b_keys, a_text, b_text, values=None, unsigned=False):
    """The expected HipEngine.group_pair() list.  a_keys / b_keys: one order-preserving integer key per selected row (a row
    selected twice is there twice), a_text / b_text: key -> text, values: the value column's entries of those rows or None."""
    a, b = np.asarray(a_keys).astype(np.int64), np.asarray(b_keys).astype(np.int64)
    if len(a) == 0:
        return []
    order = np.lexsort((b, a))                                   # stable, by A, then by B
    a, b = a[order], b[order]
    head = np.ones(len(a), dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, len(a))).tolist()
    ta = {k: a_text(k) for k in np.unique(a[starts]).tolist()}
    tb = {k: b_text(k) for k in np.unique(b[starts]).tolist()}
    texts = [(ta[x], tb[y]) for x, y in zip(a[starts].tolist(), b[starts].tolist())]
    if values is None:
        return list(zip(texts, counts))
    wide = np.asarray(values).astype(np.uint64 if unsigned else np.int64)[order]
    sums, mins, maxs = np.add.reduceat(wide, starts), np.minimum.reduceat(wide, starts), np.maximum.reduceat(wide, starts)
    return list(zip(texts, counts, sums.tolist(), mins.tolist(), maxs.tolist()))


def fold_group_pair(columns, value_column, rows):
    """The same list by a dict fold.  rows: [(text of A, text of B, value or None), ...] of the selected rows."""
    acc = {}
    for ta, tb, v in rows:
        c, s, lo, hi = acc.get((ta, tb), (0, 0, None, None))
        if v is None:
            acc[(ta, tb)] = (c + 1, 0, None, None)
        else:
            acc[(ta, tb)] = (c + 1, s + v, v if lo is None else min(lo, v), v if hi is None else max(hi, v))
    keys = sorted(acc, key=lambda k: (grp.key_order(columns[0], k[0]), grp.key_order(columns[1], k[1])))
    if value_column is None:
        return [(k, acc[k][0]) for k in keys]
    wrap = (lambda s: s & M64) if value_column == "command_id" else (lambda s: s)
    return [(k, acc[k][0], wrap(acc[k][1]), acc[k][2], acc[k][3]) for k in keys]


class CsvCells:
    """The cells of the group and value columns of a CSV, read once through the oracle; order-preserving codes per column."""

    def __init__(self, orc, columns):
        self.orc = orc
        self.text = {c: [orc.cell(r, c) for r in range(orc.n)] for c in columns}
        self.words, self.code = {}, {}
        for c, cells in self.text.items():
            self.words[c] = sorted(set(cells), key=lambda t: grp.key_order(c, t))
            rank = {t: i for i, t in enumerate(self.words[c])}
            self.code[c] = np.array([rank[t] for t in cells], dtype=np.int64)

    def fold(self, ids, columns, value):
        a, b = self.text[columns[0]], self.text[columns[1]]
        v = self.text[value] if value else None
        return fold_group_pair(columns, value, [(a[r], b[r], int(v[r]) if v else None) for r in ids])

    def numpy(self, ids, columns, value):
        rows = np.asarray(ids, dtype=np.int64)
        vals = None
        if value:
            vals = np.array([int(x) for x in self.text[value]], dtype=np.uint64 if value == "command_id" else np.int64)[rows]
        return numpy_group_pair(self.code[columns[0]][rows], self.code[columns[1]][rows], key_text(None, self.words[columns[0]]),
                                key_text(None, self.words[columns[1]]), vals, value == "command_id")


def test_numpy_reference_against_dict_fold():
    chains = grp.golden_chains()
    assert len(chains) >= 20
    columns = sorted({c for p in PAIRS for c in p} | {v for v in VALUES if v})
    assert ("user_name", "risk_level") in PAIRS and ("risk_level", "user_name") in PAIRS and any(a == b for a, b in PAIRS)
    saw_duplicates = saw_empty = False
    for idx in ([], pq.DEFAULT_INDEXES):
        orc = q.OracleTable(CSV2K, idx)
        cells = CsvCells(orc, columns)
        for chain in chains[:30] + [None]:
            ids = orc.select_ids(chain)[0]
            saw_duplicates |= len(set(ids)) < len(ids)
            saw_empty |= not ids
            for pair in PAIRS:
                for value in VALUES:
                    got, want = cells.numpy(ids, pair, value), cells.fold(ids, pair, value)
                    assert got == want, (idx, chain, pair, value)
                    assert sum(g[1] for g in got) == len(ids)
                    if pair[0] == pair[1]:
                        assert all(k[0] == k[1] for k, *_ in got)
    assert saw_duplicates, "index mode must return some row twice for some chain"


def test_numpy_reference_wraps_and_orders():
    """command_id sums wrap modulo 2^64 and compare unsigned; i32 keys order numerically, not as text."""
    a = np.array([-2, 10, 9, -2, 10], dtype=np.int64)
    b = np.array([1, 0, 0, 1, 0], dtype=np.int64)
    v = np.array([M64, 5, 7, 3, 1 << 63], dtype=np.uint64)
    got = numpy_group_pair(a, b, key_text("exit_code"), key_text("sudo_used"), v, True)
    assert got == [(("-2", "true"), 2, 2, 3, M64), (("9", "false"), 1, 7, 7, 7), (("10", "false"), 2, (1 << 63) + 5, 5, 1 << 63)]
    assert numpy_group_pair(a[:0], b[:0], str, str) == []
