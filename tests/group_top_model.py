"""A numpy model of "the top N groups" (executeQueryGroupTopHIP): GROUP BY one column, ORDER BY an aggregate, LIMIT.  No
engine code in it: the groups are numpy.unique over the selected rows' order-preserving codes, the aggregates numpy's
ufunc.at folds, the order numpy.lexsort with the group key as the last resort in both directions.

    fold(codes, values, rows, u64)            every group of the rows: keys ascending, counts, sums, mins, maxs
    order(keys, by_array, descending, limit)  the listed groups' indices
    top(model, column, value_column, ids, by, descending, limit)   what HipEngine.group_top_result returns, from a ColumnModel

Values: an i32 column folds in int64 (exact), command_id in uint64 (the sum wraps modulo 2^64, min / max unsigned)."""
import numpy as np

M64 = (1 << 64) - 1
BY = ("key", "count", "sum", "min", "max")


def fold(codes, values, rows, u64=False):
    """codes / values: one entry per table row; rows: the selected rows, duplicates counted as often as they are listed."""
    rows = np.asarray(rows, dtype=np.int64)
    keys, inverse, counts = np.unique(np.asarray(codes)[rows], return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    out = {"key": keys, "count": counts.astype(np.uint64)}
    if values is not None:
        dt = np.uint64 if u64 else np.int64
        v = np.asarray(values)[rows].astype(dt)
        info = np.iinfo(dt)
        s, lo, hi = np.zeros(len(keys), dt), np.full(len(keys), info.max, dt), np.full(len(keys), info.min, dt)
        np.add.at(s, inverse, v)                                 # uint64: modulo 2^64
        np.minimum.at(lo, inverse, v)
        np.maximum.at(hi, inverse, v)
        out.update(sum=s, min=lo, max=hi)
    return out


def order(keys, by_array, descending=False, limit=0):
    """Indices of the listed groups: by `by_array` (ascending, or reversed), ties by ascending key in both directions."""
    primary = ~np.asarray(by_array) if descending else np.asarray(by_array)      # ~x reverses signed and unsigned order alike
    idx = np.lexsort((np.asarray(keys), primary))
    return idx[:limit] if limit and limit > 0 else idx


def key_text(model, column, code):
    v = model.m[column]
    if not isinstance(v, np.ndarray):
        return v[1][int(code)].decode("latin-1")
    if column == "sudo_used":
        return "true" if int(code) else "false"
    return str(int(code))


def top(model, column, value_column, ids, by="count", descending=True, limit=10):
    u64 = value_column == "command_id"
    groups = fold(model.codes(column), model.m[value_column] if value_column else None, ids, u64)
    idx = order(groups["key"], groups[by], descending, limit or 0)
    rows = []
    for i in idx.tolist():
        row = (key_text(model, column, groups["key"][i]), int(groups["count"][i]))
        if value_column:
            row += (int(groups["sum"][i]), int(groups["min"][i]), int(groups["max"][i]))
        rows.append(row)
    return {"rows": rows, "total": len(ids), "groups_total": len(groups["key"])}
