"""A CPU model of an engine without host rows (HipEngine.from_columns, a "column engine"): no GPU code in it.

ColumnModel holds the twelve columns in the form from_columns takes -- numeric columns as numpy arrays, string columns as
(codes | None, ascending dictionary) -- and has two parts.

Writers.  apply (UPDATE), concat (batch and single INSERT) and without (DELETE) are the model operations
tests/test_gpu_update.py and tests/test_gpu_insert_batch.py compare fresh engines over; ColumnModel.update / insert_batch /
insert_one / delete wrap them and track what decides the engine's refusals and routes: every shard's rows and capacity
(shard_alloc / shard_grow: capacity_for) and every string column's code width (0: a single-valued column without a buffer).
A writer the engine must refuse returns None and leaves the model as it was.

Readers, each computed without the engine.  The rows of a chain in scan mode come from the oracle's columnar scan
(orc_scan_columns) over the model's arrays; chains with LIKE / IN, which the oracle does not know, from the Python evaluator
chain_true of tests/test_gpu_set_predicates.py.  select_ids with indexes is the oracle's own walk (orc_select_ids_v) over a
`record` array filled from the model (RecordTable: an OracleTable over records instead of a CSV, its perms from
orc_index_build): rows in probe order, once per probe.  Every other form is folded from the model's cells over those rows by
the reference folds the suite already has; group_first is group_first_model.first_rows and order_ids_by Python's stable
`sorted` once per key, both over the order-preserving codes (tests/test_gpu_many_shards.py checks the two row by row).  tests/test_column_model.py checks all of it on the CPU against the golden ID lists
and the folds taken over OracleTable(csv).

The two newest forms, for tests/concurrent_sets.py: group_top is group_top_model's fold and order, value_set the same fold with
the HAVING compared in Python ints; a chain that names value sets becomes the IN-list chain over the model's members
(resolve_sets) and is evaluated leaf by leaf with numpy (member_mask).  tests/test_gpu_concurrent_sets.py holds them against the
plain-dict members_of, group_top_matrix's expectation and chain_true."""
import ctypes as C

import numpy as np

import group_first_model as gfm
import group_top_model as gtm
import qpelib as q
import test_gpu_count_distinct as cd
import test_gpu_group_buckets as gb
import test_gpu_group_count as grp
import test_gpu_order_by as ob
import test_gpu_set_predicates as sp
import test_group_pair_reference as gpr

pq = q.pq
STRINGS = [c for c in pq.COLUMNS if pq.COLUMN_KIND[pq.COL[c]] == pq.KIND_DICT]
NUMERIC = [c for c in pq.COLUMNS if pq.COLUMN_KIND[pq.COL[c]] != pq.KIND_DICT]
M64 = (1 << 64) - 1
GROUP_MAX_BINS = 65536                                           # HIP_GROUP_MAX_BINS: a group column of more values is refused
SET_OPERATORS = ("LIKE", "NOT LIKE", "IN", "NOT IN")
VALUE_SET_OPERATORS = ("IN SET", "NOT IN SET")
HAVING_OPS = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, ">": lambda a, b: a > b,
              "<=": lambda a, b: a <= b, ">=": lambda a, b: a >= b}


# ---- the model operations of the writers ------------------------------------------------------------------------------------
def rows_of(m):
    return len(m["command_id"])


def copy_model(m):
    return {k: (v.copy() if isinstance(v, np.ndarray) else (None if v[0] is None else v[0].copy(), list(v[1]))) for k, v in m.items()}


def code_dtype(count):
    return np.uint8 if count <= 256 else np.uint16 if count <= 65536 else np.uint32


def coded(texts, dtype=np.uint8, extra=()):
    """Per-row strings -> (codes, dictionary): the batch's own ascending dictionary (`extra`: strings in it that no row carries)."""
    values = sorted(set(texts) | set(extra))
    rank = {v: i for i, v in enumerate(values)}
    return np.array([rank[v] for v in texts], dtype=dtype), values


def concat(m, b):
    """The model of the old rows followed by the batch's: dictionaries the sorted unions, codes their positions in them."""
    out = {}
    for name, v in m.items():
        if isinstance(v, np.ndarray):
            out[name] = np.concatenate([v, np.asarray(b[name]).astype(v.dtype)])
            continue
        (oc, ov), (nc, nv) = v, b[name]
        merged = sorted(set(ov) | set(nv))
        if len(merged) == 1:
            out[name] = (None, merged)
            continue
        pos = {s: i for i, s in enumerate(merged)}
        lut_old, lut_new = np.array([pos[s] for s in ov]), np.array([pos[s] for s in nv])
        old = lut_old[oc] if oc is not None else np.full(rows_of(m), lut_old[0])
        new = lut_new[nc] if nc is not None else np.full(rows_of(b), lut_new[0])
        out[name] = (np.concatenate([old, new]).astype(code_dtype(len(merged))), merged)
    return out


def typed(column, value):
    if column == "sudo_used":
        return 1 if str(value).lower() == "true" or str(value) == "1" else 0
    return int(value)


def apply(m, assignments, mask):
    """The model after UPDATE SET assignments for the rows of `mask`."""
    out = copy_model(m)
    for column, value in assignments.items():
        if pq.COLUMN_KIND[pq.COL[column]] != pq.KIND_DICT:
            out[column][mask] = typed(column, value)
            continue
        codes, values = out[column]
        text = value if isinstance(value, bytes) else value.encode()
        if text not in values:
            rank = sum(v < text for v in values)
            values.insert(rank, text)
            if codes is not None:
                codes[codes >= rank] += 1
        if codes is not None:
            codes[mask] = values.index(text)
    return out


def without(m, mask):
    """The model after DELETE of the rows of `mask` (the dictionaries stay)."""
    return {k: (v[~mask] if isinstance(v, np.ndarray) else (None if v[0] is None else v[0][~mask], list(v[1]))) for k, v in m.items()}


# ---- what decides refusals and routes ---------------------------------------------------------------------------------------
def capacity_for(count):
    """Rows a shard of `count` rows has room for (shard_alloc, shard_grow)."""
    return (count + count // 16 + pq.TILE_ROWS) // pq.TILE_ROWS * pq.TILE_ROWS


def code_limit(width):
    """Strings a dictionary may hold at a code width (0: no buffer, one value)."""
    return 1 if width == 0 else 256 if width == 1 else 65536 if width == 2 else 0xFFFFFFFF


def width_for_count(count):
    return 1 if count <= 256 else 2 if count <= 65536 else 4


def partition(n, parts):
    """Rows of each of `parts` shards of an `n`-row table (shard_range: the first n % parts shards hold one row more)."""
    return [n // parts + (1 if s < n % parts else 0) for s in range(parts)]


def as_bytes(value):
    return value if isinstance(value, bytes) else str(value).encode("latin-1")


# ---- chains --------------------------------------------------------------------------------------------------------------------
def leaves_of(chain):
    for item in (chain or [])[0::2]:
        if isinstance(item, list):
            yield from leaves_of(item)
        else:
            yield item


def has_set_leaf(chain):
    return any(leaf[1] in SET_OPERATORS for leaf in leaves_of(chain))


def parse_in_list(text):
    """The items of pq.in_list's text: "('a', 'it''s')" -> ["a", "it's"]."""
    body, out, i = text.strip()[1:-1], [], 0
    while i < len(body):
        if body[i] != "'":
            i += 1
            continue
        i, item = i + 1, ""
        while True:
            j = body.index("'", i)
            item += body[i:j]
            if body[j + 1:j + 2] == "'":
                item, i = item + "'", j + 2
            else:
                i = j + 1
                break
        out.append(item)
    return out


def register_in_lists(chain):
    """chain_true looks the items of an IN list up by its text."""
    for leaf in leaves_of(chain):
        if leaf[1] in ("IN", "NOT IN") and leaf[2] not in sp._ITEMS:
            sp._ITEMS[leaf[2]] = parse_in_list(leaf[2])


class MemberLeaf(tuple):
    """The IN / NOT IN leaf a value-set leaf stands for (resolve_sets): an ordinary leaf for chain_true, with the members
    kept beside the text so that ColumnModel.member_mask need not parse them back."""
    members = ()


def resolve_sets(chain, sets):
    """The chain with every IN SET / NOT IN SET leaf replaced by the IN / NOT IN leaf over the MODEL's members of the set the
    leaf names (sets: the leaf's value text -> key texts, ColumnModel.value_set's)."""
    if chain is None:
        return None
    out = []
    for k, item in enumerate(chain):
        if k % 2 == 1 or (not isinstance(item, list) and item[1] not in VALUE_SET_OPERATORS):
            out.append(item)
        elif isinstance(item, list):
            out.append(resolve_sets(item, sets))
        else:
            leaf = MemberLeaf(sp.IN(item[0], list(sets[item[2]]), item[1].startswith("NOT")))
            leaf.members = tuple(sets[item[2]])
            out.append(leaf)
    return out


def has_member_leaf(chain):
    return any(isinstance(leaf, MemberLeaf) for leaf in leaves_of(chain))


def without_set_leaves(chain):
    """The chain with every LIKE / IN leaf replaced by a nested condition that holds for every row: the index walk makes the
    same probes (a nested node is no probe, and neither is a set condition), and its re-filter lets through every row the
    whole chain does."""
    out = []
    for k, item in enumerate(chain):
        if k % 2 == 1:
            out.append(item)
        elif isinstance(item, list):
            out.append(without_set_leaves(item))
        else:
            out.append([("command_id", ">=", "0")] if item[1] in SET_OPERATORS else item)
    return out


# ---- records ---------------------------------------------------------------------------------------------------------------------
class RecordTable(q.OracleTable):
    """OracleTable over a `record` array instead of a CSV."""

    def __init__(self, records, n, indexes=()):
        self.lib = q.load_oracle()
        self.n = n
        self._records = records
        self.rows = C.cast(records, C.POINTER(q.Record))
        self.set_indexes(indexes)


def columns_of_records(rows, n):
    """Oracle-loaded records -> the columns dict from_columns takes (dictionaries and codes as a load builds them)."""
    import kernel_model as km
    spec, arrays = km.columns_from_records(rows, n)
    out = {}
    for name in pq.COLUMNS:
        if name in STRINGS:
            col = spec.schema.col[pq.COL[name]]
            out[name] = (arrays[name], [col.dict[k] for k in range(col.dict_count)])
        else:
            out[name] = arrays[name]
    return out


class ColumnModel:
    def __init__(self, columns, n_shards=1):
        self.m = copy_model(columns)
        self.shard_rows = partition(rows_of(self.m), n_shards)
        self.shard_capacity = [capacity_for(k) for k in self.shard_rows]
        self.width = {c: 0 if self.m[c][0] is None else self.m[c][0].dtype.itemsize for c in STRINGS}
        self.route = None                                        # what the last writer did, for the records
        self._cache = {}

    @property
    def n(self):
        return rows_of(self.m)

    def _changed(self, m):
        self.m = m
        self._cache = {}

    # ---- writers ----
    def new_string_refusal(self, column, text):
        """Why an engine without host rows cannot take `text` into `column` in place, or None."""
        values = self.m[column][1]
        if text in values or len(values) + 1 <= code_limit(self.width[column]):
            return None
        return f"{column}: a second value for a column without a buffer" if self.width[column] == 0 else \
            f"{column}: string {len(values) + 1} of a dictionary that is full for {self.width[column]}-byte codes"

    def update_refusal(self, assignments):
        for column, value in assignments.items():
            if column in STRINGS:
                why = self.new_string_refusal(column, as_bytes(value))
                if why:
                    return why
        return None

    def update(self, assignments, chain):
        """UPDATE SET assignments WHERE chain: -> the rows the WHERE selects (scan semantics, the values from before the update),
        or None when the engine must refuse."""
        if self.update_refusal(assignments):
            return None
        mask = self.mask(chain)
        new = [c for c, v in assignments.items() if c in STRINGS and as_bytes(v) not in self.m[c][1]]
        self.route = dict(bumped=new)
        self._changed(apply(self.m, assignments, mask))
        return int(np.count_nonzero(mask))

    def insert_batch(self, b):
        """Batch INSERT (never refused for room or width: the shard grows, the codes widen); -> the rows appended."""
        B, route = rows_of(b), dict(grown=False, widened=[], materialised=[], remapped=[])
        after = concat(self.m, b)
        for c in STRINGS:
            old, union, tw = self.m[c][1], after[c][1], self.width[c]
            need = width_for_count(len(union))
            fw = (need if len(union) > 1 else 0) if tw == 0 else max(need, tw)
            identity = union[:len(old)] == old
            if tw == 0 and fw:
                route["materialised"].append(c)
            elif fw != tw:
                route["widened"].append(c)
            elif not identity:
                route["remapped"].append(c)
            self.width[c] = fw
        if self.shard_rows[-1] + B > self.shard_capacity[-1]:
            self.shard_capacity[-1] = capacity_for(self.shard_rows[-1] + B)
            route["grown"] = True
        self.shard_rows[-1] += B
        self.route = route
        self._changed(after)
        return B

    def insert_refusal(self, row):
        if self.shard_rows[-1] + 1 > self.shard_capacity[-1]:
            return "the last shard is full"
        for c in STRINGS:
            why = self.new_string_refusal(c, as_bytes(row[c]))
            if why:
                return why
        return None

    def insert_one(self, row):
        """executeQueryInsertHIP of {column: value}: -> True, or None when the engine must refuse."""
        if self.insert_refusal(row):
            return None
        b = {c: coded([as_bytes(row[c])]) if c in STRINGS else np.array([typed(c, row[c])], dtype=self.m[c].dtype) for c in pq.COLUMNS}
        self.route = dict(bumped=[c for c in STRINGS if as_bytes(row[c]) not in self.m[c][1]])
        self.shard_rows[-1] += 1
        self._changed(concat(self.m, b))
        return True

    def delete(self, chain):
        """DELETE WHERE chain: the rows renumber, order kept, every shard keeps what is left of its range; -> rows deleted."""
        mask = self.mask(chain)
        start = 0
        for s, k in enumerate(self.shard_rows):
            self.shard_rows[s] = k - int(np.count_nonzero(mask[start:start + k]))
            start += k
        self.route = dict(shards=list(self.shard_rows))
        self._changed(without(self.m, mask))
        return int(np.count_nonzero(mask))

    # ---- the table as the oracle reads it ----
    def codes(self, column):
        """One order-preserving integer per row: the code of a string column (0 without a buffer), the value otherwise."""
        v = self.m[column]
        if isinstance(v, np.ndarray):
            return v
        return v[0] if v[0] is not None else np.zeros(self.n, dtype=np.uint8)

    def cells(self, column):
        """Every row's cell as get_attribute_string_value prints it."""
        key = ("cells", column)
        if key not in self._cache:
            v = self.m[column]
            if column in STRINGS:
                words = np.array([w.decode("latin-1") for w in v[1]], dtype=object)
                out = words[self.codes(column)].tolist()
            elif column == "sudo_used":
                out = ["true" if x else "false" for x in v.tolist()]
            else:
                out = [str(x) for x in v.tolist()]
            self._cache[key] = out
        return self._cache[key]

    def cell(self, row, column):
        return self.cells(column)[row]

    def numbers(self, column):
        key = ("numbers", column)
        if key not in self._cache:
            self._cache[key] = self.m[column].tolist()           # Python ints
        return self._cache[key]

    def records(self):
        """The rows as a ctypes array of `record` (strings cut to their fields without a terminator, as strncpy leaves them)."""
        if "records" not in self._cache:
            n = self.n
            buf = np.zeros((max(n, 1), C.sizeof(q.Record)), dtype=np.uint8)
            for name in pq.COLUMNS:
                field = getattr(q.Record, name)
                if name in STRINGS:
                    words = np.array(self.m[name][1], dtype=f"S{field.size}")
                    buf[:n, field.offset:field.offset + field.size] = words.view(np.uint8).reshape(len(words), field.size)[self.codes(name)]
                else:
                    v = np.ascontiguousarray(self.m[name])
                    buf[:n, field.offset:field.offset + v.dtype.itemsize] = v.view(np.uint8).reshape(n, v.dtype.itemsize)
            self._cache["records"] = ((q.Record * max(n, 1)).from_buffer(buf), buf)
        return self._cache["records"][0]

    def table(self, indexes):
        key = ("table", tuple(indexes))
        if key not in self._cache:
            self._cache[key] = RecordTable(self.records(), self.n, indexes)
        return self._cache[key]

    def orc_columns(self):
        if "orc" not in self._cache:
            oc, keep = q.OrcColumns(), []
            oc.n_rows = self.n
            for name in NUMERIC:
                a = np.ascontiguousarray(self.m[name])
                keep.append(a)
                setattr(oc, name, a.ctypes.data)
            for k, name in enumerate(q.ORC_STR):
                a, words = np.ascontiguousarray(self.codes(name)), self.m[name][1]
                d = (C.c_char_p * len(words))(*words)
                keep += [a, d]
                oc.str_code[k], oc.str_code_width[k], oc.str_dict[k] = a.ctypes.data, a.dtype.itemsize, C.cast(d, C.POINTER(C.c_char_p))
            self._cache["orc"] = (oc, keep)
        return self._cache["orc"][0]

    # ---- rows of a chain ----
    def python_mask(self, chain):
        """chain_true over the rows: evaluated once per distinct combination of the columns the chain reads, on a row that
        carries it."""
        register_in_lists(chain)
        n = self.n
        columns = sorted({leaf[0] for leaf in leaves_of(chain) if leaf[0] in pq.COLUMNS})
        if n == 0:
            return np.zeros(0, dtype=bool)
        recs = self.records()
        if not columns:
            return np.full(n, bool(sp.chain_true(recs[0], chain)))
        keys = np.stack([self.codes(c).astype(np.uint64).view(np.int64) if self.codes(c).dtype == np.uint64 else self.codes(c).astype(np.int64)
                         for c in columns], axis=1)
        _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        truth = np.array([bool(sp.chain_true(recs[int(r)], chain)) for r in first])
        return truth[np.asarray(inverse).reshape(-1)]

    def member_mask(self, chain):
        """A chain that resolve_sets made: evaluateWhereClause's right-recursive fold, no precedence, over one mask per leaf
        -- a MemberLeaf by numpy.isin over the column (a set of 60 000 members is no matter for it), any other leaf by mask()
        of the leaf alone.  tests/test_gpu_concurrent_sets.py holds it against python_mask row by row."""
        acc = None
        items, ops = chain[0::2], chain[1::2]
        for k in range(len(items) - 1, -1, -1):
            it = items[k]
            if isinstance(it, list):
                m = self.member_mask(it)
            elif isinstance(it, MemberLeaf):
                if it[0] in STRINGS:
                    words = {t.encode("latin-1") for t in it.members}
                    m = np.array([w in words for w in self.m[it[0]][1]], dtype=bool)[self.codes(it[0])]
                else:
                    m = np.isin(self.m[it[0]].astype(np.int64), np.array([int(t) for t in it.members], dtype=np.int64))
                m = m != (it[1] == "NOT IN")
            else:
                m = self.mask([it])
            acc = m if acc is None else (m | acc) if ops[k] == "OR" else (m & acc)
        return acc

    def mask(self, chain):
        """The rows for which the WHERE is true (scan semantics)."""
        if not chain:
            return np.ones(self.n, dtype=bool)
        if has_member_leaf(chain):
            return self.member_mask(chain) if self.n else np.zeros(0, dtype=bool)
        if has_set_leaf(chain):
            return self.python_mask(chain)
        out = np.zeros(self.n, dtype=bool)
        out[self.scan_rows(chain)] = True
        return out

    def scan_rows(self, chain):
        """Scan mode: ascending rows."""
        if not chain:
            return np.arange(self.n, dtype=np.int64)
        if has_set_leaf(chain):
            return np.flatnonzero(self.mask(chain))
        wl = q.WhereList(chain)
        out = np.zeros(max(self.n, 1), dtype=np.uint32)
        k = q.load_oracle().orc_scan_columns(C.byref(self.orc_columns()), wl.ptr, 0, out.ctypes.data_as(C.POINTER(C.c_uint32)), self.n, 1)
        return out[:k].astype(np.int64)

    def select_ids(self, chain, indexes=(), probe_bool=False):
        """executeQuerySelectIdsHIP: scan mode without a probe, otherwise the probes' rows in probe order, re-filtered
        (probe_bool: the walk of an engine under PQPS_PROBE_BOOL=1, BOOL indexes probed too)."""
        if not indexes or not chain:
            return self.scan_rows(chain).tolist()
        if not has_set_leaf(chain):
            return self.table(indexes).select_ids(chain, probe_bool=probe_bool)[0]
        ids = self.table(indexes).select_ids(without_set_leaves(chain), probe_bool=probe_bool)[0]
        mask = self.mask(chain)
        return [r for r in ids if mask[r]]

    # ---- the other forms, folded over the rows of select_ids ----
    def group_refused(self, column):
        return column in STRINGS and len(self.m[column][1]) > GROUP_MAX_BINS

    def group_count(self, column, ids):
        cells = self.cells(column)
        return grp.expected_from_cells(column, [cells[r] for r in ids])

    def aggregate(self, value_column, group_column, ids):
        values, groups, acc = self.numbers(value_column), self.cells(group_column) if group_column else None, {}
        for r in ids:
            key, v = groups[r] if groups else None, values[r]
            c, s, lo, hi = acc.get(key, (0, 0, v, v))
            acc[key] = (c + 1, s + v, min(lo, v), max(hi, v))
        keys = sorted(acc, key=lambda k: grp.key_order(group_column, k)) if group_column else list(acc)
        wrap = (lambda s: s & M64) if value_column == "command_id" else (lambda s: s)
        return [(k, acc[k][0], wrap(acc[k][1]), acc[k][2], acc[k][3]) for k in keys]

    def count_distinct(self, value_column, group_column, ids):
        return cd.oracle_distinct(self, ids, value_column, group_column)

    def order_ids(self, column, ids, descending=False, limit=None):
        cells = self.cells(column)
        keys = [ob.cell_key(column, cells[r]) for r in ids]
        return ob.cut(ob.sort_rows(ids, keys, descending), limit), len(ids)

    def group_top(self, column, value_column, rows, by="count", descending=True, limit=10):
        """HipEngine.group_top_result without `seconds`: the groups of group_top_model.fold over the listed rows (duplicates
        counted), the first `limit` (None or <= 0: all) in group_top_model.order's order."""
        return gtm.top(self, column, value_column, np.asarray(rows, dtype=np.int64), by, descending, limit)

    def value_set(self, column, rows, having=None):
        """hipEngineCreateSetHIP over the inner rows `rows` (scan semantics: scan_rows(chain), each row once): -> (the members'
        key texts in key order, len(rows)).  having = (aggregate, value column | None, op, constant) with the header's
        arithmetic: an i32 sum in int64 compared signed, a command_id sum mod 2^64 compared unsigned, MIN and MAX in value
        order (group_top_model.fold's dtypes; compared as Python ints).  Only values that some inner row carries are folded,
        so a value without inner rows is never a member."""
        f = gtm.fold(self.codes(column), self.m[having[1]] if having and having[1] else None, rows, bool(having) and having[1] == "command_id")
        keys = f["key"].tolist()
        if having is not None:
            agg, _, op, constant = having
            keys = [k for k, x in zip(keys, f[agg].tolist()) if HAVING_OPS[op](int(x), int(constant))]
        return [gtm.key_text(self, column, k) for k in keys], len(rows)

    def group_pair(self, columns, value_column, ids):
        rows = np.asarray(ids, dtype=np.int64)
        text = [gpr.key_text(c, self.m[c][1] if c in STRINGS else None) for c in columns]
        values = self.m[value_column][rows] if value_column else None
        return gpr.numpy_group_pair(self.codes(columns[0])[rows], self.codes(columns[1])[rows], text[0], text[1], values,
                                    value_column == "command_id")

    def group_buckets(self, column, prefix, width, value_column, ids):
        cells = self.cells(column)
        values = self.numbers(value_column) if value_column else None
        return gb.fold([cells[r] for r in ids], [values[r] for r in ids] if value_column else None, prefix, width, value_column)

    def group_first(self, group_column, order_column, ids, descending=False):
        """executeQueryGroupFirstHIP: ([(key_text or None, row, order_text), ...] in key order, len(ids)) -- per group the
        candidate that comes first by (order key, row): group_first_model.first_rows over the order-preserving codes."""
        rows = np.asarray(ids, dtype=np.int64)
        groups = self.codes(group_column)[rows] if group_column else None
        _, first, _ = gfm.first_rows(rows, self.codes(order_column)[rows], groups, descending)
        gcells, ocells = self.cells(group_column) if group_column else None, self.cells(order_column)
        return [(gcells[r] if group_column else None, r, ocells[r]) for r in first.tolist()], len(ids)

    def order_ids_by(self, keys, ids, limit=None):
        """executeQueryOrderIdsByHIP: (rows, len(ids)) -- `keys` column names or (column, descending) pairs, the first the
        most significant; rows equal in all keys in ascending row number.  Python's stable `sorted`, once per key from the
        last to the first, over each key's order-preserving integers (no key is packed)."""
        pairs = [(k, False) if isinstance(k, (str, bytes)) else (k[0], bool(k[1])) for k in keys]
        rows = sorted(ids)
        for column, descending in reversed(pairs):
            image = self.codes(column).tolist()
            rows = sorted(rows, key=image.__getitem__, reverse=descending)
        return ob.cut(rows, limit), len(ids)

    def project(self, ids, columns=None):
        cells = [self.cells(c) for c in (columns or pq.COLUMNS)]
        return [[col[r] for col in cells] for r in ids]
