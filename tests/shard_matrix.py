"""Every query form over three and five shards, against tests/column_model.py: the table, the case list, the driver.

The host code that puts a multi-shard answer together (gather_shards and the index-mode union, group_combine / first_combine
under shard_reduce, the k-way merges of pair_sparse, distinct_sort and order_sort with order_chain_cmp, order_collect with
order_topk's host sort, the scattered projection) runs with k = 2 in the rest of the suite.  A two-way merge never has a
shard run dry between two that still hold entries, a key in three runs, a tie over three shards or a second non-zero row0.
Here one seeded table of 5 123 rows is built so that every such situation occurs under the partitions of three and of five
shards (table(); tests/test_gpu_many_shards.py asserts each property against the partition on the CPU), every WHERE route
(ROUTES) is asked in every form (cases()), with ib.HOST_INDEX and with no index, and every answer is compared for equality
with the CPU model.  No expected answer comes from an engine.

    python tests/shard_matrix.py run <devices> [family]      the matrix (family: one of FAMILIES, default all of them)
    python tests/shard_matrix.py history <devices>           a writer history on the same table, a fixed subset after each step

<devices> is the PQPS_DEVICES value the engines are created under ("0,0,0": three shards on one card).  Both print the number
of cases and OK, or exit non-zero with the first case that differs.  PQPS_PROBE_BOOL=1 in the environment is followed by the
model (BOOL indexes probed too).

Both ask from one thread.  tests/concurrent_matrix.py asks the same cases of the same table from several threads at once, and
replays the history's writers (model_step / engine_step, recorded through History's `recorder`) under readers that never stop."""
import ctypes as C
import os
import sys

import numpy as np

import column_model as cm
import qpelib as q
import test_gpu_insert_batch as ib

pq = q.pq
N = 5 * 1024 + 3
LAYOUTS = (3, 5)
INDEXES = ib.HOST_INDEX
INDEX_CONFIGS = {"host_index": INDEXES, "no_index": ()}
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1
RAW, DIR = b"ls -la", b"/home/u"
SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
BASES = [b"cat", b"cd", b"grep", b"ls", b"make", b"rm", b"ssh", b"vim"]
HOSTS = [b"host-%03d" % i for i in range(256)]
COMMON = [b"student%d" % i for i in range(1, 291)]               # insertion order: "student10" sorts in front of "student2"
TIE = 7                                                          # risk_level of the runs across the shard boundaries
MIN_ROW, MAX_ROW = 2600, 5050                                    # a middle shard and the last one, in both layouts
ID_MIN_ROW, ID_MAX_ROW, ID_2_63_ROW = 5000, 2500, 100


def starts(n, parts):
    """First row of every shard and the end: [0, ..., n]."""
    return np.concatenate([[0], np.cumsum(cm.partition(n, parts))]).tolist()


def boundaries():
    return sorted({b for k in LAYOUTS for b in starts(N, k)[1:-1]})


def only_name(k, s):
    return b"only%d-in-shard%d" % (k, s)


def skip_name(k):
    return b"shards0and2-of%d" % k


def only_rows(k, s):
    """Three rows inside shard s of the k-shard layout (no two special names share a row)."""
    first = starts(N, k)[s]
    return [first + d for d in ((10, 500, 1200) if k == 3 else (20, 400, 900))]


def skip_rows(k):
    """Rows of shards 0 and 2 of the k-shard layout."""
    return [50, 60, 3500, 3510] if k == 3 else [70, 80, 2100, 2110]


def stamp(i):
    return b"2025-01-01T%02d:%02d:%02d.000Z" % (i // 3600, i // 60 % 60, i % 60)


def table():
    """The columns HipEngine.from_columns takes; every property the module's header names is asserted on the CPU by
    tests/test_gpu_many_shards.py."""
    rng = np.random.default_rng(5123)
    row = np.arange(N)
    names = np.array(COMMON, dtype=object)[rng.integers(0, len(COMMON), N)]
    for k in LAYOUTS:
        for s in range(k):
            names[only_rows(k, s)] = only_name(k, s)
        names[skip_rows(k)] = skip_name(k)
    command_id = 1000 + 7 * rng.permutation(N).astype(np.uint64)
    command_id[row % 5 == 3] += np.uint64(1 << 63)
    command_id[ID_MIN_ROW], command_id[ID_MAX_ROW], command_id[ID_2_63_ROW] = 1, M64, 1 << 63
    exit_code = rng.integers(0, 3, N).astype(np.int32)           # full range: two keys with it need the 64-bit packed key
    exit_code[MIN_ROW], exit_code[MAX_ROW] = INT32_MIN, INT32_MAX
    risk_level = rng.integers(1, 6, N).astype(np.int32)
    for b in boundaries():
        risk_level[b - 4:b + 4] = TIE
    risk_level[MIN_ROW], risk_level[MAX_ROW] = 0, 9
    return {
        "command_id": command_id, "exit_code": exit_code, "risk_level": risk_level,
        "user_id": (1000 + row // 256).astype(np.int32),                       # the band column; increasing with the row
        "sudo_used": (rng.random(N) < 0.3).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, N).astype(np.uint8), list(SHELLS)),
        "base_command": (rng.integers(0, 8, N).astype(np.uint8), list(BASES)),
        "host_name": (rng.integers(0, 256, N).astype(np.uint8), list(HOSTS)),
        "user_name": cm.coded(list(names), dtype=np.uint16),
        "timestamp": ((N - 1 - row).astype(np.uint16), [stamp(i) for i in range(N)]),   # decreasing with the row, unique
        "raw_command": (None, [RAW]), "working_directory": (None, [DIR]),
    }


def rows_like(B, seed, first_id):
    """A batch of B rows of the table's distributions: its own dictionaries, later timestamps, a user name new to the table."""
    rng = np.random.default_rng([seed, B])
    names = [COMMON[i] for i in rng.integers(0, len(COMMON), B)]
    names[0] = b"student1000-batch%d" % seed
    return {
        "command_id": np.arange(first_id, first_id + B, dtype=np.uint64), "exit_code": rng.integers(0, 3, B).astype(np.int32),
        "risk_level": rng.integers(1, 6, B).astype(np.int32), "user_id": (1100 + np.arange(B) // 256).astype(np.int32),
        "sudo_used": (rng.random(B) < 0.3).astype(np.uint8),
        "shell_type": cm.coded([SHELLS[i] for i in rng.integers(0, 4, B)]), "base_command": cm.coded([BASES[i] for i in rng.integers(0, 8, B)]),
        "host_name": cm.coded([HOSTS[i] for i in rng.integers(0, 256, B)]), "user_name": cm.coded(names, dtype=np.uint16),
        "timestamp": cm.coded([b"2026-%02d-01T00:%02d:%02d.000Z" % (seed, i // 60, i % 60) for i in range(B)], dtype=np.uint16),
        "raw_command": (None, [RAW]), "working_directory": (None, [DIR]),
    }


# ---- the WHERE routes -------------------------------------------------------------------------------------------------------
def rows_between(first, last):
    """The WHERE of the rows first .. last of the unchanged table (timestamp is unique and decreases with the row)."""
    return [("timestamp", "<=", stamp(N - 1 - first).decode()), "AND", ("timestamp", ">=", stamp(N - 1 - last).decode())]


def wide_chain():
    chain = []
    for i in range(40):
        chain += [("timestamp", "=", stamp(N - 1 - (128 * i + 5)).decode()), "OR"]
    return chain + [("base_command", "=", "make")]


SEVEN = [COMMON[i] for i in (0, 40, 80, 120, 160, 200, 240)]
# name: (chain, (scan passes, member passes) of its plan, index probes under INDEXES, index probes with BOOL indexes probed too)
ROUTES = {
    "none": (None, (1, 0), 0, 0),
    "fused": ([("shell_type", "=", "zsh"), "AND", ("base_command", "!=", "rm")], (1, 0), 0, 0),
    "plane": ([("sudo_used", "=", "TRUE"), "AND", ("shell_type", "=", "bash")], (1, 0), 0, 1),
    "wide": (wide_chain(), (2, 0), 0, 0),
    "member": ([("user_name", "NOT IN", pq.in_list(SEVEN)), "AND", ("exit_code", "<=", "1")], (1, 1), 0, 0),
    "one_value": ([("exit_code", "=", "1"), "AND", ("base_command", "!=", "rm")], (1, 0), 0, 0),   # every group's exit_code the same
    "probe": ([("risk_level", ">", "3")], (1, 0), 1, 1),
    "or_probes": ([("risk_level", ">=", "4"), "OR", ("user_id", "<=", "1003")], (1, 0), 2, 2),
    "nothing": ([("risk_level", "=", "77")], (1, 0), 1, 1),
    "ends_fused": (rows_between(0, 299) + ["OR", ("timestamp", "<=", stamp(N - 1 - 4800).decode())], (1, 0), 0, 0),
    "band_inside": ([("user_id", "=", "1002")], (1, 0), 1, 1),
    "band_across_3": ([("user_id", "=", "1006")], (1, 0), 1, 1),
    "band_across_5": ([("user_id", "=", "1004")], (1, 0), 1, 1),
    "band_ends": ([("user_id", "<=", "1000"), "OR", ("user_id", ">=", "1019")], (1, 0), 2, 2),
    "band_all": ([("user_id", ">=", "1000")], (1, 0), 1, 1),
}
HISTORY_ROUTES = ("fused", "or_probes")                          # a fused route and a list route (two probes, rows twice)


def spec_of(m):
    s = pq.SchemaSpec()
    for name, v in m.items():
        if isinstance(v, np.ndarray):
            s.set_numeric(name, v.dtype.itemsize)
        else:
            s.set_dict(name, 1 if v[0] is None else v[0].dtype.itemsize, v[1])
    return s


def passes(m, chain):
    """(scan passes, member passes) of the WHERE over the model's dictionaries (hipCompileWherePlan)."""
    plan = pq.compile_plan_sets(spec_of(m), chain)
    members = sum(member is not None for _, _, member in plan)
    return len(plan) - members, members


def probes(chain, indexes, probe_bool=False):
    """The index probes of a WHERE: its top-level conditions, other than LIKE / IN, on a column with an INT or UINT64 index
    (with probe_bool a BOOL index too) -- what list_probes walks."""
    kinds = {pq.FIELD_INT, pq.FIELD_UINT64} | ({pq.FIELD_BOOL} if probe_bool else set())
    indexed = {name for name, kind in indexes if kind in kinds}
    return sum(not isinstance(item, list) and item[1] not in cm.SET_OPERATORS and item[0] in indexed for item in (chain or [])[0::2])


# ---- ORDER BY several keys -----------------------------------------------------------------------------------------------------
KEY_LISTS = {
    pq.ORDER_PACK32: [("risk_level", True), ("user_name", False), ("shell_type", True)],
    pq.ORDER_PACK64: [("exit_code", False), ("user_name", True), ("host_name", False)],
    pq.ORDER_CHAIN: [("exit_code", True), ("risk_level", False), ("command_id", True)],
}


def key_form(model, keys):
    """The form hipOrderKeyPlan gives the key list over the model's dictionaries and i32 ranges."""
    counts = {c: len(model.m[c][1]) for c in cm.STRINGS}
    bounds = {c: (int(model.m[c].min()), int(model.m[c].max())) for c in ("exit_code", "user_id", "risk_level") if model.n}
    return pq.order_key_plan(keys, counts, bounds)["form"]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
FAMILIES = ("rows", "groups", "order", "order_by", "first")
CELLS = ["command_id", "user_name", "timestamp", "risk_level"]
TICKETS = (("plane", False), ("probe", False), ("band_ends", True))         # (route, count only)


def shard_counts(ids, shard_rows):
    """How many of the listed rows (duplicates and all) each shard holds."""
    edges = np.concatenate([[0], np.cumsum(shard_rows)])
    return np.histogram(np.asarray(ids, dtype=np.int64), bins=edges)[0].tolist() if len(ids) else [0] * len(shard_rows)


def limits_of(ids, shard_rows):
    """LIMIT values for a selection: 1; one below, at and one above the matches of a single shard (the last shard that has
    any); more than all matches; none."""
    held = [c for c in shard_counts(ids, shard_rows) if c]
    c = held[-1] if held else 1
    return [1, max(1, c - 1), c, c + 1, len(ids) + 7, None]


def columnar_rows(res_of, eng):
    res = res_of()
    try:
        return res["rows"], res.get("matches")
    finally:
        eng.free_columnar(res)


def cases(model, indexes, probe_bool=False, routes=None, families=FAMILIES, full=True, eng=None):
    """[(what, the engine's answer, the model's answer)] as callables for the state the model is in: every route in every
    form (full=False: each form once per route, the subset the history asks after every step)."""
    out, ids, orders = [], {}, {}

    def rows(name):
        if name not in ids:
            ids[name] = model.select_ids(ROUTES[name][0], indexes, probe_bool)
        return ids[name]

    def add(what, engine_says, model_says):
        out.append((what, engine_says, model_says))

    def ordered(name, column, desc):
        """The whole order, computed once for every LIMIT."""
        if (name, column, desc) not in orders:
            orders[name, column, desc] = model.order_ids(column, rows(name), desc, None)[0]
        return orders[name, column, desc]

    for name in (routes or ROUTES):
        chain = ROUTES[name][0]
        if "rows" in families:
            add((name, "ids"), lambda chain=chain: eng.select_ids(chain), lambda name=name: rows(name))
            # (COUNT(*) never probes: the scan-mode count, every row once)
            add((name, "count"), lambda chain=chain: eng.count(chain), lambda chain=chain: len(model.scan_rows(chain)))
            for columns in (CELLS, None) if full else (CELLS,):
                add((name, "cells", columns), lambda chain=chain, columns=columns: columnar_rows(lambda: eng.select_columnar(columns, chain), eng)[0],
                    lambda name=name, columns=columns: model.project(rows(name), columns))
        if "groups" in families:
            for column in ("user_name", "risk_level", "sudo_used", "timestamp") if full else ("user_name",):
                add((name, "group", column), lambda chain=chain, column=column: eng.group_count(column, chain),
                    lambda name=name, column=column: model.group_count(column, rows(name)))
            for value, group in (("exit_code", "user_name"), ("command_id", None), ("command_id", "shell_type"), ("risk_level", "sudo_used")) if full \
                    else (("command_id", "shell_type"),):
                add((name, "aggregate", value, group), lambda chain=chain, value=value, group=group: eng.aggregate(value, group, chain),
                    lambda name=name, value=value, group=group: model.aggregate(value, group, rows(name)))
            # a bitmap; the sort form of command_id, alone and grouped; exit_code, whose full range takes the sort form with the
            # same few values in every group; a grouped bitmap
            for value, group in (("host_name", None), ("command_id", None), ("command_id", "shell_type"), ("exit_code", "shell_type"),
                                 ("user_name", "risk_level")) if full else (("host_name", None), ("command_id", None), ("exit_code", "shell_type")):
                add((name, "distinct", value, group), lambda chain=chain, value=value, group=group: eng.count_distinct(value, group, chain),
                    lambda name=name, value=value, group=group: model.count_distinct(value, group, rows(name)))
            for pair in (("shell_type", "risk_level"), ("user_name", "host_name")):              # dense, sparse
                for value in (None, "command_id", "exit_code") if full else ("command_id",):
                    add((name, "pair", pair, value), lambda chain=chain, pair=pair, value=value: eng.group_pair(pair, value, chain),
                        lambda name=name, pair=pair, value=value: model.group_pair(pair, value, rows(name)))
            for column, prefix, width in (("user_name", 9, None), ("user_id", None, 4)):
                for value in (None, "risk_level") if full else ("risk_level",):
                    add((name, "buckets", column, value),
                        lambda chain=chain, column=column, prefix=prefix, width=width, value=value: eng.group_buckets(column, prefix=prefix, width=width, value_column=value, chain=chain),
                        lambda name=name, column=column, prefix=prefix, width=width, value=value: model.group_buckets(column, prefix, width, value, rows(name)))
        if "order" in families:
            if full:
                shapes = [(c, d, k) for c in ("risk_level", "user_name", "command_id") for d in (False, True) for k in limits_of(rows(name), model.shard_rows)]
                shapes += [(c, d, 20) for c in ("user_id", "timestamp") for d in (False, True)]
            else:
                shapes = [("risk_level", True, 20), ("command_id", False, None)]
            for column, desc, limit in shapes:
                add((name, "order", column, desc, limit), lambda chain=chain, column=column, desc=desc, limit=limit: eng.order_ids(column, chain, desc, limit),
                    lambda name=name, column=column, desc=desc, limit=limit: (cm.ob.cut(ordered(name, column, desc), limit), len(rows(name))))

            def ordered_model(name=name):
                return model.project(cm.ob.cut(ordered(name, "user_name", True), 25)), len(rows(name))

            add((name, "select_ordered"), lambda chain=chain: columnar_rows(lambda: eng.select_ordered(None, chain, "user_name", True, 25), eng), ordered_model)
        if "order_by" in families:
            for form, keys in KEY_LISTS.items():
                for limit in (20, None) if full else (20,):
                    add((name, "order_by", form, limit), lambda chain=chain, keys=keys, limit=limit: eng.order_ids_by(keys, chain, limit),
                        lambda name=name, keys=keys, limit=limit: model.order_ids_by(keys, rows(name), limit))

            def by_model(name=name):
                order, matches = model.order_ids_by(KEY_LISTS[pq.ORDER_CHAIN], rows(name), 25)
                return model.project(order, CELLS), matches

            add((name, "select_ordered_by"),
                lambda chain=chain: columnar_rows(lambda: eng.select_ordered_by(CELLS, chain, KEY_LISTS[pq.ORDER_CHAIN], 25), eng), by_model)
        if "first" in families:
            shapes = [(g, c, d) for g in ("user_name", None) for c in ("risk_level", "command_id") for d in (False, True)] if full \
                else [("user_name", "risk_level", False), (None, "command_id", True)]
            for group, column, desc in shapes:
                add((name, "first", group, column, desc), lambda chain=chain, group=group, column=column, desc=desc: eng.group_first(group, column, chain, desc),
                    lambda name=name, group=group, column=column, desc=desc: model.group_first(group, column, rows(name), desc))

            def first_model(name=name):
                groups, total = model.group_first("shell_type", "command_id", rows(name), True)
                return model.project([r for _, r, _ in groups], CELLS), total

            add((name, "select_group_first"),
                lambda chain=chain: columnar_rows(lambda: eng.select_group_first(CELLS, chain, "shell_type", "command_id", True), eng), first_model)
    if "rows" in families:
        add(("tickets",), lambda: tickets_in_flight(eng), lambda: [len(model.scan_rows(ROUTES[r][0])) if count_only else rows(r) for r, count_only in TICKETS])
    return out


def tickets_in_flight(eng, while_held=None):
    """Three tickets issued before the first is awaited; -> their answers (the IDs read from the device).  `while_held` is
    called with the three tickets held and none awaited."""
    if not isinstance(eng, pq.HipEngine):
        return eng.tickets_in_flight(while_held)                    # a stand-in without a device (tests/concurrent_matrix.py)
    tickets = [eng.select_async(ROUTES[r][0], count_only) for r, count_only in TICKETS]
    out = []
    ctx = pq.Context(0)
    try:
        assert all(tickets)
        if while_held:
            while_held()
        for tk, (_, count_only) in reversed(list(zip(tickets, TICKETS))):
            n, res = eng.await_ticket(tk)
            assert n >= 0
            if count_only:
                out.append(int(n))
                continue
            got = np.zeros(max(n, 1), dtype=np.uint32)
            if n:
                ctx.download(got.ctypes.data, res.ids_dev, 4 * n)
            out.append(got[:n].tolist())
    finally:
        for tk in tickets:
            if tk:
                eng.release_ticket(tk)
        ctx.close()
    return out[::-1]


def ask(call):
    try:
        return call()
    except pq.PqpsError:
        return "refused"


def compare(eng, todo, note=None):
    """Every case asked of the engine; the first that differs ends the process."""
    for what, engine_says, model_says in todo:
        got, want = ask(engine_says), model_says()
        if got != want:
            print("DIFFERENT", what, note, "\n got ", repr(got)[:1500], "\n want", repr(want)[:1500], flush=True)
            sys.exit(1)
    return len(todo)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def run(devices, families=FAMILIES):
    n_shards = len(devices.split(","))
    probe_bool = os.environ.get("PQPS_PROBE_BOOL") == "1"
    columns, count = table(), 0
    for config, indexes in INDEX_CONFIGS.items():
        model = cm.ColumnModel(columns, n_shards)
        eng = pq.HipEngine.from_columns(N, columns, indexes)
        try:
            assert eng.shards() == model.shard_rows, (eng.shards(), model.shard_rows)
            for form, keys in KEY_LISTS.items():
                assert key_form(model, keys) == form, (form, keys)
            count += compare(eng, cases(model, indexes, probe_bool, families=families, eng=eng), config)
        finally:
            eng.close()
    print("CASES", count, "OK", flush=True)


# ---- a writer step: the model's prediction, the engine's call ------------------------------------------------------------------
WRITERS = ("UPDATE", "batch INSERT", "INSERT", "DELETE")


def model_step(model, kind, args):
    """The step applied to the model; -> what the engine must return (rows matched / appended / deleted, True), None for a
    step it must refuse (the model is unchanged then)."""
    if kind == "UPDATE":
        return model.update(*args)
    if kind == "batch INSERT":
        return model.insert_batch(*args)
    if kind == "INSERT":
        return model.insert_one(*args)
    assert kind == "DELETE", kind
    return model.delete(*args)


def engine_step(eng, kind, args):
    """The step asked of the engine; -> what it returned, "refused" for a refusal."""
    if not isinstance(eng, pq.HipEngine):
        return eng.writer(kind, args)                                # a stand-in without a device (tests/concurrent_matrix.py)
    if kind == "UPDATE":
        return ask(lambda: eng.update(*args))
    if kind == "batch INSERT":
        return ask(lambda: eng.insert_columns(cm.rows_of(args[0]), args[0]))
    if kind == "INSERT":
        r = pq.Record()
        for column, value in args[0].items():
            setattr(r, column, value)
        return True if pq.lib().executeQueryInsertHIP(eng.e, b"commands", C.byref(r)) else "refused"
    assert kind == "DELETE", kind
    rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", pq.WhereList(args[0]).ptr)
    ok, k = bool(rs.contents.success), rs.contents.numRecords
    pq.lib().freeResultSet(rs)
    return k if ok else "refused"


class History:
    """An engine over table() with INDEXES, the model beside it; every writer is the model's prediction, refusals included.
    `recorder(model, step)` is called with step None for the untouched table and with (kind, args, prediction) after every
    writer has been applied to the model."""

    def __init__(self, n_shards, dry=False, recorder=None):
        columns = table()
        self.model = cm.ColumnModel(columns, n_shards)
        self.eng = None if dry else pq.HipEngine.from_columns(N, columns, INDEXES)      # dry: the model's side alone, on the CPU
        self.probe_bool = os.environ.get("PQPS_PROBE_BOOL") == "1"
        self.log, self.count = [], 0
        self.recorder = recorder
        if recorder:
            recorder(self.model, None)

    def check(self):
        eng, model = self.eng, self.model
        todo = cases(model, INDEXES, self.probe_bool, routes=HISTORY_ROUTES, full=False, eng=eng)
        if eng is None:
            self.count += len([model_says() for _, _, model_says in todo])
            return
        eng.n = eng.e.contents.num_records
        assert eng.n == model.n and eng.shards() == model.shard_rows, (eng.n, eng.shards(), model.shard_rows, self.log)
        self.count += compare(eng, todo, self.log)

    def step(self, kind, args, entry):
        """One writer: the model first, then the engine, whose return must be the model's prediction."""
        want = model_step(self.model, kind, args)
        self.log.append(entry(want))
        if self.recorder:
            self.recorder(self.model, (kind, args, want))
        if self.eng is not None:
            got = engine_step(self.eng, kind, args)
            assert got == ("refused" if want is None else want), (got, self.log)
        return want

    def update(self, assignments, chain):
        return self.step("UPDATE", (assignments, chain), lambda want: ("UPDATE", assignments, want))

    def batch(self, b):
        return self.step("batch INSERT", (b,), lambda want: ("batch INSERT", want, self.model.route))

    def insert(self, row):
        return self.step("INSERT", (row,), lambda want: ("INSERT", want))

    def delete(self, chain):
        return self.step("DELETE", (chain,), lambda want: ("DELETE", want, list(self.model.shard_rows)))


def one_row(command_id, **over):
    row = {"command_id": command_id, "raw_command": RAW, "base_command": b"ls", "shell_type": b"zsh", "exit_code": 2, "timestamp": stamp(7),
           "sudo_used": True, "working_directory": DIR, "user_id": 1003, "user_name": COMMON[3], "host_name": b"host-003", "risk_level": 4}
    row.update(over)
    return row


def history(devices, dry=False, recorder=None):
    """The scripted writers; `recorder`: see History.  On a single shard (tests/concurrent_matrix.py) the same steps take their
    row ranges from the three-shard layout, and what they say about shards 1 and -1 has nothing to hold for."""
    n_shards = len(devices.split(","))
    sharded = n_shards > 1
    first = starts(N, n_shards if sharded else LAYOUTS[0])
    h = History(n_shards, dry, recorder)
    model = h.model
    try:
        for column in ("user_id", "risk_level"):                      # the i32 ranges cached before any writer
            assert dry or h.eng.group_count(column)
        h.check()
        # 1. exactly the rows of shard 1: an empty shard in the middle
        assert h.delete(rows_between(first[1], first[2] - 1)) == first[2] - first[1]
        assert not sharded or (model.shard_rows[1] == 0 and all(model.shard_rows[:1] + model.shard_rows[2:]))
        h.check()
        # 2. a WHERE that matches in the first and the last shard only: a string new to user_name (the codes are bumped on every
        #    shard, the empty one included) and an i32 past the cached range; then an UPDATE the engine must refuse
        chain = ROUTES["band_ends"][0]
        held = shard_counts(np.flatnonzero(model.mask(chain)), model.shard_rows)
        assert held[0] and held[-1] and not any(held[1:-1])
        assert h.update({"user_name": "mmm-middle", "risk_level": 12}, chain) == sum(held)
        assert model.route == dict(bumped=["user_name"])
        h.check()
        assert h.update({"raw_command": "a second raw command"}, chain) is None
        # 3. a batch that outgrows the last shard
        B = model.shard_capacity[-1] - model.shard_rows[-1] + 1
        h.batch(rows_like(B, 3, 3_000_000))
        assert model.route["grown"]
        h.check()
        # 4. the rows of the last shard: an empty shard at the end, after growth; then a single INSERT, and one refused
        last = rows_between(first[-2], N - 1)[0]
        assert h.delete([last, "OR", ("timestamp", ">=", "2026")]) == (N - first[-2]) + B
        assert not sharded or (model.shard_rows[-1] == 0 and model.shard_rows[1] == 0)
        h.check()
        assert h.insert(one_row(7_000_001, user_name=b"aaa-first", timestamp=b"2027-01-01T00:00:00.000Z")) is True
        assert model.shard_rows[-1] == (1 if sharded else first[1] + 1)
        h.check()
        assert h.insert(one_row(7_000_002, raw_command=b"a second raw command")) is None
        # 5. everything deleted, then a batch into the empty table
        h.delete([("user_id", ">=", "0")])
        assert model.n == 0 and not any(model.shard_rows)
        h.check()
        h.batch(rows_like(1500, 5, 5_000_000))
        assert model.shard_rows == [0] * (n_shards - 1) + [1500]
        h.check()
    finally:
        if h.eng:
            h.eng.close()
    return h


def main(argv):
    what, devices = argv[1], argv[2]
    os.environ["PQPS_DEVICES"] = devices                            # read when an engine is created
    if what == "run":
        run(devices, tuple(argv[3:]) or FAMILIES)
    elif what == "history":
        print("CASES", history(devices).count, "OK", flush=True)
    else:
        raise SystemExit(f"shard_matrix: unknown command {what!r}")


if __name__ == "__main__":
    main(sys.argv)
