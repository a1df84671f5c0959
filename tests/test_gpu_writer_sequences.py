"""Sequences of writers on an engine without host rows, every step compared with tests/column_model.py.

tests/test_gpu_update.py and tests/test_gpu_insert_batch.py compare a mutated engine with a FRESH engine over the numpy-updated
columns: both sides run the same kernels, so a defect they share is invisible, and their histories are short.  Here the
reference is the CPU model (the oracle's scan and index walk over the model's arrays, the suite's reference folds over its
cells; tests/test_column_model.py checks it without a GPU), and the table goes through the states only a history reaches: a
shard a DELETE emptied and writers after it, growth + widening + materialisation in one batch, pqps_bump_codes at the width a
batch widened to, a table deleted to nothing and refilled, a dictionary filled to the last code of its width, i32 bounds
cached before the writers that leave them.

After every step check() asks select_ids and count over the 26 chains of test_gpu_insert_batch.py, group_count, aggregate,
count_distinct (a bitmap shape and command_id: the sort form), order_ids, group_pair (dense, and the sort form once the product
of user_name x host_name exceeds 65 536), group_buckets, select_ordered, group_first (a narrow key and command_id), order_ids_by
(two keys), select_group_first, the cells of select_columnar and three tickets in flight at once -- and compares each answer
exactly.  A refusal the model predicts (a writer the engine cannot make in place; a
group column of more than 65 536 values) must be a refusal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import column_model as cm
import qpelib as q
import test_gpu_insert_batch as ib
import test_gpu_update as up

pq = q.pq
pytestmark = pytest.mark.gpu

CHAINS = ib.CHAINS
INDEXES = ib.HOST_INDEX
REFUSED = "refused"
SEVEN = [b"student%d" % i for i in (1000, 1004, 1008, 1012, 1016, 1020, 1024)]
STAMP3, DIR2 = b"2024-12-31T23:59:59.000Z", b"/tmp"
ORDER_KEYS = [("user_name", True), ("exit_code", False)]


def ask(call):
    try:
        return call()
    except pq.PqpsError:
        return REFUSED


def columnar_rows(res_of, eng):
    res = res_of()
    try:
        return res["rows"], res.get("matches")
    finally:
        eng.free_columnar(res)


def queries(model, eng=None):
    """[(what, the engine's answer, the model's answer)] as callables, for the state the model is in."""
    ids = {}

    def rows(k):
        if k not in ids:
            ids[k] = model.select_ids(CHAINS[k], INDEXES)
        return ids[k]

    def grouped(columns, want):
        return (lambda: REFUSED) if any(model.group_refused(c) for c in columns if c) else want

    out = []
    for k, chain in enumerate(CHAINS):
        out.append((("ids", k), lambda chain=chain: eng.select_ids(chain), lambda k=k: rows(k)))
        out.append((("count", k), lambda chain=chain: eng.count(chain), lambda k=k: len(rows(k))))
    for column in ("risk_level", "user_name", "sudo_used", "host_name", "shell_type", "exit_code", "user_id", "base_command", "timestamp"):
        for k in (0, 5):
            out.append((("group", column, k), lambda column=column, k=k: eng.group_count(column, CHAINS[k]),
                        grouped([column], lambda column=column, k=k: model.group_count(column, rows(k)))))
    for value, group, k in (("risk_level", "shell_type", 0), ("command_id", None, 2), ("exit_code", "sudo_used", 0), ("exit_code", "user_name", 12)):
        out.append((("aggregate", value, group, k), lambda value=value, group=group, k=k: eng.aggregate(value, group, CHAINS[k]),
                    grouped([group], lambda value=value, group=group, k=k: model.aggregate(value, group, rows(k)))))
    for value, group, k in (("user_name", "risk_level", 0), ("host_name", None, 0), ("command_id", None, 0), ("command_id", "sudo_used", 2)):
        out.append((("distinct", value, group, k), lambda value=value, group=group, k=k: eng.count_distinct(value, group, CHAINS[k]),
                    grouped([group], lambda value=value, group=group, k=k: model.count_distinct(value, group, rows(k)))))
    for column in ("risk_level", "exit_code", "user_name", "host_name"):
        for k, desc in ((0, False), (6, True)):
            out.append((("order", column, k, desc), lambda column=column, k=k, desc=desc: eng.order_ids(column, CHAINS[k], desc, 60),
                        lambda column=column, k=k, desc=desc: model.order_ids(column, rows(k), desc, 60)))
    pairs = [(("shell_type", "risk_level"), None, 0), (("shell_type", "risk_level"), "exit_code", 5), (("sudo_used", "base_command"), "command_id", 2)]
    if len(model.m["user_name"][1]) * len(model.m["host_name"][1]) > cm.GROUP_MAX_BINS:
        pairs += [(("user_name", "host_name"), None, 0), (("user_name", "host_name"), "exit_code", 2)]
    for pair, value, k in pairs:
        out.append((("pair", pair, value, k), lambda pair=pair, value=value, k=k: eng.group_pair(pair, value, CHAINS[k]),
                    grouped(pair, lambda pair=pair, value=value, k=k: model.group_pair(pair, value, rows(k)))))
    shapes = [("user_name", 9, None), ("user_id", None, 16), ("exit_code", None, 4)]
    if model.width["timestamp"]:
        shapes.append(("timestamp", 13, None))
    for column, prefix, width in shapes:
        for value in (None, "risk_level"):
            out.append((("buckets", column, prefix, width, value),
                        lambda column=column, prefix=prefix, width=width, value=value: eng.group_buckets(column, prefix=prefix, width=width, value_column=value),
                        lambda column=column, prefix=prefix, width=width, value=value: model.group_buckets(column, prefix, width, value, rows(0))))

    def ordered_model():
        order, matches = model.order_ids("user_name", rows(1), True, 25)
        return model.project(order), matches

    out.append((("ordered",), lambda: columnar_rows(lambda: eng.select_ordered(None, CHAINS[1], "user_name", True, 25), eng), ordered_model))
    for group, column, k, desc in (("user_name", "exit_code", 0, False), ("shell_type", "command_id", 2, True)):
        out.append((("first", group, column, k, desc), lambda group=group, column=column, k=k, desc=desc: eng.group_first(group, column, CHAINS[k], desc),
                    grouped([group], lambda group=group, column=column, k=k, desc=desc: model.group_first(group, column, rows(k), desc))))
    out.append((("order by", 5), lambda: eng.order_ids_by(ORDER_KEYS, CHAINS[5], 60), lambda: model.order_ids_by(ORDER_KEYS, rows(5), 60)))

    def first_model():
        groups, total = model.group_first("risk_level", "host_name", rows(6), True)
        return model.project([r for _, r, _ in groups]), total

    out.append((("first rows",), lambda: columnar_rows(lambda: eng.select_group_first(None, CHAINS[6], "risk_level", "host_name", True), eng), first_model))
    for k in (4, ib.CELLS):
        out.append((("cells", k), lambda k=k: columnar_rows(lambda: eng.select_columnar(None, CHAINS[k]), eng)[0], lambda k=k: model.project(rows(k))))
    return out


def expected(model):
    """The model's side of check() alone (what the CPU reference costs)."""
    return {what: want() for what, _, want in queries(model)} | {("tickets",): ticket_answers(model)}


TICKETS = ((7, False), (2, False), (5, True))                    # (chain, count only): a scan of the plane, an index probe, a COUNT


def ticket_answers(model):
    return [len(model.select_ids(CHAINS[k], INDEXES)) if count_only else model.select_ids(CHAINS[k], INDEXES) for k, count_only in TICKETS]


def tickets_in_flight(eng):
    """Three tickets issued before the first is awaited; -> their answers (the IDs read from the device)."""
    tickets = [eng.select_async(CHAINS[k], count_only) for k, count_only in TICKETS]
    out = []
    ctx = pq.Context(0)
    try:
        assert all(tickets)
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


def record_of(row):
    r = pq.Record()
    for column, value in row.items():
        setattr(r, column, value)
    return r


class Run:
    """An engine over base_model() with HOST_INDEX, the model beside it, and the writers made so far."""

    def __init__(self):
        m = ib.base_model()
        self.eng = ib.engine_of(m, INDEXES)
        self.model = cm.ColumnModel(m, len(self.eng.shards()))
        self.log = []

    def close(self):
        self.eng.close()

    def note(self, what):
        self.log.append((what, self.model.route))

    def check(self):
        eng, model = self.eng, self.model
        eng.n = eng.e.contents.num_records
        assert eng.n == model.n and eng.shards() == model.shard_rows, self.log
        for what, engine_says, model_says in queries(model, eng):
            got, want = ask(engine_says), model_says()
            assert got == want, (what, self.log)
        got, want = tickets_in_flight(eng), ticket_answers(model)
        assert got == want, ("tickets", self.log)

    # the writers: the model says what must come back, refusals included
    def update(self, assignments, chain):
        want = self.model.update(assignments, chain)
        self.note(("UPDATE", assignments, chain, want))
        if want is None:
            with pytest.raises(pq.PqpsError):
                self.eng.update(assignments, chain)
        else:
            assert self.eng.update(assignments, chain) == want, self.log
        return want

    def batch(self, b):
        want = self.model.insert_batch(b)
        self.note(("batch INSERT", want))
        assert self.eng.insert_columns(cm.rows_of(b), b) == want, self.log

    def insert(self, row):
        want = self.model.insert_one(row)
        self.note(("INSERT", row, want))
        assert bool(pq.lib().executeQueryInsertHIP(self.eng.e, b"commands", C.byref(record_of(row)))) == (want is True), self.log
        return want

    def delete(self, chain):
        want = self.model.delete(chain)
        self.note(("DELETE", chain, want))
        rs = pq.lib().executeQueryDeleteHIP(self.eng.e, b"commands", pq.WhereList(chain).ptr)
        ok, k = bool(rs.contents.success), rs.contents.numRecords
        pq.lib().freeResultSet(rs)
        assert ok and k == want, self.log


def passes(model, chain):
    """(scan passes, member passes) of the WHERE over the model's dictionaries."""
    plan = pq.compile_plan_sets(up.model_spec(model.m), chain)
    members = sum(member is not None for _, _, member in plan)
    return len(plan) - members, members


def texts_with(b, column, new):
    """The batch's strings of `column` with `new` in the first rows."""
    texts = list(ib.column_text(b, column))
    texts[:len(new)] = new
    return cm.coded(texts, dtype=np.uint16)


# ---- the scripted history: step k needs the writers of steps 1 .. k - 1 --------------------------------------------------------
def step_1(run, checked):
    """The i32 bounds cached before any writer."""
    for column in ("exit_code", "user_id", "risk_level"):
        assert run.eng.group_count(column)
    assert run.eng.group_buckets("user_id", width=16) and run.eng.group_buckets("exit_code", width=4)
    if checked:
        run.check()


def step_2(run, checked):
    """The fused UPDATE: one pass that reads the plane, assigns the byte column and puts an i32 outside the cached range."""
    chain = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
    assert passes(run.model, chain) == (1, 0)
    assert run.update({"exit_code": -7, "sudo_used": "TRUE"}, chain) > 50
    if checked:
        run.check()


def step_3(run, checked):
    """40 rows with names in front of, between and behind all old ones: no identity, remapped in place, no growth."""
    run.batch(ib.new_users(40, 1))
    assert run.model.route == dict(grown=False, widened=[], materialised=[], remapped=["user_name"])
    if checked:
        run.check()


def step_4(run, checked):
    """DELETE of the first shard's rows: on two shards shard 0 is left with no rows and shard 1 starts at row 0."""
    first = run.model.shard_rows[0] if len(run.model.shard_rows) > 1 else cm.partition(ib.N, 2)[0]
    run.delete([("command_id", "<=", str(int(run.model.m["command_id"][first - 1])))])
    assert run.model.n == ib.N + 40 - first and (len(run.model.shard_rows) == 1 or run.model.shard_rows[0] == 0)
    if checked:
        run.check()


def step_5(run, checked):
    """The flags route (a member pass) with a new string: the codes are bumped on a table with an empty shard."""
    chain = [("user_name", "IN", pq.in_list(SEVEN))]
    assert passes(run.model, chain) == (1, 1)
    assert run.update({"user_name": "mmm-middle", "risk_level": 5}, chain) > 100
    assert run.model.route == dict(bumped=["user_name"])
    if checked:
        run.check()


def step_6(run, checked):
    """One batch that outgrows the last shard, widens host_name on every shard, materialises two columns and leaves the cached
    exit_code range on both sides."""
    B = run.model.shard_capacity[-1] - run.model.shard_rows[-1] + 1
    b = ib.make_batch(B, 6)
    b["host_name"] = texts_with(b, "host_name", [b"host-100x"] * 4)
    b["timestamp"] = cm.coded([ib.STAMP2 if i % 3 == 0 else ib.STAMP for i in range(B)])
    b["working_directory"] = cm.coded([DIR2 if i % 5 == 0 else ib.DIR for i in range(B)])
    b["exit_code"][:2] = (-9, 7)
    run.batch(b)
    assert run.model.route == dict(grown=True, widened=["host_name"], materialised=["timestamp", "working_directory"], remapped=[])
    assert run.model.width["host_name"] == 2 and len(run.model.m["host_name"][1]) == 257
    if checked:
        run.check()


def one_row(command_id, **over):
    row = {"command_id": command_id, "raw_command": ib.RAW, "base_command": b"ls", "shell_type": b"zsh", "exit_code": 2, "timestamp": ib.STAMP,
           "sudo_used": True, "working_directory": ib.DIR, "user_id": 1003, "user_name": b"student1003", "host_name": b"host-003", "risk_level": 4}
    row.update(over)
    return row


def step_7(run, checked):
    """A single INSERT whose host_name sorts first: pqps_bump_codes at width 2; then one the engine must refuse."""
    assert run.insert(one_row(7_000_001, host_name=b"a-host-first")) is True
    assert run.model.route == dict(bumped=["host_name"]) and run.model.width["host_name"] == 2
    if checked:
        run.check()
    assert run.insert(one_row(7_000_002, raw_command=b"a second raw command")) is None      # raw_command has no buffer
    if checked:
        run.check()


def step_8(run, checked):
    """UPDATE of the widened, indexed column by a condition on itself, to a string new to it."""
    assert run.update({"host_name": "host-000a"}, [("host_name", ">=", "host-200")]) > 500
    assert run.model.route == dict(bumped=["host_name"])
    if checked:
        run.check()


def step_9(run, checked):
    """Every row deleted; every form answers on the empty table; 3 000 rows into it with a string new to every dictionary."""
    run.delete([("command_id", ">", "0")])
    assert run.model.n == 0
    if checked:
        run.check()
    B = 3000
    b = ib.make_batch(B, 9)
    for column, new in (("raw_command", b"cat /etc/passwd"), ("base_command", b"awk"), ("shell_type", b"ash"), ("timestamp", STAMP3),
                        ("working_directory", b"/var/log"), ("user_name", b"student1010x"), ("host_name", b"host-300")):
        b[column] = texts_with(b, column, [new] * 7)
    run.batch(b)
    assert run.model.route["materialised"] == ["raw_command"] and not run.model.route["grown"]
    if checked:
        run.check()


def step_10(run, checked):
    """user_name filled to the last 2-byte code by strings no row carries; the next name is refused to an UPDATE and widens
    the codes to 4 bytes in a batch."""
    names = run.model.m["user_name"][1]
    filler = [b"filler-%05d" % i for i in range(65536 - len(names))]
    b = ib.make_batch(4, 10, user_name=cm.coded([names[0], names[-1], names[3], names[3]], dtype=np.uint16, extra=filler))
    run.batch(b)
    assert run.model.route["widened"] == ["user_name"] and run.model.width["user_name"] == 2 and len(run.model.m["user_name"][1]) == 65536
    if checked:
        run.check()
    chain = [("risk_level", "=", "2")]
    assert run.update({"user_name": "name-65537"}, chain) is None
    if checked:
        run.check()
    run.batch(ib.make_batch(5, 11, user_name=cm.coded([b"name-65537"] * 5)))
    assert run.model.route["widened"] == ["user_name"] and run.model.width["user_name"] == 4 and run.model.group_refused("user_name")
    if checked:
        run.check()
    assert run.update({"user_name": "name-65538"}, chain) > 0                     # 4-byte codes have room
    if checked:
        run.check()


STEPS = (step_1, step_2, step_3, step_4, step_5, step_6, step_7, step_8, step_9, step_10)


@pytest.mark.parametrize("step", range(1, len(STEPS) + 1))
def test_history(step):
    run = Run()
    try:
        for k in range(step - 1):
            STEPS[k](run, False)
        STEPS[step - 1](run, True)
    finally:
        run.close()


# ---- the seeded random tail ------------------------------------------------------------------------------------------------------
NEW_STRINGS = {
    "raw_command": (b"ls -l %d", b"zcat f%d"), "base_command": (b"awk%d", b"zip%d"), "shell_type": (b"ash%d", b"tcsh%d"),
    "timestamp": (b"2024-01-01T00:00:%02d.000Z", b"2025-03-03T03:03:%02d.000Z"), "working_directory": (b"/a/%d", b"/var/%d"),
    "user_name": (b"aaa-%d", b"student10%02dq", b"zzz-%d"), "host_name": (b"a-host-%d", b"host-%03dx", b"zz-host-%d"),
}
I32_RANGE = {"exit_code": (-9, 12), "user_id": (990, 1060), "risk_level": (0, 9)}


def new_string(rng, column):
    shapes = NEW_STRINGS[column]
    return shapes[int(rng.integers(len(shapes)))] % int(rng.integers(60))


def random_value(rng, model, column):
    if column in I32_RANGE:
        return int(rng.integers(*I32_RANGE[column]))
    if column == "sudo_used":
        return bool(rng.integers(2))
    if column == "command_id":
        return int(rng.integers(1, 1 << 40))
    values = model.m[column][1]
    return values[int(rng.integers(len(values)))] if rng.random() < 0.6 else new_string(rng, column)


def random_batch(rng, model, B, seed):
    b = ib.make_batch(B, seed)
    b["exit_code"] = rng.integers(*I32_RANGE["exit_code"], B).astype(np.int32)
    for column in cm.STRINGS:
        new = [new_string(rng, column) for _ in range(int(rng.integers(0, 4)))]
        if new:
            texts = list(ib.column_text(b, column))
            for s in new[:B]:
                texts[int(rng.integers(B))] = s
            b[column] = cm.coded(texts, dtype=np.uint16, extra=new)            # (one of them may be a string no row carries)
    return b


def random_tail(run, seed, writers=12):
    rng = np.random.default_rng(seed)
    step_1(run, False)
    run.check()
    for k in range(writers):
        move = rng.choice(["update", "batch", "insert", "delete"], p=[0.35, 0.3, 0.2, 0.15])
        if move == "update":
            columns = rng.choice(pq.COLUMNS, size=int(rng.integers(1, 4)), replace=False)
            run.update({str(c): random_value(rng, run.model, str(c)) for c in columns}, CHAINS[int(rng.integers(len(CHAINS)))])
        elif move == "batch":
            run.batch(random_batch(rng, run.model, int(rng.integers(1, 601)), 100 * seed + k))
        elif move == "insert":
            run.insert({c: random_value(rng, run.model, c) for c in pq.COLUMNS})
        else:
            run.delete(CHAINS[int(rng.integers(1, len(CHAINS)))])
        assert run.model.n <= 20_000
        run.check()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tail(seed):
    run = Run()
    try:
        random_tail(run, seed)
    finally:
        run.close()


# ---- two shards ---------------------------------------------------------------------------------------------------------------------
def shard_history():
    run = Run()
    try:
        for step in STEPS:
            step(run, True)
    finally:
        run.close()


def shard_tail():
    run = Run()
    try:
        random_tail(run, 1)
    finally:
        run.close()


@pytest.mark.parametrize("what", ["history", "tail"])
def test_two_shards_on_one_gpu(what):
    """The scripted history and seed 1 on an engine of two shards (PQPS_DEVICES read when the engine is created: a child process)."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_writer_sequences as T; r = T.Run(); "
            "print('SHARDS', len(r.eng.shards())); r.close(); T.shard_%s(); print('DONE')") % (str(q.ROOT / "tests"), what)
    two_cards = pq.lib().pqps_device_count() >= 2
    env = dict(os.environ, PQPS_DEVICES="0,1" if two_cards else "0,0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.split() == ["SHARDS", "2", "DONE"]
