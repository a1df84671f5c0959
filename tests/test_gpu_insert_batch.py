"""Batch INSERT through the engine (executeQueryInsertColumnsHIP / executeQueryInsertRowsHIP, HipEngine.insert_columns /
insert_rows) on engines without host rows.

After every append the engine must answer exactly as a FRESH engine built by from_columns over the concatenated model -- the
old rows followed by the batch's rows, the dictionaries the sorted unions: select_ids (scan and index mode), count,
group_count, aggregate, count_distinct, order_ids on appended columns, the cells of select_columnar and LIKE / IN chains.  A
refused batch raises PqpsError and leaves every answer as it was.  The model and the indexes are those of test_gpu_update.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qpelib as q
from column_model import apply, coded, concat, copy_model, rows_of, without     # the model operations: shared with the writer sequences

pq = q.pq
pytestmark = pytest.mark.gpu

N = 5003                                                         # a partial last step, a partial last tile
INDEXES = [("risk_level", pq.FIELD_INT), ("user_id", pq.FIELD_INT), ("sudo_used", pq.FIELD_BOOL), ("user_name", pq.FIELD_STRING)]
HOST_INDEX = INDEXES + [("host_name", pq.FIELD_STRING)]
SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
USERS = [b"student%d" % (1000 + i) for i in range(50)]
HOSTS = [b"host-%03d" % i for i in range(256)]                   # a full 1-byte dictionary
BASES = [b"cat", b"cd", b"grep", b"ls", b"make", b"rm", b"ssh", b"vim"]
RAW, STAMP, DIR = b"ls -la", b"2025-01-01T00:00:00.000Z", b"/home/u"
STAMP2 = b"2025-06-01T12:00:00.000Z"
FIRST_ID = 1_000_000                                             # command_id of batch rows: above every old one


def base_model():
    rng = np.random.default_rng(2024)
    user = rng.integers(0, 50, N)
    m = {
        "command_id": np.arange(1, N + 1, dtype=np.uint64),
        "exit_code": rng.integers(0, 3, N).astype(np.int32),
        "user_id": (1000 + user).astype(np.int32),
        "risk_level": rng.integers(1, 6, N).astype(np.int32),
        "sudo_used": (rng.random(N) < 0.3).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, N).astype(np.uint8), list(SHELLS)),
        "user_name": (user.astype(np.uint8), list(USERS)),
        "host_name": (rng.integers(0, 256, N).astype(np.uint8), list(HOSTS)),
        "base_command": (rng.integers(0, 8, N).astype(np.uint8), list(BASES)),
        "raw_command": (None, [RAW]),                            # single-valued: no device buffer
        "timestamp": (None, [STAMP]),
        "working_directory": (None, [DIR]),
    }
    return m


def engine_of(m, indexes=INDEXES):
    return pq.HipEngine.from_columns(rows_of(m), m, indexes)


def make_batch(B, seed, **over):
    """B rows of the model's distributions with only known strings, every dictionary whole; `over` replaces columns."""
    rng = np.random.default_rng(seed)
    user = rng.integers(0, 50, B)
    b = {
        "command_id": np.arange(FIRST_ID * seed + 1, FIRST_ID * seed + B + 1, dtype=np.uint64),
        "exit_code": rng.integers(0, 3, B).astype(np.int32),
        "user_id": (1000 + user).astype(np.int32),
        "risk_level": rng.integers(1, 6, B).astype(np.int32),
        "sudo_used": (rng.random(B) < 0.3).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, B).astype(np.uint8), list(SHELLS)),
        "user_name": (user.astype(np.uint8), list(USERS)),
        "host_name": (rng.integers(0, 256, B).astype(np.uint8), list(HOSTS)),
        "base_command": (rng.integers(0, 8, B).astype(np.uint8), list(BASES)),
        "raw_command": (None, [RAW]),
        "timestamp": (None, [STAMP]),
        "working_directory": (None, [DIR]),
    }
    b.update(over)
    return b


def column_text(m, column):
    codes, values = m[column]
    return np.array(values, dtype=object)[codes] if codes is not None else np.array([values[0]] * rows_of(m), dtype=object)


def records_of(b):
    """The batch as `record`s (the rows form)."""
    text = {name: column_text(b, name) for name, v in b.items() if not isinstance(v, np.ndarray)}
    out = []
    for i in range(rows_of(b)):
        r = pq.Record()
        r.command_id, r.exit_code, r.user_id = int(b["command_id"][i]), int(b["exit_code"][i]), int(b["user_id"][i])
        r.risk_level, r.sudo_used = int(b["risk_level"][i]), bool(b["sudo_used"][i])
        for name, values in text.items():
            setattr(r, name, values[i])
        out.append(r)
    return out


CHAINS = [
    None,
    [("risk_level", "=", "5")],
    [("risk_level", ">", "3")],                                  # index mode: a probe of risk_level
    [("risk_level", "=", "9")],
    [("user_id", "=", "1007")],
    [("user_id", ">=", "1040"), "AND", ("sudo_used", "=", "TRUE")],
    [("sudo_used", "=", "TRUE")],
    [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")],   # scan mode: reads the plane
    [("exit_code", "<", "0"), "OR", ("shell_type", "=", "zsh")],
    [("user_name", ">=", "student1044")],                        # index mode: a probe of the string index
    [("host_name", "<", "host-100"), "AND", ("risk_level", "<=", "2")],
    [("base_command", "=", "make")],
    # the appended rows, by what only they carry
    [("command_id", ">", str(FIRST_ID))],
    [("command_id", ">", str(FIRST_ID)), "AND", ("risk_level", "=", "5")],
    [("user_name", "=", "student1020x")],
    [("user_name", "<", "student1000")],
    [("user_name", ">", "student1049")],
    [("host_name", "=", "host-100x")],
    [("host_name", ">=", "host-100x"), "AND", ("host_name", "<", "host-102")],
    [("timestamp", "=", STAMP2.decode())],
    [("timestamp", "<", STAMP2.decode()), "AND", ("risk_level", "=", "1")],
    # LIKE / IN: windows, and member passes
    [("user_name", "LIKE", "student102%")],
    [("host_name", "LIKE", "%7")],
    [("user_name", "IN", pq.in_list([b"aaa-first", b"student1003", b"zzz-last"]))],
    [("user_name", "NOT IN", pq.in_list([b"student%d" % i for i in (1000, 1004, 1008, 1012, 1016, 1020, 1024)])), "AND", ("risk_level", ">=", "4")],
    [("user_id", "IN", pq.in_list([1001, 1003, 1005, 1007, 1009, 1011]))],
]
CELLS = 13                                                       # the chain whose rows' cells are compared


def answers(eng, order_columns=("risk_level",), group_columns=()):
    out = {}
    for k, chain in enumerate(CHAINS):
        out["ids", k] = eng.select_ids(chain)
        out["count", k] = eng.count(chain)
    for column in ("risk_level", "user_name", "sudo_used", "host_name", "shell_type", "exit_code", "base_command") + tuple(group_columns):
        out["group", column] = eng.group_count(column)
        out["group where", column] = eng.group_count(column, CHAINS[5])
    out["aggregate"] = eng.aggregate("risk_level", "shell_type")
    out["aggregate id"] = eng.aggregate("command_id", None, CHAINS[2])
    out["aggregate exit"] = eng.aggregate("exit_code", "sudo_used")
    out["aggregate user"] = eng.aggregate("exit_code", "user_name", CHAINS[12])
    out["distinct"] = eng.count_distinct("user_name", "risk_level")
    out["distinct all"] = eng.count_distinct("host_name")
    for column in order_columns:
        out["order", column] = eng.order_ids(column, None, False, 60)
        out["order desc", column] = eng.order_ids(column, CHAINS[6], True, 60)
    for k in (4, CELLS):
        res = eng.select_columnar(None, CHAINS[k])
        out["cells", k] = res["rows"]
        eng.free_columnar(res)
    return out


def same_answers(eng, model, indexes=INDEXES, order_columns=("risk_level",), group_columns=(), what=None):
    assert eng.n == rows_of(model) and sum(eng.shards()) == rows_of(model)
    fresh = engine_of(model, indexes)
    try:
        got, want = answers(eng, order_columns, group_columns), answers(fresh, order_columns, group_columns)
        for key in want:
            assert got[key] == want[key], (key, what)
    finally:
        fresh.close()


def check_append(model, batches, indexes=INDEXES, order_columns=("risk_level", "user_name"), group_columns=(), rows_form=False,
                 before=None, after=None):
    """The batches one after the other on a fresh engine over `model`; -> the model after them."""
    eng = engine_of(model, indexes)
    try:
        if before:
            before(eng)
        for b in batches:
            k = eng.insert_rows(records_of(b)) if rows_form else eng.insert_columns(rows_of(b), b)
            assert k == rows_of(b)
            model = concat(model, b)
        if after:
            model = after(eng, model)
        same_answers(eng, model, indexes, order_columns, group_columns, what=[rows_of(b) for b in batches])
    finally:
        eng.close()
    return model


def new_users(B, seed):
    """Known names and three new ones: one in front of every old name, one between two, one behind all."""
    rng = np.random.default_rng(seed)
    names = [b"aaa-first", b"student1020x", b"zzz-last", b"student1005", b"student1049"]
    return make_batch(B, seed, user_name=coded([names[i] for i in rng.integers(0, len(names), B)]))


def test_capacity_formula_of_the_model():
    """5 003 rows leave room for 3 189 more: the edge the head-room cases stand on."""
    assert (N + N // 16 + pq.TILE_ROWS) // pq.TILE_ROWS * pq.TILE_ROWS == 8192 and 8192 - N == 3189


@pytest.mark.parametrize("B", [1, 7])
def test_known_strings_only(B):
    """Every merge is an identity: no remap pass, the codes of the old rows stay."""
    m = base_model()
    after = check_append(m, [make_batch(B, 1)])
    assert after["user_name"][1] == USERS and np.array_equal(after["user_name"][0][:N], m["user_name"][0])
    # the batch's dictionaries hold only what its rows carry: sparse subsets of the table's
    b = make_batch(B, 1)
    for name in ("shell_type", "user_name", "host_name", "base_command"):
        b[name] = coded(list(column_text(b, name)))
    check_append(m, [b])


def test_new_user_names_in_front_between_and_behind():
    m = base_model()
    after = check_append(m, [new_users(40, 1)])
    names = after["user_name"][1]
    assert names[0] == b"aaa-first" and names[-1] == b"zzz-last" and names[22] == b"student1020x" and len(names) == 53


def test_new_string_behind_all_is_an_identity_merge():
    m = base_model()
    check_append(m, [make_batch(5, 1, user_name=coded([b"zzz-last"] * 5), shell_type=coded([b"zsh", b"zzsh", b"zsh", b"zzsh", b"zsh"]))],
                 order_columns=("user_name", "shell_type"))


def test_a_string_no_row_carries_still_enters():
    m = base_model()
    after = check_append(m, [make_batch(3, 1, base_command=coded([b"ls", b"cat", b"ls"], extra=[b"awk", b"zip"]))], order_columns=("base_command",))
    assert after["base_command"][1][0] == b"awk" and len(after["base_command"][1]) == 10


def test_257th_host_name_widens_the_codes():
    """u8 -> u16, by value and through a string index on the column."""
    m = base_model()
    hosts = [b"host-100x"] * 4 + [b"host-007", b"host-255", b"host-100"]
    after = check_append(m, [make_batch(7, 1, host_name=coded(hosts))], indexes=HOST_INDEX, order_columns=("host_name",))
    assert len(after["host_name"][1]) == 257 and after["host_name"][0].dtype == np.uint16


def test_second_timestamp_materialises_the_column():
    m = base_model()
    check_append(m, [make_batch(9, 1, timestamp=(None, [STAMP2]))], order_columns=("timestamp",), group_columns=("timestamp",))
    stamps = [STAMP2, STAMP, STAMP2, b"2024-12-31T23:59:59.000Z", STAMP]
    check_append(m, [make_batch(5, 1, timestamp=coded(stamps), working_directory=coded([b"/tmp", b"/", DIR, b"/tmp", DIR]))],
                 order_columns=("timestamp", "working_directory"), group_columns=("timestamp", "working_directory"))


def test_batch_codes_wider_and_narrower_than_the_columns():
    m = base_model()
    b = new_users(33, 1)
    b["shell_type"] = (b["shell_type"][0].astype(np.uint16), SHELLS)      # 2-byte codes into a 1-byte column
    b["base_command"] = (b["base_command"][0].astype(np.uint32), BASES)
    b["user_name"] = (b["user_name"][0].astype(np.uint32), b["user_name"][1])
    check_append(m, [b])
    # and a table whose codes are wider than the batch's
    wide = copy_model(m)
    wide["user_name"] = (wide["user_name"][0].astype(np.uint16), wide["user_name"][1])
    wide["shell_type"] = (wide["shell_type"][0].astype(np.uint32), wide["shell_type"][1])
    check_append(wide, [new_users(33, 1)], order_columns=("user_name", "shell_type"))


@pytest.mark.parametrize("B", [3189, 3190])
def test_head_room_filled_and_outgrown(B):
    """3 189 rows fill the shard's 8 192 exactly, 3 190 are the first batch that grows it; new names ride along."""
    m = base_model()

    def cache_bounds(eng):                                       # cached i32 ranges must follow the batch
        assert len(eng.group_count("exit_code")) == 3

    b = new_users(B, 1)
    b["exit_code"] = b["exit_code"] - 5                          # below every old value
    check_append(m, [b], before=cache_bounds, order_columns=("exit_code", "user_name"))


def test_two_batches_in_a_row():
    m = base_model()
    check_append(m, [new_users(3000, 1), make_batch(1000, 2, host_name=coded([b"host-100x", b"host-001"] * 500)), make_batch(1, 3)],
                 indexes=HOST_INDEX, order_columns=("host_name", "user_name"))


def one_record(command_id, user_name):
    r = pq.Record()
    r.command_id, r.raw_command, r.base_command, r.shell_type, r.exit_code = command_id, RAW, b"ls", b"zsh", 2
    r.timestamp, r.sudo_used, r.working_directory, r.user_id, r.user_name, r.host_name, r.risk_level = STAMP, True, DIR, 1003, user_name, b"host-003", 4
    return r


def one_row_batch(command_id, user_name):
    return {"command_id": np.array([command_id], dtype=np.uint64), "exit_code": np.array([2], dtype=np.int32),
            "user_id": np.array([1003], dtype=np.int32), "risk_level": np.array([4], dtype=np.int32), "sudo_used": np.array([1], dtype=np.uint8),
            "shell_type": coded([b"zsh"]), "user_name": coded([user_name]), "host_name": coded([b"host-003"]), "base_command": coded([b"ls"]),
            "raw_command": (None, [RAW]), "timestamp": (None, [STAMP]), "working_directory": (None, [DIR])}


def writers_after(eng, model):
    """An UPDATE, a DELETE and a single INSERT on the engine a batch has grown; -> the model after them."""
    mask = column_text(model, "user_name") == b"student1020x"
    assert mask.any()
    assert eng.update({"risk_level": 5, "user_name": "student1020y"}, [("user_name", "=", "student1020x")]) == int(np.count_nonzero(mask))
    model = apply(model, {"risk_level": 5, "user_name": "student1020y"}, mask)
    gone = (model["risk_level"] == 2) & (model["sudo_used"] == 1)
    wl = pq.WhereList([("risk_level", "=", "2"), "AND", ("sudo_used", "=", "TRUE")])
    rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
    assert rs.contents.success
    pq.lib().freeResultSet(rs)
    model = without(model, gone)
    eng.n = eng.e.contents.num_records
    assert pq.lib().executeQueryInsertHIP(eng.e, b"commands", C.byref(one_record(7_000_001, b"mmm-middle")))
    eng.n = eng.e.contents.num_records
    return concat(model, one_row_batch(7_000_001, b"mmm-middle"))


def test_update_delete_and_insert_after_a_batch():
    check_append(base_model(), [new_users(500, 1)], after=writers_after)


def test_rows_form():
    m = base_model()
    b = new_users(61, 1)
    for name in ("shell_type", "host_name", "base_command"):
        b[name] = coded(list(column_text(b, name)))
    b["host_name"] = coded([b"host-100x"] + list(column_text(b, "host_name"))[1:])
    b["timestamp"] = coded([STAMP2 if i % 3 == 0 else STAMP for i in range(61)])
    check_append(m, [b], indexes=HOST_INDEX, rows_form=True, order_columns=("host_name", "timestamp"), group_columns=("timestamp",))
    eng = engine_of(m)
    try:
        assert eng.insert_rows([]) == 0 and eng.insert_columns(0, make_batch(1, 1)) == 0 and eng.n == N
    finally:
        eng.close()


def refused_batches():
    B = 6
    ok = lambda **over: (B, make_batch(B, 1, **over))
    bad_id = np.arange(FIRST_ID, FIRST_ID + B, dtype=np.uint64)
    bad_id[4] = 0
    return {
        "dictionary not ascending": ok(shell_type=(np.zeros(B, dtype=np.uint8), [b"zsh", b"bash"])),
        "dictionary with a duplicate": ok(user_name=(np.zeros(B, dtype=np.uint8), [b"a", b"b", b"b"])),
        "empty string": ok(host_name=(np.ones(B, dtype=np.uint8), [b"", b"host-001"])),
        "string too long for its field": ok(shell_type=(np.zeros(B, dtype=np.uint8), [b"s" * 20])),
        "exit_code 8 bytes wide": ok(exit_code=np.zeros(B, dtype=np.int64)),
        "sudo_used 2 bytes wide": ok(sudo_used=np.zeros(B, dtype=np.uint16)),
        "command_id 4 bytes wide": ok(command_id=np.arange(1, B + 1, dtype=np.uint32)),
        "codes 8 bytes wide": ok(user_name=(np.zeros(B, dtype=np.uint64), USERS)),
        "no codes, two strings": ok(timestamp=(None, [STAMP, STAMP2])),
        "empty dictionary": ok(base_command=(np.zeros(B, dtype=np.uint8), [])),
        "command_id 0": ok(command_id=bad_id),
        "sudo_used 2": ok(sudo_used=np.array([0, 1, 0, 2, 0, 1], dtype=np.uint8)),
        "code at the dictionary count": ok(shell_type=(np.array([0, 1, 2, 3, 4, 0], dtype=np.uint8), SHELLS)),
        "code past the dictionary count, behind new strings": ok(user_name=(np.array([0, 1, 2, 200, 1, 0], dtype=np.uint8), [b"aaa-first", b"mmm", b"zzz-last"])),
        "2-byte code past the dictionary count": ok(base_command=(np.array([0, 1, 2, 3, 300, 0], dtype=np.uint16), BASES)),
        "4-byte code past the dictionary count": ok(host_name=(np.array([0, 1, 2, 3, 1 << 20, 0], dtype=np.uint32), HOSTS)),
        "more than INT_MAX rows in all": ((1 << 31) - N, make_batch(B, 1)),
    }


def test_refusals_leave_the_engine_as_it_was():
    m = base_model()
    eng = engine_of(m)
    try:
        before = answers(eng)
        for what, (n_rows, b) in refused_batches().items():
            with pytest.raises(pq.PqpsError):
                eng.insert_columns(n_rows, b)
            assert eng.n == N, what
        bad = records_of(make_batch(3, 1))
        bad[1].command_id = 0
        with pytest.raises(pq.PqpsError):
            eng.insert_rows(bad)
        bad = records_of(make_batch(3, 1))
        bad[2].user_name = b""
        with pytest.raises(pq.PqpsError):
            eng.insert_rows(bad)
        assert pq.lib().executeQueryInsertRowsHIP(eng.e, b"commands", None, 3, None) == -1
        assert pq.lib().executeQueryInsertColumnsHIP(eng.e, b"commands", 3, None, None) == -1
        # a thread that holds a ticket is refused
        ticket = eng.select_async([("risk_level", "=", "3")])
        assert ticket
        with pytest.raises(pq.PqpsError):
            eng.insert_columns(6, make_batch(6, 1))
        eng.await_ticket(ticket)
        eng.release_ticket(ticket)
        after = answers(eng)
        for key in before:
            assert after[key] == before[key], key
        assert eng.n == N and eng.shards() == [N]
        b = new_users(6, 1)
        assert eng.insert_columns(6, b) == 6
        same_answers(eng, concat(m, b))
    finally:
        eng.close()


def shard_cases():
    """What the two-shard child runs (and what runs here on one shard)."""
    m = base_model()
    check_append(m, [make_batch(7, 1)])
    check_append(m, [new_users(40, 1)])
    hosts = [b"host-100x"] * 4 + [b"host-007", b"host-255", b"host-100"]
    check_append(m, [make_batch(7, 1, host_name=coded(hosts), timestamp=(None, [STAMP2]))], indexes=HOST_INDEX,
                 order_columns=("host_name", "timestamp"), group_columns=("timestamp",))
    eng = engine_of(m)
    last = eng.shards()[-1]
    eng.close()
    room = (last + last // 16 + pq.TILE_ROWS) // pq.TILE_ROWS * pq.TILE_ROWS - last
    for B in (room, room + 1):
        check_append(m, [new_users(B, 1)])
    check_append(m, [new_users(500, 1)], after=writers_after)
    b = new_users(61, 1)
    check_append(m, [b, make_batch(3, 2)], rows_form=True)


def test_two_shards_on_one_gpu():
    """The same cases on an engine of two shards (PQPS_DEVICES read when the engine is created: a child process)."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_insert_batch as T; e = T.engine_of(T.base_model()); "
            "print('SHARDS', len(e.shards())); e.close(); T.shard_cases(); print('DONE')") % str(q.ROOT / "tests")
    two_cards = pq.lib().pqps_device_count() >= 2
    env = dict(os.environ, PQPS_DEVICES="0,1" if two_cards else "0,0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.split() == ["SHARDS", "2", "DONE"]
