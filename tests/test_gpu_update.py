"""UPDATE SET ... WHERE through the engine (executeQueryUpdateHIP / HipEngine.update) on engines without host rows.

After every update the engine must answer exactly as a FRESH engine built by from_columns from the numpy-updated columns and
the updated dictionaries: select_ids (scan and index mode, also probing updated columns), count, group_count, aggregate,
count_distinct, order_ids on the updated column and the cells of select_columnar.  The rows an update selects are computed
here with numpy from the values before it.  A refused update raises PqpsError and leaves every answer as it was."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qpelib as q
from column_model import apply                                  # the model operation: shared with the writer sequences

pq = q.pq
pytestmark = pytest.mark.gpu

N = 5003                                                         # a partial last step, a partial last tile
INDEXES = [("risk_level", pq.FIELD_INT), ("user_id", pq.FIELD_INT), ("sudo_used", pq.FIELD_BOOL), ("user_name", pq.FIELD_STRING)]
SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
USERS = [b"student%d" % (1000 + i) for i in range(50)]
HOSTS = [b"host-%03d" % i for i in range(256)]                   # a full 1-byte dictionary
BASES = [b"cat", b"cd", b"grep", b"ls", b"make", b"rm", b"ssh", b"vim"]
I32 = ("exit_code", "user_id", "risk_level")


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
        "raw_command": (None, [b"ls -la"]),                      # single-valued: no device buffer
        "timestamp": (None, [b"2025-01-01T00:00:00.000Z"]),
        "working_directory": (None, [b"/home/u"]),
    }
    return m


def engine_of(m):
    return pq.HipEngine.from_columns(N, m, INDEXES)


def column_text(m, column):
    """Every row's value of `column` as bytes / int, for masks written in terms of strings."""
    v = m[column]
    if isinstance(v, np.ndarray):
        return v
    codes, values = v
    return np.array(values, dtype=object)[codes] if codes is not None else np.array([values[0]] * N, dtype=object)


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
    [("user_name", ">=", "student1044")],
    [("host_name", "<", "host-100"), "AND", ("risk_level", "<=", "2")],
    [("base_command", "=", "make")],
]


def answers(eng, order_columns=("risk_level",)):
    out = {}
    for k, chain in enumerate(CHAINS):
        out["ids", k] = eng.select_ids(chain)
        out["count", k] = eng.count(chain)
    for column in ("risk_level", "user_name", "sudo_used", "host_name", "shell_type", "exit_code", "base_command"):
        out["group", column] = eng.group_count(column)
        out["group where", column] = eng.group_count(column, CHAINS[5])
    out["aggregate"] = eng.aggregate("risk_level", "shell_type")
    out["aggregate id"] = eng.aggregate("command_id", None, CHAINS[2])
    out["aggregate exit"] = eng.aggregate("exit_code", "sudo_used")
    out["distinct"] = eng.count_distinct("user_name", "risk_level")
    out["distinct all"] = eng.count_distinct("host_name")
    for column in order_columns:
        out["order", column] = eng.order_ids(column, None, False, 60)
        out["order desc", column] = eng.order_ids(column, CHAINS[6], True, 60)
    res = eng.select_columnar(None, CHAINS[4])
    out["cells"] = res["rows"]
    eng.free_columnar(res)
    return out


def check_update(model, assignments, chain, mask, order_columns=("risk_level",), before=None):
    """One update on a fresh engine over `model`; -> the model after it."""
    eng = engine_of(model)
    try:
        if before:
            before(eng)
        assert eng.update(assignments, chain) == int(np.count_nonzero(mask))
        after = apply(model, assignments, mask)
        fresh = engine_of(after)
        try:
            got, want = answers(eng, order_columns), answers(fresh, order_columns)
            for key in want:
                assert got[key] == want[key], (key, assignments, chain)
        finally:
            fresh.close()
    finally:
        eng.close()
    return after


def test_i32_target_where_on_the_same_column():
    m = base_model()
    after = check_update(m, {"risk_level": 5}, [("risk_level", "=", "3")], m["risk_level"] == 3)
    assert np.count_nonzero(after["risk_level"] == 3) == 0
    check_update(m, {"risk_level": "2"}, [("risk_level", ">", "2"), "AND", ("risk_level", "<", "5")],
                 (m["risk_level"] > 2) & (m["risk_level"] < 5))


def test_null_where_every_row():
    m = base_model()
    check_update(m, {"exit_code": -4}, None, np.ones(N, dtype=bool), order_columns=("exit_code",))


def test_where_that_matches_nothing():
    m = base_model()
    after = check_update(m, {"risk_level": 1, "user_name": "nobody"}, [("user_id", "=", "77")], np.zeros(N, dtype=bool))
    assert np.array_equal(after["risk_level"], m["risk_level"])


def test_sudo_used_then_a_scan_of_the_plane():
    m = base_model()
    mask = (m["user_id"] >= 1020) & (m["sudo_used"] == 0)
    check_update(m, {"sudo_used": "TRUE"}, [("user_id", ">=", "1020"), "AND", ("sudo_used", "=", "FALSE")], mask)
    check_update(m, {"sudo_used": False}, [("sudo_used", "=", "TRUE")], m["sudo_used"] == 1)


def test_string_already_in_the_dictionary():
    m = base_model()
    check_update(m, {"user_name": "student1002"}, [("user_name", "=", "student1044")], m["user_name"][0] == 44,
                 order_columns=("user_name",))
    check_update(m, {"host_name": HOSTS[255]}, [("risk_level", "=", "1")], m["risk_level"] == 1, order_columns=("host_name",))


def test_new_string_between_two_existing_ones():
    m = base_model()
    mask = (m["user_name"][0] >= 30) & (m["risk_level"] == 4)
    after = check_update(m, {"user_name": "student1020x"}, [("user_name", ">=", "student1030"), "AND", ("risk_level", "=", "4")], mask,
                         order_columns=("user_name",))
    assert after["user_name"][1][21] == b"student1020x" and len(after["user_name"][1]) == 51
    check_update(m, {"shell_type": "a-first-shell", "base_command": "zz-last"}, [("exit_code", "=", "1")], m["exit_code"] == 1,
                 order_columns=("shell_type", "base_command"))


def test_i32_value_outside_the_cached_bounds():
    m = base_model()

    def cache_bounds(eng):
        assert [k for k, _ in eng.group_count("risk_level")] == ["1", "2", "3", "4", "5"]
        assert len(eng.group_count("exit_code")) == 3

    mask = m["user_id"] == 1003
    check_update(m, {"risk_level": 9, "exit_code": -7}, [("user_id", "=", "1003")], mask, order_columns=("risk_level", "exit_code"),
                 before=cache_bounds)


def test_two_and_three_columns_in_one_call():
    m = base_model()
    mask = m["shell_type"][0] == 2
    check_update(m, {"risk_level": 4, "sudo_used": "1"}, [("shell_type", "=", "sh")], mask)
    check_update(m, {"command_id": 99999999999, "user_id": 1049, "user_name": "student1049"}, [("shell_type", "=", "sh")], mask,
                 order_columns=("command_id", "user_id"))


def model_spec(m):
    s = pq.SchemaSpec()
    for name, v in m.items():
        if isinstance(v, np.ndarray):
            s.set_numeric(name, v.dtype.itemsize)
        else:
            s.set_dict(name, 1, v[1])
    return s


def test_in_list_that_is_a_member_pass():
    """An IN list of six far-apart runs is a pass of its own in front of the scan: the flags route."""
    m = base_model()
    ids = [1001, 1003, 1005, 1007, 1009, 1011]
    chain = [("user_id", "IN", pq.in_list(ids)), "AND", ("risk_level", ">=", "2")]
    assert sum(member is not None for _, _, member in pq.compile_plan_sets(model_spec(m), chain)) == 1
    mask = np.isin(m["user_id"], ids) & (m["risk_level"] >= 2)
    check_update(m, {"user_id": 1001, "risk_level": 1}, chain, mask, order_columns=("user_id",))
    names = [b"student%d" % i for i in (1000, 1004, 1008, 1012, 1016, 1020, 1024)]
    chain = [("user_name", "NOT IN", pq.in_list(names))]
    assert sum(member is not None for _, _, member in pq.compile_plan_sets(model_spec(m), chain)) == 1
    check_update(m, {"user_name": "student1000"}, chain, ~np.isin(m["user_name"][0], [0, 4, 8, 12, 16, 20, 24]), order_columns=("user_name",))


def test_like_in_the_where():
    m = base_model()
    mask = np.array([v.endswith(b"7") for v in column_text(m, "host_name")])
    check_update(m, {"risk_level": 3}, [("host_name", "LIKE", "%7")], mask)


def test_single_valued_column_its_own_value():
    m = base_model()
    check_update(m, {"working_directory": "/home/u", "risk_level": 2}, [("risk_level", "=", "5")], m["risk_level"] == 5)
    check_update(m, {"timestamp": "2025-01-01T00:00:00.000Z"}, [("risk_level", "=", "5")], m["risk_level"] == 5)


def shard_cases():
    """What the two-shard child runs (and what runs here on one shard)."""
    m = base_model()
    check_update(m, {"risk_level": 5}, [("risk_level", "=", "3")], m["risk_level"] == 3)
    check_update(m, {"sudo_used": "TRUE", "user_name": "student1020x"}, [("user_id", ">=", "1020"), "AND", ("sudo_used", "=", "FALSE")],
                 (m["user_id"] >= 1020) & (m["sudo_used"] == 0), order_columns=("user_name",))
    ids = [1001, 1003, 1005, 1007, 1009, 1011]
    check_update(m, {"exit_code": 2}, [("user_id", "IN", pq.in_list(ids))], np.isin(m["user_id"], ids), order_columns=("exit_code",))
    # rows of the second shard only: the first shard's indexes stay, its answers too
    check_update(m, {"risk_level": 1}, [("command_id", ">", "4000")], m["command_id"] > 4000)


def test_two_shards_on_one_gpu():
    """The same cases on an engine of two shards (PQPS_DEVICES read when the engine is created: a child process)."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_update as T; e = T.engine_of(T.base_model()); "
            "print('SHARDS', len(e.shards())); e.close(); T.shard_cases(); print('DONE')") % str(q.ROOT / "tests")
    two_cards = pq.lib().pqps_device_count() >= 2
    env = dict(os.environ, PQPS_DEVICES="0,1" if two_cards else "0,0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.split() == ["SHARDS", "2", "DONE"]


REFUSED = {
    "unknown column": {"risk": 1},
    "empty string": {"host_name": ""},
    "string too long": {"shell_type": "s" * 20},
    "command_id 0": {"command_id": 0},
    "no assignment": {},
    "single-valued column, another value": {"working_directory": "/tmp"},
    "257th value of a 1-byte dictionary": {"host_name": "host-new"},
}


def test_refusals_leave_the_engine_as_it_was():
    m = base_model()
    eng = engine_of(m)
    try:
        before = answers(eng)
        for what, assignments in REFUSED.items():
            with pytest.raises(pq.PqpsError):
                eng.update(assignments, [("risk_level", "=", "3")])
        # the same column twice cannot be said with a dict; and the plain return value of the C function
        names = (C.c_char_p * 2)(b"risk_level", b"risk_level")
        values = (C.c_char_p * 2)(b"1", b"2")
        assert pq.lib().executeQueryUpdateHIP(eng.e, b"commands", names, values, 2, None, None) == -1
        assert pq.lib().executeQueryUpdateHIP(eng.e, b"commands", names, values, 13, None, None) == -1
        # a WHERE that cannot be compiled
        with pytest.raises(pq.PqpsError):
            eng.update({"risk_level": 1}, [("risk_level", "LIKE", "3%")])
        # a thread that holds a ticket is refused
        ticket = eng.select_async([("risk_level", "=", "3")])
        assert ticket
        with pytest.raises(pq.PqpsError):
            eng.update({"risk_level": 1}, [("risk_level", "=", "3")])
        eng.await_ticket(ticket)
        eng.release_ticket(ticket)
        after = answers(eng)
        for key in before:
            assert after[key] == before[key], key
        assert eng.update({"risk_level": 1}, [("risk_level", "=", "3")]) == int(np.count_nonzero(m["risk_level"] == 3))
    finally:
        eng.close()
