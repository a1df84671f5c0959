"""Batch INSERT on an engine with host rows and a CSV (HipEngine(csv)): insert_rows appends the batch to the file in
write_csv_row's format -- the bytes that many single INSERTs leave --, grows the host rows and takes the device route of the
engines without host rows.  Afterwards the file is the original bytes followed by the new lines, engine.record(i) shows the new
rows, and the engine answers as a fresh engine opened on that file.  insert_columns is refused there, the file untouched."""
import ctypes as C
import shutil

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

CSV2K = q.ROOT / "tests" / "golden" / "commands_2k.csv"
INDEXES = [("risk_level", pq.FIELD_INT), ("user_id", pq.FIELD_INT), ("user_name", pq.FIELD_STRING)]
CHAINS = [
    None,
    [("risk_level", ">", "3")],
    [("user_id", "=", "1007")],
    [("command_id", ">=", "900000")],
    [("command_id", ">=", "900000"), "AND", ("sudo_used", "=", "TRUE")],
    [("user_name", "=", "aaa_batch_user")],
    [("user_name", ">=", "zzz")],
    [("host_name", "=", "batch-host-3"), "OR", ("shell_type", "=", "zsh")],
    [("timestamp", ">=", "2031-")],
    [("user_name", "LIKE", "%batch%")],
    [("host_name", "IN", pq.in_list([b"batch-host-1", b"batch-host-5", b"nowhere"]))],
]


def make_records(B, first_id=900_000, tag=b"batch"):
    """Rows with names in front of, among and behind the file's, hosts and timestamps the file does not hold."""
    rng = np.random.default_rng(B)
    names = [b"aaa_" + tag + b"_user", b"student1030", b"student1020_" + tag, b"zzz_" + tag + b"_user"]
    out = []
    for i in range(B):
        r = pq.Record()
        r.command_id, r.raw_command, r.base_command = first_id + i, b"tar -xzf a.tgz", b"tar"
        r.shell_type, r.exit_code, r.timestamp = [b"bash", b"zsh", b"tcsh"][i % 3], int(rng.integers(-2, 3)), b"2031-01-%02dT00:00:00.000Z" % (1 + i % 28)
        r.sudo_used, r.working_directory, r.user_id = bool(i % 4 == 1), b"/srv/batch", 1000 + i % 50
        r.user_name, r.host_name, r.risk_level = names[int(rng.integers(0, 4))], b"batch-host-%d" % (i % 7), int(rng.integers(1, 6))
        out.append(r)
    return out


def line_of(r):
    """write_csv_row's format (engine/hip/executeEngine-hip.c)."""
    return b"%d,%s,%s,%s,%d,%s,%d,%s,%d,%s,%s,%d\n" % (r.command_id, r.raw_command, r.base_command, r.shell_type, r.exit_code, r.timestamp,
                                                       int(r.sudo_used), r.working_directory, r.user_id, r.user_name, r.host_name, r.risk_level)


def answers(eng):
    out = {}
    for k, chain in enumerate(CHAINS):
        out["ids", k] = eng.select_ids(chain)
        out["count", k] = eng.count(chain)
    for column in ("user_name", "host_name", "risk_level", "sudo_used", "shell_type", "exit_code"):
        out["group", column] = eng.group_count(column)
    out["aggregate"] = eng.aggregate("exit_code", "user_name", CHAINS[1])
    out["distinct"] = eng.count_distinct("user_name", "shell_type")
    out["order"] = eng.order_ids("user_name", None, True, 40)
    out["order stamp"] = eng.order_ids("timestamp", CHAINS[3], False, 40)
    out["rows"] = eng.select(None, CHAINS[4])["rows"]
    return out


def same_as_a_fresh_engine(eng, path):
    fresh = pq.HipEngine(path, INDEXES)
    try:
        assert fresh.n == eng.n
        got, want = answers(eng), answers(fresh)
        for key in want:
            assert got[key] == want[key], key
    finally:
        fresh.close()


def test_rows_go_to_the_file_the_host_rows_and_the_device(tmp_path):
    path = tmp_path / "data.csv"
    shutil.copy(CSV2K, path)
    original = path.read_bytes()
    assert original.endswith(b"\n")
    eng = pq.HipEngine(path, INDEXES)
    try:
        n0 = eng.n
        batch = make_records(300)
        assert eng.insert_rows(batch) == 300 and eng.n == n0 + 300
        text = original + b"".join(line_of(r) for r in batch)
        assert path.read_bytes() == text
        for i in (0, 1, 150, 299):
            r, w = eng.record(n0 + i), batch[i]
            assert (r.command_id, r.exit_code, r.user_id, r.risk_level, bool(r.sudo_used)) == (w.command_id, w.exit_code, w.user_id, w.risk_level, bool(w.sudo_used))
            assert (r.user_name, r.host_name, r.timestamp, r.raw_command) == (w.user_name, w.host_name, w.timestamp, w.raw_command)
        assert eng.record(n0 - 1).command_id != 0                 # (the old rows, in a row store that has moved)
        same_as_a_fresh_engine(eng, path)
        # a second batch, one row, then a single INSERT: the same bytes as single INSERTs leave
        (one,) = make_records(1, first_id=950_000, tag=b"second")
        assert eng.insert_rows([one]) == 1
        single = make_records(2, first_id=960_000, tag=b"single")[1]
        assert pq.lib().executeQueryInsertHIP(eng.e, b"commands", C.byref(single))
        eng.n = eng.e.contents.num_records
        text += line_of(one) + line_of(single)
        assert path.read_bytes() == text and eng.n == n0 + 302
        same_as_a_fresh_engine(eng, path)
    finally:
        eng.close()


def test_refusals_leave_the_file_untouched(tmp_path):
    path = tmp_path / "data.csv"
    shutil.copy(CSV2K, path)
    original = path.read_bytes()
    eng = pq.HipEngine(path, INDEXES)
    try:
        n0 = eng.n
        before = answers(eng)
        # the columns form is for engines without host rows
        B = 4
        columns = {"command_id": np.arange(900_000, 900_000 + B, dtype=np.uint64), "exit_code": np.zeros(B, dtype=np.int32),
                   "user_id": np.full(B, 1001, dtype=np.int32), "risk_level": np.ones(B, dtype=np.int32), "sudo_used": np.zeros(B, dtype=np.uint8)}
        for name in ("raw_command", "base_command", "shell_type", "timestamp", "working_directory", "user_name", "host_name"):
            columns[name] = (None, [b"x"])
        with pytest.raises(pq.PqpsError):
            eng.insert_columns(B, columns)
        # rows that INSERT's rules refuse: nothing of the batch is taken
        bad = make_records(5)
        bad[3].command_id = 0
        with pytest.raises(pq.PqpsError):
            eng.insert_rows(bad)
        bad = make_records(5)
        bad[4].host_name = b""
        with pytest.raises(pq.PqpsError):
            eng.insert_rows(bad)
        assert eng.insert_rows([]) == 0
        assert path.read_bytes() == original and eng.n == n0
        after = answers(eng)
        for key in before:
            assert after[key] == before[key], key
    finally:
        eng.close()
