"""UPDATE on an engine with host rows and a CSV (HipEngine(csv)): the flags come to the host, the host rows change, the CSV
is rewritten as after a DELETE (write_csv_row's format, no header) and the device table follows -- by the same flags, or by
a rebuild from the updated rows.  After every update: the file on disk equals the table formatted here, engine.record(i)
shows the new values, and the engine answers as a fresh engine over the new file does."""
import csv

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

HEADER = ["command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp", "sudo_used",
          "working_directory", "user_id", "user_name", "host_name", "risk_level"]
COL = {name: i for i, name in enumerate(HEADER)}
N = 600
INDEXES = [("risk_level", pq.FIELD_INT), ("user_id", pq.FIELD_INT)]
CHAINS = [
    None,
    [("risk_level", ">", "3")],
    [("user_id", "=", "1007")],
    [("sudo_used", "=", "TRUE"), "AND", ("user_name", ">=", "user-128")],
    [("working_directory", "=", "/home/u")],
    [("working_directory", "!=", "/home/u"), "OR", ("exit_code", "=", "2")],
    [("user_name", "=", "user-300"), "OR", ("shell_type", "=", "zsh")],
]


def make_rows():
    """256 distinct user names (a full 1-byte dictionary), one working_directory."""
    rng = np.random.default_rng(600)
    return [[str(i + 1), "ls -la", ["ls", "cat", "make"][i % 3], ["bash", "zsh"][i % 2], str(int(rng.integers(0, 3))),
             "2025-12-01T12:00:00.000Z", "1" if rng.random() < 0.3 else "0", "/home/u", str(1000 + i % 50), "user-%03d" % (i % 256),
             "host-%d" % (i % 7), str(int(rng.integers(1, 6)))] for i in range(N)]


def write_csv(path, rows, header=True):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        if header:
            w.writerow(HEADER)
        w.writerows(rows)


def file_text(rows):
    """The table as write_csv_row prints it: no header, sudo_used as 0 / 1."""
    return "".join(",".join(r) + "\n" for r in rows)


def answers(eng):
    out = {}
    for k, chain in enumerate(CHAINS):
        out["ids", k] = eng.select_ids(chain)
        out["count", k] = eng.count(chain)
    for column in ("user_name", "working_directory", "risk_level", "sudo_used"):
        out["group", column] = eng.group_count(column)
    out["aggregate"] = eng.aggregate("risk_level", "user_name", CHAINS[3])
    out["distinct"] = eng.count_distinct("user_name", "working_directory")
    out["order"] = eng.order_ids("user_name", None, True, 40)
    out["rows"] = eng.select(None, CHAINS[2])["rows"]
    return out


def check_after(eng, path, rows, tmp_path, step):
    assert path.read_text() == file_text(rows), step
    for i in (0, 1, N // 2, N - 1):
        r, row = eng.record(i), rows[i]
        assert (r.command_id, r.exit_code, r.user_id, r.risk_level, int(r.sudo_used)) == tuple(int(row[COL[c]]) for c in
                                                                                            ("command_id", "exit_code", "user_id", "risk_level", "sudo_used")), (step, i)
        assert (r.user_name, r.working_directory, r.shell_type) == tuple(row[COL[c]].encode() for c in ("user_name", "working_directory", "shell_type")), (step, i)
    mirror = tmp_path / f"mirror_{step}.csv"
    write_csv(mirror, rows)
    fresh = pq.HipEngine(mirror, INDEXES)
    try:
        got, want = answers(eng), answers(fresh)
        for key in want:
            assert got[key] == want[key], (step, key)
    finally:
        fresh.close()


def update(eng, rows, assignments, chain, match):
    want = [i for i, r in enumerate(rows) if match(r)]
    assert eng.update(assignments, chain) == len(want)
    for i in want:
        for column, value in assignments.items():
            rows[i][COL[column]] = str(value)


def test_updates_keep_rows_csv_and_device_in_step(tmp_path):
    rows = make_rows()
    path = tmp_path / "data.csv"
    write_csv(path, rows)
    assert len({r[COL["user_name"]] for r in rows}) == 256          # the 1-byte dictionary of the engine is full from here on
    eng = pq.HipEngine(path, INDEXES)
    try:
        assert eng.n == N
        # a plain update: an i32 column, the bool column and a string that is in the dictionary
        update(eng, rows, {"risk_level": 5, "sudo_used": 1, "user_name": "user-007"}, [("risk_level", "=", "3"), "AND", ("user_id", "<", "1025")],
               lambda r: r[COL["risk_level"]] == "3" and int(r[COL["user_id"]]) < 1025)
        check_after(eng, path, rows, tmp_path, "plain")
        # no match: the file is left alone
        text = path.read_text()
        update(eng, rows, {"risk_level": 1}, [("user_id", "=", "77")], lambda r: False)
        assert path.read_text() == text
        check_after(eng, path, rows, tmp_path, "no_match")
        # a 257th user_name (the dictionary keeps the values the plain update left without rows): it outgrows its 1-byte
        # codes, the device table is rebuilt from the updated rows
        update(eng, rows, {"user_name": "user-300"}, [("user_id", "=", "1007")], lambda r: r[COL["user_id"]] == "1007")
        assert sum(r[COL["user_name"]] == "user-300" for r in rows) == N // 50
        check_after(eng, path, rows, tmp_path, "rebuild_257th_name")
        # a second working_directory for a column that had one value
        update(eng, rows, {"working_directory": "/tmp/work"}, [("shell_type", "=", "zsh"), "AND", ("exit_code", "=", "1")],
               lambda r: r[COL["shell_type"]] == "zsh" and r[COL["exit_code"]] == "1")
        assert len({r[COL["working_directory"]] for r in rows}) == 2
        check_after(eng, path, rows, tmp_path, "second_directory")
        # and the engine goes on: a NULL WHERE, then a refusal that changes nothing
        update(eng, rows, {"exit_code": -3}, None, lambda r: True)
        check_after(eng, path, rows, tmp_path, "every_row")
        text = path.read_text()
        with pytest.raises(pq.PqpsError):
            eng.update({"user_name": ""}, None)
        assert path.read_text() == text
    finally:
        eng.close()


def test_no_match_on_a_file_with_its_header(tmp_path):
    """An update that matches nothing rewrites nothing: the file keeps its bytes, header included."""
    rows = make_rows()
    path = tmp_path / "data.csv"
    write_csv(path, rows)
    before = path.read_bytes()
    eng = pq.HipEngine(path, INDEXES)
    try:
        assert eng.update({"user_name": "somebody-new", "risk_level": 2}, [("risk_level", ">", "9")]) == 0
        assert path.read_bytes() == before
        fresh = pq.HipEngine(path, INDEXES)
        try:
            got, want = answers(eng), answers(fresh)
            for key in want:
                assert got[key] == want[key], key
        finally:
            fresh.close()
    finally:
        eng.close()
