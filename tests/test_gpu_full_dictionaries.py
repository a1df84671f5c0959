"""String columns whose dictionaries fill their code width, through the engine.

A dictionary of 256 values is the fullest a 1-byte code column holds, 65536 the fullest of a 2-byte one; a literal that
sorts after every value then compiles to lo = 256 (65536) -- a window that must select nothing (hipPredicate.c:
window_dict, pqps_leaf).  Tables of 255 / 256 / 257 and 65535 / 65536 / 65537 values (code widths 1, 1, 2 and 2, 2, 4),
every operator with the literals at the dictionary's edges, alone, beside a bit-plane column, in an OR and as COUNT(*),
against bytes comparison of the decoded strings (strcmp order for NUL-free values).  Then an engine loaded from a CSV whose
dictionary grows from 255 to 256 values in place and past that through a rebuild, and loses rows, against the oracle."""
import csv
import ctypes as C

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu
OPS = ["=", "!=", "<", "<=", ">", ">="]
CMP = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
       ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
N = 300_007


def host_names(count):
    return [b"host-%06d" % i for i in range(count)]


def edge_literals(values):
    """Before the first value, the first, between two values, the last, after the last, the empty string, a prefix of the last."""
    return [b"h", values[0], values[len(values) // 2] + b"x", values[-1], b"zz", b"", values[-1][:-1]]


def table_columns(count, rng):
    codes = rng.integers(0, count, N).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[1 if count <= 256 else 2 if count <= 65536 else 4])
    codes[:2] = [0, count - 1]
    codes[-2:] = [count - 1, 0]
    cols = {"command_id": np.arange(N, dtype=np.uint64), "exit_code": rng.integers(0, 3, N).astype(np.int32),
            "user_id": rng.integers(1000, 1100, N).astype(np.int32), "risk_level": rng.integers(1, 6, N).astype(np.int32),
            "sudo_used": (rng.random(N) < 0.3).astype(np.uint8)}
    for i, name in enumerate(pq.COLUMNS):
        if pq.COLUMN_KIND[i] == pq.KIND_DICT:
            cols[name] = (codes, host_names(count)) if name == "host_name" else (None, [b"x"])
    return cols


@pytest.mark.parametrize("count", [255, 256, 257, 65535, 65536, 65537])
def test_full_dictionary_every_operator_at_the_edges(count):
    rng = np.random.default_rng(count)
    cols = table_columns(count, rng)
    codes, values = cols["host_name"]
    sudo, risk = cols["sudo_used"] != 0, cols["risk_level"]
    eng = pq.HipEngine.from_columns(N, cols)
    try:
        for lit in edge_literals(values):
            for op in OPS:
                per_code = np.array([CMP[op](v, lit) for v in values])
                want = per_code[codes]
                leaf = ("host_name", op, lit.decode())
                for chain, mask in (([leaf], want),
                                    ([leaf, "AND", ("sudo_used", "=", "TRUE")], want & sudo),
                                    ([("sudo_used", "=", "FALSE"), "AND", leaf], want & ~sudo),
                                    ([("risk_level", "=", "5"), "OR", leaf], want | (risk == 5))):
                    got = np.array(eng.select_ids(chain), dtype=np.int64)
                    assert np.array_equal(got, np.nonzero(mask)[0]), (count, op, lit, chain)
                    assert eng.count(chain) == int(mask.sum()), (count, op, lit, chain)
    finally:
        eng.close()


# ---- an engine loaded from a CSV: the dictionary grows past a code width ----------------------------------------------
HEADER = ["command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp", "sudo_used",
          "working_directory", "user_id", "user_name", "host_name", "risk_level"]


def csv_row(i, host, rng):
    return [str(i), "ls -la", "ls", ["bash", "zsh"][i % 2], str(int(rng.integers(0, 3))), "2025-12-01T12:00:00.000Z",
            "true" if rng.random() < 0.3 else "false", "/home/u", str(1000 + i % 50), "student%d" % (1000 + i % 50),
            host, str(int(rng.integers(1, 6)))]


def write_csv(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(HEADER)
        w.writerows(rows)


def record_of(row):
    r = pq.Record()
    r.command_id, r.raw_command, r.base_command, r.shell_type = int(row[0]), row[1].encode(), row[2].encode(), row[3].encode()
    r.exit_code, r.timestamp, r.sudo_used, r.working_directory = int(row[4]), row[5].encode(), row[6] == "true", row[7].encode()
    r.user_id, r.user_name, r.host_name, r.risk_level = int(row[8]), row[9].encode(), row[10].encode(), int(row[11])
    return r


def test_csv_engine_dictionary_grows_past_its_width(tmp_path):
    """255 host names; INSERT one that sorts last (256 values: still one byte), then one that sorts first (every code moves
    up: 257 values, two bytes), then DELETE rows.  After every step, every operator with the edge literals of the current
    dictionary, in scan and index mode, against the oracle over the same rows."""
    rng = np.random.default_rng(255)
    hosts = ["labhost-%03d" % i for i in range(255)]
    rows = [csv_row(i, hosts[i % 255] if i < 510 else hosts[int(rng.integers(0, 255))], rng) for i in range(3000)]
    data = tmp_path / "data.csv"
    write_csv(data, rows)
    L = pq.lib()
    eng = pq.HipEngine(data, pq.DEFAULT_INDEXES)

    def check(step):
        mirror = tmp_path / ("mirror_%s.csv" % step)
        write_csv(mirror, rows)
        orc = q.OracleTable(mirror, pq.DEFAULT_INDEXES)
        orc_scan = q.OracleTable(mirror, [])                    # COUNT(*) scans: no index-mode OR loss
        assert eng.e.contents.num_records == orc.n == len(rows), step
        values = sorted({r[10].encode() for r in rows})
        for lit in edge_literals(values):
            for op in OPS:
                leaf = ("host_name", op, lit.decode())
                for chain in ([leaf], [leaf, "AND", ("sudo_used", "=", "TRUE")], [("risk_level", ">", "3"), "AND", leaf],
                              [("exit_code", "=", "0"), "OR", leaf]):
                    assert eng.select_ids(chain) == orc.select_ids(chain)[0], (step, chain)
                    assert eng.count(chain) == len(orc_scan.select_ids(chain)[0]), (step, chain)

    try:
        check("255")
        row = csv_row(3000, "zz-last-host", rng)
        assert L.executeQueryInsertHIP(eng.e, b"commands", C.byref(record_of(row)))
        rows.append(row)
        check("256")
        row = csv_row(3001, "aa-first-host", rng)
        assert L.executeQueryInsertHIP(eng.e, b"commands", C.byref(record_of(row)))
        rows.append(row)
        check("257")
        chain = [("risk_level", "=", "2"), "OR", ("host_name", "=", hosts[7])]
        wl = pq.WhereList(chain)
        rs = L.executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
        gone = {i for i, r in enumerate(rows) if r[11] == "2" or r[10] == hosts[7]}
        assert rs.contents.success and rs.contents.numRecords == len(gone)
        L.freeResultSet(rs)
        rows[:] = [r for i, r in enumerate(rows) if i not in gone]
        check("deleted")
    finally:
        eng.close()
