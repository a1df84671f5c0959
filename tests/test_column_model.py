"""tests/column_model.py checked on the CPU: what makes the model a reference rather than a second opinion.

The golden CSVs are loaded into a ColumnModel from the oracle's records.  Every chain of select_golden.json and
select_wide_golden.json must give the golden ID list (and the golden row hash) under the case's own index configuration, and
the list of OracleTable(csv) with and without pq.DEFAULT_INDEXES; every grouped fold must equal the same fold taken the
existing way over OracleTable(csv); each writer, applied once to the 2 k model, must leave the cells a list-of-dicts
implementation written here leaves; capacities, the shard split and the refusals the model predicts are pinned."""
import ctypes as C
import json

import numpy as np
import pytest

import column_model as cm
import qpelib as q
import test_gpu_count_distinct as cd
import test_gpu_group_buckets as gb
import test_gpu_group_count as grp
import test_gpu_order_by as ob
import test_gpu_set_predicates as sp
import test_group_pair_reference as gpr
import test_oracle_golden as og

pq = q.pq
CSVS = ("commands_2k.csv", "edge_cases.csv")
CASES = [c for name in ("select_golden.json", "select_wide_golden.json") for c in json.loads((q.GOLDEN / name).read_text())]
_models = {}


def model_of(csv):
    if csv not in _models:
        orc = q.OracleTable(q.GOLDEN / csv)
        _models[csv] = (cm.ColumnModel(cm.columns_of_records(orc.rows, orc.n)), orc)
    return _models[csv]


def fresh_2k():
    return cm.ColumnModel(model_of("commands_2k.csv")[0].m)


@pytest.mark.parametrize("csv", CSVS)
def test_records_of_the_model_are_the_oracles(csv):
    """columns -> records is the inverse of records -> columns, byte for byte up to each string's terminator."""
    model, orc = model_of(csv)
    recs = model.records()
    for r in range(orc.n):
        for column in pq.COLUMNS:
            assert model.cell(r, column) == orc.cell(r, column), (r, column)
            buf = C.create_string_buffer(1200)
            orc.lib.orc_attr_string(C.byref(recs[r]), column.encode(), buf, 1200)
            assert buf.value.decode("latin-1") == orc.cell(r, column), (r, column)


def test_every_golden_case():
    assert len(CASES) > 150 and {c["csv"] for c in CASES} == set(CSVS)
    for case in CASES:
        model, _ = model_of(case["csv"])
        chain = q.chain_from_jsonable(case["where"])
        ids = model.select_ids(chain, og.INDEX_CONFIGS[case["indexes"]])
        assert len(ids) == case["num_records"], case["name"]
        if q.case_ids(case) is not None:
            assert ids == q.case_ids(case), case["name"]
        sel = case["sql"][len("SELECT "):case["sql"].index(" FROM ")]
        cols = None if sel.strip() == "*" else [c.strip() for c in sel.split(",")]
        if all(c in pq.COLUMNS for c in cols or []):
            assert og.sha_rows(model.project(ids, cols)) == case["rows_sha256"], case["name"]


@pytest.mark.parametrize("csv", CSVS)
def test_every_chain_with_and_without_the_default_indexes(csv):
    model, _ = model_of(csv)
    chains = [q.chain_from_jsonable(c["where"]) for c in CASES if c["csv"] == csv] + [None]
    probed = 0
    for idx in ([], pq.DEFAULT_INDEXES):
        orc = q.OracleTable(q.GOLDEN / csv, idx)
        for chain in chains:
            want = orc.select_ids(chain)[0]
            assert model.select_ids(chain, idx) == want, (idx, chain)
            if not idx:
                assert np.flatnonzero(model.mask(chain)).tolist() == want, chain
            probed += want != sorted(want)
    assert probed >= 5, "index mode must come back in probe order for some chains"


def test_set_chains_equal_chain_true_row_by_row():
    """LIKE / IN: the mask taken once per distinct combination of the chain's columns is the mask taken row by row; with
    indexes the probes of the other conditions stay, re-filtered with the set."""
    model, orc = model_of("commands_2k.csv")
    recs = [orc.rows[i] for i in range(orc.n)]
    users = sorted({orc.cell(r, "user_name") for r in range(orc.n)})
    chains = [
        [("user_name", "IN", pq.in_list(users[::7]))],
        [("user_name", "NOT IN", pq.in_list(users[::5])), "AND", ("risk_level", ">=", "4")],
        [("risk_level", ">", "3"), "AND", ("raw_command", "LIKE", "%a%")],
        [("host_name", "LIKE", "%1"), "OR", [("user_id", "IN", pq.in_list([1001, 1003, 1500])), "AND", ("sudo_used", "=", "true")]],
        [("user_id", "IN", pq.in_list([1001, 1003, 1005]))],
        [("command_id", "IN", pq.in_list([5, 17, 1999])), "OR", ("exit_code", ">", "100")],
        [("user_name", "IN", "()")],
        [("raw_command", "LIKE", "it''s%")],
    ]
    assert cm.parse_in_list("('a', 'it''s', '')") == ["a", "it's", ""] and cm.parse_in_list("()") == []
    for chain in chains:
        cm.register_in_lists(chain)
        want = [i for i, r in enumerate(recs) if sp.chain_true(r, chain)]
        assert model.scan_rows(chain).tolist() == want, chain
        assert model.select_ids(chain, []) == want, chain
    # index mode: risk_level > 3 is a probe, the LIKE part of the re-filter; a set condition on an indexed column is no probe
    probed = model.select_ids([("risk_level", ">", "3")], pq.DEFAULT_INDEXES)
    assert probed != sorted(probed)
    leaf = ("raw_command", "LIKE", "%a%")
    assert model.select_ids(chains[2], pq.DEFAULT_INDEXES) == [i for i in probed if sp.leaf_true(recs[i], leaf)]
    assert model.select_ids(chains[4], pq.DEFAULT_INDEXES) == [i for i, r in enumerate(recs) if sp.chain_true(r, chains[4])]


def test_grouped_folds_equal_the_folds_over_the_oracle_table():
    model, _ = model_of("commands_2k.csv")
    chains = grp.golden_chains()
    pairs = (("user_name", "risk_level"), ("sudo_used", "base_command"), ("risk_level", "risk_level"), ("base_command", "exit_code"))
    shapes = (("timestamp", 13, None), ("user_name", 9, None), ("user_id", None, 16), ("exit_code", None, 50))
    duplicates = False
    for idx in ([], pq.DEFAULT_INDEXES):
        orc = q.OracleTable(q.GOLDEN / "commands_2k.csv", idx)
        pair_cells = gpr.CsvCells(orc, sorted({c for p in pairs for c in p} | {"risk_level", "command_id"}))
        bucket_cells = gb.Cells(orc, sorted({s[0] for s in shapes} | {"risk_level", "command_id"}))
        for chain in chains[::3] + [None]:
            ids = orc.select_ids(chain)[0]
            assert model.select_ids(chain, idx) == ids
            duplicates |= len(set(ids)) < len(ids)
            for column in grp.GROUPABLE:
                assert model.group_count(column, ids) == grp.expected_from_cells(column, [orc.cell(r, column) for r in ids]), (column, chain)
            for value, group in (("risk_level", "shell_type"), ("command_id", None), ("exit_code", "sudo_used"), ("exit_code", "user_name")):
                acc = {}
                for r in ids:
                    acc.setdefault(orc.cell(r, group) if group else None, []).append(int(orc.cell(r, value)))
                keys = sorted(acc, key=lambda k: grp.key_order(group, k)) if group else list(acc)
                want = [(k, len(acc[k]), sum(acc[k]) & (cm.M64 if value == "command_id" else -1), min(acc[k]), max(acc[k])) for k in keys]
                assert model.aggregate(value, group, ids) == want, (value, group, chain)
            for value, group in (("user_name", "risk_level"), ("command_id", None), ("host_name", None), ("command_id", "sudo_used")):
                assert model.count_distinct(value, group, ids) == cd.oracle_distinct(orc, ids, value, group), (value, group, chain)
            for column in ("risk_level", "user_name", "command_id", "sudo_used"):
                keys = [ob.cell_key(column, orc.cell(r, column)) for r in ids]
                for desc in (False, True):
                    assert model.order_ids(column, ids, desc, 60) == (ob.cut(ob.sort_rows(ids, keys, desc), 60), len(ids)), (column, desc, chain)
            for pair in pairs:
                for value in (None, "risk_level", "command_id"):
                    assert model.group_pair(pair, value, ids) == pair_cells.fold(ids, pair, value), (pair, value, chain)
            for column, prefix, width in shapes:
                for value in (None, "risk_level", "command_id"):
                    assert model.group_buckets(column, prefix, width, value, ids) == bucket_cells.expected(ids, column, prefix, width, value), \
                        (column, prefix, width, value, chain)
            assert model.project(ids[:50]) == orc.project(ids[:50], None)
    assert duplicates, "index mode must return some row twice for some chain"


# ---- the writers against a list of dicts -------------------------------------------------------------------------------------
def dict_rows(model):
    return [{c: model.cell(r, c) for c in pq.COLUMNS} for r in range(model.n)]


def text_of(column, value):
    if column == "sudo_used":
        return "true" if str(value).lower() in ("true", "1") else "false"
    return value.decode("latin-1") if isinstance(value, bytes) else str(value)


def dict_update(rows, assignments, hit):
    for r in rows:
        if hit(r):
            for column, value in assignments.items():
                r[column] = text_of(column, value)
    return rows


def test_writers_against_a_list_of_dicts():
    model = fresh_2k()
    rows = dict_rows(model)
    n = model.n
    # UPDATE: a string new to its dictionary, an i32 and the boolean; the WHERE reads an assigned column
    hits = sum(r["risk_level"] == "3" and r["sudo_used"] == "false" for r in rows)
    assert 0 < hits < n
    got = model.update({"user_name": "mmm-middle", "risk_level": 5, "sudo_used": "TRUE"}, [("risk_level", "=", "3"), "AND", ("sudo_used", "=", "FALSE")])
    rows = dict_update(rows, {"user_name": "mmm-middle", "risk_level": 5, "sudo_used": "TRUE"}, lambda r: r["risk_level"] == "3" and r["sudo_used"] == "false")
    assert got == hits and dict_rows(model) == rows and b"mmm-middle" in model.m["user_name"][1]
    # an UPDATE that selects nothing still leaves its string in the dictionary (no row carries it)
    assert model.update({"host_name": "nobodys-host"}, [("risk_level", "=", "77")]) == 0
    assert dict_rows(model) == rows and b"nobodys-host" in model.m["host_name"][1]
    # DELETE: the rows renumber, order kept, the dictionaries stay
    names_before = list(model.m["user_name"][1])
    gone = sum(r["user_name"] == "mmm-middle" or int(r["exit_code"]) > 100 for r in rows)
    assert model.delete([("user_name", "=", "mmm-middle"), "OR", ("exit_code", ">", "100")]) == gone
    rows = [r for r in rows if not (r["user_name"] == "mmm-middle" or int(r["exit_code"]) > 100)]
    assert dict_rows(model) == rows and model.n == n - gone and model.m["user_name"][1] == names_before and model.shard_rows == [n - gone]
    # single INSERT: the row gets number n
    row = {"command_id": 7_000_001, "raw_command": b"zzz new command", "base_command": b"zzz", "shell_type": b"ash", "exit_code": -3,
           "timestamp": b"2031-01-01T00:00:00.000Z", "sudo_used": True, "working_directory": b"/", "user_id": 77, "user_name": b"aaa-first",
           "host_name": b"labpc-01", "risk_level": 9}
    assert model.insert_one(row) is True
    rows.append({c: text_of(c, v) for c, v in row.items()})
    assert dict_rows(model) == rows and model.cell(model.n - 1, "shell_type") == "ash" and model.m["shell_type"][1][0] == b"ash"
    # batch INSERT: the rows get n .. n + B - 1; a string no row carries still enters
    B = 5
    b = {c: (model.m[c][:B].copy() if c in cm.NUMERIC else (model.m[c][0][:B].copy(), list(model.m[c][1]))) for c in pq.COLUMNS}
    b["command_id"] = np.arange(8_000_001, 8_000_001 + B, dtype=np.uint64)
    b["host_name"] = cm.coded([b"a-host", b"zz-host", b"a-host", b"labpc-01", b"labpc-02"], extra=[b"nobodys-other-host"])
    first = [dict(r) for r in rows[:B]]
    for k, r in enumerate(first):
        r["command_id"], r["host_name"] = str(8_000_001 + k), ["a-host", "zz-host", "a-host", "labpc-01", "labpc-02"][k]
    assert model.insert_batch(b) == B
    rows += first
    assert dict_rows(model) == rows and b"nobodys-other-host" in model.m["host_name"][1]
    assert model.m["host_name"][1] == sorted(model.m["host_name"][1]) and model.scan_rows([("host_name", "=", "a-host")]).tolist() == [model.n - 5, model.n - 3]


# ---- capacity, shards, widths and the refusals they decide -------------------------------------------------------------------
def small_columns(n=5003, hosts=256):
    rng = np.random.default_rng(5)
    m = {c: rng.integers(1, 4, n).astype(np.int32) for c in ("exit_code", "user_id", "risk_level")}
    m.update(command_id=np.arange(1, n + 1, dtype=np.uint64), sudo_used=(rng.random(n) < 0.5).astype(np.uint8),
             shell_type=(rng.integers(0, 2, n).astype(np.uint8), [b"bash", b"zsh"]),
             user_name=(rng.integers(0, 3, n).astype(np.uint16), [b"ann", b"bob", b"cy"]),
             host_name=(rng.integers(0, hosts, n).astype(np.uint8), [b"host-%03d" % i for i in range(hosts)]),
             base_command=(rng.integers(0, 2, n).astype(np.uint8), [b"cat", b"ls"]),
             raw_command=(None, [b"ls -la"]), timestamp=(None, [b"2025-01-01T00:00:00.000Z"]), working_directory=(None, [b"/home/u"]))
    return m


def one_row(**over):
    row = {"command_id": 9_000_001, "raw_command": b"ls -la", "base_command": b"ls", "shell_type": b"zsh", "exit_code": 2,
           "timestamp": b"2025-01-01T00:00:00.000Z", "sudo_used": True, "working_directory": b"/home/u", "user_id": 3, "user_name": b"bob",
           "host_name": b"host-003", "risk_level": 4}
    row.update(over)
    return row


def test_capacity_and_the_shard_split():
    """5 003 rows leave room for 3 189 more (test_capacity_formula_of_the_model); two shards split as pqps_partition does."""
    assert cm.capacity_for(5003) == 8192 and 8192 - 5003 == 3189
    assert cm.capacity_for(0) == pq.TILE_ROWS and cm.capacity_for(8192) == 12288
    for n, parts in ((5003, 2), (5003, 1), (5004, 2), (10, 3), (2, 3), (0, 2)):
        want, at = [], 0
        for rank in range(parts):
            start, count = C.c_uint64(), C.c_uint64()
            pq.lib().pqps_partition(n, parts, rank, C.byref(start), C.byref(count))
            assert start.value == at
            want.append(count.value)
            at += count.value
        assert cm.partition(n, parts) == want and at == n
    assert cm.partition(5003, 2) == [2502, 2501]
    model = cm.ColumnModel(small_columns(), n_shards=2)
    assert model.shard_rows == [2502, 2501] and model.shard_capacity == [4096, 4096]
    assert model.width == dict(raw_command=0, base_command=1, shell_type=1, timestamp=0, working_directory=0, user_name=2, host_name=1)


def test_single_insert_refusals():
    model = cm.ColumnModel(small_columns())
    cells = dict_rows(model)
    # a string new to a dictionary that is full for its width; a second value for a column without a buffer
    assert "full for 1-byte" in model.insert_refusal(one_row(host_name=b"host-new"))
    assert "without a buffer" in model.insert_refusal(one_row(timestamp=b"2026"))
    assert model.insert_one(one_row(host_name=b"host-new")) is None and model.insert_one(one_row(working_directory=b"/")) is None
    assert dict_rows(model) == cells and model.shard_rows == [5003] and len(model.m["host_name"][1]) == 256
    # the last shard full: a batch fills the head-room exactly, the next row is refused, the next batch grows the shard
    assert model.insert_refusal(one_row()) is None
    b = {c: (v[:3189] if isinstance(v, np.ndarray) else (None if v[0] is None else v[0][:3189], v[1])) for c, v in model.m.items()}
    assert model.insert_batch(b) == 3189 and model.route["grown"] is False and model.shard_rows == model.shard_capacity == [8192]
    assert model.insert_refusal(one_row()) == "the last shard is full" and model.insert_one(one_row()) is None and model.n == 8192
    one = {c: (v[:1] if isinstance(v, np.ndarray) else (None if v[0] is None else v[0][:1], v[1])) for c, v in model.m.items()}
    assert model.insert_batch(one) == 1 and model.route["grown"] is True and model.shard_capacity == [cm.capacity_for(8193)] == [12288]
    assert model.insert_one(one_row(user_name=b"dee")) is True and model.n == 8194 and model.route == dict(bumped=["user_name"])


def test_update_refusals_and_the_widths_a_batch_leaves():
    model = cm.ColumnModel(small_columns())
    cells = dict_rows(model)
    assert "full for 1-byte" in model.update_refusal({"risk_level": 1, "host_name": "host-new"})
    assert "without a buffer" in model.update_refusal({"working_directory": "/tmp"})
    assert model.update({"host_name": "host-new"}, None) is None and model.update({"working_directory": "/tmp"}, None) is None
    assert dict_rows(model) == cells and len(model.m["host_name"][1]) == 256
    # its own value is no second value; a known string of a full dictionary is no new one
    assert model.update({"working_directory": "/home/u", "host_name": "host-007"}, [("risk_level", "=", "1")]) == sum(r["risk_level"] == "1" for r in cells)
    # a batch widens (1 -> 2), materialises (0 -> 1) and remaps in place; afterwards the UPDATEs above are taken
    b = {c: (v[:4] if isinstance(v, np.ndarray) else (None if v[0] is None else v[0][:4], v[1])) for c, v in model.m.items()}
    b["host_name"] = cm.coded([b"host-100x"] * 4)
    b["working_directory"] = cm.coded([b"/tmp", b"/", b"/home/u", b"/tmp"])
    b["user_name"] = cm.coded([b"aaa", b"bob", b"bob", b"aaa"])
    b["shell_type"] = cm.coded([b"zzsh"] * 4)
    assert model.insert_batch(b) == 4
    assert model.route == dict(grown=False, widened=["host_name"], materialised=["working_directory"], remapped=["user_name"])
    assert model.width["host_name"] == 2 and model.width["working_directory"] == 1 and model.width["user_name"] == 2 and model.width["timestamp"] == 0
    assert model.update_refusal({"host_name": "host-new", "working_directory": "/var"}) is None
    # 65 536 strings fill a 2-byte dictionary; a batch takes the 65 537th and widens to 4 bytes
    filler = [b"filler-%05d" % i for i in range(65536 - len(model.m["user_name"][1]))]
    b["user_name"] = cm.coded([b"bob"] * 4, extra=filler)
    model.insert_batch(b)
    assert len(model.m["user_name"][1]) == 65536 and model.width["user_name"] == 2 and not model.group_refused("user_name")
    assert "full for 2-byte" in model.update_refusal({"user_name": "one-more"}) and model.insert_refusal(one_row(user_name=b"one-more"))
    b["user_name"] = cm.coded([b"one-more"] * 4)
    model.insert_batch(b)
    assert model.width["user_name"] == 4 and model.route["widened"] == ["user_name"] and model.group_refused("user_name")
    assert model.m["user_name"][0].dtype == np.uint32 and model.cell(model.n - 1, "user_name") == "one-more"


def test_delete_keeps_each_shards_range_and_an_empty_table_answers():
    model = cm.ColumnModel(small_columns(), n_shards=2)
    assert model.delete([("command_id", "<=", "2502")]) == 2502 and model.shard_rows == [0, 2501] and model.shard_capacity == [4096, 4096]
    assert model.m["command_id"][0] == 2503
    assert model.delete([("command_id", ">", "0")]) == 2501 and model.n == 0 and model.shard_rows == [0, 0]
    idx = [("risk_level", pq.FIELD_INT), ("user_id", pq.FIELD_INT)]
    for chain in (None, [("risk_level", ">", "1")], [("user_name", "IN", pq.in_list([b"ann"]))]):
        assert model.select_ids(chain, idx) == [] and model.scan_rows(chain).tolist() == []
    assert model.group_count("user_name", []) == [] and model.aggregate("risk_level", None, []) == [] and model.order_ids("risk_level", []) == ([], 0)
    assert model.group_pair(("user_name", "host_name"), "risk_level", []) == [] and model.group_buckets("user_id", None, 16, None, []) == []
    assert model.insert_one(one_row()) is True and model.shard_rows == [0, 1] and model.select_ids([("risk_level", "=", "4")], idx) == [0]
