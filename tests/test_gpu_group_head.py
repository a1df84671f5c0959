"""The first n rows of every group (executeQueryGroupHeadHIP / HipEngine.group_head, select_group_head): per group of one
column among the rows executeQuerySelectIdsHIP returns, each once, the first n in the order of a second column, ties to the
lowest row number in both directions.  Every expected answer comes from tests/group_head_model.py over rows and cells the
oracle, HostSynth or tests/column_model.py give -- never from the engine -- except where the test IS a comparison of two
engine calls (the order_ids consequence, n = 1 against group_first, the projection).  n runs on both sides of the round cap
(PQPS_HEAD_ROUNDS_MAX): the rounds form below, the sort form above."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import group_first_model as m
import group_head_model as hm
import test_gpu_group_first as gfe
from column_model import ColumnModel

q, grp = m.q, m.grp
pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
CAP = pq.HEAD_ROUNDS_MAX
NS = (1, 2, 3, CAP, CAP + 1, 40)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    """The golden chains, with and without indexes (probes that list a row twice included); n, the columns and the direction
    take turns."""
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    model = m.CsvModel(orc)
    chains = grp.golden_chains()
    cases = [(g, o) for g in ("user_name", "shell_type", "sudo_used", "risk_level", None) for o in ("timestamp", "command_id", "exit_code", "user_name")]
    repeated = 0
    try:
        for turn, chain in enumerate(chains + [None]):
            ids = orc.select_ids(chain)[0]
            repeated += len(ids) != len(set(ids))
            for k in range(4):
                group, column = cases[(turn * 4 + k) % len(cases)]
                n, desc = NS[(turn + k) % len(NS)], (turn + k // 2) % 2 == 1
                got, total = eng.group_head(group, column, n, chain, desc)
                assert got == hm.csv_expected(model, ids, group, column, desc, n), (indexes, group, column, n, desc, chain)
                assert total == len(ids)
                if group:
                    assert [key for key, _ in got] == [key for key, _ in eng.group_count(group, chain)]
        assert indexes == "none" or repeated > 0
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_rows_of_a_group_are_order_ids_of_the_group(indexes):
    """The consequence the header states, for every group of three group columns x four order columns x both directions."""
    eng = pq.HipEngine(CSV2K, [] if indexes == "none" else pq.DEFAULT_INDEXES)
    chains = [None, [("risk_level", ">", "2")], [("sudo_used", "=", "TRUE"), "OR", [("risk_level", "=", "5"), "AND", ("shell_type", "=", "bash")]]]
    try:
        for turn, chain in enumerate(chains):
            n = (3, CAP + 3, 7)[turn]
            for group in ("shell_type", "sudo_used", "risk_level"):
                for column in ("timestamp", "command_id", "exit_code", "user_name"):
                    for desc in (False, True):
                        got, _ = eng.group_head(group, column, n, chain, desc)
                        assert got
                        for key, rows in got:
                            narrowed = [(group, "=", gfe.where_value(group, key))] + (["AND", list(chain)] if chain else [])
                            ids, _ = eng.order_ids(column, narrowed, desc, None)
                            assert [r for r, _ in rows] == list(dict.fromkeys(ids))[:n], (chain, group, key, column, desc, n)
            ids, matches = eng.order_ids("exit_code", chain, True, None)
            got, total = eng.group_head(None, "exit_code", n, chain, True)
            assert total == matches and [r for r, _ in got[0][1]] == list(dict.fromkeys(ids))[:n]
    finally:
        eng.close()


def column_expected(cm, ids, group, column, desc, n):
    ids = np.asarray(ids, dtype=np.int64)
    values, offsets, rows, _ = hm.head_rows(ids, cm.codes(column)[ids], cm.codes(group)[ids] if group else None, desc, n)
    return hm.groups_of(values, offsets, rows, (lambda r: cm.cell(r, group)) if group else None, lambda r: cm.cell(r, column))


def check_columns(eng, cm, cases, ns, chains=gfe.EDGE_CHAINS, indexes=()):
    """Every case at every n in one direction each, the direction taking turns."""
    turn = 0
    for chain in chains:
        ids = cm.select_ids(chain, indexes)
        for group, column in cases:
            for n in ns:
                desc = turn % 2 == 1
                turn += 1
                got, total = eng.group_head(group, column, n, chain, desc)
                assert total == len(ids), (group, column, n, desc, chain)
                assert got == column_expected(cm, ids, group, column, desc, n), (group, column, n, desc, chain)


@pytest.mark.gpu
def test_one_row_is_group_first_and_the_forms_agree():
    """n = 1 equals group_first; n = cap and cap + 1 (either side of the form switch) against the model, the smaller answer
    a per-group prefix of the larger one; n larger than any group lists every matching row once."""
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    orc = q.OracleTable(CSV2K, pq.DEFAULT_INDEXES)
    model = m.CsvModel(orc)
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_name", "=", "student1030"), "OR", ("exit_code", "!=", "0")], [("risk_level", ">", "9")]):
            ids = orc.select_ids(chain)[0]
            for group, column, desc in (("user_name", "timestamp", True), ("shell_type", "command_id", False), (None, "exit_code", True),
                                        ("sudo_used", "user_name", False), ("risk_level", "command_id", True)):
                first, total = eng.group_first(group, column, chain, desc)
                one, total1 = eng.group_head(group, column, 1, chain, desc)
                assert total1 == total and one == [(key, [(row, text)]) for key, row, text in first]
                below, _ = eng.group_head(group, column, CAP, chain, desc)
                above, _ = eng.group_head(group, column, CAP + 1, chain, desc)
                assert below == hm.csv_expected(model, ids, group, column, desc, CAP)
                assert above == hm.csv_expected(model, ids, group, column, desc, CAP + 1)
                assert [(key, rows[:CAP]) for key, rows in above] == below
                every, _ = eng.group_head(group, column, 10**9, chain, desc)
                assert every == hm.csv_expected(model, ids, group, column, desc, 10**9)
                assert sorted(r for _, rows in every for r, _ in rows) == sorted(set(ids))
    finally:
        eng.close()


SYNTH_SMALL = [(c, g, o) for c in ("all", "s1", "risk_gt2", "nothing", "or_tree") for g in ("user_name", "risk_level", "sudo_used", None)
               for o in ("timestamp", "command_id", "exit_code", "user_name", "sudo_used")]
SYNTH_BIG = [("all", "user_name", "command_id", 3), ("all", "risk_level", "user_name", CAP + 1), ("all", None, "exit_code", 5),
             ("s1", "shell_type", "command_id", CAP + 4), ("risk_gt2", "user_name", "user_id", 2), ("risk_gt2", "sudo_used", "user_id", 30),
             ("or_tree", "host_name", "command_id", CAP)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, 1025, 65537, (1 << 20) + 3])
def test_synthetic(n_rows):
    """timestamp is single-valued in the synthetic table: the lowest matching rows of every group."""
    host = q.HostSynth(n_rows, full=True)
    eng = pq.HipEngine.synthetic(n_rows)
    rows = {}
    cases = SYNTH_BIG if n_rows > 100000 else [(c, g, o, NS[i % len(NS)]) for i, (c, g, o) in enumerate(SYNTH_SMALL)]
    try:
        for turn, (cname, group, column, n) in enumerate(cases):
            chain = grp.SYNTH_CHAINS[cname]
            if cname not in rows:
                rows[cname] = np.asarray(host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            desc = turn % 2 == 1
            got, total = eng.group_head(group, column, n, chain, desc)
            assert total == len(rows[cname])
            assert got == hm.synth_expected(host, rows[cname], group, column, desc, n), (n_rows, cname, group, column, n, desc)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, 1025])
def test_synthetic_index_probes(n_rows):
    """WHEREs the risk_level index probes are not fused: the per-shard lists, the list kernels and the sort form."""
    host = q.HostSynth(n_rows, full=True)
    eng = pq.HipEngine.synthetic(n_rows, indexes=grp.PROBE_INDEXES)
    try:
        for turn, (cname, chain) in enumerate(grp.PROBED_CHAINS.items()):
            rows = np.asarray(host.oracle_scan(chain, nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            for k, (group, column) in enumerate((("user_name", "command_id"), ("risk_level", "exit_code"), (None, "user_name"), ("sudo_used", "timestamp"))):
                n, desc = NS[(turn + k) % len(NS)], (turn + k) % 2 == 1
                got, total = eng.group_head(group, column, n, chain, desc)
                assert total == len(rows), (n_rows, cname, group, column)
                assert got == hm.synth_expected(host, rows, group, column, desc, n), (n_rows, cname, group, column, n, desc)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("users", [4096, 4097, 8192, 8193])
def test_group_column_at_the_path_switches(users):
    """Group columns of 4096 | 4097 values (the floor leaves LDS) and 8192 | 8193 (the min table leaves LDS); command_id and
    i32 extremes as order keys, in both forms."""
    n = 30011
    rng = np.random.default_rng([31, users])
    exit_code = rng.choice(np.array([gfe.INT32_MIN, gfe.INT32_MIN + 1, -1, 0, 1, gfe.INT32_MAX - 1, gfe.INT32_MAX], np.int32), size=n)
    big = np.array([0, 5, (1 << 63) - 1, 1 << 63, gfe.M64 - 1, gfe.M64], np.uint64)
    cols = gfe.edge_columns(n, rng, users, exit_code=exit_code, command_id=rng.choice(big, size=n))
    cols["user_name"][0][:users] = np.arange(users)                 # every value occurs
    cols["user_name"][0][users:users + 3000] = np.arange(3000) % 100  # and a hundred groups have more than the cap
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, [("user_name", "exit_code"), ("user_name", "command_id"), ("user_name", "timestamp"), (None, "command_id")],
                      (2, CAP, CAP + 1), chains=gfe.EDGE_CHAINS[:2] + gfe.EDGE_CHAINS[3:])
    finally:
        eng.close()
    eng = pq.HipEngine.from_columns(n, cols, pq.DEFAULT_INDEXES)    # the list form over index probes
    try:
        check_columns(eng, cm, [("user_name", "command_id"), ("user_name", "exit_code")], (3, CAP + 2), chains=gfe.EDGE_CHAINS[1:2],
                      indexes=pq.DEFAULT_INDEXES)
    finally:
        eng.close()


@pytest.mark.gpu
def test_order_column_of_70000_values():
    """4-byte codes: nothing is refused for the size of the order column's domain, in either form."""
    n = (1 << 17) + 9
    rng = np.random.default_rng(32)
    cols = gfe.edge_columns(n, rng, 70000)
    assert cols["user_name"][0].dtype == np.uint32
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, [("risk_level", "user_name"), ("shell_type", "user_name"), (None, "user_name"), ("user_id", "user_name")],
                      (3, CAP + 1), chains=gfe.EDGE_CHAINS[:2])
        with pytest.raises(pq.PqpsError):                               # ... but the GROUP column keeps grouped COUNT's limit
            eng.group_head("user_name", "risk_level", 3)
    finally:
        eng.close()


@pytest.mark.gpu
def test_member_pass_and_in_set():
    """A fragmented IN list and a LIKE (the member pass in front of the filter pass), then IN SET: the list route."""
    n = 20011
    rng = np.random.default_rng(33)
    cols = gfe.edge_columns(n, rng, 300)
    cm = ColumnModel(cols)
    every_third = pq.in_list([w.decode() for w in cols["user_name"][1][::3]])
    chains = ([("user_name", "IN", every_third)], [("user_name", "IN", every_third), "AND", ("risk_level", ">", "2")],
              [("user_name", "LIKE", "w0000_7"), "OR", ("user_name", "NOT IN", every_third)])
    cases = [("shell_type", "command_id"), ("user_name", "exit_code"), (None, "user_name"), ("risk_level", "sudo_used")]
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, cases, (2, CAP + 1), chains=chains)
        vs = eng.value_set("user_name", [("risk_level", "=", "5")], ("count", None, ">=", "14"))
        assert 0 < vs.members < 300
        same = [("user_name", "IN", pq.in_list(vs.keys()))]         # the model's WHERE for the set's members
        for negate in (False, True):
            ids = cm.select_ids([("user_name", "NOT IN", same[0][2])] if negate else same)
            for (group, column), n_, desc in zip(cases, (3, CAP + 1, CAP, 40), (False, True, True, False)):
                got, total = eng.group_head(group, column, n_, [vs.item(negate=negate)], desc)
                assert total == len(ids) and got == column_expected(cm, ids, group, column, desc, n_), (negate, group, column, n_)
        vs.free()
    finally:
        eng.close()


def spread_columns():
    """A group's best rows at the start, in the middle and at the end of the table: over three shards its first n come from
    different shards, and a tie on the key is decided by the row across shards."""
    n = 30007
    rng = np.random.default_rng(34)
    cols = gfe.edge_columns(n, rng, 50, exit_code=rng.integers(0, 100, size=n).astype(np.int32),
                            command_id=rng.integers(1000, 2000, size=n).astype(np.uint64))
    for at, key in ((5, -5), (n // 2, -5), (n - 9, -5), (n // 2 + 1, -4), (7, -3), (n - 3, -3)):
        cols["exit_code"][at:at + 2] = key
        cols["command_id"][at:at + 2] = 10 + key
        cols["user_name"][0][at:at + 2] = 11
    return n, cols


@pytest.mark.gpu
def test_first_rows_spread_over_the_table():
    n, cols = spread_columns()
    cm = ColumnModel(cols)
    cases = [("user_name", "exit_code"), ("user_name", "command_id"), (None, "exit_code"), ("shell_type", "timestamp")]
    for indexes in ((), pq.DEFAULT_INDEXES):
        eng = pq.HipEngine.from_columns(n, cols, indexes)
        try:
            check_columns(eng, cm, cases, (5, CAP + 1), chains=gfe.EDGE_CHAINS[:2], indexes=indexes)
            got, _ = eng.group_head("user_name", "exit_code", 8, None, False)
            rows = [r for r, _ in dict(got)["w000011"]]
            assert rows == [5, 6, n // 2, n - 9, n - 8, n // 2 + 1, n // 2 + 2, 7]   # keys -5 x 5, -4 x 2, then the first -3
        finally:
            eng.close()


@pytest.mark.gpu
def test_over_three_shards():
    """Three shards on one card (a child process: the engine reads PQPS_DEVICES when it is created)."""
    env = dict(os.environ, PQPS_DEVICES="0,0,0")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "spread_over_the_table or test_synthetic[1] or test_synthetic[1025] or synthetic_index_probes or after_writers "
                              "or select_group_head or 4097 or member_pass"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


@pytest.mark.gpu
def test_after_writers():
    """insert_rows (a new group, new extremes), DELETE (the rows renumber) and UPDATE of the order column; the model is rebuilt
    by the same operations."""
    n = 6007
    rng = np.random.default_rng(35)
    cols = gfe.edge_columns(n, rng, 40)
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols, pq.DEFAULT_INDEXES)
    cases = [("user_name", "exit_code"), ("user_name", "command_id"), ("shell_type", "user_name"), (None, "exit_code"), ("risk_level", "user_id")]
    chains, ns = gfe.EDGE_CHAINS[:3], (3, CAP + 1)
    try:
        check_columns(eng, cm, cases, ns, chains, pq.DEFAULT_INDEXES)                 # caches the i32 ranges
        b = 37
        batch = gfe.edge_columns(b, rng, 3, exit_code=np.full(b, 900, np.int32), command_id=np.arange(10**12, 10**12 + b, dtype=np.uint64),
                                 risk_level=np.full(b, 7, np.int32))
        batch["user_name"][0][:3] = (0, 1, 2)
        batch["user_name"] = (batch["user_name"][0], [b"w000005x", b"w999999", b"zz_new"])
        assert eng.insert_rows(ColumnModel(batch).records()) == b
        cm.insert_batch(batch)
        check_columns(eng, cm, cases, ns, chains, pq.DEFAULT_INDEXES)
        got, _ = eng.group_head("user_name", "exit_code", 2, None, True)
        assert got[-1][0] == "zz_new" and [text for _, text in got[-1][1]] == ["900", "900"]
        where = [("risk_level", "=", "2"), "OR", ("shell_type", "=", "fish")]
        wl = pq.WhereList(where)
        rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
        assert rs.contents.success
        pq.lib().freeResultSet(rs)
        assert 0 < cm.delete(where) and eng.e.contents.num_records == cm.n
        check_columns(eng, cm, cases, ns, chains, pq.DEFAULT_INDEXES)
        for assignments, where in (({"exit_code": -(1 << 20)}, [("user_id", ">=", "1390")]), ({"user_name": "w000001"}, [("risk_level", "=", "5")])):
            assert eng.update(assignments, where) == cm.update(assignments, where)
            check_columns(eng, cm, cases, ns, chains, pq.DEFAULT_INDEXES)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_select_group_head(indexes):
    """The projection's cells equal select_columnar's on the same rows, in answer order, with the offsets of group_head."""
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_name", "=", "student1030"), "OR", ("exit_code", "!=", "0")], [("risk_level", ">", "9")]):
            plain = eng.select_columnar(None, chain)
            by_row = dict(zip(eng.select_ids(chain), plain["rows"]))
            eng.free_columnar(plain)
            for group, column, desc, n in (("user_name", "timestamp", True, 2), ("shell_type", "command_id", False, CAP + 1),
                                           (None, "exit_code", True, 5), ("sudo_used", "user_name", False, 40)):
                groups, total, raw = eng.group_head_result(group, column, n, chain, desc)
                out = eng.select_group_head(None, chain, group, column, n, desc)
                assert out["success"] and out["matches"] == total and out["numRecords"] == len(raw["rows"])
                assert out["offsets"] == raw["offsets"] and len(raw["offsets"]) == len(groups) + 1
                assert out["columns"] == list(q.COLUMNS)
                assert out["rows"] == [by_row[r] for r in raw["rows"]], (chain, group, column, desc, n)
                at = q.COLUMNS.index(column)
                assert [row[at] for row in out["rows"]] == [text for _, rows in groups for _, text in rows]
                eng.free_columnar(out)
            part = eng.select_group_head(["user_name", "command_id"], chain, "user_name", "command_id", 2, True)
            assert part["columns"] == ["user_name", "command_id"]
            keys = [k for k, _ in eng.group_count("user_name", chain)]
            assert [part["rows"][o][0] for o in part["offsets"][:-1]] == keys
            eng.free_columnar(part)
    finally:
        eng.close()


@pytest.mark.gpu
def test_two_lanes_at_once():
    """Two threads, one lane each, both forms at the same time: every answer equals the one made alone."""
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    queries = [("user_name", "timestamp", 3, [("risk_level", ">", "2")], True), ("shell_type", "command_id", CAP + 1, None, False),
               (None, "exit_code", CAP, [("risk_level", ">", "3")], True), ("risk_level", "user_name", 40, [("sudo_used", "=", "TRUE")], False)]
    try:
        alone = [eng.group_head(*query) for query in queries]
        wrong, gate = [], threading.Barrier(2)

        def worker(shift):
            try:
                gate.wait()
                for turn in range(12):
                    k = (turn + shift) % len(queries)
                    if eng.group_head(*queries[k]) != alone[k]:
                        wrong.append((shift, turn))
            except BaseException as e:                              # noqa: BLE001 -- reported by the assert below
                wrong.append(repr(e))

        threads = [threading.Thread(target=worker, args=(s,)) for s in (0, 2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not wrong, wrong
    finally:
        eng.close()


@pytest.mark.gpu
def test_round_cap_from_the_environment():
    """PQPS_HEAD_ROUNDS, read per query, moves the switch: the same answers from either form, and the form that ran shows in
    the last kernel the calling thread launched."""
    eng = pq.HipEngine(CSV2K, [])
    chain = [("risk_level", ">", "2")]
    last = lambda: pq.lib().pqps_last_kernel().decode()
    saved = os.environ.pop("PQPS_HEAD_ROUNDS", None)
    try:
        want = {n: eng.group_head("shell_type", "exit_code", n, chain, True) for n in (1, 3, CAP)}
        assert "head_scan_kernel" in last()
        for cap in ("0", "2", str(CAP + 50)):
            os.environ["PQPS_HEAD_ROUNDS"] = cap
            for n in (1, 3, CAP):
                assert eng.group_head("shell_type", "exit_code", n, chain, True) == want[n], (cap, n)
                rounds = n <= min(int(cap), CAP)
                assert ("first_scan_kernel" in last() or "head_scan_kernel" in last()) == rounds, (cap, n, last())
    finally:
        os.environ.pop("PQPS_HEAD_ROUNDS", None)
        if saved is not None:
            os.environ["PQPS_HEAD_ROUNDS"] = saved
        eng.close()


@pytest.mark.gpu
def test_refusals():
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for group, column, n in (("no_such_column", "timestamp", 3), ("user_name", "no_such_column", 3), ("command_id", "timestamp", 3),
                                 (None, "no_such_column", 3), ("user_name", "timestamp", 0), ("user_name", "timestamp", -4), (None, "timestamp", 0),
                                 ("user_name", None, 3)):
            with pytest.raises(pq.PqpsError):
                eng.group_head(group, column, n)
            with pytest.raises(pq.PqpsError):
                eng.select_group_head(None, None, group, column, n)
        for column in q.COLUMNS:                                         # every column can be the order column, in both forms
            for n in (2, CAP + 1):
                got, total = eng.group_head("shell_type", column, n, [("risk_level", ">", "3")], True)
                assert got and total > 0 and max(len(rows) for _, rows in got) == n
        got, _ = eng.group_head("user_name", "user_name", 3)             # group column == order column
        assert all(text == key for key, rows in got for _, text in rows)
    finally:
        eng.close()
    # more than 65 536 groups: an exit_code far away from the others -- as a group column only
    rng = np.random.default_rng(36)
    cols = gfe.edge_columns(5000, rng, 10)
    cols["exit_code"][7] = 1 << 20
    eng = pq.HipEngine.from_columns(5000, cols)
    try:
        for n in (2, CAP + 1):
            with pytest.raises(pq.PqpsError):
                eng.group_head("exit_code", "risk_level", n)
            got, _ = eng.group_head(None, "exit_code", n, None, True)
            assert got[0][1][0] == (7, str(1 << 20)) and len(got[0][1]) == n
    finally:
        eng.close()
    # an empty table: no groups
    eng = pq.HipEngine.from_columns(0, gfe.edge_columns(0, rng, 5))
    try:
        for n in (1, CAP + 1):
            assert eng.group_head("user_name", "risk_level", n) == ([], 0)
            assert eng.group_head(None, "command_id", n, None, True) == ([], 0)
            out = eng.select_group_head(None, None, "user_name", "risk_level", n)
            assert out["numRecords"] == 0 and out["offsets"] == [0]
            eng.free_columnar(out)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    code = gfe.RANKS_CODE.replace('eng.group_first(column, "risk_level")', 'eng.group_head(column, "risk_level", 3)')
    assert code != gfe.RANKS_CODE
    p = subprocess.run([sys.executable, "-c", code.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
