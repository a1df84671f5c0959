"""The first row of every group (executeQueryGroupFirstHIP / HipEngine.group_first, select_group_first): per group of one
column among the rows executeQuerySelectIdsHIP returns, the row that comes first in the order of a second column, ties to the
lowest row number in both directions.  Every expected answer comes from tests/group_first_model.py over rows and cells the
oracle, HostSynth or tests/column_model.py give -- never from the engine.  Covers the fused scan's three bin paths and the
two-pass form of command_id, the list path (index probes with their duplicates, WHEREs of several passes, a member pass),
single-valued group and order columns, shards, writers, the projection, the refusals and the lane rule."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import group_first_model as m
from column_model import ColumnModel

q, grp = m.q, m.grp
pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
GROUPS = ("user_name", "shell_type", "sudo_used", "risk_level", None)
ORDERS = ("timestamp", "command_id", "exit_code", "user_name", "sudo_used")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    model = m.CsvModel(orc)
    chains = grp.golden_chains()
    assert len(chains) > 50
    try:
        for chain in chains + [None]:
            ids = orc.select_ids(chain)[0]
            for group in GROUPS:
                counts = eng.group_count(group, chain) if group else None
                for column in ORDERS:
                    for desc in (False, True):
                        got, total = eng.group_first(group, column, chain, desc)
                        assert got == model.expected(ids, group, column, desc), (indexes, group, column, desc, chain)
                        assert total == len(ids)
                        if group:
                            assert [k for k, _, _ in got] == [k for k, _ in counts]
    finally:
        eng.close()


def where_value(column, text):
    return text.upper() if column == "sudo_used" else text


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1025])
def test_synthetic_index_probes(n):
    """WHEREs the risk_level index probes are not fused: the selection's per-shard lists and the list kernels.  Over two
    shards (test_over_shards) the one-row table leaves the second shard without rows: the total is the
    selection's there, never the unwritten count in front of a shard's words."""
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n, indexes=grp.PROBE_INDEXES)
    try:
        for cname, chain in grp.PROBED_CHAINS.items():
            rows = np.asarray(host.oracle_scan(chain, nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            assert len(rows) == {"probe_ge1": n, "probe_nothing": 0}.get(cname, len(rows))
            for group in ("user_name", "risk_level", "sudo_used", None):
                for column in ("timestamp", "command_id", "exit_code", "user_name"):
                    for desc in (False, True):
                        got, total = eng.group_first(group, column, chain, desc)
                        assert total == len(rows), (n, cname, group, column, desc)
                        assert got == m.synth_expected(host, rows, group, column, desc), (n, cname, group, column, desc)
    finally:
        eng.close()


@pytest.mark.gpu
def test_equals_order_ids_limit_1_of_the_group():
    """The consequence the header states: rows[g] is the first row of order_ids(WHERE AND group = key, limit 1)."""
    eng = pq.HipEngine(CSV2K, [])
    chains = [None, [("risk_level", ">", "2")], grp.S1, [("sudo_used", "=", "TRUE"), "OR", [("risk_level", "=", "5"), "AND", ("shell_type", "=", "bash")]]]
    try:
        for chain in chains:
            for group in GROUPS:
                for column, desc in (("timestamp", True), ("command_id", False), ("exit_code", True), ("user_name", False)):
                    got, total = eng.group_first(group, column, chain, desc)
                    if group is None:
                        ids, matches = eng.order_ids(column, chain, desc, 1)
                        assert matches == total and [r for _, r, _ in got] == ids
                        continue
                    for key, row, _ in got[:2] + got[-2:]:
                        narrowed = [(group, "=", where_value(group, key))] + (["AND", list(chain)] if chain else [])
                        ids, _ = eng.order_ids(column, narrowed, desc, 1)
                        assert ids == [row], (chain, group, key, column, desc)
    finally:
        eng.close()


SYNTH_SMALL = [(c, g, o, d) for c in ("all", "s1", "risk_gt2", "nothing", "or_tree") for g in ("user_name", "risk_level", "sudo_used", "shell_type", None)
               for o in ("timestamp", "command_id", "exit_code", "user_name", "sudo_used") for d in (False, True)]
SYNTH_BIG = [("all", "user_name", "command_id", True), ("all", "risk_level", "user_name", False), ("all", None, "exit_code", True),
             ("all", "user_name", "timestamp", True), ("s1", "shell_type", "command_id", False), ("risk_gt2", "sudo_used", "user_id", True),
             ("risk_gt2", "user_name", "sudo_used", False), ("or_tree", "host_name", "command_id", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1025, 65537, (1 << 20) + 3])
def test_synthetic(n):
    """timestamp is single-valued in the synthetic table: the lowest matching row of every group."""
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    rows = {}
    try:
        for cname, group, column, desc in (SYNTH_BIG if n > 100000 else SYNTH_SMALL):
            chain = grp.SYNTH_CHAINS[cname]
            if cname not in rows:
                rows[cname] = np.asarray(host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            got, total = eng.group_first(group, column, chain, desc)
            assert total == len(rows[cname])
            assert got == m.synth_expected(host, rows[cname], group, column, desc), (n, cname, group, column, desc)
    finally:
        eng.close()


@pytest.mark.gpu
def test_rounds_form_whatever_the_round_cap_says():
    """group_first is one round of the N-rows driver, always in its rounds form: PQPS_HEAD_ROUNDS moves the switch of
    group_head only.  With the variable unset and at 0 the answers are the model's and a scan-mode WHERE runs
    first_scan_kernel, while group_head(.., 1) at 0 still takes the sort form."""
    n = 4099
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    chain = grp.SYNTH_CHAINS["risk_gt2"]
    rows = np.asarray(host.oracle_scan(chain, nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
    last = lambda: pq.lib().pqps_last_kernel().decode()
    saved = os.environ.pop("PQPS_HEAD_ROUNDS", None)
    try:
        for cap in (None, "0"):
            if cap is not None:
                os.environ["PQPS_HEAD_ROUNDS"] = cap
            for group in ("host_name", "risk_level", "shell_type", "sudo_used", None):
                for column, desc in (("exit_code", True), ("command_id", False), ("user_name", False)):
                    got, total = eng.group_first(group, column, chain, desc)
                    assert "first_scan_kernel" in last(), (cap, group, column, last())
                    assert total == len(rows), (cap, group, column, desc)
                    assert got == m.synth_expected(host, rows, group, column, desc), (cap, group, column, desc)
        first, total = eng.group_first("host_name", "exit_code", chain, True)
        one, total1 = eng.group_head("host_name", "exit_code", 1, chain, True)
        assert "first_scan_kernel" not in last() and "head_scan_kernel" not in last(), last()
        assert total1 == total and one == [(key, [(row, text)]) for key, row, text in first]
    finally:
        os.environ.pop("PQPS_HEAD_ROUNDS", None)
        if saved is not None:
            os.environ["PQPS_HEAD_ROUNDS"] = saved
        eng.close()


def edge_columns(n, rng, users, **over):
    """from_columns input: user_name a dictionary of `users` words, shell_type of 4, the other strings single-valued."""
    words = [b"w%06d" % i for i in range(users)]
    codes = rng.integers(0, users, size=n).astype(np.uint8 if users <= 256 else np.uint16 if users <= 65536 else np.uint32)
    cols = {name: (None, [b"x"]) for name in q.ORC_STR}
    cols.update(command_id=np.arange(1, n + 1, dtype=np.uint64), exit_code=rng.integers(-3, 4, size=n).astype(np.int32),
                user_id=rng.integers(1000, 1400, size=n).astype(np.int32), risk_level=rng.integers(1, 6, size=n).astype(np.int32),
                sudo_used=(rng.random(n) < 0.3).astype(np.uint8), user_name=(codes, words),
                shell_type=(rng.integers(0, 4, size=n).astype(np.uint8), [b"bash", b"fish", b"sh", b"zsh"]))
    cols.update(over)
    return cols


EDGE_CHAINS = (None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("risk_level", "<", "3")], [("risk_level", ">", "9")])


def column_expected(cm, ids, group, column, desc):
    ids = np.asarray(ids, dtype=np.int64)
    _, rows, _ = m.first_rows_fast(ids, cm.codes(column)[ids], cm.codes(group)[ids] if group else None, desc)
    return [(cm.cell(r, group) if group else None, r, cm.cell(r, column)) for r in rows.tolist()]


def check_columns(eng, cm, cases, chains=EDGE_CHAINS, indexes=()):
    for chain in chains:
        ids = cm.select_ids(chain, indexes)
        for group, column in cases:
            for desc in (False, True):
                got, total = eng.group_first(group, column, chain, desc)
                assert total == len(ids), (group, column, desc, chain)
                assert got == column_expected(cm, ids, group, column, desc), (group, column, desc, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("users", [8192, 8193])
def test_group_column_at_the_lds_switch(users):
    """A group column of exactly 8192 values (the LDS table) and of 8193 (atomics into global memory)."""
    n = 70001
    rng = np.random.default_rng([21, users])
    exit_code = rng.choice(np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], np.int32), size=n)
    big = np.array([0, 5, (1 << 63) - 1, 1 << 63, M64 - 1, M64], np.uint64)
    cols = edge_columns(n, rng, users, exit_code=exit_code, command_id=rng.choice(big, size=n))
    cols["user_name"][0][:users] = np.arange(users)                 # every value occurs
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, [("user_name", "exit_code"), ("user_name", "command_id"), ("user_name", "user_name"), ("user_name", "timestamp"),
                                ("user_name", "sudo_used"), (None, "command_id"), (None, "exit_code")])
    finally:
        eng.close()
    eng = pq.HipEngine.from_columns(n, cols, pq.DEFAULT_INDEXES)    # the list form over index probes
    try:
        check_columns(eng, cm, [("user_name", "exit_code"), ("user_name", "command_id"), (None, "command_id")], indexes=pq.DEFAULT_INDEXES)
    finally:
        eng.close()


@pytest.mark.gpu
def test_order_column_of_more_than_65536_values():
    """4-byte codes: nothing is refused for the size of the order column's domain."""
    n = (1 << 17) + 9
    users = 70000
    rng = np.random.default_rng(22)
    cols = edge_columns(n, rng, users)
    assert cols["user_name"][0].dtype == np.uint32
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, [("risk_level", "user_name"), ("shell_type", "user_name"), ("sudo_used", "user_name"), (None, "user_name"),
                                ("user_id", "user_name")])
        with pytest.raises(pq.PqpsError):                               # ... but the GROUP column keeps grouped COUNT's limit
            eng.group_first("user_name", "risk_level")
    finally:
        eng.close()


@pytest.mark.gpu
def test_like_and_in_member_pass():
    """A fragmented IN list and a LIKE: the member pass in front of the filter pass, then the list form."""
    n = 20011
    rng = np.random.default_rng(23)
    cols = edge_columns(n, rng, 300)
    cm = ColumnModel(cols)
    every_third = pq.in_list([w.decode() for w in cols["user_name"][1][::3]])
    chains = ([("user_name", "IN", every_third)], [("user_name", "IN", every_third), "AND", ("risk_level", ">", "2")],
              [("user_name", "LIKE", "w0000_7"), "OR", ("user_name", "NOT IN", every_third)])
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_columns(eng, cm, [("shell_type", "command_id"), ("user_name", "exit_code"), (None, "user_name"), ("risk_level", "sudo_used")],
                      chains=chains)
    finally:
        eng.close()


def second_shard_columns():
    """Every group's extreme -- the lowest and the highest key, and for ties the key every row shares -- sits in the last rows."""
    n = 40009
    rng = np.random.default_rng(24)
    cols = edge_columns(n, rng, 50, exit_code=rng.integers(0, 100, size=n).astype(np.int32),
                        command_id=rng.integers(1000, 2000, size=n).astype(np.uint64))
    tail = n - 200
    cols["exit_code"][tail:tail + 100] = -5
    cols["exit_code"][tail + 100:] = 500
    cols["command_id"][tail:tail + 100] = 7
    cols["command_id"][tail + 100:] = M64
    cols["user_name"][0][tail:] = np.arange(200) % 50
    return n, cols


@pytest.mark.gpu
def test_extreme_on_the_last_rows():
    n, cols = second_shard_columns()
    cm = ColumnModel(cols)
    cases = [("user_name", "exit_code"), ("user_name", "command_id"), (None, "exit_code"), (None, "command_id"), ("shell_type", "timestamp")]
    for indexes in ((), pq.DEFAULT_INDEXES):
        eng = pq.HipEngine.from_columns(n, cols, indexes)
        try:
            check_columns(eng, cm, cases, indexes=indexes)
            got, _ = eng.group_first("user_name", "exit_code", None, True)
            assert all(r >= n - 100 for _, r, _ in got) and len(got) == 50
        finally:
            eng.close()


@pytest.mark.gpu
def test_over_shards():
    """Two shards on one card (a child process: the engine reads PQPS_DEVICES when it is created): the extreme of every group
    on the second shard, synthetic tables (the one-row table leaves the second shard empty), the bins at the LDS switch, the
    writers and the projection again."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "extreme_on_the_last_rows or test_synthetic[1] or test_synthetic[1025] or synthetic_index_probes or 65537 or lds_switch or after_writers or select_group_first"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


@pytest.mark.gpu
def test_after_writers():
    """insert_rows (a new group, new extremes, a string between two existing ones), DELETE (the rows renumber) and UPDATE of
    the order column; the model is rebuilt by the same operations."""
    n = 6007
    rng = np.random.default_rng(25)
    cols = edge_columns(n, rng, 40)
    cm = ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols, pq.DEFAULT_INDEXES)
    cases = [("user_name", "exit_code"), ("user_name", "command_id"), ("shell_type", "user_name"), (None, "exit_code"), ("risk_level", "user_id")]
    chains = EDGE_CHAINS[:3]
    try:
        check_columns(eng, cm, cases, chains, pq.DEFAULT_INDEXES)                     # caches the i32 ranges
        b = 37
        batch = edge_columns(b, rng, 3, exit_code=np.full(b, 900, np.int32), command_id=np.arange(10**12, 10**12 + b, dtype=np.uint64),
                             risk_level=np.full(b, 7, np.int32))
        batch["user_name"][0][:3] = (0, 1, 2)
        batch["user_name"] = (batch["user_name"][0], [b"w000005x", b"w999999", b"zz_new"])
        assert eng.insert_rows(ColumnModel(batch).records()) == b
        cm.insert_batch(batch)
        assert eng.n == cm.n == n + b
        check_columns(eng, cm, cases, chains, pq.DEFAULT_INDEXES)
        got, _ = eng.group_first("user_name", "exit_code", None, True)
        assert got[-1][0] == "zz_new" and got[-1][2] == "900"
        wl = pq.WhereList([("risk_level", "=", "2"), "OR", ("shell_type", "=", "fish")])
        rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
        assert rs.contents.success
        pq.lib().freeResultSet(rs)
        deleted = cm.delete([("risk_level", "=", "2"), "OR", ("shell_type", "=", "fish")])
        assert 0 < deleted and eng.e.contents.num_records == cm.n
        check_columns(eng, cm, cases, chains, pq.DEFAULT_INDEXES)
        for assignments, where in (({"exit_code": -(1 << 20)}, [("user_id", ">=", "1390")]), ({"user_name": "w000001"}, [("risk_level", "=", "5")])):
            assert eng.update(assignments, where) == cm.update(assignments, where)
            check_columns(eng, cm, cases, chains, pq.DEFAULT_INDEXES)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_select_group_first(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_name", "=", "student1030"), "OR", ("exit_code", "!=", "0")], [("risk_level", ">", "9")]):
            plain = eng.select_columnar(None, chain)
            by_row = dict(zip(eng.select_ids(chain), plain["rows"]))
            eng.free_columnar(plain)
            for group, column, desc in (("user_name", "timestamp", True), ("shell_type", "command_id", False), (None, "exit_code", True),
                                        ("sudo_used", "user_name", False)):
                groups, total = eng.group_first(group, column, chain, desc)
                out = eng.select_group_first(None, chain, group, column, desc)
                assert out["success"] and out["matches"] == total and out["numRecords"] == len(groups)
                assert out["columns"] == list(q.COLUMNS)
                assert out["rows"] == [by_row[r] for _, r, _ in groups], (chain, group, column, desc)
                at = q.COLUMNS.index(column)
                assert [row[at] for row in out["rows"]] == [text for _, _, text in groups]
                eng.free_columnar(out)
            part = eng.select_group_first(["user_name", "command_id"], chain, "user_name", "command_id", True)
            assert part["columns"] == ["user_name", "command_id"]
            assert [row[0] for row in part["rows"]] == [k for k, _ in eng.group_count("user_name", chain)]
            eng.free_columnar(part)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals_and_the_lane_rule(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for group, column in (("no_such_column", "timestamp"), ("user_name", "no_such_column"), ("command_id", "timestamp"), (None, "no_such_column")):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.group_first(group, column)
            with pytest.raises(pq.PqpsError):
                eng.select_group_first(None, None, group, column)
            assert time.monotonic() - t0 < 5
        for column in q.COLUMNS:                                         # every column can be the order column
            got, total = eng.group_first("shell_type", column, [("risk_level", ">", "3")], True)
            assert got and total > 0
        got, _ = eng.group_first("user_name", "user_name")               # group column == order column
        assert all(k == text for k, _, text in got)
        # a thread that holds every lane is refused at once, not left to wait for itself
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(pq.lib().hipEngineLanes(eng.e))]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.group_first("user_name", "timestamp")
        with pytest.raises(pq.PqpsError):
            eng.select_group_first(None, None, "user_name", "timestamp")
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        assert eng.group_first("user_name", "timestamp", [("risk_level", ">", "3")])[0]      # usable again
    finally:
        eng.close()
    # more than 65 536 groups: an exit_code far away from the others -- as a group column only
    rng = np.random.default_rng(26)
    cols = edge_columns(5000, rng, 10)
    cols["exit_code"][7] = 1 << 20
    eng = pq.HipEngine.from_columns(5000, cols)
    try:
        with pytest.raises(pq.PqpsError):
            eng.group_first("exit_code", "risk_level")
        got, _ = eng.group_first(None, "exit_code", None, True)
        assert got == [(None, 7, str(1 << 20))]
    finally:
        eng.close()
    # an empty table: no groups
    eng = pq.HipEngine.from_columns(0, edge_columns(0, rng, 5))
    try:
        assert eng.group_first("user_name", "risk_level") == ([], 0)
        assert eng.group_first(None, "command_id", None, True) == ([], 0)
    finally:
        eng.close()


RANKS_CODE = """
import os, sys, threading, traceback
sys.path.insert(0, ROOT_TESTS)
import qpelib as q
pq = q.pq
LOOPBACK = os.path.join(ROOT_TESTS, "loopback", "libloopback_rccl.so")
world = 2
gate = threading.Barrier(world)
ident = [None]
refused = [None] * world

def rank_main(rank):
    try:
        eng = pq.HipEngine.synthetic_rank(100003, world, rank, seed=0x5EED)
        if rank == 0:
            ident[0] = pq.HipEngine.rccl_id(LOOPBACK)
        gate.wait()
        eng.join_ranks(LOOPBACK, ident[0])
        n = 0
        for column in (None, "user_name"):
            try:
                eng.group_first(column, "risk_level")
            except pq.PqpsError:
                n += 1
        refused[rank] = n
        gate.wait()
        eng.leave_ranks()
        eng.close()
    except BaseException:
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(3)

threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for th in threads: th.start()
for th in threads: th.join()
assert refused == [2, 2], refused
print("OK")
"""


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
