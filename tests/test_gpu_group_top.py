"""The top-N groups at the engine (executeQueryGroupTopHIP / HipEngine.group_top): GROUP BY a column of any size, ORDER BY
COUNT / SUM / MIN / MAX or the key, LIMIT.  The tables, WHERE forms and checks are tests/group_top_matrix.py's; every expected
answer is tests/group_top_model.py's numpy fold over the rows ColumnModel.select_ids gives -- never an engine's, except for
the stated equivalences with group_count / aggregate.

  * wide columns: user_name with 70 000 strings (4-byte codes), exit_code spanning 100 001 values with negatives -- the wide
    bins; a second table whose exit_code holds INT_MIN and INT_MAX -- the sort route
  * every order in both directions at limits 1, 10, groupsTotal, groupsTotal + 1 and 0, with and without a value column
  * WHERE: none, one pass, several passes (41 comparisons) with fewer and with more rows than bins, a member pass (a
    fragmented IN), index probes whose duplicated rows count, no match; an empty table
  * ties: most names have one or two rows, and they come in key order in both directions
  * a CSV with 66 000 distinct raw_command strings; writers (a batch that widens the dictionary past 65 536, DELETE, UPDATE);
    the refusals (an engine joined across ranks among them) and the lane rule; three shards in child processes"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import column_model as cm
import group_top_matrix as gm
import group_top_model as gtm
import qpelib as q

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"


@pytest.mark.gpu
@pytest.mark.parametrize("column", gm.MAIN_COLUMNS)
@pytest.mark.parametrize("indexes", ["none", "indexed"])
def test_wide_columns(indexes, column):
    gm.check_main(gm.INDEXES if indexes == "indexed" else (), (column,), equivalences=False)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "indexed"])
def test_key_order_without_limit_is_group_count_and_aggregate(indexes):
    run = gm.Run(gm.table(), gm.INDEXES if indexes == "indexed" else ())
    try:
        gm.check_equivalences(run, ("none", "one_pass") + (("probes",) if indexes == "indexed" else ()))
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "indexed"])
def test_int_min_and_int_max_take_the_sort_route(indexes):
    gm.check_extremes(gm.INDEXES if indexes == "indexed" else ())


@pytest.mark.gpu
def test_empty_table():
    gm.check_empty_table()


@pytest.mark.gpu
def test_after_writers():
    gm.check_writers()


@pytest.mark.gpu
def test_csv_with_66000_commands(tmp_path):
    """group_count refuses raw_command of this CSV; group_top answers it."""
    n = 66_000
    lines = (CSV2K.read_text(encoding="latin-1").split("\n"))
    header, body = lines[0], [ln for ln in lines[1:] if ln.strip()]
    plain = [ln.split(",") for ln in body if '"' not in ln and ln.count(",") == 11]
    assert header.split(",")[:2] == ["command_id", "raw_command"] and len(plain) > 1000
    rows = []
    for i in range(n):
        f = list(plain[i % len(plain)])
        f[0], f[1] = str(i), "run-%05d" % i                       # every command once: every count ties
        rows.append(",".join(f))
    csv = tmp_path / "wide.csv"
    csv.write_text("\n".join([header] + rows) + "\n", encoding="latin-1")
    orc = q.OracleTable(csv, [])
    assert orc.n == n
    cells = [orc.cell(r, "raw_command") for r in range(n)]
    distinct = sorted(set(cells), key=lambda t: t.encode("latin-1"))
    assert len(distinct) > 65_536
    eng = pq.HipEngine(csv, [])
    try:
        with pytest.raises(pq.PqpsError):
            eng.group_count("raw_command")
        for chain in (None, [("risk_level", ">", "3")]):
            ids = orc.select_ids(chain)[0]
            code = {t: i for i, t in enumerate(distinct)}
            codes = np.array([code[t] for t in cells], dtype=np.int64)
            risk = np.array([int(orc.cell(r, "risk_level")) for r in range(n)], dtype=np.int64)
            f = gtm.fold(codes, risk, ids)
            for by, descending, limit in (("count", True, 20), ("key", False, 0), ("sum", True, 5), ("count", False, 3)):
                idx = gtm.order(f["key"], f[by], descending, limit).tolist()
                want = [(distinct[f["key"][i]], int(f["count"][i]), int(f["sum"][i]), int(f["min"][i]), int(f["max"][i])) for i in idx]
                got = eng.group_top_result("raw_command", "risk_level", by, descending, limit, chain)
                assert got["rows"] == want and got["total"] == len(ids) and got["groups_total"] == len(f["key"]), (by, descending, limit, chain)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals_and_lanes():
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for column, value, by in (("no_such_column", None, "count"), ("command_id", None, "count"), ("user_name", "no_such_column", "count"),
                                  ("user_name", "shell_type", "count"), ("user_name", "sudo_used", "sum"), ("user_name", None, 5),
                                  ("user_name", None, -1), ("user_name", None, "sum"), ("user_name", None, "min"), ("user_name", None, "max")):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.group_top(column, value, by)
            assert time.monotonic() - t0 < 5
        # a thread that holds every lane is refused at once, not left to wait for itself
        lanes = pq.lib().hipEngineLanes(eng.e)
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(lanes)]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.group_top("user_name")
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        # the query gives its lane back: more queries in a row than there are lanes, fused and over a list
        for i in range(lanes + 1):
            assert eng.group_top("user_name", "exit_code" if i % 2 else None, "count", True, 3, [("shell_type", "=", "bash")])
            assert eng.group_top("user_name", None, "key", False, 0, [("risk_level", ">", "3")])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("check", list(gm.SHARD_CHECKS))
def test_over_three_shards(check):
    """One of gm.SHARD_CHECKS again with the rows split over three shards of one card (a child process: the engine reads
    PQPS_DEVICES when it is created): a group's rows lie in several shards, and the runs are merged by key."""
    devices = "0,0,0"
    p = subprocess.run([sys.executable, str(q.ROOT / "tests" / "group_top_matrix.py"), "run", devices, check], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, PQPS_DEVICES=devices), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-3000:], p.stderr[-3000:])
    assert "shards=3 " in p.stdout and "compared=0" not in p.stdout


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
ASKED = [(column, value, by) for column in ("user_name", "user_id", "exit_code", "timestamp")
         for value, by in ((None, "count"), (None, "key"), ("risk_level", "sum"), ("command_id", "max"))]

def rank_main(rank):
    try:
        eng = pq.HipEngine.synthetic_rank(100003, world, rank, seed=0x5EED)
        if rank == 0:
            ident[0] = pq.HipEngine.rccl_id(LOOPBACK)
        gate.wait()
        eng.join_ranks(LOOPBACK, ident[0])
        n = 0
        for column, value, by in ASKED:
            for chain in (None, [("risk_level", ">", "3")]):
                try:
                    eng.group_top(column, value, by, True, 10, chain)
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
assert refused == [2 * len(ASKED)] * 2, refused
print("OK")
"""


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    """An engine joined across ranks refuses the top groups on every rank, with and without a value column, for every group
    column (a rank's engine is the synthetic table, whose widest columns hold 2000 values: the refusal comes before the
    plan, so the size of the column plays no part in it)."""
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    assert "not exchanged across ranks" in p.stderr


def test_tables_and_where_forms():
    """CPU: the tables hold what the header says, and every WHERE form compiles to the route its name says."""
    cols = gm.table()
    model = cm.ColumnModel(cols)
    gm.check_plans(model)
    assert len(cols["user_name"][1]) == gm.USERS > 65_536 and cols["user_name"][0].dtype.itemsize == 4
    assert int(cols["exit_code"].min()) == gm.EXIT_LO and int(cols["exit_code"].max()) == gm.EXIT_HI and gm.EXIT_HI - gm.EXIT_LO + 1 == 100_001
    ext = gm.table(20_000, 300, extremes=True)["exit_code"]
    assert int(ext.min()) == gm.INT32_MIN and int(ext.max()) == gm.INT32_MAX
    bins = (gm.USERS, gm.EXIT_HI - gm.EXIT_LO + 1)
    assert 0 < len(model.select_ids(gm.WHERES["several_passes"][0])) < min(bins)     # lists of fewer rows than bins ...
    assert 0 < len(model.select_ids(gm.WHERES["member"][0])) < min(bins)
    assert len(model.select_ids(gm.WHERES["dense_passes"][0])) > max(bins)           # ... and of more
    assert len(model.select_ids(gm.WHERES["probes"][0], gm.INDEXES)) > gm.USERS
    assert int(cols["command_id"].max()) >= 1 << 63


def test_group_top_is_exported():
    """CPU: the library exports the new entry points and the package wraps them (this fails before the feature exists)."""
    L = pq.lib()
    for sym in ("executeQueryGroupTopHIP", "freeGroupTopResultHIP", "hipGroupTopOrder", "pqps_filter_group_wide", "pqps_group_wide_list",
                "pqps_bins_compact", "pqps_group_sort"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "group_top", None)) and callable(getattr(pq.HipEngine, "group_top_result", None))
    fields = [f for f, _ in pq.GroupTopResult._fields_]
    assert fields[:7] == ["groupColumn", "groupKind", "valueColumn", "valueKind", "orderBy", "descending", "limit"]
    assert fields[7:10] == ["numGroups", "groupsTotal", "total"] and fields[-2:] == ["queryTime", "success"]
