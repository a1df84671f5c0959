"""ORDER BY several columns (executeQueryOrderIdsByHIP / executeQuerySelectOrderedByHIP, HipEngine.order_ids_by /
select_ordered_by).  Expected orders never come from the engine and never pack a key: for a CSV the rows of the oracle's
select_ids sorted by Python's stable `sorted`, once per key from the last to the first, over the oracle's cells (the keys of
tests/test_gpu_order_by.py); np.lexsort over the raw values for synthetic and column engines; tests/column_model.py's cells
after writers.  Rows equal in all keys come in ascending row number whatever the directions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import column_model as cm
import qpelib as q
import test_gpu_aggregate as agg
import test_gpu_group_count as grp
import test_gpu_order_by as ob
import test_gpu_set_predicates as sps
import test_gpu_update as up

pq = q.pq
CSV2K, EDGE = q.GOLDEN / "commands_2k.csv", q.GOLDEN / "edge_cases.csv"
LIMITS = (1, 20, 512, 513, 1024, 1025, None)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
KEY_LISTS = [
    [("risk_level", True), ("timestamp", True)],
    [("user_name", False), ("exit_code", True)],
    [("sudo_used", True), ("host_name", False), ("base_command", False)],
    [("shell_type", False), ("user_id", False), ("risk_level", False), ("timestamp", False)],
    [("user_id", False), ("command_id", True)],                               # CHAIN
    [("risk_level", True), ("risk_level", False), ("exit_code", False)],      # a repeated column
]


def sorted_by(cell, ids, keys):
    """ids (duplicates kept) ordered by the keys: stable sorts from the row up to the first key."""
    rows = sorted(ids)
    for column, desc in reversed(keys):
        rows = sorted(rows, key=lambda r: ob.cell_key(column, cell(r, column)), reverse=desc)
    return rows


def check_cells(eng, cell, ids, chain, key_lists=KEY_LISTS, limits=LIMITS):
    for keys in key_lists:
        full = sorted_by(cell, ids, keys)
        for limit in limits:
            got, matches = eng.order_ids_by(keys, chain, limit)
            assert matches == len(ids), (keys, limit, chain)
            assert got == ob.cut(full, limit), (keys, limit, chain)


def csv_chains(csv):
    g = grp.golden_chains()
    picked = [g[i] for i in (0, 2, 4, 7, 14, 19, 22, 53, 55, 60, 68)] + [None]     # sparse, dense, nothing, several passes
    t_values = {c: sorted({r for r in (q.OracleTable(csv, []).cell(i, c) for i in range(50))}) for c in ("user_name", "host_name")}
    sets = [[sps.IN("user_name", t_values["user_name"][::3])],
            [("host_name", "LIKE", "%1"), "OR", sps.IN("risk_level", ["4", "5"])],
            [sps.IN("exit_code", ["0", "1", "2", "127"], True), "AND", ("raw_command", "NOT LIKE", "%a%")]]
    return picked, sets


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
@pytest.mark.parametrize("csv", [CSV2K, EDGE], ids=["2k", "edge"])
def test_golden_csv(csv, indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(csv, idx)
    orc = q.OracleTable(csv, idx)
    # neither golden CSV has a single-valued column (the key lists below would lose it): that rule is exercised on the column
    # engine of test_three_full_range_i32_keys_take_the_chain and on the synthetic table, whose timestamp has one value
    assert not [c for c in q.COLUMNS if len({orc.cell(r, c) for r in range(orc.n)}) == 1]
    key_lists = list(KEY_LISTS)
    picked, sets = csv_chains(csv)
    try:
        for i, chain in enumerate(picked):                            # every limit on every third chain (None among them)
            check_cells(eng, orc.cell, orc.select_ids(chain)[0], chain, key_lists, LIMITS if i % 3 == 2 else (20, 513, None))
        if not idx:                                                  # LIKE / IN member passes: the rows by plain Python
            for chain in sets:
                ids = [r for r in range(orc.n) if sps.chain_true(orc.rows[r], chain)]
                check_cells(eng, orc.cell, ids, chain, key_lists, (20, 513, None))
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_key_is_the_one_column_query():
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for chain in (None, [("risk_level", ">", "3")], grp.S1):
            for column in q.COLUMNS:
                for desc in (False, True):
                    for limit in (20, 600, None):
                        assert eng.order_ids_by([(column, desc)], chain, limit) == eng.order_ids(column, chain, desc, limit), (column, desc, limit)
            assert eng.order_ids_by(["user_name", ("user_name", True)], chain, 30) == eng.order_ids("user_name", chain, False, 30)
    finally:
        eng.close()


def lexsort_rows(raws, descs, rows, limit=None):
    cols = [rows]
    for raw, d in reversed(list(zip(raws, descs))):
        k = raw[rows]
        if d:
            k = ~k if k.dtype == np.uint64 else -k.astype(np.int64)
        cols.append(k)
    order = rows[np.lexsort(cols)]
    return order.tolist() if not limit else order[:limit].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", [(), pq.DEFAULT_INDEXES])
def test_three_full_range_i32_keys_take_the_chain(indexes):
    """96 bits of keys fit no packed form; also single-valued string columns and no key left at all."""
    n = 70001
    rng = np.random.default_rng(31)
    pool = np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], np.int32)
    cols, _, _ = agg.edge_columns(n, rng, 300, exit_code=rng.choice(pool, size=n), user_id=rng.choice(pool, size=n))
    cols["risk_level"][:7] = pool
    eng = pq.HipEngine.from_columns(n, cols, indexes)
    names = ("exit_code", "user_id", "risk_level")
    raws = [cols[c].astype(np.int64) for c in names]
    try:
        for chain, mask in zip(agg.EDGE_CHAINS, agg.edge_masks(cols)):
            rows = np.flatnonzero(mask)
            for descs in ((False, False, False), (True, False, True), (True, True, True)):
                for limit in (1, 20, 1025, None):
                    got, matches = eng.order_ids_by(list(zip(names, descs)), chain, limit)
                    assert matches == len(rows)
                    assert got == lexsort_rows(raws, descs, rows, limit), (chain, descs, limit, indexes)
            # two full-range keys: exactly 64 bits, the wide packed key
            for limit in (20, 512, 513, None):
                got, _ = eng.order_ids_by([("user_id", True), "exit_code"], chain, limit)
                assert got == lexsort_rows([raws[1], raws[0]], (True, False), rows, limit), (chain, limit)
            # single-valued string columns carry nothing: one key is left, or none (the row order)
            assert eng.order_ids_by(["shell_type", ("exit_code", True)], chain, 20) == eng.order_ids("exit_code", chain, True, 20)
            for limit in (20, None):
                got, matches = eng.order_ids_by(["shell_type", ("base_command", True)], chain, limit)
                assert matches == len(rows) and got == sorted(rows.tolist())[:limit], (chain, limit)
    finally:
        eng.close()


@pytest.mark.gpu
def test_synthetic_table():
    n = 1 << 20
    host = q.HostSynth(n, full=True)                                 # pqps_synth_generate_host
    eng = pq.HipEngine.synthetic(n)
    key_lists = ([("risk_level", True), ("user_name", False)], [("sudo_used", False), ("shell_type", True), ("user_id", False)],
                 [("user_name", False), ("timestamp", True)], [("host_name", True), ("command_id", False)],
                 [("exit_code", False), ("base_command", False), ("risk_level", True), ("host_name", False)])
    try:
        for cname in ("all", "s1", "risk_gt1", "or_tree"):
            chain = grp.SYNTH_CHAINS[cname]
            rows = np.asarray(host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            for keys in (key_lists[:2] if cname == "all" else key_lists):
                full = lexsort_rows([ob.synth_keys(host, c) for c, _ in keys], [d for _, d in keys], rows)
                for limit in ((20, 1024) if cname == "all" else (20, 512, 1025, None)):
                    got, matches = eng.order_ids_by(keys, chain, limit)
                    assert matches == len(rows), (cname, keys, limit)
                    assert got == ob.cut(full, limit), (cname, keys, limit)
    finally:
        eng.close()


@pytest.mark.gpu
def test_writers_move_the_plan():
    """INSERT, UPDATE and DELETE that widen an i32 range and add dictionary strings between queries: the bounds and counts
    of the first query must not survive them."""
    model = cm.ColumnModel(up.base_model())
    eng = pq.HipEngine.from_columns(model.n, model.m, up.INDEXES)
    key_lists = [[("exit_code", True), ("user_name", False)], [("user_name", True), ("user_id", False), ("host_name", False)],
                 [("risk_level", False), ("exit_code", False), ("sudo_used", True), ("base_command", True)],
                 [("user_id", False), ("command_id", True)]]
    chains = [None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("user_id", ">=", "1040")]]

    def check():
        for chain in chains:
            check_cells(eng, model.cell, model.select_ids(chain, up.INDEXES), chain, key_lists, (20, 1025, None))

    try:
        check()
        want = model.update({"exit_code": -100000, "user_name": "student1020x", "risk_level": 9}, [("user_id", "=", "1003")])
        assert want is not None and eng.update({"exit_code": -100000, "user_name": "student1020x", "risk_level": 9}, [("user_id", "=", "1003")]) == want
        check()
        b = 9
        batch = {c: cm.coded([b"zz-new-%d" % (i % 3) for i in range(b)]) if c in cm.STRINGS else None for c in pq.COLUMNS}
        batch.update(command_id=np.arange(900001, 900001 + b, dtype=np.uint64), exit_code=np.arange(b, dtype=np.int32) * 70000 + INT32_MAX - 700000,
                     user_id=np.full(b, -5, np.int32), risk_level=np.arange(b, dtype=np.int32) % 5, sudo_used=np.arange(b, dtype=np.uint8) % 2)
        assert eng.insert_columns(b, batch) == model.insert_batch(batch)
        check()
        wl = pq.WhereList([("risk_level", "=", "2")])
        rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
        assert rs.contents.success
        pq.lib().freeResultSet(rs)
        model.delete([("risk_level", "=", "2")])
        assert eng.count(None) == model.n
        check()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_select_ordered_by(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_name", "=", "student1030"), "OR", ("exit_code", "!=", "0")]):
            plain = eng.select_columnar(None, chain)
            by_row = dict(zip(eng.select_ids(chain), plain["rows"]))
            eng.free_columnar(plain)
            for keys, limit in ((KEY_LISTS[0], 20), (KEY_LISTS[1], None), (KEY_LISTS[3], 1025), (KEY_LISTS[4], 7)):
                ids, matches = eng.order_ids_by(keys, chain, limit)
                out = eng.select_ordered_by(None, chain, keys, limit)
                assert out["success"] and out["matches"] == matches and out["numRecords"] == len(ids)
                assert out["rows"] == [by_row[i] for i in ids], (chain, keys, limit)
                eng.free_columnar(out)
            part = eng.select_ordered_by(["user_name", "exit_code"], chain, KEY_LISTS[1], 5)
            assert part["columns"] == ["user_name", "exit_code"] and part["numRecords"] == min(5, part["matches"])
            eng.free_columnar(part)
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV, column-engine, synthetic and writer cases again with the rows split over two shards of one card (a fresh child
    process: the engine reads PQPS_DEVICES when it is created)."""
    env = dict(os.environ, PQPS_DEVICES="0,0")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or full_range or synthetic_table or writers or select_ordered_by"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


@pytest.mark.gpu
def test_refusals():
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    L = pq.lib()
    try:
        for keys in ([], ["user_name"] * 5, ["no_such_column"], ["user_name", "no_such_column"]):
            with pytest.raises(pq.PqpsError):
                eng.order_ids_by(keys, None, 20)
            with pytest.raises(pq.PqpsError):
                eng.select_ordered_by(None, None, keys, 20)
        arr = (pq.OrderKey * 2)()
        arr[0].column = b"user_name"                                 # arr[1].column stays NULL
        ids = pq.C.POINTER(pq.C.c_uint)()
        assert L.executeQueryOrderIdsByHIP(eng.e, None, arr, 2, 20, pq.C.byref(ids), None, None) == -1
        assert L.executeQueryOrderIdsByHIP(eng.e, None, None, 1, 20, pq.C.byref(ids), None, None) == -1
        # nothing is refused for the size of a domain or for command_id among the keys
        assert eng.order_ids_by(["timestamp", "raw_command", "user_name", "command_id"], [("risk_level", ">", "3")], 5)[1] > 0
    finally:
        eng.close()


RANKS_CODE = agg.RANKS_CODE.replace('eng.aggregate("risk_level", column, None)',
                                    'eng.order_ids_by(["risk_level", "user_name"], None, 20 if column else None)')


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    assert RANKS_CODE != agg.RANKS_CODE
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_order_by_several_columns_is_exported():
    """CPU: the library exports the calls and the package wraps them."""
    L = pq.lib()
    for sym in ("executeQueryOrderIdsByHIP", "executeQuerySelectOrderedByHIP", "hipOrderKeyPlan", "pqps_filter_topk_multi",
                "pqps_topk_list_multi", "pqps_sort_list_multi", "pqps_sort_list_chain"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "order_ids_by", None))
    assert callable(getattr(pq.HipEngine, "select_ordered_by", None))
