"""ORDER BY one column [DESC] with LIMIT (executeQueryOrderIdsHIP / executeQuerySelectOrderedHIP, HipEngine.order_ids /
select_ordered) over the rows executeQuerySelectIdsHIP returns.  Every expected order comes from the oracle -- the rows of
oracle.select_ids(chain) sorted in Python by (key of oracle.cell(r, column), r) for a CSV, numpy over HostSynth +
oracle_scan for the synthetic tables, numpy over the arrays handed to HipEngine.from_columns -- never from the engine.
Keys: i32 columns signed, command_id unsigned, false before true, strings as bytes; DESC reverses the key, never the row.
Covers the fused top-K kernel, the list path (index probes with their duplicates, WHERE lists of several passes), the full
sort, K at and past its bounds, shards, INSERT / DELETE, the projection and the refusals."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import qpelib as q
import test_gpu_aggregate as agg
import test_gpu_group_count as grp

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
TOPK_MAX, TOPK_MAX_WIDE = 1024, 512                     # PQPS_TOPK_MAX / PQPS_TOPK_MAX_WIDE (include/pqps_hip.h)
I32 = ("exit_code", "user_id", "risk_level")
GOLDEN_ORDER = ("command_id", "exit_code", "risk_level", "user_name", "timestamp", "sudo_used", "base_command")
LIMITS = (1, 20, TOPK_MAX_WIDE, TOPK_MAX_WIDE + 1, TOPK_MAX, TOPK_MAX + 1, None)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def cell_key(column, text):
    if column in I32 or column == "command_id":
        return int(text)                                 # i32 signed, command_id printed unsigned
    if column == "sudo_used":
        return text == "true"
    return text.encode("latin-1")                        # strcmp byte order


def sort_rows(rows, keys, descending):
    """rows (with their keys) by key, ties by ascending row in both directions: a stable sort on the row first."""
    pairs = sorted(zip(rows, keys), key=lambda p: p[0])
    return [r for r, _ in sorted(pairs, key=lambda p: p[1], reverse=descending)]


def cut(order, limit):
    return order if not limit or limit <= 0 else order[:limit]


def check_csv(eng, orc, chain, columns=GOLDEN_ORDER, limits=LIMITS):
    ids = orc.select_ids(chain)[0]
    for column in columns:
        keys = [cell_key(column, orc.cell(r, column)) for r in ids]
        for desc in (False, True):
            full = sort_rows(ids, keys, desc)
            for limit in limits:
                got, matches = eng.order_ids(column, chain, desc, limit)
                assert matches == len(ids), (column, desc, limit, chain)
                assert got == cut(full, limit), (column, desc, limit, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    chains = grp.golden_chains()
    assert len(chains) > 50
    try:
        for chain in chains + [None]:
            check_csv(eng, orc, chain)
    finally:
        eng.close()


def synth_keys(host, column):
    """Keys of the synthetic columns whose order is the required one: ranks of the words for dictionary columns."""
    a = host.arr[column]
    if column in host.values:
        words = host.values[column]
        rank = np.empty(len(words), np.int64)
        rank[sorted(range(len(words)), key=lambda i: words[i])] = np.arange(len(words))
        return rank[a.astype(np.int64)]
    return a


def numpy_order(keys, rows, descending, limit):
    """rows ordered by (keys[rows] asc / desc, row asc)."""
    k = keys[rows]
    if descending:
        k = ~k if k.dtype == np.uint64 else -k.astype(np.int64)
    order = rows[np.lexsort((rows, k))]
    return order.tolist() if not limit else order[:limit].tolist()


SYNTH_ORDERS = (("command_id", True, (20, TOPK_MAX_WIDE, TOPK_MAX, None)), ("risk_level", False, (1, 20, TOPK_MAX, None)),
                ("risk_level", True, (20,)), ("user_name", False, (20, TOPK_MAX, TOPK_MAX + 1)), ("timestamp", False, (20, None)))


def check_synthetic(n, chains=("all", "s1", "risk_gt1"), orders=SYNTH_ORDERS):
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    try:
        for cname in chains:
            chain = grp.SYNTH_CHAINS[cname]
            rows = np.asarray(host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            for column, desc, limits in orders:
                keys = synth_keys(host, column)
                for limit in limits:
                    got, matches = eng.order_ids(column, chain, desc, limit)
                    assert matches == len(rows), (n, cname, column, desc, limit)
                    assert got == numpy_order(keys, rows, desc, limit), (n, cname, column, desc, limit)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 65537, (1 << 20) + 3])
def test_synthetic_small(n):
    check_synthetic(n)


@pytest.mark.gpu
def test_synthetic_large():
    check_synthetic(30_000_007, orders=(("command_id", True, (20, TOPK_MAX_WIDE)), ("risk_level", False, (20, TOPK_MAX)),
                                        ("user_name", False, (20,)), ("timestamp", False, (20,))))
    # the full sort of a sparse answer
    check_synthetic(30_000_007, chains=("s1",), orders=(("user_id", False, (None,)),))


def check_edge(cols, n, column, unsigned=False, indexes=(), limits=(1, 20, TOPK_MAX, TOPK_MAX + 1, None)):
    eng = pq.HipEngine.from_columns(n, cols, indexes)
    v = cols[column]
    keys = (v[0] if isinstance(v, tuple) else v).astype(np.uint64 if unsigned else np.int64)
    try:
        for chain, mask in zip(agg.EDGE_CHAINS, agg.edge_masks(cols)):
            rows = np.flatnonzero(mask)
            for desc in (False, True):
                for limit in limits:
                    got, matches = eng.order_ids(column, chain, desc, limit)
                    assert matches == len(rows), (column, chain, desc, limit, indexes)
                    assert got == numpy_order(keys, rows, desc, limit), (column, chain, desc, limit, indexes)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", [(), pq.DEFAULT_INDEXES])
def test_signed_i32_keys(indexes):
    n = 70001
    rng = np.random.default_rng(11)
    exit_code = rng.choice(np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], np.int32), size=n)
    cols, _, _ = agg.edge_columns(n, rng, 300, exit_code=exit_code)
    check_edge(cols, n, "exit_code", indexes=indexes)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", [(), pq.DEFAULT_INDEXES])
def test_command_id_unsigned(indexes):
    n = 70001
    rng = np.random.default_rng(12)
    big = np.array([0, 5, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, (1 << 64) - 2, (1 << 64) - 1], np.uint64)
    cols, _, _ = agg.edge_columns(n, rng, 20, command_id=rng.choice(big, size=n))
    check_edge(cols, n, "command_id", unsigned=True, indexes=indexes,
               limits=(1, 20, TOPK_MAX_WIDE, TOPK_MAX_WIDE + 1, None))


@pytest.mark.gpu
@pytest.mark.parametrize("dict_size", [300, 70000])
def test_wide_dictionaries(dict_size):
    """u16 and u32 codes; the words are handed over in strcmp order, so the code is the key."""
    n = (1 << 17) + 9
    rng = np.random.default_rng(13)
    cols, _, _ = agg.edge_columns(n, rng, 300)
    words = [f"w{i:06d}".encode() for i in range(dict_size)]
    codes = rng.integers(0, dict_size, size=n).astype(np.uint16 if dict_size <= 65536 else np.uint32)
    cols["user_name"] = (codes, words)
    check_edge(cols, n, "user_name")


@pytest.mark.gpu
def test_every_row_tied():
    n = 50003
    rng = np.random.default_rng(14)
    cols, _, _ = agg.edge_columns(n, rng, 10, user_id=np.full(n, 7, np.int32))
    check_edge(cols, n, "user_id")
    check_edge(cols, n, "user_id", indexes=pq.DEFAULT_INDEXES, limits=(20, None))


@pytest.mark.gpu
def test_limit_past_matches_and_empty():
    eng = pq.HipEngine(CSV2K, [])
    orc = q.OracleTable(CSV2K, [])
    try:
        chain = [("risk_level", ">", "4")]
        k = len(orc.select_ids(chain)[0])
        got, matches = eng.order_ids("user_name", chain, False, k + 100)
        assert matches == k and len(got) == k
        assert eng.order_ids("user_name", [("risk_level", ">", "9")], True, 20) == ([], 0)
        assert eng.order_ids("user_name", [("risk_level", ">", "9")], True, None) == ([], 0)
        out = eng.select_ordered(["command_id"], [("risk_level", ">", "9")], "command_id", True, 20)
        assert out["success"] and out["numRecords"] == 0 and out["matches"] == 0
        eng.free_columnar(out)
    finally:
        eng.close()
    rng = np.random.default_rng(15)
    cols, _, _ = agg.edge_columns(0, rng, 5)
    eng = pq.HipEngine.from_columns(0, cols)
    try:
        for limit in (20, None):
            assert eng.order_ids("risk_level", None, False, limit) == ([], 0)
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV, small synthetic and from_columns cases again with the rows split over two shards of one card (a child process:
    the engine reads PQPS_DEVICES when it is created) -- fused path, list path and full sort."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or synthetic_small or signed_i32 or unsigned or insert_and_delete or select_ordered"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


@pytest.mark.gpu
def test_insert_and_delete(tmp_path):
    csv = tmp_path / "data.csv"
    shutil.copy(CSV2K, csv)
    L = pq.lib()
    eng = pq.HipEngine(csv, pq.DEFAULT_INDEXES)
    chains = [None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("user_id", ">=", "1040")]]
    columns = ("user_name", "exit_code", "command_id", "sudo_used")
    try:
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        names = sorted({orc.cell(r, "user_name") for r in range(orc.n)})
        middle = (names[len(names) // 2] + "_new").encode()          # between two existing words: the codes above it move
        assert middle.decode() not in names
        check_csv(eng, orc, None, columns, (20,))
        assert L.executeQueryInsertHIP(eng.e, b"Commands", ctypes.byref(grp.make_record(900001, 3, 1041, middle)))
        assert L.executeQueryInsertHIP(eng.e, b"Commands", ctypes.byref(grp.make_record(900002, -7, 1001, b"aaa_new_user")))
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)                 # the CSV now holds the two rows at its end
        assert orc.n == eng.e.contents.num_records
        for chain in chains:
            check_csv(eng, orc, chain, columns, (1, 20, TOPK_MAX + 1, None))
        lines = csv.read_bytes().split(b"\n")
        body = [ln for ln in lines[1:] if ln.strip()]
        wl = pq.WhereList([("risk_level", ">=", "4"), "OR", ("shell_type", "=", "fish")])
        keep = [i for i in range(orc.n) if not q.load_oracle().orc_eval_where(ctypes.byref(orc.rows[i]), wl.ptr)]
        rs = L.executeQueryDeleteHIP(eng.e, b"Commands", wl.ptr)
        assert rs.contents.success
        L.freeResultSet(rs)
        survivors = tmp_path / "survivors.csv"
        survivors.write_bytes(b"\n".join([lines[0]] + [body[i] for i in keep]) + b"\n")
        orc = q.OracleTable(survivors, pq.DEFAULT_INDEXES)
        assert orc.n == eng.e.contents.num_records == len(keep)
        for chain in chains:
            check_csv(eng, orc, chain, columns, (1, 20, TOPK_MAX + 1, None))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_select_ordered(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    L = pq.lib()
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_name", "=", "student1030"), "OR", ("exit_code", "!=", "0")]):
            plain = eng.select_columnar(None, chain)
            by_row = dict(zip(eng.select_ids(chain), plain["rows"]))
            eng.free_columnar(plain)
            for column, desc, limit in (("timestamp", True, 20), ("command_id", False, None), ("user_name", False, TOPK_MAX + 1),
                                        ("risk_level", True, 7)):
                ids, matches = eng.order_ids(column, chain, desc, limit)
                out = eng.select_ordered(None, chain, column, desc, limit)
                assert out["success"] and out["matches"] == matches and out["numRecords"] == len(ids)
                assert out["columns"] == list(q.COLUMNS)
                assert out["rows"] == [by_row[i] for i in ids], (chain, column, desc, limit)
                head = L.hipColumnarHead(out["handle"], 3)
                h = head.contents
                assert h.numRecords == len(ids)                          # the footer counts every row
                for i in range(min(3, len(ids))):
                    assert [h.data[i][j].decode("latin-1") for j in range(h.numColumns)] == out["rows"][i]
                L.freeResultSetHead(head, 3)
                eng.free_columnar(out)
            part = eng.select_ordered(["user_name", "command_id"], chain, "user_name", True, 5)
            assert part["columns"] == ["user_name", "command_id"] and part["numRecords"] == min(5, part["matches"])
            eng.free_columnar(part)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals():
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        with pytest.raises(pq.PqpsError):
            eng.order_ids("no_such_column", None, False, 20)
        with pytest.raises(pq.PqpsError):
            eng.select_ordered(None, None, "no_such_column", False, 20)
        for column in q.COLUMNS:                                         # every column can be an order column
            assert eng.order_ids(column, [("risk_level", ">", "3")], True, 5)[1] > 0
    finally:
        eng.close()


RANKS_CODE = agg.RANKS_CODE.replace('eng.aggregate("risk_level", column, None)',
                                    'eng.order_ids("risk_level", None, False, 20 if column else None)')


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    assert RANKS_CODE != agg.RANKS_CODE
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_order_by_is_exported():
    """CPU: the library exports ORDER BY and the package wraps it."""
    L = pq.lib()
    for sym in ("executeQueryOrderIdsHIP", "executeQuerySelectOrderedHIP", "pqps_filter_topk", "pqps_topk_list", "pqps_sort_list",
                "pqps_topk_scratch_bytes"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "order_ids", None))
    assert callable(getattr(pq.HipEngine, "select_ordered", None))
