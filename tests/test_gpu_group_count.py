"""Grouped COUNT(*) (executeQueryGroupCountHIP / HipEngine.group_count): per value of one column, how many of the rows
executeQuerySelectIdsHIP returns carry it.  Every expected answer comes from the oracle -- Counter(oracle.cell(r, col) for r
in oracle.select_ids(chain)) over a CSV, or numpy over HostSynth + oracle_scan for the synthetic tables -- never from the
engine itself.  Covers the fused kernel's three bin paths (D <= 16 in registers, D <= 16 384 in LDS, up to 65 536 in global
memory), the list path (index probes, WHERE lists of several passes), single-valued columns, shards, INSERT / DELETE and the
refusals."""
import collections
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import qpelib as q

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
GROUPABLE = [c for c in q.COLUMNS if c != "command_id"]
I32 = ("exit_code", "user_id", "risk_level")
SYNTH_GROUPS = ("user_name", "risk_level", "sudo_used", "shell_type", "host_name", "base_command", "user_id", "exit_code", "raw_command")
S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
SYNTH_CHAINS = {
    "all": None,
    "s1": S1,
    "risk_gt2": [("risk_level", ">", "2")],
    "risk_gt1": [("risk_level", ">", "1")],
    "nothing": [("risk_level", ">", "9")],
    "or_tree": [("sudo_used", "=", "TRUE"), "OR", [("risk_level", "=", "5"), "AND", ("shell_type", "=", "bash")]],
}
# with PROBE_INDEXES each is one probe of the risk_level index (every row, some rows, none): the list path, never fused
PROBE_INDEXES = [("risk_level", 1)]
PROBED_CHAINS = {
    "probe_ge1": [("risk_level", ">=", "1")],
    "probe_gt2": [("risk_level", ">", "2")],
    "probe_nothing": [("risk_level", ">", "9")],
}


def key_order(column, text):
    if column in I32:
        return int(text)
    if column == "sudo_used":
        return text == "true"
    return text.encode("latin-1")                              # strcmp byte order


def expected_from_cells(column, cells):
    cnt = collections.Counter(cells)
    return sorted(cnt.items(), key=lambda kv: key_order(column, kv[0]))


def oracle_groups(orc, chain, column):
    ids, k, _ = orc.select_ids(chain)
    assert len(ids) == k
    return expected_from_cells(column, [orc.cell(r, column) for r in ids]), k


def golden_chains():
    seen, out = set(), []
    for name in ("select_golden.json", "select_wide_golden.json"):
        for case in json.loads((q.GOLDEN / name).read_text()):
            if case["csv"] != "commands_2k.csv":
                continue
            key = json.dumps(case["where"])
            if key not in seen:
                seen.add(key)
                out.append(q.chain_from_jsonable(case["where"]))
    return out


def check_groups(eng, orc, chain, column):
    want, k = oracle_groups(orc, chain, column)
    got = eng.group_count(column, chain)
    assert got == want, (column, chain)
    assert sum(c for _, c in got) == k


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain_every_column(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    chains = golden_chains()
    assert len(chains) > 50
    try:
        for chain in chains + [None]:
            ids = orc.select_ids(chain)[0]
            assert eng.select_ids(chain) == ids
            for column in GROUPABLE:
                want = expected_from_cells(column, [orc.cell(r, column) for r in ids])
                got = eng.group_count(column, chain)
                assert got == want, (indexes, column, chain)
                assert sum(c for _, c in got) == len(ids)
    finally:
        eng.close()


@pytest.mark.gpu
def test_50k_csv_high_cardinality(tmp_path):
    """timestamp / raw_command / user_name of the 50 k-row file: at least one of them has more than 16 384 values and takes
    the global-memory bins."""
    gold = json.loads((q.GOLDEN / "commands_50k_golden.json").read_text())
    path = tmp_path / "commands_50k.csv"
    subprocess.run([sys.executable, str(q.ROOT / "scripts" / "make_csv.py"), str(gold["rows"]), str(path)], check=True)
    orc = q.OracleTable(path, pq.DEFAULT_INDEXES)
    distinct = {c: len({orc.cell(r, c) for r in range(orc.n)}) for c in ("timestamp", "raw_command", "user_name")}
    assert max(distinct.values()) > 16384, distinct
    eng = pq.HipEngine(path, pq.DEFAULT_INDEXES)
    try:
        for chain in (None, [("risk_level", ">", "2")], [("user_id", ">=", "1500"), "AND", ("sudo_used", "=", "TRUE")], S1):
            for column in ("timestamp", "raw_command", "user_name"):
                check_groups(eng, orc, chain, column)
    finally:
        eng.close()


def synth_expected(host, chain, column):
    ids = host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1))
    vals = host.arr[column][ids]
    keys, counts = np.unique(vals, return_counts=True)
    out = []
    for k, c in zip(keys.tolist(), counts.tolist()):
        if column in host.values:
            text = host.values[column][int(k)].decode("latin-1")
        elif column == "sudo_used":
            text = "true" if k else "false"
        else:
            text = str(int(k))
        out.append((text, int(c)))
    return out, len(ids)


def check_synthetic(n, chains=SYNTH_CHAINS, columns=SYNTH_GROUPS, indexes=()):
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n, indexes=indexes)
    try:
        for cname, chain in chains.items():
            for column in columns:
                want, k = synth_expected(host, chain, column)
                got = eng.group_count(column, chain)
                assert got == want, (n, cname, column)
                assert sum(c for _, c in got) == k == eng.count(chain or [])
                if cname.endswith("nothing"):
                    assert got == []
                if cname == "probe_ge1":
                    assert k == n
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 65537, (1 << 20) + 3])
def test_synthetic_small(n):
    check_synthetic(n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1025])
def test_synthetic_index_probes(n):
    """WHEREs the risk_level index probes are not fused: the selection's per-shard lists and the list kernels.  Over two
    shards (test_over_shards) the one-row table leaves the second shard without rows."""
    check_synthetic(n, chains=PROBED_CHAINS, indexes=PROBE_INDEXES)


@pytest.mark.gpu
def test_synthetic_large():
    check_synthetic(30_000_007, chains={k: SYNTH_CHAINS[k] for k in ("all", "s1", "risk_gt1")},
                    columns=("user_name", "risk_level", "sudo_used", "host_name", "user_id", "raw_command"))


@pytest.mark.gpu
def test_global_bins_over_a_wide_dictionary():
    """A dictionary column of 40 000 values (global-memory bins) on an engine over caller-supplied columns."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 40000, size=n).astype(np.uint16)
    risk = rng.integers(1, 6, size=n).astype(np.int32)
    words = [f"w{i:05d}".encode() for i in range(40000)]
    cols = {name: (None, [b"x"]) for name in q.ORC_STR + ["shell_type", "base_command"]}
    cols.update(command_id=np.arange(n, dtype=np.uint64), exit_code=np.zeros(n, np.int32), user_id=np.full(n, 1001, np.int32),
                risk_level=risk, sudo_used=np.zeros(n, np.uint8), user_name=(codes, words))
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        for chain, mask in ((None, np.ones(n, bool)), ([("risk_level", ">", "3")], risk > 3), ([("risk_level", ">", "9")], risk > 9)):
            keys, counts = np.unique(codes[mask], return_counts=True)
            want = [(words[k].decode(), int(c)) for k, c in zip(keys.tolist(), counts.tolist())]
            assert eng.group_count("user_name", chain) == want
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV and small synthetic cases again with the rows split over two shards of one card (a child process: the engine
    reads PQPS_DEVICES when it is created)."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or synthetic_small or synthetic_index_probes or insert_and_delete or wide_dictionary"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


def make_record(command_id, exit_code, user_id, user_name):
    r = pq.Record()
    r.command_id, r.exit_code, r.user_id, r.risk_level, r.sudo_used = command_id, exit_code, user_id, 4, True
    r.raw_command, r.base_command, r.shell_type = b"echo group", b"echo", b"bash"
    r.timestamp, r.working_directory, r.user_name, r.host_name = b"2025-12-01T12:00:00.000Z", b"/home/test", user_name, b"test-host"
    return r


@pytest.mark.gpu
def test_insert_and_delete(tmp_path):
    csv = tmp_path / "data.csv"
    shutil.copy(CSV2K, csv)
    L = pq.lib()
    eng = pq.HipEngine(csv, pq.DEFAULT_INDEXES)
    chains = [None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("user_id", ">=", "1040")]]
    try:
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        for column in ("exit_code", "user_id", "user_name"):          # caches the i32 ranges
            check_groups(eng, orc, None, column)
        hi_exit = max(int(orc.cell(r, "exit_code")) for r in range(orc.n))
        lo_user = min(int(orc.cell(r, "user_id")) for r in range(orc.n))
        # a new dictionary value, an exit_code above and a user_id below the cached ranges
        assert L.executeQueryInsertHIP(eng.e, b"Commands", C_ref(make_record(900001, hi_exit + 40, lo_user - 25, b"aaa_new_user")))
        assert L.executeQueryInsertHIP(eng.e, b"Commands", C_ref(make_record(900002, hi_exit + 3, lo_user + 1, b"zzz_new_user")))
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)                 # the CSV now holds the two rows at its end
        assert orc.n == eng.e.contents.num_records
        for chain in chains:
            for column in GROUPABLE:
                check_groups(eng, orc, chain, column)
        # DELETE: survivors compared with a fresh oracle over exactly those rows
        lines = csv.read_bytes().split(b"\n")
        body = [ln for ln in lines[1:] if ln.strip()]
        wl = pq.WhereList([("risk_level", ">=", "4"), "OR", ("shell_type", "=", "fish")])
        keep = [i for i in range(orc.n) if not q.load_oracle().orc_eval_where(C_ref(orc.rows[i]), wl.ptr)]
        rs = L.executeQueryDeleteHIP(eng.e, b"Commands", wl.ptr)
        assert rs.contents.success
        L.freeResultSet(rs)
        survivors = tmp_path / "survivors.csv"
        survivors.write_bytes(b"\n".join([lines[0]] + [body[i] for i in keep]) + b"\n")
        orc = q.OracleTable(survivors, pq.DEFAULT_INDEXES)
        assert orc.n == eng.e.contents.num_records == len(keep)
        for chain in chains:
            for column in GROUPABLE:
                check_groups(eng, orc, chain, column)
    finally:
        eng.close()


def C_ref(obj):
    import ctypes
    return ctypes.byref(obj)


@pytest.mark.gpu
def test_refusals(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for column in ("command_id", "no_such_column"):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.group_count(column, None)
            assert time.monotonic() - t0 < 5
        # a thread that holds every lane is refused at once, not left to wait for itself
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(pq.lib().hipEngineLanes(eng.e))]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.group_count("user_name", None)
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        assert eng.group_count("risk_level", [("risk_level", ">", "3")])            # usable again
    finally:
        eng.close()
    # more than 65 536 groups: an exit_code far away from the others
    csv = tmp_path / "wide.csv"
    shutil.copy(CSV2K, csv)
    eng = pq.HipEngine(csv, [])
    try:
        assert pq.lib().executeQueryInsertHIP(eng.e, b"Commands", C_ref(make_record(900003, 1 << 20, 1001, b"student1001")))
        with pytest.raises(pq.PqpsError):
            eng.group_count("exit_code", None)
        assert sum(c for _, c in eng.group_count("user_name", None)) == eng.e.contents.num_records
    finally:
        eng.close()


def test_group_count_is_exported():
    """CPU: the library exports the grouped COUNT and the package wraps it."""
    L = pq.lib()
    for sym in ("executeQueryGroupCountHIP", "freeGroupResultHIP", "pqps_filter_group", "pqps_group_list", "pqps_column_bounds"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "group_count", None))
