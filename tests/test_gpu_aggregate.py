"""COUNT / SUM / MIN / MAX of a value column (executeQueryAggregateHIP / HipEngine.aggregate), overall and per group, over the
rows executeQuerySelectIdsHIP returns.  Every expected answer comes from the oracle -- int(oracle.cell(r, col)) over
oracle.select_ids(chain) for a CSV, numpy over HostSynth + oracle_scan for the synthetic tables, plain numpy over the columns
handed to HipEngine.from_columns -- never from the engine itself.  Covers the fused kernel's three paths (no GROUP BY in
registers, up to 2 304 bins in LDS, up to 65 536 in global memory), the list path (index probes with their duplicates, WHERE
lists of several passes), single-valued group columns, i32 sums past 2^32, signed and unsigned orders, the u64 sum modulo
2^64, shards, INSERT / DELETE and the refusals."""
import collections
import os
import shutil
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

import qpelib as q
import test_gpu_group_count as grp

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
VALUES = ("command_id", "exit_code", "user_id", "risk_level")
GOLDEN_GROUPS = (None, "user_name", "risk_level", "sudo_used", "base_command")
M64 = (1 << 64) - 1


def fold(column, value_column, pairs):
    """[(key_text or None, value), ...] -> the expected aggregate() list, in key order."""
    acc = collections.OrderedDict()
    for key, v in pairs:
        c, s, lo, hi = acc.get(key, (0, 0, None, None))
        acc[key] = (c + 1, s + v, v if lo is None else min(lo, v), v if hi is None else max(hi, v))
    keys = sorted(acc, key=(lambda k: grp.key_order(column, k))) if column else list(acc)
    wrap = (lambda s: s & M64) if value_column == "command_id" else (lambda s: s)
    return [(k, acc[k][0], wrap(acc[k][1]), acc[k][2], acc[k][3]) for k in keys]


def oracle_aggregate(orc, ids, value_column, column):
    return fold(column, value_column, [(orc.cell(r, column) if column else None, int(orc.cell(r, value_column))) for r in ids])


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
            ids = orc.select_ids(chain)[0]
            if indexes == "none":
                assert eng.count(chain or []) == len(ids)
            for column in GOLDEN_GROUPS:
                counts = eng.group_count(column, chain) if column else None
                for value in VALUES:
                    got = eng.aggregate(value, column, chain)
                    assert got == oracle_aggregate(orc, ids, value, column), (indexes, value, column, chain)
                    assert sum(g[1] for g in got) == len(ids)
                    if column:
                        assert [(k, c) for k, c, _, _, _ in got] == counts
    finally:
        eng.close()


def synth_groups(host, ids, column):
    """(row order, group starts, key texts) of the rows `ids` grouped by `column` (None: one group)."""
    if column is None:
        return None, np.zeros(1 if len(ids) else 0, np.int64), [None] * (1 if len(ids) else 0)
    keys = host.arr[column][ids].astype(np.int64)
    order = np.argsort(keys, kind="stable")
    uniq, starts = np.unique(keys[order], return_index=True)
    texts = []
    for k in uniq.tolist():
        if column in host.values:
            texts.append(host.values[column][int(k)].decode("latin-1"))
        elif column == "sudo_used":
            texts.append("true" if k else "false")
        else:
            texts.append(str(int(k)))
    return order, starts, texts


def synth_aggregate(host, ids, value_column, groups):
    order, starts, texts = groups
    if not texts:
        return []
    wide = host.arr[value_column][ids].astype(np.uint64 if value_column == "command_id" else np.int64)
    if order is not None:
        wide = wide[order]
    counts = np.diff(np.append(starts, len(wide)))
    sums, mins, maxs = np.add.reduceat(wide, starts), np.minimum.reduceat(wide, starts), np.maximum.reduceat(wide, starts)
    return [(t, int(c), int(s), int(lo), int(hi)) for t, c, s, lo, hi in zip(texts, counts.tolist(), sums.tolist(), mins.tolist(), maxs.tolist())]


SYNTH_GROUPS = (None, "user_name", "risk_level", "sudo_used", "host_name", "base_command", "user_id", "raw_command")


def check_synthetic(n, chains=grp.SYNTH_CHAINS, groups=SYNTH_GROUPS, values=VALUES, indexes=()):
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n, indexes=indexes)
    try:
        for cname, chain in chains.items():
            ids = host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1))
            assert eng.count(chain or []) == len(ids)
            for column in groups:
                g = synth_groups(host, ids, column)
                for value in values:
                    got = eng.aggregate(value, column, chain)
                    assert got == synth_aggregate(host, ids, value, g), (n, cname, value, column)
                    if cname.endswith("nothing"):
                        assert got == []
            if cname == "probe_ge1":
                assert len(ids) == n
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
    check_synthetic(n, chains=grp.PROBED_CHAINS, indexes=grp.PROBE_INDEXES)


@pytest.mark.gpu
def test_synthetic_large():
    check_synthetic(30_000_007, chains={k: grp.SYNTH_CHAINS[k] for k in ("all", "s1", "risk_gt1")},
                    groups=(None, "user_name", "risk_level", "host_name"), values=("command_id", "risk_level", "exit_code"))


def edge_columns(n, rng, dict_size, **numeric):
    """from_columns input: user_name a dictionary of `dict_size` words with random codes, the rest constant unless given."""
    codes = rng.integers(0, dict_size, size=n).astype(np.uint16 if dict_size > 256 else np.uint8)
    words = [f"w{i:05d}".encode() for i in range(dict_size)]
    cols = {name: (None, [b"x"]) for name in q.ORC_STR + ["shell_type", "base_command"]}
    cols.update(command_id=np.arange(n, dtype=np.uint64), exit_code=np.zeros(n, np.int32), user_id=np.full(n, 1001, np.int32),
                risk_level=rng.integers(1, 6, size=n).astype(np.int32), sudo_used=(rng.random(n) < 0.3).astype(np.uint8),
                user_name=(codes, words))
    cols.update(numeric)
    return cols, codes, words


def numpy_aggregate(vals, keys, words, mask, unsigned):
    wide = vals.astype(np.uint64 if unsigned else np.int64)[mask]
    if keys is None:
        return [] if not mask.any() else [(None, int(mask.sum()), int(wide.sum()), int(wide.min()), int(wide.max()))]
    k = keys[mask]
    order = np.argsort(k, kind="stable")
    k, wide = k[order], wide[order]
    uniq, starts = np.unique(k, return_index=True)
    if len(uniq) == 0:
        return []
    counts = np.diff(np.append(starts, len(k)))
    sums, mins, maxs = np.add.reduceat(wide, starts), np.minimum.reduceat(wide, starts), np.maximum.reduceat(wide, starts)
    return [(words[key], int(c), int(s), int(lo), int(hi))
            for key, c, s, lo, hi in zip(uniq.tolist(), counts.tolist(), sums.tolist(), mins.tolist(), maxs.tolist())]


EDGE_CHAINS = (None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("risk_level", "<", "3")], [("risk_level", ">", "9")])


def edge_masks(cols):
    risk, sudo = cols["risk_level"], cols["sudo_used"]
    return (np.ones(len(risk), bool), risk > 3, (sudo == 1) & (risk < 3), risk > 9)


def check_edge(cols, codes, words, value, unsigned, groups=(None, "user_name"), indexes=()):
    n = len(codes)
    eng = pq.HipEngine.from_columns(n, cols, indexes)
    wtext = [w.decode() for w in words]
    try:
        for chain, mask in zip(EDGE_CHAINS, edge_masks(cols)):
            if indexes:                                         # index probes: the same rows as the mask, each once
                assert sorted(eng.select_ids(chain)) == np.flatnonzero(mask).tolist(), chain
            for column in groups:
                want = numpy_aggregate(cols[value], codes if column else None, wtext, mask, unsigned)
                assert eng.aggregate(value, column, chain) == want, (value, column, chain, indexes)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dict_size", [12, 2000, 40000])
def test_int32_max_sums_past_32_bits(dict_size):
    """exit_code = INT32_MAX on 2^20 + 3 rows: a 32-bit accumulator overflows.  12 words: LDS table; 2000: LDS table at the
    synthetic user_name's size; 40 000: global bins."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(11)
    cols, codes, words = edge_columns(n, rng, dict_size, exit_code=np.full(n, 2**31 - 1, np.int32))
    check_edge(cols, codes, words, "exit_code", False)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        assert eng.aggregate("exit_code") == [(None, n, n * (2**31 - 1), 2**31 - 1, 2**31 - 1)]
        assert eng.average("exit_code") == [(None, 2**31 - 1)]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_signed_min_max(indexes):
    """INT32_MIN and negative values mixed with small positive ones: min / max in signed order."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(12)
    v = rng.integers(-(2**31), 2**31, size=n, dtype=np.int64)
    v[rng.integers(0, n, size=50)] = -(2**31)
    v[::7] = rng.integers(-5, 3, size=len(v[::7]))
    cols, codes, words = edge_columns(n, rng, 2000, exit_code=v.astype(np.int32),
                                      user_id=rng.integers(-(2**31), -1, size=n, dtype=np.int64).astype(np.int32))
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    for value in ("exit_code", "user_id"):
        check_edge(cols, codes, words, value, False, indexes=idx)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_command_id_unsigned(indexes):
    """command_id values at or above 2^63: unsigned min / max, the sum wraps modulo 2^64."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(13)
    ids = rng.integers(0, 2**63, size=n, dtype=np.uint64) | np.uint64(1 << 63)
    ids[::5] = rng.integers(0, 1000, size=len(ids[::5]), dtype=np.uint64)
    ids[3] = np.uint64(M64)
    cols, codes, words = edge_columns(n, rng, 40000, command_id=ids)
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    check_edge(cols, codes, words, "command_id", True, indexes=idx)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        (_, c, s, lo, hi), = eng.aggregate("command_id")
        assert (c, s, lo, hi) == (n, sum(int(x) for x in ids) & M64, int(ids.min()), M64)
        assert s < sum(int(x) for x in ids)                                        # it did wrap
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV, synthetic and edge cases again with the rows split over two shards of one card (a child process: the engine
    reads PQPS_DEVICES when it is created)."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or synthetic_small or synthetic_index_probes or insert_and_delete or int32_max or command_id_unsigned"],
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

    def check_all(orc):
        for chain in chains:
            ids = orc.select_ids(chain)[0]
            for column in (None, "user_name", "exit_code"):
                for value in VALUES:
                    assert eng.aggregate(value, column, chain) == oracle_aggregate(orc, ids, value, column), (value, column, chain)

    try:
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        check_all(orc)                                                  # caches the i32 ranges
        hi_exit = max(int(orc.cell(r, "exit_code")) for r in range(orc.n))
        hi_id = max(int(orc.cell(r, "command_id")) for r in range(orc.n))
        # a new maximum of exit_code and command_id, in a new group
        assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(hi_id + 1000, hi_exit + 40, 1001, b"zzz_agg_user")))
        (_, _, _, _, top_exit), = eng.aggregate("exit_code")
        (_, _, _, _, top_id), = eng.aggregate("command_id")
        assert (top_exit, top_id) == (hi_exit + 40, hi_id + 1000)
        assert ("zzz_agg_user", 1, hi_exit + 40, hi_exit + 40, hi_exit + 40) in eng.aggregate("exit_code", "user_name")
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)                    # the CSV now holds the new row at its end
        assert orc.n == eng.e.contents.num_records
        check_all(orc)
        # DELETE: survivors compared with a fresh oracle over exactly those rows
        lines = csv.read_bytes().split(b"\n")
        body = [ln for ln in lines[1:] if ln.strip()]
        wl = pq.WhereList([("risk_level", ">=", "4"), "OR", ("shell_type", "=", "fish")])
        keep = [i for i in range(orc.n) if not q.load_oracle().orc_eval_where(grp.C_ref(orc.rows[i]), wl.ptr)]
        rs = L.executeQueryDeleteHIP(eng.e, b"Commands", wl.ptr)
        assert rs.contents.success
        L.freeResultSet(rs)
        survivors = tmp_path / "survivors.csv"
        survivors.write_bytes(b"\n".join([lines[0]] + [body[i] for i in keep]) + b"\n")
        orc = q.OracleTable(survivors, pq.DEFAULT_INDEXES)
        assert orc.n == eng.e.contents.num_records == len(keep)
        check_all(orc)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for value, column in (("user_name", None), ("sudo_used", None), ("shell_type", "risk_level"), ("no_such_column", None),
                              ("risk_level", "no_such_column"), ("risk_level", "command_id")):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.aggregate(value, column, None)
            assert time.monotonic() - t0 < 5
        # a thread that holds every lane is refused at once, not left to wait for itself
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(pq.lib().hipEngineLanes(eng.e))]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.aggregate("risk_level", "user_name", None)
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        assert eng.aggregate("risk_level", "user_name", [("risk_level", ">", "3")])      # usable again
    finally:
        eng.close()
    # more than 65 536 groups: an exit_code far away from the others
    csv = tmp_path / "wide.csv"
    shutil.copy(CSV2K, csv)
    eng = pq.HipEngine(csv, [])
    try:
        assert pq.lib().executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900003, 1 << 20, 1001, b"student1001")))
        with pytest.raises(pq.PqpsError):
            eng.aggregate("risk_level", "exit_code", None)
        (_, c, _, _, hi), = eng.aggregate("exit_code")
        assert (c, hi) == (eng.e.contents.num_records, 1 << 20)
    finally:
        eng.close()


RANKS_CODE = textwrap.dedent("""
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
                    eng.aggregate("risk_level", column, None)
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
""")


@pytest.mark.gpu
def test_refused_on_joined_ranks():
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_aggregate_is_exported():
    """CPU: the library exports the aggregates and the package wraps them."""
    L = pq.lib()
    for sym in ("executeQueryAggregateHIP", "freeAggregateResultHIP", "pqps_filter_aggregate", "pqps_aggregate_list"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "aggregate", None))
    fields = [f for f, _ in pq.AggregateResult._fields_]
    assert fields[:5] == ["valueColumn", "valueKind", "groupColumn", "groupKind", "numGroups"]
    assert fields[-2:] == ["queryTime", "success"]
