"""COUNT(DISTINCT value column) (executeQueryCountDistinctHIP / HipEngine.count_distinct), overall and per group, over the
rows executeQuerySelectIdsHIP returns.  Every expected answer comes from the oracle -- the set of oracle.cell(r, col) over
oracle.select_ids(chain) for a CSV, numpy over HostSynth + oracle_scan for the synthetic tables, plain numpy over the
columns handed to HipEngine.from_columns -- never from the engine itself.  Covers the fused kernel's three bitmap forms
(registers, LDS, global memory) and their boundaries, the list path (index probes with their duplicates), the sort path
(command_id, an i32 range over the bitmap cap), single-valued columns, the value column equal to the group column, shards
(whose counts must not be added), INSERT / DELETE and the refusals."""
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
GOLDEN_VALUES = ("command_id", "exit_code", "user_id", "risk_level", "sudo_used", "user_name", "base_command", "timestamp", "shell_type")
GOLDEN_GROUPS = (None, "user_name", "risk_level", "sudo_used", "base_command")


def last_kernel():
    return pq.lib().pqps_last_kernel().decode()


def oracle_distinct(orc, ids, value, column):
    acc = {}
    for r in ids:
        acc.setdefault(orc.cell(r, column) if column else None, set()).add(orc.cell(r, value))
    keys = sorted(acc, key=lambda k: grp.key_order(column, k)) if column else list(acc)
    return [(k, len(acc[k])) for k in keys]


def numpy_distinct(vals, keys, texts):
    """[(texts[key] or None, distinct values), ...] of vals per key (keys None: one group) in key order."""
    if len(vals) == 0:
        return []
    v = vals.astype(np.uint64).astype(np.int64) if vals.dtype == np.uint64 else vals.astype(np.int64)
    if keys is None:
        return [(None, int(len(np.unique(v))))]
    k = keys.astype(np.int64)
    order = np.lexsort((v, k))
    k, v = k[order], v[order]
    new = np.ones(len(k), bool)
    new[1:] = (k[1:] != k[:-1]) | (v[1:] != v[:-1])
    uniq, counts = np.unique(k[new], return_counts=True)
    return [(texts(int(g)), int(c)) for g, c in zip(uniq.tolist(), counts.tolist())]


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    chains = grp.golden_chains()
    assert len(chains) > 50
    kernels = set()
    try:
        for chain in chains + [None]:
            ids = orc.select_ids(chain)[0]
            for column in GOLDEN_GROUPS:
                counts = eng.group_count(column, chain) if column else None
                for value in GOLDEN_VALUES:
                    got, total = eng.count_distinct_total(value, column, chain)
                    kernels.add(last_kernel().split("<")[0])
                    assert got == oracle_distinct(orc, ids, value, column), (indexes, value, column, chain)
                    assert total == len(ids), (indexes, value, column, chain)
                    if column:
                        assert [k for k, _ in got] == [k for k, _ in counts]
                    assert all(d >= 1 for _, d in got)
        assert {"dist_unique_kernel", "dist_scan_kernel" if indexes == "none" else "dist_list_kernel"} <= kernels, kernels
    finally:
        eng.close()


def synth_text(host, column):
    if column in host.values:
        return lambda k: host.values[column][k].decode("latin-1")
    if column == "sudo_used":
        return lambda k: "true" if k else "false"
    return str


SYNTH_VALUES = ("user_name", "host_name", "base_command", "risk_level", "sudo_used", "exit_code", "command_id", "raw_command")
SYNTH_GROUPS = (None, "user_name", "risk_level", "sudo_used", "host_name")


def check_synthetic(n, chains=grp.SYNTH_CHAINS, groups=SYNTH_GROUPS, values=SYNTH_VALUES):
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    try:
        for cname, chain in chains.items():
            ids = host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1))
            assert eng.count(chain or []) == len(ids)
            for column in groups:
                keys = host.arr[column][ids] if column else None
                for value in values:
                    got, total = eng.count_distinct_total(value, column, chain)
                    assert got == numpy_distinct(host.arr[value][ids], keys, synth_text(host, column)), (n, cname, value, column)
                    assert total == len(ids)
                    if cname == "nothing":
                        assert got == []
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1025, 65537])
def test_synthetic_small(n):
    check_synthetic(n)


@pytest.mark.gpu
def test_synthetic_large():
    check_synthetic(30_000_007, chains={k: grp.SYNTH_CHAINS[k] for k in ("all", "s1", "risk_gt1", "nothing")},
                    groups=(None, "user_name", "host_name"), values=("user_name", "host_name", "base_command", "command_id"))


@pytest.mark.gpu
def test_paths_on_the_synthetic_table():
    """Which kernel each bench shape runs, and that its answer is numpy's."""
    n = 1 << 20
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    cases = [  # WHERE, value, group, kernel
        (grp.S1, "user_name", None, "dist_scan_kernel<DIST_LDS, GROUPED=false"),
        ([("risk_level", ">", "1")], "host_name", None, "dist_scan_kernel<DIST_REG, GROUPED=false"),
        ([("risk_level", ">", "1")], "risk_level", "sudo_used", "dist_scan_kernel<DIST_REG, GROUPED=true"),
        (None, "user_name", "host_name", "dist_scan_kernel<DIST_LDS, GROUPED=true"),
        ([("risk_level", ">", "1")], "base_command", "user_name", "dist_scan_kernel<DIST_LDS, GROUPED=true"),
        (grp.S1, "command_id", None, "dist_unique_kernel<wide> (sort)"),
        ([("risk_level", ">", "1")], "command_id", "host_name", "dist_unique_kernel<wide> (sort)"),
        ([("risk_level", ">", "1")], "raw_command", "host_name", ""),            # single-valued: no kernel of its own
    ]
    try:
        for chain, value, column, kernel in cases:
            ids = host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1))
            got = eng.count_distinct(value, column, chain)
            if kernel:
                assert last_kernel().startswith(kernel), (value, column, last_kernel())
            keys = host.arr[column][ids] if column else None
            assert got == numpy_distinct(host.arr[value][ids], keys, synth_text(host, column)), (value, column)
    finally:
        eng.close()


def dict_columns(n, rng, dict_size, **extra):
    """from_columns input: user_name a dictionary of `dict_size` words with random codes (every word used once at least
    where n allows), the other string columns single-valued, exit_code 0 .. 19, risk_level 1 .. 5."""
    codes = rng.integers(0, dict_size, size=n)
    codes[: min(n, dict_size)] = np.arange(min(n, dict_size))
    codes = codes.astype(np.uint8 if dict_size <= 256 else np.uint16 if dict_size <= 65536 else np.uint32)
    words = [f"w{i:06d}".encode() for i in range(dict_size)]
    cols = {name: (None, [b"x"]) for name in q.ORC_STR + ["shell_type", "base_command"]}
    cols.update(command_id=np.arange(n, dtype=np.uint64), exit_code=rng.integers(0, 20, size=n).astype(np.int32),
                user_id=np.full(n, 1001, np.int32), risk_level=rng.integers(1, 6, size=n).astype(np.int32),
                sudo_used=(rng.random(n) < 0.3).astype(np.uint8), user_name=(codes, words))
    cols.update(extra)
    return cols


EDGE_CHAINS = (None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("risk_level", "<", "3")], [("risk_level", ">", "9")])


def edge_mask(cols, chain):
    risk, sudo = cols["risk_level"], cols["sudo_used"]
    return {0: np.ones(len(risk), bool), 1: risk > 3, 2: (sudo == 1) & (risk < 3), 3: risk > 9}[EDGE_CHAINS.index(chain)]


def column_values(cols, name):
    v = cols[name]
    return v[0] if isinstance(v, tuple) else v


def column_text(cols, name):
    v = cols[name]
    if isinstance(v, tuple):
        return lambda k: v[1][k].decode()
    if name == "sudo_used":
        return lambda k: "true" if k else "false"
    return str


def check_edge(eng, cols, value, column, kernel=None, chains=EDGE_CHAINS):
    for chain in chains:
        mask = edge_mask(cols, chain)
        keys = column_values(cols, column)[mask] if column else None
        want = numpy_distinct(column_values(cols, value)[mask], keys, column_text(cols, column) if column else None)
        got, total = eng.count_distinct_total(value, column, chain)
        assert got == want, (value, column, chain)
        assert total == int(mask.sum())
        if kernel and mask.any():
            assert kernel in last_kernel(), (value, column, chain, last_kernel())


@pytest.mark.gpu
@pytest.mark.parametrize("dict_size", [31, 32, 33, 64, 65])
def test_register_boundaries(dict_size):
    """Dv around one and two words: up to 64 bits of G x Dv in registers, the LDS bitmap above; grouped by sudo_used
    (G = 2) and risk_level (G = 5), and the value column grouped by itself (every group gives 1)."""
    n = (1 << 16) + 5
    cols = dict_columns(n, np.random.default_rng(dict_size), dict_size)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_edge(eng, cols, "user_name", None, "DIST_REG" if dict_size <= 64 else "DIST_LDS")
        check_edge(eng, cols, "user_name", "sudo_used", "DIST_REG" if 2 * dict_size <= 64 else "DIST_LDS")
        check_edge(eng, cols, "user_name", "risk_level", "DIST_REG" if 5 * dict_size <= 64 else "DIST_LDS")
        check_edge(eng, cols, "user_name", "user_name", "DIST_LDS" if dict_size * ((dict_size + 31) // 32) <= 16384 else "DIST_GLOBAL")
        got = eng.count_distinct("user_name", "user_name")
        assert [d for _, d in got] == [1] * dict_size
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dict_size,groups,form", [(32768, 16, "DIST_LDS"), (32769, 16, "DIST_GLOBAL"), (32768, 17, "DIST_GLOBAL"),
                                                   (40000, 20, "DIST_GLOBAL")])
def test_lds_global_boundary(dict_size, groups, form):
    """16 384 words (64 KiB) is the last LDS bitmap: Dv = 32 768 x 16 groups; one more value or one more group is global."""
    n = (1 << 18) + 7
    rng = np.random.default_rng(dict_size + groups)
    cols = dict_columns(n, rng, dict_size, exit_code=rng.integers(0, groups, size=n).astype(np.int32))
    cols["exit_code"][:groups] = np.arange(groups)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        check_edge(eng, cols, "user_name", "exit_code", form)
        check_edge(eng, cols, "user_name", None, "DIST_LDS")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_sort_path_over_the_cap(indexes):
    """exit_code holding -2^31 and 2^31 - 1: a range of 2^32 values, over the bitmap cap -- the narrow sort; command_id
    the wide sort.  With indexes the probes' lists feed the same sorts."""
    n = (1 << 18) + 3
    rng = np.random.default_rng(5)
    ex = rng.integers(-(2**31), 2**31, size=n, dtype=np.int64)
    ex[::3] = rng.integers(-5, 5, size=len(ex[::3]))
    ex[0], ex[1] = -(2**31), 2**31 - 1
    cid = rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    cid[::4] = cid[1::4]                                                   # duplicates
    cid[2] = np.uint64(2**64 - 1)
    cols = dict_columns(n, rng, 2000, exit_code=ex.astype(np.int32), command_id=cid)
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine.from_columns(n, cols, idx)
    try:
        for column in (None, "user_name", "risk_level", "sudo_used"):
            check_edge(eng, cols, "exit_code", column, "dist_unique_kernel<narrow>")
            check_edge(eng, cols, "command_id", column, "dist_unique_kernel<wide>")
    finally:
        eng.close()


@pytest.mark.gpu
def test_list_path_with_duplicates():
    """Index probes whose lists repeat a row: the duplicates count in the total, not in the distinct counts."""
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    orc = q.OracleTable(CSV2K, pq.DEFAULT_INDEXES)
    try:
        seen = False
        for chain in grp.golden_chains():
            ids = orc.select_ids(chain)[0]
            if len(ids) == len(set(ids)):
                continue
            seen = True
            for value, column in (("user_name", None), ("risk_level", "sudo_used"), ("base_command", "user_name")):
                got, total = eng.count_distinct_total(value, column, chain)
                assert "dist_list_kernel" in last_kernel()
                assert got == oracle_distinct(orc, ids, value, column)
                assert total == len(ids) > len(set(ids))
        assert seen, "no golden chain repeats a row in index mode"
    finally:
        eng.close()


@pytest.mark.gpu
def test_shards_merge_sets_not_counts():
    """Values present in every shard: the per-shard distinct counts add up to more than the table's.  With one shard the
    answer is checked all the same; test_over_shards runs this with two."""
    n = (1 << 18) + 9
    rng = np.random.default_rng(21)
    cols = dict_columns(n, rng, 300)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        rows = eng.shards()
        bounds = np.cumsum([0] + rows)
        for value, column, chain in (("user_name", None, None), ("risk_level", None, None), ("user_name", "risk_level", EDGE_CHAINS[1]),
                                     ("exit_code", "sudo_used", None), ("command_id", None, EDGE_CHAINS[2]), ("user_name", "exit_code", None)):
            mask = edge_mask(cols, chain)
            vals = column_values(cols, value)
            keys = column_values(cols, column) if column else None
            want = numpy_distinct(vals[mask], None if keys is None else keys[mask], column_text(cols, column) if column else None)
            assert eng.count_distinct(value, column, chain) == want, (value, column, chain)
            if len(rows) > 1 and value != "command_id":
                per_shard = [numpy_distinct(vals[lo:hi][mask[lo:hi]], None if keys is None else keys[lo:hi][mask[lo:hi]],
                                            column_text(cols, column) if column else None) for lo, hi in zip(bounds[:-1], bounds[1:])]
                assert all(per_shard)                                         # values in every shard
                assert sum(d for p in per_shard for _, d in p) > sum(d for _, d in want)
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV, synthetic, edge and INSERT / DELETE cases again with the rows split over two shards of one card (a child
    process: the engine reads PQPS_DEVICES when it is created)."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "--tb=short", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or synthetic_small or insert_and_delete or shards_merge or sort_path or boundaries or list_path"],
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
            for column in (None, "user_name", "risk_level"):
                for value in ("user_name", "exit_code", "user_id", "command_id", "host_name"):
                    assert eng.count_distinct(value, column, chain) == oracle_distinct(orc, ids, value, column), (value, column, chain)

    try:
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        check_all(orc)                                                  # caches the i32 ranges
        (_, users), = eng.count_distinct("user_name")
        (_, exits), = eng.count_distinct("exit_code")
        hi_exit = max(int(orc.cell(r, "exit_code")) for r in range(orc.n))
        lo_user = min(int(orc.cell(r, "user_id")) for r in range(orc.n))
        existing = orc.cell(0, "user_name").encode()
        # a new user_name adds one; an existing one adds nothing; exit_code and user_id past the cached ranges
        assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900001, hi_exit + 40, lo_user - 25, b"zzz_distinct_user")))
        assert eng.count_distinct("user_name") == [(None, users + 1)]
        assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900002, hi_exit + 40, lo_user - 25, existing)))
        assert eng.count_distinct("user_name") == [(None, users + 1)]
        assert eng.count_distinct("exit_code") == [(None, exits + 1)]
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)                    # the CSV now holds the new rows at its end
        assert orc.n == eng.e.contents.num_records
        check_all(orc)
        # DELETE (the new rows among others, risk_level 4): the new user's only row goes, and with it one distinct value;
        # the survivors compared with a fresh oracle over exactly those rows
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
        left = {orc.cell(r, "user_name") for r in range(orc.n)}
        assert "zzz_distinct_user" not in left
        assert eng.count_distinct("user_name") == [(None, len(left))]
        assert "zzz_distinct_user" not in [k for k, _ in eng.count_distinct("user_id", "user_name")]
        check_all(orc)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for value, column in (("no_such_column", None), ("user_name", "no_such_column"), ("user_name", "command_id")):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.count_distinct(value, column, None)
            assert time.monotonic() - t0 < 5
        # a thread that holds every lane is refused at once, not left to wait for itself
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(pq.lib().hipEngineLanes(eng.e))]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.count_distinct("user_name", "host_name", None)
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        assert eng.count_distinct("user_name", "host_name", [("risk_level", ">", "3")])      # usable again
    finally:
        eng.close()
    # more than 65 536 groups refused; the same column as a value is not refused (its domain is only large)
    csv = tmp_path / "wide.csv"
    shutil.copy(CSV2K, csv)
    eng = pq.HipEngine(csv, [])
    try:
        orc = q.OracleTable(csv, [])
        exits = len({orc.cell(r, "exit_code") for r in range(orc.n)})
        assert pq.lib().executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900003, 1 << 20, 1001, b"student1001")))
        with pytest.raises(pq.PqpsError):
            eng.count_distinct("risk_level", "exit_code", None)
        assert eng.count_distinct("exit_code") == [(None, exits + 1)]
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
                    eng.count_distinct("host_name", column, None)
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


def test_count_distinct_is_exported():
    """CPU: the library exports COUNT(DISTINCT) and its device entry points, and the package wraps them."""
    L = pq.lib()
    for sym in ("executeQueryCountDistinctHIP", "freeDistinctResultHIP", "pqps_filter_distinct", "pqps_distinct_list",
                "pqps_distinct_count", "pqps_distinct_sort", "pqps_distinct_bitmap_words"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "count_distinct", None))
    fields = [f for f, _ in pq.DistinctResult._fields_]
    assert fields[:5] == ["valueColumn", "valueKind", "groupColumn", "groupKind", "numGroups"]
    assert fields[5:8] == ["total", "keys", "keyText"] and fields[8] == "distinct"
    assert fields[-2:] == ["queryTime", "success"]
    assert L.pqps_distinct_bitmap_words(33, 16) == 32 and L.pqps_distinct_bitmap_words(32768, 16) == 16384
