"""GROUP BY buckets (executeQueryGroupBucketsHIP / HipEngine.group_buckets): COUNT(*) or COUNT / SUM / MIN / MAX per prefix of
a string column or per range of an i32 column, over the rows executeQuerySelectIdsHIP returns.  Every expected answer comes
from the oracle -- Counter(oracle.cell(r, col)[:k]) as bytes and int(cell) // w over oracle.select_ids(chain) for a CSV, numpy
over HostSynth + oracle_scan for the synthetic table, plain numpy over the columns handed to HipEngine.from_columns -- never
from the engine itself.  Covers the fused and the list path (index probes with their duplicates, WHEREs of several passes,
fragmented LIKE / IN sets), a timestamp dictionary of 100 000 values that group_count refuses, the single-valued column,
shards, INSERT / DELETE / UPDATE, the marginal identity against group_count, and the refusals."""
import collections
import csv
import datetime
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
M64 = (1 << 64) - 1
# (column, prefix, width)
GOLDEN_SHAPES = (("timestamp", 7, None), ("timestamp", 10, None), ("timestamp", 13, None), ("working_directory", 6, None),
                 ("user_name", 9, None), ("user_id", None, 1), ("user_id", None, 7), ("user_id", None, 100),
                 ("exit_code", None, 50), ("risk_level", None, 2))
GOLDEN_VALUES = (None, "risk_level", "command_id")


def bucket_of(text, prefix, width):
    """(sort key, key text) of the bucket of a cell"""
    if prefix is not None:
        b = text.encode("latin-1")[:prefix]
        return b, b.decode("latin-1")
    lower = int(text) // width * width
    return lower, str(lower)


def fold(cells, values, prefix, width, value_column):
    """cells (and values, or None) of the selected rows -> the expected group_buckets() list, in key order"""
    acc = {}
    for i, text in enumerate(cells):
        key = bucket_of(text, prefix, width)
        v = values[i] if values is not None else 0
        c, s, lo, hi = acc.get(key, (0, 0, None, None))
        acc[key] = (c + 1, s + v, v if lo is None else min(lo, v), v if hi is None else max(hi, v))
    keys = sorted(acc)
    if values is None:
        return [(k[1], acc[k][0]) for k in keys]
    wrap = (lambda s: s & M64) if value_column == "command_id" else (lambda s: s)
    return [(k[1], acc[k][0], wrap(acc[k][1]), acc[k][2], acc[k][3]) for k in keys]


class Cells:
    """every cell of the columns the shapes use, read from the oracle once"""

    def __init__(self, orc, columns):
        self.text = {c: [orc.cell(r, c) for r in range(orc.n)] for c in columns}

    def expected(self, ids, column, prefix, width, value):
        cells = [self.text[column][r] for r in ids]
        values = [int(self.text[value][r]) for r in ids] if value else None
        return fold(cells, values, prefix, width, value)


SHAPE_COLUMNS = sorted({s[0] for s in GOLDEN_SHAPES} | {v for v in GOLDEN_VALUES if v})


def check_marginals(eng, got, column, prefix, width, chain):
    """adding group_count's counts over the values of a bucket gives the bucket's count"""
    sums = collections.OrderedDict()
    for text, c in eng.group_count(column, chain):
        key = bucket_of(text, prefix, width)[1]
        sums[key] = sums.get(key, 0) + c
    assert [(k, c) for k, c in sums.items()] == [g[:2] for g in got], (column, prefix, width, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    cells = Cells(orc, SHAPE_COLUMNS)
    chains = grp.golden_chains()
    assert len(chains) > 50
    try:
        for n_chain, chain in enumerate(chains + [None]):
            ids = orc.select_ids(chain)[0]
            assert eng.select_ids(chain) == ids
            for column, prefix, width in GOLDEN_SHAPES:
                for value in GOLDEN_VALUES:
                    got = eng.group_buckets(column, prefix=prefix, width=width, value_column=value, chain=chain)
                    assert got == cells.expected(ids, column, prefix, width, value), (indexes, column, prefix, width, value, chain)
                    assert sum(g[1] for g in got) == len(ids)
                if n_chain % 4 == 0 or chain is None:
                    check_marginals(eng, eng.group_buckets(column, prefix=prefix, width=width, chain=chain), column, prefix, width, chain)
            # a prefix longer than every string, and a width of 1, are group_count itself
            for column in ("timestamp", "user_name", "working_directory"):
                assert eng.group_buckets(column, prefix=2000, chain=chain) == eng.group_count(column, chain)
            assert eng.group_buckets("user_id", width=1, chain=chain) == eng.group_count("user_id", chain)
    finally:
        eng.close()


def iso_timestamps(count, days=40):
    """`count` ascending, distinct ISO-8601 strings spread over `days` days"""
    t0 = datetime.datetime(2026, 1, 10, 0, 0, 0)
    step_ms = days * 86400 * 1000 // count
    out = []
    for i in range(count):
        t = t0 + datetime.timedelta(milliseconds=i * step_ms + (i * 7919) % step_ms)
        out.append(t.strftime("%Y-%m-%dT%H:%M:%S.").encode() + b"%03dZ" % (t.microsecond // 1000))
    assert out == sorted(set(out))
    return out


def big_timestamp_columns(n, dict_size, rng):
    stamps = iso_timestamps(dict_size)
    codes = rng.integers(0, dict_size, size=n).astype(np.uint32)
    users = [f"user{i:04d}".encode() for i in range(600)]
    ucodes = rng.integers(0, len(users), size=n).astype(np.uint16)
    cols = {name: (None, [b"x"]) for name in q.ORC_STR + ["shell_type", "base_command"]}
    cols.update(command_id=np.arange(n, dtype=np.uint64) | (np.arange(n, dtype=np.uint64) % np.uint64(5) << np.uint64(61)),
                exit_code=rng.integers(-3, 130, size=n).astype(np.int32), user_id=rng.integers(-100000, 100000, size=n).astype(np.int32),
                risk_level=rng.integers(1, 6, size=n).astype(np.int32), sudo_used=(rng.random(n) < 0.3).astype(np.uint8),
                timestamp=(codes, stamps), user_name=(ucodes, users))
    return cols, stamps, users


def numpy_buckets(bucket_ids, texts, mask, values=None, unsigned=False):
    """per-row bucket ids + the buckets' texts -> the expected list over the rows of `mask`"""
    b = bucket_ids[mask]
    order = np.argsort(b, kind="stable")
    b = b[order]
    uniq, starts = np.unique(b, return_index=True)
    if len(uniq) == 0:
        return []
    counts = np.diff(np.append(starts, len(b)))
    if values is None:
        return [(texts[k], int(c)) for k, c in zip(uniq.tolist(), counts.tolist())]
    wide = values.astype(np.uint64 if unsigned else np.int64)[mask][order]
    sums, mins, maxs = np.add.reduceat(wide, starts), np.minimum.reduceat(wide, starts), np.maximum.reduceat(wide, starts)
    return [(texts[k], int(c), int(s), int(lo), int(hi))
            for k, c, s, lo, hi in zip(uniq.tolist(), counts.tolist(), sums.tolist(), mins.tolist(), maxs.tolist())]


def prefix_ids(dictionary, codes, k):
    """bucket id per row and the buckets' texts for PREFIX(k) over an ascending dictionary"""
    texts = sorted({v[:k] for v in dictionary})
    index = {t: i for i, t in enumerate(texts)}
    per_code = np.array([index[v[:k]] for v in dictionary], dtype=np.int64)
    return per_code[codes], [t.decode("latin-1") for t in texts]


@pytest.mark.gpu
def test_more_than_65536_timestamps():
    """A timestamp dictionary of 100 000 values: group_count refuses it, the day and hour buckets answer; a user_id column that
    spans 200 000 values likewise.  One WHERE takes the fused path; the IN list and the LIKE are fragmented enough for a member
    pass, so the list path runs."""
    n, dict_size = 200_003, 100_000
    rng = np.random.default_rng(65536)
    cols, stamps, users = big_timestamp_columns(n, dict_size, rng)
    codes, ucodes, risk = cols["timestamp"][0], cols["user_name"][0], cols["risk_level"]
    some_users = users[::3]
    hour_like = np.array([v[11:12] == b"1" for v in stamps])              # LIKE '%T1_:%': hours 10 .. 19 of every day
    chains = (
        (None, np.ones(n, bool)),
        ([("risk_level", ">", "3")], risk > 3),
        ([("user_name", "IN", pq.in_list(some_users))], np.isin(ucodes, np.arange(0, len(users), 3))),
        ([("timestamp", "LIKE", "%T1_:%"), "AND", ("risk_level", "<", "3")], hour_like[codes] & (risk < 3)),
        ([("risk_level", ">", "9")], np.zeros(n, bool)),
    )
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        with pytest.raises(pq.PqpsError):
            eng.group_count("timestamp")
        with pytest.raises(pq.PqpsError):
            eng.group_count("user_id")
        with pytest.raises(pq.PqpsError):
            eng.group_buckets("timestamp", prefix=24)                     # 100 000 buckets
        for chain, mask in chains:
            assert eng.count(chain or []) == int(mask.sum())
            for k in (13, 10):
                ids, texts = prefix_ids(stamps, codes, k)
                assert eng.group_buckets("timestamp", prefix=k, chain=chain) == numpy_buckets(ids, texts, mask), (k, chain)
                assert eng.group_buckets("timestamp", prefix=k, value_column="exit_code", chain=chain) == \
                    numpy_buckets(ids, texts, mask, cols["exit_code"]), (k, chain)
            ids, texts = prefix_ids(stamps, codes, 10)
            assert eng.group_buckets("timestamp", prefix=10, value_column="command_id", chain=chain) == \
                numpy_buckets(ids, texts, mask, cols["command_id"], unsigned=True), chain
            lower = cols["user_id"].astype(np.int64) // 1000
            wtexts = {int(v): str(int(v) * 1000) for v in np.unique(lower)}
            assert eng.group_buckets("user_id", width=1000, chain=chain) == numpy_buckets(lower, wtexts, mask), chain
        assert len(eng.group_buckets("timestamp", prefix=13)) > 900
    finally:
        eng.close()


SYNTH_CHAINS = {k: grp.SYNTH_CHAINS[k] for k in ("s1", "risk_gt2", "nothing", "or_tree")}


def check_synthetic_engine(n, chains=SYNTH_CHAINS, indexes=()):
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n, indexes=indexes)
    try:
        for cname, chain in chains.items():
            rows = host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1))
            mask = np.zeros(n, bool)
            mask[rows] = True
            assert eng.count(chain or []) == len(rows)
            uid = host.arr["user_id"].astype(np.int64) // 16
            texts = {int(v): str(int(v) * 16) for v in np.unique(uid)}
            assert eng.group_buckets("user_id", width=16, chain=chain) == numpy_buckets(uid, texts, mask), cname
            assert eng.group_buckets("user_id", width=16, value_column="risk_level", chain=chain) == \
                numpy_buckets(uid, texts, mask, host.arr["risk_level"]), cname
            ids, ptexts = prefix_ids(host.values["user_name"], host.arr["user_name"], 9)
            assert eng.group_buckets("user_name", prefix=9, chain=chain) == numpy_buckets(ids, ptexts, mask), cname
            assert eng.group_buckets("user_name", prefix=9, value_column="command_id", chain=chain) == \
                numpy_buckets(ids, ptexts, mask, host.arr["command_id"], unsigned=True), cname
            # the single-valued column: one bucket from the selection, the ungrouped aggregate with a value
            raw = host.values["raw_command"][0][:3].decode("latin-1")
            assert eng.group_buckets("raw_command", prefix=3, chain=chain) == ([(raw, len(rows))] if len(rows) else []), cname
            risk = host.arr["risk_level"][rows].astype(np.int64)
            want = [(raw, len(rows), int(risk.sum()), int(risk.min()), int(risk.max()))] if len(rows) else []
            assert eng.group_buckets("raw_command", prefix=3, value_column="risk_level", chain=chain) == want, cname
            if cname.endswith("nothing"):
                assert len(rows) == 0
            if cname == "probe_ge1":
                assert len(rows) == n
    finally:
        eng.close()


@pytest.mark.gpu
def test_synthetic_engine():
    check_synthetic_engine((1 << 20) + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1025])
def test_synthetic_engine_small(n):
    """One row: over two shards one of them has no rows at all.  These WHEREs are fused."""
    check_synthetic_engine(n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1025])
def test_synthetic_engine_index_probes(n):
    """WHEREs the risk_level index probes are not fused: the selection's per-shard lists and the list kernels.  Over two
    shards (test_over_shards) the one-row table leaves the second shard without rows."""
    check_synthetic_engine(n, chains=grp.PROBED_CHAINS, indexes=grp.PROBE_INDEXES)


@pytest.mark.gpu
def test_over_shards():
    """The CSV, wide-dictionary, synthetic and writer cases again with the rows split over two shards of one card (a child
    process: the engine reads PQPS_DEVICES when it is created).  The one-row table leaves the second shard empty."""
    env = dict(os.environ, PQPS_DEVICES="0,0")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or more_than_65536 or synthetic_engine or writers"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


WRITER_SHAPES = (("timestamp", 10, None), ("timestamp", 13, None), ("user_name", 9, None), ("user_id", None, 7), ("user_id", None, 100),
                 ("exit_code", None, 50))
WRITER_CHAINS = (None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("user_id", ">=", "1040")],
                 [("timestamp", ">=", "2026-03"), "AND", ("timestamp", "<", "2026-06")])


def check_table(eng, path, step):
    orc = q.OracleTable(path, pq.DEFAULT_INDEXES)
    assert orc.n == eng.e.contents.num_records, step
    cells = Cells(orc, sorted({s[0] for s in WRITER_SHAPES} | {"risk_level"}))
    for chain in WRITER_CHAINS:
        ids = orc.select_ids(chain)[0]
        for column, prefix, width in WRITER_SHAPES:
            for value in (None, "risk_level"):
                got = eng.group_buckets(column, prefix=prefix, width=width, value_column=value, chain=chain)
                assert got == cells.expected(ids, column, prefix, width, value), (step, column, prefix, width, value, chain)
    return orc


@pytest.mark.gpu
def test_writers(tmp_path):
    """INSERT of a new string inside a bucket and of one that opens a new bucket, a DELETE that empties a bucket (the cached
    i32 range stays wider than the data), an UPDATE."""
    path = tmp_path / "data.csv"
    shutil.copy(CSV2K, path)
    L = pq.lib()
    eng = pq.HipEngine(path, pq.DEFAULT_INDEXES)
    try:
        orc = check_table(eng, path, "start")                          # caches the i32 ranges
        stamps = sorted({orc.cell(r, "timestamp") for r in range(orc.n)})
        inside = stamps[len(stamps) // 2][:13] + ":59:59.999Z"          # a new value inside an existing hour
        assert inside not in stamps
        hi_user = max(int(orc.cell(r, "user_id")) for r in range(orc.n))
        for k, (stamp, user_id) in enumerate(((inside, 1001), ("2031-01-01T00:00:00.000Z", hi_user + 500), ("2020-02-02T02:02:02.020Z", 1002))):
            r = grp.make_record(900001 + k, 3, user_id, b"student1001")
            r.timestamp = stamp.encode()
            assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(r))
        hours = dict(eng.group_buckets("timestamp", prefix=13))
        assert hours["2031-01-01T00"] == 1 and hours["2020-02-02T02"] == 1 and hours[inside[:13]] >= 2
        orc = check_table(eng, path, "insert")                         # the CSV now holds the three rows at its end
        # DELETE: the new last hour and the far user_id go (make_record's risk_level is 4); survivors from a fresh oracle
        lines = path.read_bytes().split(b"\n")
        body = [ln for ln in lines[1:] if ln.strip()]
        wl = pq.WhereList([("risk_level", ">=", "4"), "OR", ("shell_type", "=", "fish")])
        keep = [i for i in range(orc.n) if not q.load_oracle().orc_eval_where(grp.C_ref(orc.rows[i]), wl.ptr)]
        rs = L.executeQueryDeleteHIP(eng.e, b"Commands", wl.ptr)
        assert rs.contents.success
        L.freeResultSet(rs)
        survivors = tmp_path / "survivors.csv"
        survivors.write_bytes(b"\n".join([lines[0]] + [body[i] for i in keep]) + b"\n")
        hours = dict(eng.group_buckets("timestamp", prefix=13))
        assert "2031-01-01T00" not in hours and "2020-02-02T02" not in hours
        assert max(int(k) for k, _ in eng.group_buckets("user_id", width=100)) <= hi_user
        check_table(eng, survivors, "delete")
        # UPDATE: every risk_level 1 row moves to one new hour and one user_id
        rows = list(csv.reader(open(survivors, newline="")))
        new_stamp = "2027-05-05T05:05:05.000Z"
        hit = [r for r in rows[1:] if r[11] == "1"]
        assert hit and eng.update({"timestamp": new_stamp, "user_id": 1003}, [("risk_level", "=", "1")]) == len(hit)
        for r in hit:
            r[5], r[8] = new_stamp, "1003"
        mirror = tmp_path / "mirror.csv"
        with open(mirror, "w", newline="") as f:
            csv.writer(f, lineterminator="\n").writerows(rows)
        assert dict(eng.group_buckets("timestamp", prefix=13))["2027-05-05T05"] == len(hit)
        check_table(eng, mirror, "update")
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        refused = (dict(column="timestamp", prefix=0), dict(column="timestamp", prefix=-1), dict(column="user_id", width=0),
                   dict(column="user_id", width=-5), dict(column="user_id", prefix=3), dict(column="sudo_used", prefix=1),
                   dict(column="timestamp", width=10), dict(column="sudo_used", width=1), dict(column="command_id", width=100),
                   dict(column="command_id", prefix=2), dict(column="no_such_column", prefix=2), dict(column="no_such_column", width=2),
                   dict(column="timestamp", prefix=10, value_column="user_name"), dict(column="timestamp", prefix=10, value_column="sudo_used"),
                   dict(column="user_id", width=10, value_column="no_such_column"))
        for kw in refused:
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.group_buckets(**kw)
            assert time.monotonic() - t0 < 5, kw
        for kw in (dict(column="timestamp"), dict(column="timestamp", prefix=3, width=3)):
            with pytest.raises(ValueError):
                eng.group_buckets(**kw)
        # a thread that holds every lane is refused at once, not left to wait for itself
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(pq.lib().hipEngineLanes(eng.e))]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.group_buckets("timestamp", prefix=10)
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        assert eng.group_buckets("timestamp", prefix=10, chain=[("risk_level", ">", "3")])      # usable again
    finally:
        eng.close()
    # more than 65 536 buckets: an exit_code far away from the others -- but a wider bucket takes the column
    path = tmp_path / "wide.csv"
    shutil.copy(CSV2K, path)
    eng = pq.HipEngine(path, [])
    try:
        assert pq.lib().executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900003, 1 << 20, 1001, b"student1001")))
        with pytest.raises(pq.PqpsError):
            eng.group_count("exit_code", None)
        with pytest.raises(pq.PqpsError):
            eng.group_buckets("exit_code", width=1)
        got = eng.group_buckets("exit_code", width=1000)
        assert got[-1] == (str((1 << 20) // 1000 * 1000), 1) and sum(c for _, c in got) == eng.e.contents.num_records
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
            for kw in (dict(column="user_name", prefix=9), dict(column="user_id", width=16, value_column="risk_level")):
                try:
                    eng.group_buckets(**kw)
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


def test_group_buckets_is_exported():
    """CPU: the library exports the bucketed GROUP BY and the package wraps it."""
    L = pq.lib()
    for sym in ("executeQueryGroupBucketsHIP", "freeBucketResultHIP", "hipBucketBounds", "pqps_filter_group_buckets", "pqps_group_buckets_list",
                "pqps_filter_aggregate_buckets", "pqps_aggregate_buckets_list"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "group_buckets", None))
    fields = [f for f, _ in pq.BucketResult._fields_]
    assert fields[:6] == ["groupColumn", "groupKind", "bucketMode", "bucketArg", "valueColumn", "valueKind"]
    assert fields[-2:] == ["queryTime", "success"]
