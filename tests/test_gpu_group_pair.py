"""GROUP BY two columns (executeQueryGroupPairHIP / HipEngine.group_pair): COUNT(*), or COUNT / SUM / MIN / MAX of a numeric
column, per pair of values over the rows executeQuerySelectIdsHIP returns.  Every expected answer comes from the oracle (a
dict fold over oracle.select_ids and oracle.cell for a CSV) or from numpy over host copies of the columns
(test_group_pair_reference.numpy_group_pair, itself checked without a GPU) -- never from the engine; the marginal checks
against group_count / aggregate are extra.  All comparisons are exact.  Covers the dense fused kernel (LDS and global bins,
with and without a value), the dense list path (index probes with their duplicates, WHERE lists of several passes), the
sort path (D > 65 536, the 2^32 product included), single-valued columns, both sides of every path switch, shards, INSERT /
DELETE, the refusals and the lane rules."""
import functools
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import qpelib as q
import test_gpu_aggregate as agg
import test_gpu_group_count as grp
import test_group_pair_reference as ref

pq = q.pq
CSV2K = q.GOLDEN / "commands_2k.csv"
M64 = (1 << 64) - 1
NUMERIC = ("command_id", "exit_code", "user_id", "risk_level")
GOLDEN_PAIRS = (("user_name", "risk_level"), ("sudo_used", "base_command"), ("risk_level", "risk_level"), ("base_command", "user_name"))
# which path each synthetic pair takes (D = bins of A x bins of B; user_id = 1000 + the user's code: 2000 values)
SYNTH_PAIRS = (("host_name", "shell_type"),     # 16 x 4: LDS for both forms
               ("user_name", "sudo_used"),      # 4 000: LDS count, global atomics with a value
               ("user_name", "host_name"),      # 32 000: global count
               ("user_name", "base_command"),   # 222 000: sort
               ("user_name", "user_id"),        # 4 000 000: sort, only diagonal pairs occur
               ("raw_command", "user_name"),    # a single-valued column: the one-column form on user_name
               ("raw_command", "timestamp"))    # both single-valued: one group
SYNTH_VALUES = (None, "exit_code", "command_id")


def marginal(pairs):
    """group_pair() rows summed over B: the aggregate() / group_count() rows of A."""
    out = []
    for (ta, _), c, *rest in pairs:
        if out and out[-1][0] == ta:
            o = out[-1]
            out[-1] = (ta, o[1] + c) + ((o[2] + rest[0], min(o[3], rest[1]), max(o[4], rest[2])) if rest else ())
        else:
            out.append((ta, c) + tuple(rest))
    return out


def wrap_sums(rows, value):
    return [(k, c, s & M64, lo, hi) for k, c, s, lo, hi in rows] if value == "command_id" else rows


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_golden_csv_every_chain(indexes):
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    eng = pq.HipEngine(CSV2K, idx)
    orc = q.OracleTable(CSV2K, idx)
    cells = ref.CsvCells(orc, sorted({c for p in GOLDEN_PAIRS for c in p} | set(NUMERIC)))
    chains = grp.golden_chains()
    assert len(chains) > 50
    duplicates = False
    try:
        for chain in chains + [None]:
            ids = orc.select_ids(chain)[0]
            duplicates |= len(set(ids)) < len(ids)
            for pair in GOLDEN_PAIRS:
                counts = eng.group_count(pair[0], chain)
                for value in (None,) + NUMERIC:
                    got, total, _ = eng.group_pair_total(pair, value, chain)
                    assert got == cells.fold(ids, pair, value), (indexes, pair, value, chain)
                    assert total == len(ids) == sum(g[1] for g in got)
                    if value is None:
                        assert marginal(got) == counts, (indexes, pair, chain)
                    else:
                        assert wrap_sums(marginal(got), value) == eng.aggregate(value, pair[0], chain), (indexes, pair, value, chain)
        assert duplicates == (indexes == "default"), "index mode must return some row more than once"
    finally:
        eng.close()


SYNTH_CHAINS = {**grp.SYNTH_CHAINS, **grp.PROBED_CHAINS}


@functools.lru_cache(maxsize=2)
def synth_host(n):
    return q.HostSynth(n, full=True)


@functools.lru_cache(maxsize=8)
def synth_ids(n, cname):
    return synth_host(n).oracle_scan(SYNTH_CHAINS[cname] or [], nthreads=min(16, os.cpu_count() or 1))


def synth_expected(host, ids, pair, value):
    a, b = pair
    return ref.numpy_group_pair(host.arr[a][ids], host.arr[b][ids], ref.key_text(a, host.values.get(a)), ref.key_text(b, host.values.get(b)),
                                host.arr[value][ids] if value else None, value == "command_id")


def check_synthetic(n, pair, chains=tuple(grp.SYNTH_CHAINS), values=SYNTH_VALUES, indexes=()):
    host = synth_host(n)
    eng = pq.HipEngine.synthetic(n, indexes=indexes)
    try:
        for cname in chains:
            ids = synth_ids(n, cname)
            for value in values:
                got, total, _ = eng.group_pair_total(pair, value, SYNTH_CHAINS[cname])
                assert got == synth_expected(host, ids, pair, value), (n, cname, pair, value)
                assert total == len(ids)
                if cname.endswith("nothing"):
                    assert got == []
                if cname == "probe_ge1":
                    assert total == n
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SYNTH_PAIRS, ids=["x".join(p) for p in SYNTH_PAIRS])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 65537, (1 << 20) + 3])
def test_synthetic_small(n, pair):
    check_synthetic(n, pair)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SYNTH_PAIRS[:4] + SYNTH_PAIRS[5:6], ids=["x".join(p) for p in SYNTH_PAIRS[:4] + SYNTH_PAIRS[5:6]])
@pytest.mark.parametrize("n", [1, 1025])
def test_synthetic_index_probes(n, pair):
    """WHEREs the risk_level index probes are not fused: the selection's per-shard lists and the list kernels.  Over two
    shards (test_over_shards) the one-row table leaves the second shard without rows.  The pairs: the dense forms,
    one sort and the one-column form of a single-valued column."""
    check_synthetic(n, pair, chains=tuple(grp.PROBED_CHAINS), indexes=grp.PROBE_INDEXES)


LARGE_PAIRS = (("host_name", "shell_type"), ("user_name", "sudo_used"), ("user_name", "host_name"), ("user_name", "base_command"))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", LARGE_PAIRS, ids=["x".join(p) for p in LARGE_PAIRS])
def test_synthetic_large(pair):
    """30 000 007 rows: every wave of the persistent grid loops.  LDS, LDS count / global with a value, global count, sort."""
    check_synthetic(30_000_007, pair, chains=("all", "s1", "risk_gt1"), values=(None, "exit_code"))


def pair_columns(n, rng, size_a, size_b, occupied=None, **numeric):
    """from_columns input: user_name a dictionary of `size_a` words and host_name one of `size_b`, random codes with both
    ends of both present; `occupied`: only about that many different pairs.  -> (columns, codes of A, codes of B, words of A,
    words of B)."""
    def codes(size):
        c = rng.integers(0, size, size=n)
        c[0], c[n - 1] = 0, size - 1
        return c
    ca = codes(size_a)
    cb = codes(size_b)[::-1].copy()
    if occupied:
        pick = rng.integers(0, occupied, size=n)
        pa, pb = rng.integers(0, size_a, size=occupied), rng.integers(0, size_b, size=occupied)
        ca[1:n - 1], cb[1:n - 1] = pa[pick][1:n - 1], pb[pick][1:n - 1]
    cols, _, _ = agg.edge_columns(n, rng, 12, **numeric)
    wa = [f"a{i:05d}".encode() for i in range(size_a)]
    cols["user_name"] = (ca.astype(np.uint16 if size_a > 256 else np.uint8), wa)
    wb = [f"b{i:05d}".encode() for i in range(size_b)]
    cols["host_name"] = (cb.astype(np.uint16 if size_b > 256 else np.uint8), wb)
    return cols, ca, cb, wa, wb


def check_pair_edge(cols, ca, cb, wa, wb, values, indexes=(), swap=False):
    n = len(ca)
    pair, keys, texts = ("user_name", "host_name"), (ca, cb), (ref.key_text(None, wa), ref.key_text(None, wb))
    if swap:
        pair, keys, texts = pair[::-1], keys[::-1], texts[::-1]
    eng = pq.HipEngine.from_columns(n, cols, indexes)
    try:
        for chain, mask in zip(agg.EDGE_CHAINS, agg.edge_masks(cols)):
            rows = np.flatnonzero(mask)
            if indexes:                                          # index probes: the same rows as the mask, each once
                assert sorted(eng.select_ids(chain)) == rows.tolist(), chain
            for value in values:
                want = ref.numpy_group_pair(keys[0][rows], keys[1][rows], texts[0], texts[1], cols[value][rows] if value else None,
                                            value == "command_id")
                got, total, _ = eng.group_pair_total(pair, value, chain)
                assert got == want, (pair, value, chain, indexes)
                assert total == len(rows)
    finally:
        eng.close()


# D on both sides of every path switch: the count's LDS histogram (16 384), the value table (2 304), the dense cap (65 536;
# 65 537 is prime and no column may span more than 65 536 values, so the first product beyond the cap used here is 65 538).
PATH_EDGES = {"16384": (128, 128), "16385": (3277, 5), "2304": (48, 48), "2305": (461, 5), "65536": (256, 256), "65535": (257, 255),
              "65535b": (4369, 15), "65538": (21846, 3), "65792": (257, 256)}


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
@pytest.mark.parametrize("edge", list(PATH_EDGES))
def test_path_edges(edge, indexes):
    n = 70_001
    size_a, size_b = PATH_EDGES[edge]
    rng = np.random.default_rng([21, size_a, size_b])
    cols, ca, cb, wa, wb = pair_columns(n, rng, size_a, size_b, exit_code=rng.integers(-1000, 1000, size=n).astype(np.int32))
    idx = [] if indexes == "none" else pq.DEFAULT_INDEXES
    check_pair_edge(cols, ca, cb, wa, wb, (None, "risk_level", "command_id"), indexes=idx, swap=edge in ("2305", "65535"))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(2000, 2000), (200, 200)], ids=["sort", "dense"])
def test_few_hundred_pairs_occur(sizes):
    n = 70_001
    rng = np.random.default_rng(22)
    cols, ca, cb, wa, wb = pair_columns(n, rng, sizes[0], sizes[1], occupied=300)
    assert 200 < len(set(zip(ca.tolist(), cb.tolist()))) <= 304
    check_pair_edge(cols, ca, cb, wa, wb, (None, "risk_level"))


@pytest.mark.gpu
@pytest.mark.parametrize("indexes", ["none", "default"])
def test_product_of_two_full_ranges(indexes):
    """exit_code over [-32 768, 32 767] x user_id over [0, 65 535]: D = 2^32, which a 32-bit product would read as 0."""
    n = 5000
    rng = np.random.default_rng(23)
    pool_a, pool_b = rng.integers(-32768, 32768, size=3000), rng.integers(0, 65536, size=3000)
    pick = np.concatenate([np.arange(3000), rng.integers(0, 3000, size=n - 3000)])     # every pair of the pool occurs
    a, b = pool_a[pick], pool_b[pick]
    a[:8] = [-32768, -32768, 32767, 32767, -32768, 32767, -32768, 32767]
    b[:8] = [0, 65535, 0, 65535, 0, 65535, 65535, 0]
    assert 2900 < len(set(zip(a.tolist(), b.tolist()))) <= 3008
    cols, _, _ = agg.edge_columns(n, rng, 12, exit_code=a.astype(np.int32), user_id=b.astype(np.int32))
    eng = pq.HipEngine.from_columns(n, cols, [] if indexes == "none" else pq.DEFAULT_INDEXES)
    try:
        for chain, mask in zip(agg.EDGE_CHAINS, agg.edge_masks(cols)):
            rows = np.flatnonzero(mask)
            for pair, keys in ((("exit_code", "user_id"), (a, b)), (("user_id", "exit_code"), (b, a))):
                for value in (None, "risk_level", "command_id"):
                    want = ref.numpy_group_pair(keys[0][rows], keys[1][rows], str, str, cols[value][rows] if value else None, value == "command_id")
                    assert eng.group_pair(pair, value, chain) == want, (pair, value, chain)
        corners = {k for k, _ in eng.group_pair(("exit_code", "user_id"))}
        assert {("-32768", "0"), ("-32768", "65535"), ("32767", "0"), ("32767", "65535")} <= corners
    finally:
        eng.close()


@pytest.mark.gpu
def test_refusals(tmp_path):
    eng = pq.HipEngine(CSV2K, pq.DEFAULT_INDEXES)
    try:
        for pair, value in ((("command_id", "user_name"), None), (("user_name", "command_id"), None), (("no_such_column", "user_name"), None),
                            (("user_name", "no_such_column"), None), (("user_name", "risk_level"), "no_such_column"),
                            (("user_name", "risk_level"), "shell_type"), (("user_name", "risk_level"), "sudo_used")):
            t0 = time.monotonic()
            with pytest.raises(pq.PqpsError):
                eng.group_pair(pair, value, None)
            assert time.monotonic() - t0 < 5
        # a thread that holds every lane is refused at once, not left to wait for itself
        lanes = pq.lib().hipEngineLanes(eng.e)
        tickets = [eng.select_async([("risk_level", ">", "3")]) for _ in range(lanes)]
        assert all(tickets)
        t0 = time.monotonic()
        with pytest.raises(pq.PqpsError):
            eng.group_pair(("user_name", "risk_level"), None, None)
        assert time.monotonic() - t0 < 5
        for tk in tickets:
            eng.release_ticket(tk)
        # a two-column query gives its lane back: more queries in a row than there are lanes, on every path
        for i in range(lanes + 1):
            assert eng.group_pair(("user_name", "risk_level"), "exit_code" if i % 2 else None, [("risk_level", ">", "3")])
            assert eng.group_pair(("user_name", "base_command"), None, [("risk_level", ">", "3")])
    finally:
        eng.close()
    # an i32 group column spanning 65 537 values is refused as A and as B; the engine stays usable
    n = 70_001
    rng = np.random.default_rng(24)
    wide = rng.integers(0, 65537, size=n)
    wide[0], wide[1] = 0, 65536
    cols, codes, words = agg.edge_columns(n, rng, 12, exit_code=wide.astype(np.int32))
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        for pair in (("exit_code", "user_name"), ("user_name", "exit_code"), ("exit_code", "exit_code")):
            with pytest.raises(pq.PqpsError):
                eng.group_pair(pair, None, None)
        want = ref.numpy_group_pair(codes, cols["risk_level"], ref.key_text(None, words), str, wide, False)
        assert eng.group_pair(("user_name", "risk_level"), "exit_code") == want
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(12, 5), (300, 300)], ids=["dense", "sort"])
def test_sums_past_32_bits_and_modulo_2_64(sizes):
    """exit_code = INT32_MAX: an i32 sum within one pair passes 2^32.  command_id at or above 2^63: the sum of a pair wraps
    modulo 2^64, min / max compare unsigned."""
    n = 70_001
    rng = np.random.default_rng(25)
    ids = rng.integers(0, 2**63, size=n, dtype=np.uint64) | np.uint64(1 << 63)
    ids[::5] = rng.integers(0, 1000, size=len(ids[::5]), dtype=np.uint64)
    ids[3] = np.uint64(M64)
    cols, ca, cb, wa, wb = pair_columns(n, rng, sizes[0], sizes[1], occupied=40, exit_code=np.full(n, 2**31 - 1, np.int32), command_id=ids)
    check_pair_edge(cols, ca, cb, wa, wb, ("exit_code", "command_id"))
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        rows = eng.group_pair(("user_name", "host_name"), "exit_code")
        assert max(s for _, _, s, _, _ in rows) > 1 << 32
        assert all(s == c * (2**31 - 1) for _, c, s, _, _ in rows)
        big = [int(x) for x in ids]
        assert sum(s for _, _, s, _, _ in eng.group_pair(("user_name", "host_name"), "command_id")) & M64 == sum(big) & M64 != sum(big)
    finally:
        eng.close()


@pytest.mark.gpu
def test_insert_and_delete(tmp_path):
    csv = tmp_path / "data.csv"
    shutil.copy(CSV2K, csv)
    L = pq.lib()
    eng = pq.HipEngine(csv, pq.DEFAULT_INDEXES)
    chains = [None, [("risk_level", ">", "3")], [("sudo_used", "=", "TRUE"), "AND", ("user_id", ">=", "1040")]]
    pairs = (("user_name", "risk_level"), ("user_name", "raw_command"))   # dense, and a product over the cap: sort
    columns = sorted({c for p in pairs for c in p} | {"command_id", "exit_code"})

    def check_all(orc, deleted=False):
        cells = ref.CsvCells(orc, columns)
        sizes = {c: len(cells.words[c]) for c in columns}
        # (the engine's dictionaries keep the words of deleted rows, so the second pair stays on the sort path after DELETE)
        assert sizes["user_name"] * 16 <= 65536 and (deleted or 65536 < sizes["user_name"] * sizes["raw_command"])
        for chain in chains:
            ids = orc.select_ids(chain)[0]
            for pair in pairs:
                for value in (None, "exit_code", "command_id"):
                    assert eng.group_pair(pair, value, chain) == cells.fold(ids, pair, value), (pair, value, chain)

    try:
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        check_all(orc)                                                  # caches the i32 ranges
        users = sorted({orc.cell(r, "user_name") for r in range(orc.n)}, key=lambda t: t.encode("latin-1"))
        between = (users[len(users) // 2] + "_x").encode("latin-1")     # a new name between two existing ones: codes are bumped
        assert users[len(users) // 2].encode("latin-1") < between < users[len(users) // 2 + 1].encode("latin-1")
        assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(grp.make_record(900001, 3, 1001, between)))
        r = grp.make_record(900002, 5, 1002, b"student1002")
        r.risk_level = 9                                                # widens the range of risk_level
        assert L.executeQueryInsertHIP(eng.e, b"Commands", grp.C_ref(r))
        orc = q.OracleTable(csv, pq.DEFAULT_INDEXES)
        assert orc.n == eng.e.contents.num_records
        check_all(orc)
        assert ((between.decode("latin-1"), "4"), 1) in eng.group_pair(("user_name", "risk_level"))
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
        check_all(orc, deleted=True)
    finally:
        eng.close()


@pytest.mark.gpu
def test_over_shards():
    """The CSV (dense fused, dense list through the index probes), small synthetic tables (every path, the sort included) and
    INSERT / DELETE again with the rows split over two shards of one card, so that most pairs have rows in both shards: their
    counts and sums must be added, their min / max merged (a child process: the engine reads PQPS_DEVICES when it is created).
    The one-row tables leave the second shard empty."""
    devices = "0,1" if pq.lib().pqps_device_count() >= 2 else "0,0"
    env = dict(os.environ, PQPS_DEVICES=devices)
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", __file__,
                        "-k", "golden_csv or (synthetic_small and (65537 or [1- or [1025-)) or synthetic_index_probes or insert_and_delete or product_of_two or few_hundred"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=str(q.ROOT))
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout


def test_group_pair_is_exported():
    """CPU: the library exports the two-column GROUP BY and the package wraps it."""
    L = pq.lib()
    for sym in ("executeQueryGroupPairHIP", "freeGroupPairResultHIP", "pqps_filter_group_pair", "pqps_group_pair_list", "pqps_group_pair_sort"):
        assert hasattr(L, sym), sym
    assert callable(getattr(pq.HipEngine, "group_pair", None))
    fields = [f for f, _ in pq.GroupPairResult._fields_]
    assert fields[:4] == ["groupColumn", "groupKind", "valueColumn", "valueKind"] and fields[-2:] == ["queryTime", "success"]
