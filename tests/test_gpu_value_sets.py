"""Value sets at the engine: IN (SELECT column FROM commands WHERE ... [GROUP BY column HAVING agg op n]) through
HipEngine.value_set / ValueSet.item / HipEngine.in_select.

The model is plain Python: a set is computed from the records with dicts (from the columns with numpy on the column engines),
and an outer chain is evaluated by test_gpu_set_predicates.chain_true after every set leaf has been replaced by the IN leaf over
the MODEL's members (resolve()).  An engine answer over a chain with a set is compared with the model, or with the same call over
that IN-list chain, which takes the engine's older route (a bitmap compiled on the host and uploaded).

    python tests/test_gpu_value_sets.py shards     shard_digest() as JSON, under whatever PQPS_DEVICES says
"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import group_top_matrix as gm
import qpelib as q
import test_gpu_group_count as grp
import test_gpu_set_predicates as sp

pq = q.pq
pytestmark = pytest.mark.gpu
CSV2K, EDGE = q.GOLDEN / "commands_2k.csv", q.GOLDEN / "edge_cases.csv"
M64 = (1 << 64) - 1
OPS = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, ">": lambda a, b: a > b,
       "<=": lambda a, b: a <= b, ">=": lambda a, b: a >= b}


def text(v):
    return v.decode("latin-1") if isinstance(v, bytes) else str(v)


def resolve(chain, sets):
    """The chain with every set leaf replaced by the IN leaf over the model's members (sets: id text -> values)."""
    if chain is None:
        return None
    out = []
    for k, item in enumerate(chain):
        if k % 2 == 1 or (not isinstance(item, list) and item[1] not in ("IN SET", "NOT IN SET")):
            out.append(item)
        elif isinstance(item, list):
            out.append(resolve(item, sets))
        else:
            out.append(sp.IN(item[0], [text(v) for v in sorted(sets[item[2]])], item[1].startswith("NOT")))
    return out


def aggregate_of(agg, values, value_column):
    if agg == "count":
        return len(values)
    if agg == "sum":
        return sum(values) & M64 if value_column == "command_id" else sum(values)
    return min(values) if agg == "min" else max(values)


def members_of(cells, values, rows, having):
    """S from dicts: cells[r] = the value of B in row r, values[r] = the value column's (None without one)."""
    per = {}
    for r in rows:
        per.setdefault(cells[r], []).append(values[r] if values is not None else 0)
    if having is None:
        return set(per)
    agg, vcol, op, const = having
    return {v for v, xs in per.items() if OPS[op](aggregate_of(agg, xs, vcol), int(const))}


class CsvTable:
    """An engine over a CSV, its records, and the model's members of every set made so far."""

    def __init__(self, csv, indexes):
        self.eng = pq.HipEngine(csv, list(indexes))
        self.indexed = bool(indexes)
        self.sets = {}
        self.reload()

    def reload(self):
        self.recs = [self.eng.record(i) for i in range(self.eng.e.contents.num_records)]

    def rows(self, chain):
        if chain is None:
            return list(range(len(self.recs)))
        plain = resolve(chain, self.sets)
        return [i for i, r in enumerate(self.recs) if sp.chain_true(r, plain)]

    def model_set(self, column, chain, having):
        rows = self.rows(chain)
        cells = [sp.field(r, column) for r in self.recs]
        values = [sp.field(r, having[1]) for r in self.recs] if having and having[1] else None
        return members_of(cells, values, rows, having), len(rows)

    def make(self, column, chain=None, having=None):
        """The engine's set, checked against the model's: members, rows, keys, and IN / NOT IN over the whole table."""
        want, n_rows = self.model_set(column, chain, having)
        vs = self.eng.value_set(column, chain, having)
        what = (column, chain, having)
        assert (vs.members, vs.rows) == (len(want), n_rows), what
        assert vs.keys() == [text(v) for v in sorted(want)], what
        self.sets[str(vs.id)] = want
        for negate in (False, True):
            outer = [vs.item(negate=negate)]
            rows = self.rows(outer)
            assert self.eng.count(outer) == len(rows) and self.eng.select_ids(outer) == rows, (what, negate)
        return vs

    def close(self):
        self.eng.close()


_tables = {}


def table(csv, indexed):
    key = (str(csv), indexed)
    if key not in _tables:
        _tables[key] = CsvTable(csv, pq.DEFAULT_INDEXES if indexed else ())
    return _tables[key]


@pytest.fixture(scope="module", autouse=True)
def _close_tables():
    yield
    for t in _tables.values():
        t.close()
    _tables.clear()


def many_leaves(last):
    chain = []
    for k in range(40):
        chain += [("user_id", "=", str(1000 + 2 * k)), "OR"]
    return chain + [last]


SETS_2K = [
    ("user_name", None, None),
    ("user_name", [("risk_level", "=", "5")], None),
    ("host_name", [("sudo_used", "=", "true"), "AND", ("risk_level", ">=", "4")], None),
    ("risk_level", [("exit_code", "!=", "0")], None),
    ("exit_code", None, None),
    ("user_id", [("shell_type", "=", "zsh")], None),
    ("host_name", [("sudo_used", "=", "true")], ("count", None, ">=", "10")),
    ("user_name", None, ("count", None, "<", "20")),
    ("user_name", [("risk_level", ">", "2")], ("count", None, "=", "3")),
    ("user_name", [("risk_level", ">", "2")], ("count", None, "!=", "3")),
    ("user_id", [("exit_code", "=", "0")], ("sum", "risk_level", ">", "40")),
    ("user_name", None, ("sum", "exit_code", "<=", "300")),
    ("base_command", None, ("sum", "command_id", ">", "20000")),
    ("user_name", None, ("max", "exit_code", ">", "100")),
    ("user_name", [("sudo_used", "=", "false")], ("max", "risk_level", "<", "4")),
    ("host_name", None, ("min", "command_id", "<=", "7")),
    ("shell_type", None, ("max", "command_id", "=", "1999")),
    ("working_directory", [("risk_level", "=", "1")], ("max", "user_id", ">=", "1080")),
    ("user_name", many_leaves(("risk_level", "=", "5")), None),                                   # more than 32 leaves
    ("user_name", many_leaves(("risk_level", "=", "5")), ("count", None, ">", "1")),
    ("user_name", [("raw_command", "LIKE", "%a%e%"), "AND", ("risk_level", ">", "1")], None),     # a member pass inside the build
    ("host_name", [("raw_command", "LIKE", "%a%e%")], ("sum", "risk_level", ">", "80")),
    ("user_name", [("risk_level", "=", "77")], None),                                             # the empty set
    ("user_name", None, ("count", None, "<", "1")),
    ("shell_type", None, ("count", None, ">=", "0")),                                             # the whole domain
    ("timestamp", [("risk_level", "=", "5")], ("count", None, "=", "1")),                         # 2000 bins
]
SETS_EDGE = [
    ("user_name", None, None), ("shell_type", [("risk_level", ">", "2")], None), ("exit_code", None, None), ("risk_level", None, None),
    ("host_name", None, ("count", None, ">", "2")), ("exit_code", None, ("sum", "user_id", "<", "0")),
    ("user_name", None, ("sum", "command_id", ">=", "9223372036854775808")), ("base_command", None, ("min", "user_id", "=", "-2147483648")),
    ("risk_level", None, ("max", "user_id", "=", "2147483647")), ("shell_type", None, ("max", "command_id", "=", "18446744073709551615")),
    ("raw_command", [("sudo_used", "=", "true")], ("min", "exit_code", "<", "0")), ("user_name", [("risk_level", "=", "77")], None),
]


@pytest.mark.parametrize("indexed", [False, True], ids=["none", "indexed"])
@pytest.mark.parametrize("csv, specs", [(CSV2K, SETS_2K), (EDGE, SETS_EDGE)], ids=["2k", "edge"])
def test_golden_sets(csv, specs, indexed):
    t = table(csv, indexed)
    made = [t.make(*spec) for spec in specs]
    assert any(vs.members == 0 for vs in made) and len({vs.id for vs in made}) == len(made)
    for vs in made:
        vs.free()


def test_chain_naming_an_earlier_set_and_cross_column():
    t = table(CSV2K, False)
    risky = t.make("user_name", [("risk_level", "=", "5"), "AND", ("sudo_used", "=", "true")])
    hosts = t.make("host_name", [risky.item()], ("count", None, ">", "100"))           # an inner chain that names a set
    nested = t.make("user_name", [hosts.item(negate=True), "OR", [risky.item(), "AND", ("exit_code", "!=", "0")]])
    levels = t.make("risk_level", [("sudo_used", "=", "true")], ("count", None, "<", "200"))
    assert 0 < levels.members < 5
    for attribute in ("exit_code", "user_id", "risk_level"):                               # exit_code 0 lies below, 126 .. 130 above 1 .. 5
        for negate in (False, True):
            outer = [levels.item(attribute, negate), "AND", nested.item()]
            assert t.eng.select_ids(outer) == t.rows(outer), (attribute, negate)
    assert t.eng.count([levels.item("exit_code")]) == sum(1 for r in t.recs if r.exit_code in t.sets[str(levels.id)]) > 0
    # in_select: the item alone, the set kept alive by the engine
    item = t.eng.in_select("user_name", "user_name", [("risk_level", "=", "5"), "AND", ("sudo_used", "=", "true")], negate=True)
    assert item[:2] == ("user_name", "NOT IN SET") and item[2] not in t.sets
    assert t.eng.select_ids([item]) == t.eng.select_ids([risky.item(negate=True)]) == t.rows([risky.item(negate=True)])
    for vs in (risky, hosts, nested, levels):
        vs.free()


def forms(eng, chain):
    """Each reader form once over `chain`."""
    return {
        "count": eng.count(chain), "select_ids": eng.select_ids(chain), "group_count": eng.group_count("host_name", chain),
        "aggregate": eng.aggregate("exit_code", "shell_type", chain), "order_ids": eng.order_ids("user_id", chain, True, 25),
        "count_distinct": eng.count_distinct("user_name", "risk_level", chain), "group_pair": eng.group_pair(("shell_type", "risk_level"), "user_id", chain),
        "group_buckets": eng.group_buckets("user_name", prefix=9, chain=chain), "group_first": eng.group_first("host_name", "exit_code", chain, True),
        "group_top": eng.group_top("base_command", "risk_level", "sum", True, 7, chain),
    }


@pytest.mark.parametrize("indexed", [False, True], ids=["none", "indexed"])
def test_every_reader_form_over_a_chain_with_a_set(indexed):
    t = table(CSV2K, indexed)
    heavy = t.make("user_name", [("risk_level", ">=", "3")], ("count", None, ">=", "5"))
    quiet = t.make("host_name", [("sudo_used", "=", "true")], ("sum", "risk_level", "<", "400"))
    assert 0 < heavy.members < 88
    for chain in ([heavy.item()], [("risk_level", ">", "1"), "AND", [heavy.item(), "OR", quiet.item(negate=True)]],
                  [("user_id", ">=", "1040"), "OR", heavy.item(negate=True)]):
        got, want = forms(t.eng, chain), forms(t.eng, resolve(chain, t.sets))
        for name in want:
            assert got[name] == want[name], (name, chain)
        assert got["count"] == len(t.rows(chain))
    assert sorted(t.eng.select_ids([heavy.item()])) == t.rows([heavy.item()])
    heavy.free()
    quiet.free()


def test_update_and_delete_over_a_chain_with_a_set(tmp_path):
    answers = []
    for use_set in (True, False):
        csv = tmp_path / f"copy{int(use_set)}.csv"
        shutil.copy(CSV2K, csv)
        t = CsvTable(csv, ())
        try:
            out = []
            for writer in ("update", "delete"):
                vs = t.make("user_name", [("risk_level", ">=", "3")], ("count", None, ">=", "4"))
                chain = [vs.item(), "AND", ("sudo_used", "=", "false")]
                rows = t.rows(chain)
                assert rows
                run = chain if use_set else resolve(chain, t.sets)
                if writer == "update":
                    assert t.eng.update({"exit_code": "77"}, run) == len(rows)
                else:
                    rs = pq.lib().executeQueryDeleteHIP(t.eng.e, b"commands", pq.WhereList(run).ptr)
                    assert rs.contents.success and rs.contents.numRecords == len(rows)
                    pq.lib().freeResultSet(rs)
                with pytest.raises(pq.PqpsError):
                    t.eng.select_ids([vs.item()])                    # the writer made it stale
                vs.free()
                t.reload()
                out.append((t.eng.count(None), t.eng.select_ids([("exit_code", "=", "77")]), t.eng.group_count("user_name")))
                assert out[-1][1] == [i for i, r in enumerate(t.recs) if r.exit_code == 77]
            answers.append((out, csv.read_bytes()))
        finally:
            t.close()
    assert answers[0] == answers[1], "the set chain and the IN-list chain leave the same table and the same CSV"


# ---- the synthetic table and the column engines: numpy folds ---------------------------------------------------------------
def numpy_set(codes, values, rows, having, n_bins=None):
    """-> (sorted member bins, rows) from bincounts over the inner rows; codes are bins (code, or value - lo)."""
    n_bins = int(codes.max()) + 1 if n_bins is None else n_bins
    b = codes[rows].astype(np.int64)
    count = np.bincount(b, minlength=n_bins)
    live = count > 0
    if having is None:
        return np.flatnonzero(live), len(rows)
    agg, vcol, op, const = having
    if agg == "count":
        x = count
    else:
        v = values[rows].astype(np.int64)
        if agg == "sum":
            x = np.zeros(n_bins, dtype=np.int64)
            np.add.at(x, b, v)
        else:
            x = np.full(n_bins, np.iinfo(np.int64).max if agg == "min" else np.iinfo(np.int64).min)
            (np.minimum if agg == "min" else np.maximum).at(x, b, v)
    return np.flatnonzero(live & OPS[op](x, int(const))), len(rows)


def test_synthetic_table_of_2_20_rows():
    n = 1 << 20
    host = q.HostSynth(n, seed=0x5EED, full=True)
    eng = pq.HipEngine.synthetic(n, seed=0x5EED)
    try:
        users = host.arr["user_name"]
        for chain, having in (([("risk_level", "=", "5")], ("count", None, ">=", "8")), (None, ("count", None, "<", "400")),
                              ([("sudo_used", "=", "TRUE")], None), ([("shell_type", "=", "zsh")], ("sum", "exit_code", ">", "3000"))):
            rows = np.arange(n) if chain is None else host.oracle_scan(chain).astype(np.int64)
            want, n_rows = numpy_set(users, host.arr["exit_code"], rows, having, len(pq.SYNTH_USERS_DICT))
            vs = eng.value_set("user_name", chain, having)
            assert (vs.members, vs.rows) == (len(want), n_rows) and 0 < len(want) < len(pq.SYNTH_USERS_DICT), (chain, having)
            assert vs.keys() == [pq.SYNTH_USERS_DICT[k].decode() for k in want]
            member = np.zeros(len(pq.SYNTH_USERS_DICT), dtype=bool)
            member[want] = True
            assert eng.count([vs.item()]) == int(member[users].sum())
            outer = [vs.item(negate=True), "AND", ("risk_level", "=", "4")]
            ids = np.flatnonzero(~member[users] & (host.arr["risk_level"] == 4))
            assert np.array_equal(np.array(eng.select_ids(outer), dtype=np.int64), ids)
            vs.free()
        # a single-valued string column has no buffer to group by: one value, in S iff the HAVING holds over every inner row
        k = int((host.arr["risk_level"] == 5).sum())
        for having, members in ((None, 1), (("count", None, "=", str(k)), 1), (("count", None, "<", str(k)), 0), (("max", "risk_level", "=", "5"), 1)):
            vs = eng.value_set("raw_command", [("risk_level", "=", "5")], having)
            assert (vs.members, vs.rows) == (members, k) and vs.keys() == ["cmd"][:members]
            assert eng.count([vs.item()]) == (n if members else 0) and eng.count([vs.item(negate=True)]) == (0 if members else n)
            vs.free()
    finally:
        eng.close()


def wide_checks(run, n_shards_hint=None):
    """The 70 000-string column and the i32 column over 100 001 values: the wide bins with HAVING, the global presence bitmap
    without; -> a digest of the answers."""
    m, eng, out = run.model, run.eng, []
    names, exits = m.codes("user_name"), m.m["exit_code"].astype(np.int64)
    for column, codes, n_bins in (("user_name", names, gm.USERS), ("exit_code", exits - gm.EXIT_LO, gm.EXIT_HI - gm.EXIT_LO + 1)):
        for where in ("none", "one_pass", "several_passes", "member"):
            chain = gm.WHERES[where][0]
            rows = np.asarray(m.select_ids(chain), dtype=np.int64)
            for having in (None, ("count", None, ">=", "3"), ("sum", "risk_level", ">", "9"), ("max", "command_id", "<", str(1 << 63))):
                if having and having[1] == "command_id":
                    mx = np.zeros(n_bins, dtype=np.uint64)
                    np.maximum.at(mx, codes[rows], m.m["command_id"][rows])
                    live = np.bincount(codes[rows], minlength=n_bins) > 0
                    want = np.flatnonzero(live & (mx < np.uint64(1 << 63)))
                else:
                    want, _ = numpy_set(codes, m.m[having[1]] if having and having[1] else None, rows, having, n_bins)
                vs = eng.value_set(column, chain, having)
                assert (vs.members, vs.rows) == (len(want), len(rows)), (column, where, having)
                member = np.zeros(n_bins, dtype=bool)
                member[want] = True
                assert eng.count([vs.item()]) == int(member[codes].sum()), (column, where, having)
                outer = [vs.item(negate=True), "AND", ("shell_type", "=", "fish")]
                ids = np.flatnonzero(~member[codes] & (m.m["shell_type"][0] == gm.SHELLS.index(b"fish")))
                got = eng.select_ids(outer)
                assert np.array_equal(np.array(got, dtype=np.int64), ids), (column, where, having)
                keys = vs.keys()
                if column == "exit_code":
                    assert keys == [str(k + gm.EXIT_LO) for k in want]
                else:
                    assert keys == [b.decode() for b in np.array(m.m["user_name"][1], dtype=object)[want]]
                out.append([column, where, str(having), vs.members, vs.rows, zlib.crc32(" ".join(keys).encode()), len(got)])
                vs.free()
    return out


def test_wide_columns_on_a_column_engine():
    run = gm.Run(gm.table())
    try:
        assert len(wide_checks(run)) == 32
    finally:
        run.close()


def test_domains_that_fit_no_route_are_refused():
    n = 4096
    cols = gm.table(n, 300)
    cols["exit_code"] = cols["exit_code"].copy()
    cols["exit_code"][:2] = [-(1 << 26) - 5, 1 << 26]                       # more than 2^27 values: no bitmap without HAVING
    cols["user_id"] = cols["user_id"].copy()
    cols["user_id"][:2] = [0, (256 << 20) // 32]                             # 32 B x (2^23 + 1) bins: past the budget with a value
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        with pytest.raises(pq.PqpsError):
            eng.value_set("exit_code")
        with pytest.raises(pq.PqpsError):
            eng.value_set("user_id", None, ("sum", "risk_level", ">", "0"))
        vs = eng.value_set("user_id", None, ("count", None, ">", "1"))      # 4 B a bin fit
        want, _ = numpy_set(cols["user_id"].astype(np.int64), None, np.arange(n), ("count", None, ">", "1"))
        assert vs.members == len(want) and vs.keys() == [str(k) for k in want]
        vs.free()
        vs = eng.value_set("user_id")                                        # and so does the bitmap without HAVING
        assert vs.members == len(np.unique(cols["user_id"]))
        assert eng.count([vs.item("exit_code")]) == int(np.isin(cols["exit_code"], cols["user_id"]).sum())
        vs.free()
    finally:
        eng.close()


# ---- lifetime and refusals --------------------------------------------------------------------------------------------------
def test_stale_after_each_writer_and_use_after_free(tmp_path):
    csv = tmp_path / "data.csv"
    shutil.copy(CSV2K, csv)
    eng = pq.HipEngine(csv, pq.DEFAULT_INDEXES)
    L = pq.lib()

    def fresh():
        vs = eng.value_set("user_name", [("risk_level", "=", "5")])
        assert eng.count([vs.item()]) > 0
        return vs

    def stale(vs):
        assert eng.count([vs.item()]) == -1
        for call in (lambda: eng.select_ids([vs.item(negate=True)]), lambda: eng.group_count("host_name", [vs.item()]), vs.keys,
                     lambda: eng.value_set("host_name", [vs.item()]), lambda: eng.update({"exit_code": "3"}, [vs.item()])):
            with pytest.raises(pq.PqpsError):
                call()
        vs.free()

    try:
        vs = fresh()
        assert L.executeQueryInsertHIP(eng.e, b"commands", C.byref(grp.make_record(900001, 3, 1001, b"student1001")))
        stale(vs)
        vs = fresh()
        assert eng.insert_rows([grp.make_record(900002, 4, 1002, b"aaa_new"), grp.make_record(900003, 4, 1002, b"zzz_new")]) == 2
        stale(vs)
        vs = fresh()
        rs = L.executeQueryDeleteHIP(eng.e, b"commands", pq.WhereList([("command_id", ">=", "900001")]).ptr)
        assert rs.contents.success and rs.contents.numRecords == 3
        L.freeResultSet(rs)
        stale(vs)
        vs = fresh()
        assert eng.update({"risk_level": "2"}, [("command_id", "=", "5")]) == 1
        stale(vs)
        # a refused writer changes nothing and leaves the sets alone
        vs = fresh()
        with pytest.raises(pq.PqpsError):
            eng.update({"no_such_column": "1"}, None)
        assert eng.count([vs.item()]) > 0
        # use after free, and an id that never was
        item = vs.item()
        vs.free()
        vs.free()
        assert eng.count([item]) == -1 and eng.count([("user_name", "IN SET", "4000000")]) == -1
        with pytest.raises(pq.PqpsError):
            vs.keys()
    finally:
        eng.close()


def test_refusals_limits_and_tickets(capfd):
    eng = pq.HipEngine(CSV2K, ())
    try:
        for column, chain, having in (("no_such_column", None, None), ("command_id", None, None), ("sudo_used", None, None),
                                      ("user_name", None, ("sum", "shell_type", ">", "1")), ("user_name", None, ("max", "sudo_used", ">", "0")),
                                      ("user_name", None, ("sum", None, ">", "1")), ("user_name", None, ("min", "no_such_column", ">", "1")),
                                      ("user_name", None, ("key", None, ">", "1")), ("user_name", None, (7, None, ">", "1")),
                                      ("user_name", None, ("count", None, "==", "1")), ("user_name", None, ("count", None, ">", "-1")),
                                      ("user_name", None, ("count", None, ">", "1x")), ("user_name", None, ("sum", "exit_code", ">", "9223372036854775808")),
                                      ("user_name", None, ("sum", "command_id", ">", "-1")), ("user_name", [("user_name", "LIKE", "%"), "AND", ("risk_level", "LIKE", "1")], None)):
            with pytest.raises(pq.PqpsError):
                eng.value_set(column, chain, having)
        assert eng.count([("command_id", "IN SET", "1")]) == -1
        made = [eng.value_set("risk_level") for _ in range(64)]
        with pytest.raises(pq.PqpsError):
            eng.value_set("risk_level")                                    # the 65th
        made.pop().free()
        made.append(eng.value_set("risk_level"))
        assert len({vs.id for vs in made}) == 64 and eng.count([made[-1].item()]) == eng.n
        # from a thread that holds a ticket: making a set is a reader and legal, freeing one waits like a writer and is refused
        ticket = eng.select_async([("risk_level", ">", "3")])
        assert ticket
        extra = made.pop()
        with pytest.raises(pq.PqpsError):
            extra.free()
        assert eng.count([extra.item()]) == eng.n
        eng.release_ticket(ticket)
        made.pop().free()                                                  # (room for one more)
        ticket = eng.select_async([("risk_level", ">", "3")])
        beside = eng.value_set("host_name", [extra.item()], ("count", None, ">", "0"))
        assert beside.members == 16
        eng.release_ticket(ticket)
        extra.free()
        beside.free()
        assert eng.count([extra.item()]) == -1
        err = capfd.readouterr().err
        assert "stale" not in err and "does not exist" in err
        # what is left goes with the engine
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
        vs = eng.value_set("user_name", [("risk_level", "=", "5")])       # before the join: an ordinary engine
        assert vs.members > 0
        if rank == 0:
            ident[0] = pq.HipEngine.rccl_id(LOOPBACK)
        gate.wait()
        eng.join_ranks(LOOPBACK, ident[0])
        n = 0
        for column, having in (("user_name", None), ("host_name", ("count", None, ">", "3")), ("user_id", ("sum", "risk_level", ">", "3"))):
            try:
                eng.value_set(column, None, having)
            except pq.PqpsError:
                n += 1
        n += eng.count([vs.item()]) == -1                                  # a WHERE of several passes, as every member pass
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
assert refused == [4, 4], refused
print("OK")
"""


def test_refused_on_joined_ranks():
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    assert "joined across ranks" in p.stderr


# ---- several shards -----------------------------------------------------------------------------------------------------------
def shard_digest():
    """A handful of the checks above, as data: what one shard and three shards must agree on."""
    out = {"shards": None}
    t = CsvTable(CSV2K, ())
    try:
        out["shards"] = len(t.eng.shards())
        made = [t.make(*spec) for spec in SETS_2K[::3]]
        heavy = t.make("user_name", [("risk_level", ">=", "3")], ("count", None, ">=", "5"))
        chain = [("risk_level", ">", "1"), "AND", [heavy.item(), "OR", made[2].item(negate=True)]]
        got, want = forms(t.eng, chain), forms(t.eng, resolve(chain, t.sets))
        assert got == want
        out["csv"] = [[vs.members, vs.rows, vs.keys()] for vs in made] + [json.loads(json.dumps(got, default=str))]
    finally:
        t.close()
    run = gm.Run(gm.table(40_000, 70_000))
    try:
        out["wide"] = wide_checks(run)
    finally:
        run.close()
    return out


def test_over_three_shards():
    devices = "0,0,0"
    p = subprocess.run([sys.executable, str(q.ROOT / "tests" / "test_gpu_value_sets.py"), "shards"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, PQPS_DEVICES=devices), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip(), (p.stdout[-3000:], p.stderr[-3000:])
    three = json.loads(p.stdout.strip().splitlines()[-1])
    assert three.pop("shards") == 3
    one = json.loads(json.dumps(shard_digest()))
    assert one.pop("shards") == 1
    assert three == one


if __name__ == "__main__":
    assert sys.argv[1:] == ["shards"], sys.argv
    print(json.dumps(shard_digest()))
