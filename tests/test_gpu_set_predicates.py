"""LIKE / NOT LIKE / IN / NOT IN through HipEngine.

Expected answers come from Python over the parsed records (`re` for LIKE, sets for IN) and from the engine's own `=` / OR
path, which the QPESeq golden files pin; the synthetic tables are checked against the CPU twin of the generator."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import kernel_model as km
import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu
NUMERIC = ("command_id", "exit_code", "user_id", "risk_level")
STRINGS = [c for c in pq.COLUMNS if pq.COLUMN_KIND[pq.COL[c]] == pq.KIND_DICT]
LOOPBACK = q.ROOT / "tests" / "loopback" / "libloopback_rccl.so"


# ---- the chains in plain Python over the records ---------------------------------------------------------------------------
def like_regex(pattern: bytes):
    out, i = b"", 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"\\" and pattern[i + 1:i + 2] in (b"%", b"_", b"\\"):
            out += re.escape(pattern[i + 1:i + 2])
            i += 1
        else:
            out += b".*" if c == b"%" else b"." if c == b"_" else re.escape(c)
        i += 1
    return re.compile(out, re.DOTALL)


_ITEMS = {}


def IN(attr, items, negate=False):
    text = pq.in_list(items)
    _ITEMS[text] = list(items)
    return (attr, "NOT IN" if negate else "IN", text)


def field(rec, attr):
    if attr in STRINGS:                                          # the C string from the field's start (an overlong one runs on)
        return C.string_at(C.addressof(rec) + getattr(pq.Record, attr).offset)
    return int(getattr(rec, attr))


def leaf_true(rec, leaf):
    attr, op, value = leaf[:3]
    if attr not in pq.COLUMNS:
        return False                                             # an unknown attribute is never true
    v = field(rec, attr)
    if op in ("LIKE", "NOT LIKE"):
        return (like_regex(value.encode("latin-1")).fullmatch(v) is not None) != op.startswith("NOT")
    if op in ("IN", "NOT IN"):
        items = _ITEMS[value]
        if attr in STRINGS:
            want = {t.encode("latin-1") if isinstance(t, str) else t for t in items}
        elif attr == "sudo_used":
            want = {1 if str(t).lower() in ("true", "1") else 0 for t in items}
        else:
            want = {int(t) for t in items}
        return (v in want) != op.startswith("NOT")
    lit = value.encode("latin-1") if attr in STRINGS else (1 if value.lower() in ("true", "1") else 0) if attr == "sudo_used" else int(value)
    return {"=": v == lit, "!=": v != lit, "<": v < lit, ">": v > lit, "<=": v <= lit, ">=": v >= lit}[op]


def chain_true(rec, chain):
    """evaluateWhereClause: right-recursive, no precedence."""
    items, ops = chain[0::2], chain[1::2]
    acc = None
    for k in range(len(items) - 1, -1, -1):
        it = items[k]
        m = chain_true(rec, it) if isinstance(it, list) else leaf_true(rec, it)
        acc = m if acc is None else (m or acc) if ops[k] == "OR" else (m and acc)
    return acc


class Table:
    """One CSV: an engine without indexes, its records, and the compiler's schema of it."""

    def __init__(self, name):
        self.csv = q.GOLDEN / name
        self.eng = pq.HipEngine(self.csv, [])
        self.n = self.eng.n
        self.recs = [self.eng.record(i) for i in range(self.n)]
        orc = q.OracleTable(self.csv, [])
        self.spec, _ = km.columns_from_records(orc.rows, orc.n)
        self.values = {c: sorted({field(r, c) for r in self.recs}) for c in pq.COLUMNS}

    def expect(self, chain):
        return [i for i, r in enumerate(self.recs) if chain_true(r, chain)]

    def member_passes(self, chain):
        return sum(m is not None for _, _, m in pq.compile_plan_sets(self.spec, chain))


_tables = {}


def table(name):
    if name not in _tables:
        _tables[name] = Table(name)
    return _tables[name]


def scattered(values, k):
    """k of the sorted values, no two of them neighbours."""
    step = max(2, (len(values) - 1) // max(k - 1, 1))
    return [values[i] for i in range(0, len(values), step)][:k]


def text(v):
    return v.decode("latin-1") if isinstance(v, bytes) else str(v)


def chains_for(t):
    """About 40 chains: every string and numeric column under the four operators, nested and mixed with comparisons."""
    out = []
    for c in STRINGS:
        vals = t.values[c]
        few, many = scattered(vals, 3), scattered(vals, 7)
        out.append([IN(c, [text(v) for v in few])])
        out.append([IN(c, [text(v) for v in many], True), "AND", ("risk_level", ">", "1")])
        probe = text(vals[len(vals) // 2])
        out.append([(c, "LIKE", pq.like_escape(probe[:max(1, len(probe) // 2)]) + "%")])
        out.append([("sudo_used", "=", "true"), "OR", (c, "NOT LIKE", "%" + pq.like_escape(probe[1:3]) + "%")])
    for c in NUMERIC:
        vals = t.values[c]
        out.append([IN(c, [text(v) for v in scattered(vals, 3)])])
        out.append([("shell_type", "!=", "zsh"), "AND", [IN(c, [text(v) for v in scattered(vals, 8)], True), "OR", ("sudo_used", "=", "true")]])
    out += [
        [IN("sudo_used", ["true"])], [IN("sudo_used", ["false", "1"], True)], [IN("risk_level", [])], [IN("user_name", [], True)],
        [("raw_command", "LIKE", "%")], [("raw_command", "LIKE", "%a%"), "AND", ("raw_command", "NOT LIKE", "%e%")],
        [("raw_command", "LIKE", "_%s"), "OR", [("base_command", "LIKE", "__"), "AND", IN("exit_code", ["0", "1"])]],
        [("working_directory", "LIKE", "/home/%"), "AND", IN("user_name", [text(v) for v in scattered(t.values["user_name"], 9)]),
         "OR", IN("command_id", [text(v) for v in scattered(t.values["command_id"], 12)])],
        [("timestamp", "LIKE", "2025-0_-1%"), "AND", ("risk_level", ">=", "2")],
        [IN("exit_code", ["-1", "0", "2", "126", "127", "130", "255"]), "AND", ("user_id", "<", "1060")],
        [("host_name", "NOT LIKE", "labpc-0_"), "AND", IN("shell_type", ["bash", "zsh"])],
        [("nonexistent", "IN", "('x')"), "OR", ("risk_level", "=", "5")],
        [IN("user_name", [text(v) for v in scattered(t.values["user_name"], 20)])],
        [IN("command_id", [text(v) for v in scattered(t.values["command_id"], 30)], True), "AND", ("sudo_used", "=", "false")],
        [IN("user_id", [text(v) for v in scattered(t.values["user_id"], 10)]), "OR", ("raw_command", "LIKE", "%o%")],
        [("timestamp", "NOT LIKE", "%7%"), "AND", [("risk_level", "<", "3"), "OR", IN("host_name", [text(v) for v in scattered(t.values["host_name"], 6)])]],
    ]
    return out


@pytest.mark.parametrize("csv", ["commands_2k.csv", "edge_cases.csv"])
def test_select_and_count_equal_python(csv):
    t = table(csv)
    chains = chains_for(t)
    assert len(chains) >= 40
    with_pass = without = 0
    for chain in chains:
        want = t.expect(chain)
        assert t.eng.select_ids(chain) == want, chain
        assert t.eng.count(chain) == len(want), chain
        if t.member_passes(chain):
            with_pass += 1
        else:
            without += 1
    if csv == "commands_2k.csv":
        assert with_pass >= 10 and without >= 10, (with_pass, without)
        assert any(0 < len(t.expect(c)) < t.n for c in chains)


def test_refused_where_fails_the_query():
    t = table("commands_2k.csv")
    for leaf in (("risk_level", "LIKE", "3%"), ("host_name", "IN", "labpc-01, labpc-02"), ("host_name", "IN", "('labpc-01)"), ("host_name", "IN", "(a,,b)")):
        assert t.eng.count([leaf]) == -1
        with pytest.raises(pq.PqpsError):
            t.eng.select_ids([("risk_level", ">", "1"), "AND", leaf])
    assert t.eng.count([("risk_level", "like", "3%")]) == 0          # any other unknown operator: never true


def test_index_mode_refilters_with_the_set():
    t = table("commands_2k.csv")
    eng = pq.HipEngine(t.csv, pq.DEFAULT_INDEXES)
    try:
        probed = eng.select_ids([("risk_level", ">", "3")])
        assert probed != sorted(probed), "index order, not row order"
        for leaf in (("raw_command", "LIKE", "%a%"), ("raw_command", "NOT LIKE", "%e%"), IN("user_name", [text(v) for v in scattered(t.values["user_name"], 6)]),
                     IN("host_name", [text(v) for v in scattered(t.values["host_name"], 2)])):
            got = eng.select_ids([("risk_level", ">", "3"), "AND", leaf])
            assert got == [i for i in probed if leaf_true(t.recs[i], leaf)], leaf
        # a set condition on an indexed column is no probe: the answer comes in row order
        ids = [text(v) for v in scattered(t.values["command_id"], 9)]
        assert eng.select_ids([IN("command_id", ids)]) == t.expect([IN("command_id", ids)])
    finally:
        eng.close()


def or_chain(attr, values):
    out = []
    for v in values:
        out += [(attr, "=", text(v)), "OR"]
    return out[:-1]


def test_aggregates_equal_the_or_chain():
    t = table("commands_2k.csv")
    users = scattered(t.values["user_name"], 6)
    sub = None
    for cand in (b"rm -rf", b"grep", b"ssh", b"git", b"cat", b"-la", b"sudo", b"py"):
        hits = [v for v in t.values["raw_command"] if cand in v]
        if 6 <= len(hits) <= 60:
            sub = cand
            break
    assert sub is not None
    pairs = [([IN("user_name", [text(v) for v in users])], or_chain("user_name", users)),
             ([("raw_command", "LIKE", "%" + pq.like_escape(sub.decode()) + "%")], or_chain("raw_command", hits))]
    assert t.member_passes(pairs[0][0]) == 1
    for sets, ors in pairs:
        want = t.expect(sets)
        assert 0 < len(want) < t.n and t.eng.select_ids(ors) == want
        for call in (lambda c: t.eng.group_count("shell_type", c), lambda c: t.eng.group_count("user_name", c),
                     lambda c: t.eng.aggregate("exit_code", None, c), lambda c: t.eng.aggregate("command_id", "host_name", c),
                     lambda c: t.eng.count_distinct_total("user_name", "risk_level", c), lambda c: t.eng.count_distinct("command_id", None, c),
                     lambda c: t.eng.order_ids("exit_code", c, descending=True, limit=10), lambda c: t.eng.order_ids("raw_command", c, limit=10),
                     lambda c: t.eng.group_pair(("shell_type", "risk_level"), None, c), lambda c: t.eng.group_pair(("host_name", "sudo_used"), "user_id", c)):
            assert call(sets) == call(ors)


# ---- a synthetic engine of 100 001 rows ---------------------------------------------------------------------------------------------
SYNTH_ROWS, SYNTH_SEED = 100_001, 0x5E75


def synth_chains(host):
    rng = np.random.default_rng(3)
    users = sorted(rng.choice(pq.SYNTH_USERS, 50, replace=False).tolist())
    ids = sorted(rng.choice(host.arr["command_id"], 300, replace=False).tolist())
    chains = {"users": [("user_name", "IN", pq.in_list([pq.SYNTH_USERS_DICT[u] for u in users]))],
              "ids": [("command_id", "IN", pq.in_list(ids))]}
    want = {"users": np.nonzero(np.isin(host.arr["user_name"], users))[0],
            "ids": np.nonzero(np.isin(host.arr["command_id"], np.array(ids, dtype=np.uint64)))[0]}
    return chains, want


SHARD_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    import numpy as np
    import qpelib as q
    import test_gpu_set_predicates as me
    pq = q.pq
    host = q.HostSynth(me.SYNTH_ROWS, seed=me.SYNTH_SEED)
    chains, want = me.synth_chains(host)
    eng = pq.HipEngine.synthetic(me.SYNTH_ROWS, seed=me.SYNTH_SEED)
    print("SHARDS", eng.shards())
    for name in chains:
        got = np.array(eng.select_ids(chains[name]), dtype=np.int64)
        print("SAME", name, bool(np.array_equal(got, want[name])), eng.count(chains[name]) == len(want[name]))
    eng.close()
""")


def test_synthetic_engine_sync_async_and_two_shards():
    host = q.HostSynth(SYNTH_ROWS, seed=SYNTH_SEED)
    chains, want = synth_chains(host)
    assert 0 < len(want["users"]) < SYNTH_ROWS and 300 <= len(want["ids"]) < SYNTH_ROWS
    eng = pq.HipEngine.synthetic(SYNTH_ROWS, seed=SYNTH_SEED)
    ctx = pq.Context(0)
    try:
        for name, chain in chains.items():
            assert np.array_equal(np.array(eng.select_ids(chain), dtype=np.int64), want[name]), name
            assert eng.count(chain) == len(want[name])
        # two lanes at once, awaited out of order; a COUNT ticket beside them
        names = list(chains)
        tickets = [eng.select_async(chains[n]) for n in names] + [eng.select_async(chains["users"], count_only=True)]
        try:
            assert eng.await_ticket(tickets[2])[0] == len(want["users"])
            for i in (1, 0):
                k, r = eng.await_ticket(tickets[i])
                assert k == len(want[names[i]])
                ids = np.zeros(max(k, 1), dtype=np.uint32)
                ctx.download(ids.ctypes.data, r.ids_dev, 4 * k)
                assert np.array_equal(ids[:k], want[names[i]]), names[i]
        finally:
            for tk in tickets:
                eng.release_ticket(tk)
    finally:
        ctx.close()
        eng.close()
    env = dict(os.environ, PQPS_DEVICES="0,1" if pq.lib().pqps_device_count() >= 2 else "0,0")
    p = subprocess.run([sys.executable, "-c", SHARD_CHILD % str(q.ROOT / "tests")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines[0] == f"SHARDS [{(SYNTH_ROWS + 1) // 2}, {SYNTH_ROWS // 2}]"
    assert lines[1:] == ["SAME users True True", "SAME ids True True"]


def test_delete_with_a_member_pass_equals_the_or_chain(tmp_path):
    t = table("commands_2k.csv")
    hosts = scattered(t.values["host_name"], 5)
    assert t.member_passes([IN("host_name", [text(v) for v in hosts])]) == 1
    left = {}
    for name, chain in (("in", [IN("host_name", [text(v) for v in hosts])]), ("or", or_chain("host_name", hosts))):
        csv = tmp_path / f"{name}.csv"
        shutil.copy(t.csv, csv)
        eng = pq.HipEngine(csv, pq.DEFAULT_INDEXES)
        try:
            wl = pq.WhereList(chain)
            rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
            assert rs.contents.success
            deleted = rs.contents.numRecords
            pq.lib().freeResultSet(rs)
            rows = eng.select(["command_id", "host_name"], [])["rows"]
            left[name] = (deleted, rows, csv.read_bytes(), eng.select_ids([("risk_level", ">", "3")]))
        finally:
            eng.close()
    gone = t.expect([IN("host_name", [text(v) for v in hosts])])
    assert left["in"][0] == len(gone) > 0 and len(left["in"][1]) == t.n - len(gone)
    assert left["in"] == left["or"]
    assert [int(r[0]) for r in left["in"][1]] == [int(t.recs[i].command_id) for i in range(t.n) if i not in set(gone)]


RANK_WORKER = textwrap.dedent("""
    import json, os, sys, threading, traceback
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import qpelib as q
    pq = q.pq
    world, n = 2, int(os.environ["ROWS"])
    chains = json.loads(os.environ["CHAINS"])
    gate = threading.Barrier(world)
    ident = [None]
    out = [None] * world

    def rank_main(rank):
        try:
            eng = pq.HipEngine.synthetic_rank(n, world, rank, seed=21)
            if rank == 0:
                ident[0] = pq.HipEngine.rccl_id(LOOPBACK)
            gate.wait()
            eng.join_ranks(LOOPBACK, ident[0])
            ctx = pq.Context(0)
            tk = eng.select_async([tuple(chains["two"])])
            k, r = eng.await_ticket(tk)
            ids = np.zeros(max(k, 1), dtype=np.uint32)
            if k > 0:
                ctx.download(ids.ctypes.data, r.ids_dev, 4 * k)
            eng.release_ticket(tk)
            gate.wait()
            # a WHERE with a member pass is several passes: refused on a joined engine, on every rank alike
            refused = eng.count([tuple(chains["many"])])
            tk = eng.select_async([tuple(chains["many"])])
            refused_async = eng.await_ticket(tk)[0] if tk else -1
            if tk:
                eng.release_ticket(tk)
            gate.wait()
            again = eng.count([tuple(chains["two"])])
            out[rank] = [int(k), ids[:k].tolist(), int(refused), int(refused_async), int(again)]
            gate.wait()
            eng.leave_ranks()
            ctx.close()
            eng.close()
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            os._exit(3)

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join()
    with open(os.environ["OUT_FILE"], "w") as f:
        json.dump(out, f)
    print("OK")
""")


def test_rank_joined_engine_answers_windows_and_refuses_member_passes(tmp_path):
    assert LOOPBACK.exists(), "build it first: make -C tests/loopback (python __graft_entry__.py does)"
    rows = 200_001
    users = [pq.SYNTH_USERS_DICT[i].decode() for i in (5, 300, 777, 1200, 1600, 1999)]
    chains = {"two": ["user_name", "IN", pq.in_list(users[:2])], "many": ["user_name", "IN", pq.in_list(users)]}
    script = tmp_path / "worker.py"
    script.write_text(f"ROOT = {str(q.ROOT)!r}\nLOOPBACK = {str(LOOPBACK)!r}\n" + RANK_WORKER)
    import json
    env = dict(os.environ, ROWS=str(rows), CHAINS=json.dumps(chains), OUT_FILE=str(tmp_path / "out.json"), OMP_NUM_THREADS="1",
               PQPS_EXCHANGE_TIMEOUT_S="60")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-1500:], p.stderr[-3000:])
    got = json.loads((tmp_path / "out.json").read_text())
    host = q.HostSynth(rows, seed=21)
    want = np.nonzero(np.isin(host.arr["user_name"], [5, 300]))[0]
    assert len(want) > 0
    for r in range(2):
        k, ids, refused, refused_async, again = got[r]
        assert k == len(want) and np.array_equal(np.array(ids), want), r
        assert refused == -1 and refused_async == -1 and again == len(want), (r, refused, refused_async, again)
