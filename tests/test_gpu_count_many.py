"""HipEngine.count_many (executeQueryCountManyHIP) against the CPU model of tests/column_model.py, on the 5 123-row table of
tests/shard_matrix.py: one shard and three, with shard_matrix's HOST_INDEX and with no index.

One call of CHAINS mixes every route: chains that are fused into shared scans (more than 16 of them: several batches),
chains of 7 and more comparisons, a plan of two scan passes, fragmented IN / NOT IN and LIKE (member passes), IN SET, chains
on indexed columns, constants of both values, an unknown attribute, no WHERE at all.  Every answer must equal the model's
count of the chain, in order, and what engine.count(chain) returns.  The same call follows the model through an
insert_rows, an UPDATE and a DELETE.  No expected answer comes from an engine.

This file is its own driver (PQPS_DEVICES is read when an engine is created):
    python tests/test_gpu_count_many.py run <devices> <host_index | no_index>
prints the number of answers compared and OK."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import column_model as cm
import qpelib as q
import shard_matrix as sm

pq = q.pq
SET_CHAIN = [("risk_level", ">=", "5")]                          # the inner WHERE of the value set over user_name
SEVEN_IDS = [("user_id", "=", str(1000 + 3 * i)) for i in range(7)]


def ladder(items, op="OR"):
    out = []
    for it in items:
        out += [it, op]
    return out[:-1]


def chains_of(set_items):
    """The chains of one call; set_items: the IN SET / NOT IN SET items of a live value set, or () after a writer (the set is
    stale then, and a chain that names it fails the whole call, which run() checks)."""
    r = sm.ROUTES
    fusable = [
        [("sudo_used", "=", "TRUE")],
        [("risk_level", ">", "3")], [("risk_level", "<=", "3")],                                  # one leaf, both polarities
        [("risk_level", ">=", "4")],                                                              # the same window as `> 3`
        [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">=", "4")],
        [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">=", "4"), "AND", ("user_name", "=", "student7")],
        [("exit_code", "!=", "0"), "AND", ("host_name", "=", "host-007")],
        [("exit_code", "!=", "0"), "AND", ("host_name", "=", "host-007")],                        # a duplicate
        [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student30")],
        [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student31")],
        [("user_name", "LIKE", "student1%")],                                                     # a prefix: one window
        [("user_name", "IN", pq.in_list(["student5", "student50"]))],                             # two windows
        [("command_id", ">=", str(1 << 63))],
        [("command_id", "<", "2000"), "OR", [("shell_type", "=", "fish"), "AND", ("base_command", "=", "vim")]],
        [("timestamp", "<", sm.stamp(100).decode())],
        [("exit_code", "=", str(sm.INT32_MIN)), "OR", ("exit_code", "=", str(sm.INT32_MAX))],
        ladder(SEVEN_IDS[:6]),                                                                    # six comparisons: still fused
        [("host_name", ">=", "host-200"), "AND", [("shell_type", "!=", "sh"), "OR", ("sudo_used", "=", "TRUE")]],
        [("risk_level", "=", str(sm.TIE))],
        [("base_command", "<=", "grep")],
    ]
    routed = [
        ladder(SEVEN_IDS),                                                                        # seven comparisons: alone
        ladder(SEVEN_IDS + [("risk_level", "=", "9"), ("shell_type", "=", "zsh")]),
        [("user_name", "IN", pq.in_list(sm.SEVEN))],                                              # fragmented: a member pass
        [("user_name", "LIKE", "%7")],
        [("user_name", "LIKE", "%7"), "AND", ("sudo_used", "=", "TRUE")],
        [("raw_command", "=", sm.RAW.decode())], [("raw_command", "!=", sm.RAW.decode())],       # constants: true, false
        [("working_directory", "=", "/nowhere"), "OR", ("raw_command", "<", "a")],
        [("no_such_column", "=", "1")],                                                           # counts nothing, as COUNT does
        [("no_such_column", "=", "1"), "OR", ("risk_level", ">", "3")],
        None,
    ]
    sets = [[set_items[0]], [set_items[1], "AND", ("risk_level", "<", "5")]] if set_items else []
    return fusable + [chain for chain, _, _, _ in r.values()] + routed + sets


def model_counts(model, chains, sets):
    return [int(np.count_nonzero(model.mask(cm.resolve_sets(chain, sets)))) for chain in chains]


def check_call(eng, model, chains, sets, note):
    want = model_counts(model, chains, sets)
    got = eng.count_many(chains)
    assert got == want, (note, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])
    single = [eng.count(chain) for chain in chains]
    assert single == want, (note, "COUNT itself", [(i, g, w) for i, (g, w) in enumerate(zip(single, want)) if g != w])
    return len(chains)


def raw_call(eng, chains, fill=-7):
    """executeQueryCountManyHIP itself: -> (return value, the counts array as the call left it)."""
    lists = [pq.WhereList(chain) for chain in chains]
    W = C.POINTER(pq.WhereClause)
    ptrs = (W * max(1, len(lists)))()
    for i, wl in enumerate(lists):
        if wl.head is not None:
            ptrs[i] = C.pointer(wl.head)
    counts = (C.c_longlong * max(1, len(lists)))(*([fill] * max(1, len(lists))))
    return pq.lib().executeQueryCountManyHIP(eng.e, ptrs, len(lists), counts), list(counts)


def launches_of(eng, call):
    L = pq.lib()
    assert L.hipEngineKernelTiming(eng.e, 1) == 0
    try:
        call()
        scan, query, n = C.c_double(), C.c_double(), C.c_int()
        assert L.hipEngineKernelTime(eng.e, C.byref(scan), C.byref(query), C.byref(n)) == 0
    finally:
        assert L.hipEngineKernelTiming(eng.e, 0) == 0
    return n.value


def run(devices, config):
    n_shards = len(devices.split(","))
    indexes = sm.INDEX_CONFIGS[config]
    columns = sm.table()
    model = cm.ColumnModel(columns, n_shards)
    eng = pq.HipEngine.from_columns(sm.N, columns, indexes)
    compared = 0
    try:
        assert eng.shards() == model.shard_rows
        vs = eng.value_set("user_name", SET_CHAIN)
        keys = model.value_set("user_name", model.scan_rows(SET_CHAIN))[0]
        assert vs.members == len(keys) and 0 < len(keys) < 300
        set_items = (vs.item(), vs.item(negate=True))
        sets = {str(vs.id): keys}
        chains = chains_of(set_items)
        assert 40 <= len(chains) <= 50
        # what the call is made of: more fused chains than one batch takes, and every other route
        plans = [pq.compile_plan_sets(sm.spec_of(model.m), chain) for chain in chains_of(())]       # (the chains in front of the set's)
        fused = [p for p in plans if len(p) == 1 and p[0][2] is None and 1 <= p[0][0].n_leaves <= pq.TT_LEAVES]
        assert len(fused) > 2 * pq.COUNT_MANY_MAX - 8 and sum(len(p) > 1 for p in plans) >= 5
        assert sum(len(p) == 1 and p[0][0].n_leaves > pq.TT_LEAVES for p in plans) >= 2
        assert sum(len(p) == 1 and p[0][0].n_leaves == 0 for p in plans) >= 4
        compared += check_call(eng, model, chains, sets, "untouched")
        assert eng.count_many([]) == []
        assert raw_call(eng, []) == (0, [-7])
        assert eng.count_many([None]) == [sm.N]
        # a clause that does not compile fails the call and leaves the counts alone
        for bad in ([("risk_level", "IN", "(1, 2")], [("shell_type", "LIKE", "%sh"), "AND", ("risk_level", "LIKE", "1%")]):
            rc, left = raw_call(eng, chains[:5] + [bad] + chains[5:8])
            assert rc == -1 and left == [-7] * 9, (bad, rc, left)
        assert raw_call(eng, chains[:3]) == (3, model_counts(model, chains[:3], sets))
        L = pq.lib()
        W = C.POINTER(pq.WhereClause)
        one = (C.c_longlong * 1)(-7)
        assert L.executeQueryCountManyHIP(None, (W * 1)(), 1, one) == -1 and L.executeQueryCountManyHIP(eng.e, (W * 1)(), 1, None) == -1
        assert L.executeQueryCountManyHIP(eng.e, (W * 1)(), -1, one) == -1 and L.executeQueryCountManyHIP(eng.e, None, 1, one) == -1 and one[0] == -7
        if n_shards == 1:
            sixteen = chains[:pq.COUNT_MANY_MAX]
            assert all(p in fused for p in plans[:pq.COUNT_MANY_MAX])
            assert launches_of(eng, lambda: eng.count_many(sixteen)) == 1, "one launch for sixteen fused chains, not sixteen"
            assert launches_of(eng, lambda: [eng.count(chain) for chain in sixteen]) == pq.COUNT_MANY_MAX
            assert launches_of(eng, lambda: eng.count_many(chains[:pq.COUNT_MANY_MAX + 1])) == 2
        # the writers
        batch = sm.rows_like(41, 9, 9_000_000)
        assert eng.insert_rows(cm.ColumnModel(batch).records()) == 41
        model.insert_batch(batch)
        eng.n = eng.e.contents.num_records
        assert eng.n == model.n == sm.N + 41 and eng.shards() == model.shard_rows
        rc, left = raw_call(eng, [chains[0], [set_items[0]]])
        assert rc == -1 and left == [-7, -7], "the set is stale after a writer: the clause fails to compile"
        chains = chains_of(())
        compared += check_call(eng, model, chains, {}, "after insert_rows")
        update = ({"risk_level": 4, "user_name": "student7", "sudo_used": True}, [("exit_code", "=", "2"), "AND", ("shell_type", "=", "fish")])
        assert eng.update(*update) == model.update(*update) > 0
        compared += check_call(eng, model, chains, {}, "after UPDATE")
        where = [("risk_level", "=", "2"), "OR", ("host_name", "<", "host-040")]
        rs = L.executeQueryDeleteHIP(eng.e, b"commands", pq.WhereList(where).ptr)
        assert rs.contents.success and rs.contents.numRecords == model.delete(where) > 500
        L.freeResultSet(rs)
        assert eng.shards() == model.shard_rows
        compared += check_call(eng, model, chains, {}, "after DELETE")
        vs.free()
    finally:
        eng.close()
    print("COMPARED", compared, "OK", flush=True)


def drive(devices, config, **env):
    p = subprocess.run([sys.executable, __file__, "run", devices, config], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PQPS_DEVICES=devices, **env), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["OK"], (devices, config, p.stdout[-3000:], p.stderr[-3000:])
    return int(p.stdout.split()[-2])


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(sm.INDEX_CONFIGS))
@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_one_call_of_every_route(devices, config):
    assert drive(devices, config) == len(chains_of((0, 0))) + 3 * len(chains_of(()))


@pytest.mark.gpu
def test_with_bool_indexes_probed():
    """PQPS_PROBE_BOOL=1 changes the ID answers of index mode, never a COUNT."""
    assert drive("0,0,0", "host_index", PQPS_PROBE_BOOL="1") > 150


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
            for chains in ([None], [[("risk_level", ">", "3")], [("sudo_used", "=", "TRUE")]]):
                try:
                    eng.count_many(chains)
                except pq.PqpsError:
                    n += 1
            assert eng.count_many([]) == []
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


def test_the_call_mixes_every_route():
    """CPU: the chains of the call against the plans the compiler gives them over the table's dictionaries."""
    model = cm.ColumnModel(sm.table(), 3)
    chains = chains_of(())
    plans = [pq.compile_plan_sets(sm.spec_of(model.m), chain) for chain in chains]
    one_pass = [p[0][0] for p in plans if len(p) == 1]
    assert sum(1 <= p.n_leaves <= pq.TT_LEAVES for p in one_pass) > pq.COUNT_MANY_MAX
    assert sum(p.n_leaves > pq.TT_LEAVES for p in one_pass) >= 2 and sum(p.n_leaves == 0 for p in one_pass) >= 4
    assert sum(any(member is not None for _, _, member in p) for p in plans) >= 4 and sum(len(p) == 2 and p[0][2] is None for p in plans) >= 1
    want = model_counts(model, chains, {})
    assert want[1] + want[2] == sm.N and want[1] == want[3] and want[6] == want[7] and want[-1] == sm.N and want[-3] == 0
    assert sum(0 < w < sm.N for w in want) > 30


if __name__ == "__main__":
    assert sys.argv[1] == "run"
    os.environ["PQPS_DEVICES"] = sys.argv[2]
    run(sys.argv[2], sys.argv[3])
