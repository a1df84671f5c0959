"""hipCountManyPack (engine/hip/hipPredicate.c): the batches of "several COUNT(*), one scan", checked on the CPU.

Chains are compiled by hipCompileWherePlan, packed, and every batch is evaluated with the numpy model of the new kernel
(count_many_model: hit masks per shared leaf, then the programs backwards).  Each query's mask must equal
kernel_model.evaluate of its OWN predicate over its own columns -- the model the rest of the suite trusts."""
import ctypes as C
import random

import numpy as np
import pytest

import count_many_model as cm
import kernel_model as km
import qpelib as q
from test_member_compile import HOSTS, ROWS, SHELLS, SPEC, TEXT, USERS

pq = q.pq
N = len(ROWS["command_id"])


def atoms(rng):
    """One random comparison; the pools are small so that chains share windows."""
    kind = rng.randrange(9)
    op = rng.choice(["=", "!=", "<", "<=", ">", ">="])
    if kind == 0:
        return ("risk_level", op, str(rng.choice([1, 3, 3, 4])))
    if kind == 1:
        return ("exit_code", op, str(rng.choice([-1, 0, 0, 127])))
    if kind == 2:
        return ("user_id", op, str(rng.choice([1500, 2000, 2999])))
    if kind == 3:
        return ("command_id", op, str(rng.choice([0, 2000, 2**63])))
    if kind == 4:
        return ("sudo_used", rng.choice(["=", "!="]), rng.choice(["TRUE", "FALSE"]))
    if kind == 5:
        return ("host_name", op, rng.choice(HOSTS[:4]).decode())
    if kind == 6:
        return ("shell_type", rng.choice(["=", "!="]), rng.choice(SHELLS).decode())
    if kind == 7:
        return ("user_name", op, rng.choice(USERS[5:8]).decode())
    return ("risk_level", "IN", "(1, 4)")


def random_chain(rng, depth=0):
    n = rng.choice([1, 1, 2, 2, 3])
    chain = []
    for i in range(n):
        if i:
            chain.append(rng.choice(["AND", "OR"]))
        chain.append(random_chain(rng, depth + 1) if depth < 1 and rng.random() < 0.3 else atoms(rng))
    return chain


def one_pass(chain):
    passes = pq.compile_plan(SPEC, chain)
    assert len(passes) == 1
    return passes[0]


def own_mask(pred, ids):
    m = km.evaluate(pred, [ROWS[pq.COLUMNS[i]] for i in ids])
    return np.full(N, m) if isinstance(m, bool) else m


def check_pack(queries, max_queries=pq.COUNT_MANY_MAX):
    """Packs, checks the shape of every batch, evaluates it, compares with every query's own predicate.  -> (batches, places)"""
    batches, places = pq.count_many_pack(queries, max_queries)
    masks = []
    for prog, ids in batches:
        assert 1 <= prog.n_queries <= max_queries and prog.n_leaves <= pq.MAX_LEAVES and prog.n_columns == len(ids) <= pq.MAX_COLUMNS
        assert ids == sorted(set(ids)), "the batch's columns are a union without repeats"
        keys = [(prog.leaf[k].column, prog.leaf[k].lo, prog.leaf[k].span) for k in range(prog.n_leaves)]
        assert keys == sorted(set(keys)), "distinct leaves, sorted by column slot"
        assert all(prog.leaf[k].negate == 0 for k in range(prog.n_leaves))
        used_leaves = {prog.query[i].leaf[s] for i in range(prog.n_queries) for s in range(prog.query[i].n_steps)}
        assert used_leaves == set(range(prog.n_leaves)), "no leaf without a query"
        assert {prog.leaf[k].column for k in range(prog.n_leaves)} == set(range(prog.n_columns)), "no column without a leaf"
        masks.append(cm.evaluate(prog, [ROWS[pq.COLUMNS[i]] for i in ids], N))
    at = 0                                                       # greedy, in the caller's order: batch numbers never go back
    seen = {}
    for i, ((pred, ids), (batch, pos)) in enumerate(zip(queries, places)):
        if pred.n_leaves == 0:
            assert (batch, pos) == (pq.COUNT_CONSTANT, pred.truth & 1)
        elif pred.n_leaves > pq.TT_LEAVES:
            assert (batch, pos) == (pq.COUNT_ALONE, 0)
        else:
            assert at <= batch <= at + 1 and batch < len(batches)
            at = batch
            assert pos == seen.get(batch, 0), "positions in order of arrival"
            seen[batch] = pos + 1
            assert batches[batch][0].query[pos].n_steps == pred.n_leaves
            assert np.array_equal(masks[batch][pos], own_mask(pred, ids)), f"query {i}"
    assert all(seen.get(b, 0) == prog.n_queries for b, (prog, _) in enumerate(batches))
    return batches, places


def test_forty_mixed_chains():
    rng = random.Random(0xC0047)
    chains = [random_chain(rng) for _ in range(40)]
    chains[7] = None                                             # no WHERE: the constant true
    chains[11] = [("timestamp", "!=", "nothing")]                # a single-valued column folds
    queries = [one_pass(c) for c in chains]
    assert any(p.n_leaves == 0 for p, _ in queries) and any(p.n_leaves >= 3 for p, _ in queries)
    batches, places = check_pack(queries)
    assert len(batches) >= 2
    # the same list with a lower cap: more batches, the same answers
    small, _ = check_pack(queries, 4)
    assert len(small) > len(batches) and all(prog.n_queries <= 4 for prog, _ in small)


def test_both_polarities_share_one_leaf():
    batches, places = check_pack([one_pass([("risk_level", ">", "3")]), one_pass([("risk_level", "<=", "3")])])
    (prog, ids), = batches
    assert prog.n_leaves == 1 and prog.n_queries == 2 and ids == [pq.COL["risk_level"]]
    a, b = prog.query[0], prog.query[1]
    assert (a.on_true[0], a.on_false[0]) == (b.on_false[0], b.on_true[0]) and {a.on_true[0], a.on_false[0]} == {pq.ACCEPT, pq.REJECT}
    m = cm.evaluate(prog, [ROWS["risk_level"]])
    assert np.array_equal(m[0], ROWS["risk_level"] > 3) and np.array_equal(m[1], ROWS["risk_level"] <= 3)


def test_one_window_on_two_columns_is_two_leaves():
    batches, _ = check_pack([one_pass([("risk_level", "=", "2")]), one_pass([("exit_code", "=", "2")])])
    (prog, ids), = batches
    assert prog.n_leaves == 2 and prog.n_columns == 2
    assert (prog.leaf[0].lo, prog.leaf[0].span) == (prog.leaf[1].lo, prog.leaf[1].span) and prog.leaf[0].column != prog.leaf[1].column


def test_a_duplicate_clause_is_two_queries_over_the_same_leaves():
    chain = [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">=", "4")]
    batches, places = check_pack([one_pass(chain), one_pass(chain)])
    (prog, _), = batches
    assert prog.n_queries == 2 and prog.n_leaves == 2 and places == [(0, 0), (0, 1)]
    assert bytes(prog.query[0]) == bytes(prog.query[1])


def test_the_17th_query_opens_a_batch():
    queries = [one_pass([("risk_level", "=", str(i % 3))]) for i in range(17)]
    batches, places = check_pack(queries)
    assert [prog.n_queries for prog, _ in batches] == [16, 1]
    assert places[15] == (0, 15) and places[16] == (1, 0)


def test_the_33rd_distinct_leaf_opens_a_batch():
    # eleven queries of three new windows each: 33 distinct leaves
    queries = [one_pass([("user_id", "=", str(1000 + 3 * i)), "OR", ("user_id", "=", str(1001 + 3 * i)), "OR", ("user_id", "=", str(1002 + 3 * i))])
               for i in range(11)]
    batches, places = check_pack(queries)
    assert [(prog.n_queries, prog.n_leaves) for prog, _ in batches] == [(10, 30), (1, 3)]
    # ... while a query that brings no new leaf still fits the full batch
    queries = queries[:10] + [one_pass([("user_id", "=", "1000"), "OR", ("user_id", "=", "1001")])] * 2 + queries[10:]
    batches, places = check_pack(queries)
    assert [(prog.n_queries, prog.n_leaves) for prog, _ in batches] == [(12, 30), (1, 3)]
    # exactly 32: 8 queries of 4
    queries = [one_pass([("exit_code", "=", str(8 * i + j)) if j % 2 == 0 else "OR" for j in range(7)]) for i in range(8)]
    batches, _ = check_pack(queries)
    assert [(prog.n_queries, prog.n_leaves) for prog, _ in batches] == [(8, 32)]


def test_a_seven_leaf_query_is_alone_and_constants_are_reported():
    seven = []
    for i in range(7):
        seven += [("exit_code", "=", str(i)), "OR"]
    queries = [one_pass(seven[:-1]), one_pass(None), one_pass([("timestamp", "=", "nothing")]), one_pass([("risk_level", "<", "2")]),
               one_pass(seven[:-3])]
    assert [p.n_leaves for p, _ in queries] == [7, 0, 0, 1, 6]
    batches, places = check_pack(queries)
    assert places == [(pq.COUNT_ALONE, 0), (pq.COUNT_CONSTANT, 1), (pq.COUNT_CONSTANT, 0), (0, 0), (0, 1)]
    assert len(batches) == 1
    # nothing to launch at all
    assert pq.count_many_pack([queries[0], queries[1]]) == ([], [(pq.COUNT_ALONE, 0), (pq.COUNT_CONSTANT, 1)])
    assert pq.count_many_pack([]) == ([], [])


def test_every_multi_valued_column_in_one_union():
    names = ["command_id", "exit_code", "user_id", "risk_level", "sudo_used", "raw_command", "host_name", "user_name", "shell_type",
             "base_command"]
    queries = [one_pass([(name, "!=", "0" if pq.COLUMN_KIND[pq.COL[name]] != pq.KIND_DICT else TEXT[name][1].decode("latin-1"))]) for name in names]
    batches, _ = check_pack(queries)
    (prog, ids), = batches
    assert ids == sorted(pq.COL[name] for name in names)


def _raw_pack(n, arr, cap, batches, nb, places):
    return pq.lib().hipCountManyPack(arr, n, cap, batches, nb, places)


def test_refusals_leave_the_outputs_alone():
    pred, ids = one_pass([("risk_level", ">", "3"), "AND", ("sudo_used", "=", "TRUE")])
    cid = (C.c_int * pq.MAX_COLUMNS)(*(ids + [-1] * (pq.MAX_COLUMNS - len(ids))))
    arr = (pq.CountPackQuery * 1)()
    arr[0].pred, arr[0].column_ids = C.pointer(pred), C.cast(cid, C.POINTER(C.c_int))
    batches, places, nb = (pq.CountBatch * 1)(), (pq.CountPlace * 1)(), C.c_int(77)
    C.memset(batches, 0xAB, C.sizeof(batches))
    C.memset(places, 0xCD, C.sizeof(places))
    before = bytes(batches), bytes(places)

    def refused(rc):
        assert rc == -1 and nb.value == 77 and (bytes(batches), bytes(places)) == before

    refused(_raw_pack(1, None, 16, batches, C.byref(nb), places))
    refused(_raw_pack(1, arr, 16, None, C.byref(nb), places))
    refused(_raw_pack(1, arr, 16, batches, None, places))
    refused(_raw_pack(1, arr, 16, batches, C.byref(nb), None))
    refused(_raw_pack(-1, arr, 16, batches, C.byref(nb), places))
    refused(_raw_pack(1, arr, 0, batches, C.byref(nb), places))
    refused(_raw_pack(1, arr, 17, batches, C.byref(nb), places))
    arr[0].pred = None
    refused(_raw_pack(1, arr, 16, batches, C.byref(nb), places))
    arr[0].pred, arr[0].column_ids = C.pointer(pred), None
    refused(_raw_pack(1, arr, 16, batches, C.byref(nb), places))
    arr[0].column_ids = C.cast(cid, C.POINTER(C.c_int))
    for field, step, value in (("on_true", 0, 0), ("on_false", 0, 0), ("on_true", 1, 1), ("on_false", 1, 0), ("on_true", 0, 2), ("order", 1, 2)):
        bad = pq.Predicate()
        C.memmove(C.byref(bad), C.byref(pred), C.sizeof(bad))
        getattr(bad, field)[step] = value                        # a jump backwards, onto itself, past the end; a leaf slot past the end
        arr[0].pred = C.pointer(bad)
        refused(_raw_pack(1, arr, 16, batches, C.byref(nb), places))
    bad = pq.Predicate()
    C.memmove(C.byref(bad), C.byref(pred), C.sizeof(bad))
    bad.leaf[1].column = 2                                       # a column slot the predicate does not have
    arr[0].pred = C.pointer(bad)
    refused(_raw_pack(1, arr, 16, batches, C.byref(nb), places))
    # and the good one goes through
    arr[0].pred = C.pointer(pred)
    assert _raw_pack(1, arr, 16, batches, C.byref(nb), places) == 0 and nb.value == 1 and places[0].batch == 0
    with pytest.raises(ValueError):
        pq.count_many_pack([(pred, ids)], 0)
