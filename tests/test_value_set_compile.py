"""IN SET / NOT IN SET in engine/hip/hipPredicate.c (hipCompileWherePlanSets) and the HAVING helper (hipCompileHaving), on the
CPU.  The set table is handed to the compiler as the engine hands it over; a compiled plan is evaluated with the numpy model of
the filter kernel, a set's member pass from a bitmap made here, and compared with plain Python sets."""
import ctypes as C

import numpy as np
import pytest

import kernel_model as km
import qpelib as q
import test_member_compile as tm

pq = q.pq
SPEC, ROWS, USERS = tm.SPEC, tm.ROWS, tm.USERS
I32, DICT = pq.KIND_I32, pq.KIND_DICT

# the sets the chains below may name: values of B in bin space (code, or value - base)
USER_SET = {1, 5, 64, len(USERS) - 1}
RISK_SET = {0, 2, 3}                                   # risk_level values 1, 3, 4 over base 1
SETS = [
    dict(id=7, column="user_name", kind=DICT, base=0, n_bits=len(USERS), members=len(USER_SET), bins=USER_SET),
    dict(id=9, column="risk_level", kind=I32, base=1, n_bits=4, members=len(RISK_SET), bins=RISK_SET),
    dict(id=11, column="exit_code", kind=I32, base=(-3) & 0xFFFFFFFF, n_bits=40, members=3, bins={0, 3, 39}),   # -3, 0, 36
    dict(id=12, column="user_name", kind=DICT, base=0, n_bits=len(USERS), members=0, bins=set()),
    dict(id=13, column="user_name", kind=DICT, base=0, n_bits=len(USERS), members=len(USERS), bins=set(range(len(USERS)))),
    dict(id=14, column="risk_level", kind=I32, base=0, n_bits=6, members=2, bins={0, 5}, stale=1),
    dict(id=15, column="host_name", kind=DICT, base=0, n_bits=len(tm.HOSTS), members=1, bins={0}),
]
BY_ID = {d["id"]: d for d in SETS}


def words_of(d):
    w = [0] * ((d["n_bits"] + 31) // 32)
    for b in d["bins"]:
        w[b >> 5] |= 1 << (b & 31)
    return w


def plan_mask(chain, sets=SETS):
    """-> (mask of the rows the plan selects, the passes); a set's member pass takes the words of the set it names."""
    passes = pq.compile_plan_sets(SPEC, chain, sets=sets)
    flags = []
    for pred, ids, member in passes:
        if member is not None:
            if member["set"]:
                assert member["words"] == [] and member["form"] == pq.MEMBER_BITMAP
                member = dict(member, words=words_of(BY_ID[member["set"]]))
            mask = tm.member_mask(member, ROWS)
        else:
            mask = km.evaluate(pred, [flags[i - pq.MAX_COLUMNS] if i >= pq.MAX_COLUMNS else ROWS[pq.COLUMNS[i]] for i in ids])
        if isinstance(mask, bool):
            mask = np.full(tm.N_ROWS, mask)
        flags.append(np.asarray(mask).astype(np.uint8))
    return flags[-1].astype(bool), passes


def in_set(attribute, d):
    """the rows whose value of `attribute` is in set d, by plain Python"""
    base = d["base"] - (1 << 32) if d["kind"] == I32 and d["base"] >= 1 << 31 else d["base"]
    values = {b + base for b in d["bins"]}
    return np.array([int(v) in values for v in ROWS[attribute]])


def test_in_set_is_a_member_pass_with_the_sets_shape():
    mask, passes = plan_mask([("user_name", "IN SET", "7")])
    assert len(passes) == 2
    member = passes[0][2]
    assert member["set"] == 7 and member["column"] == pq.COL["user_name"] and member["form"] == pq.MEMBER_BITMAP
    assert member["base"] == 0 and member["n_bits"] == len(USERS) and member["words"] == []
    pred, ids, none = passes[1]
    assert none is None and ids == [pq.MAX_COLUMNS] and pred.n_leaves == 1
    assert (pred.leaf[0].lo, pred.leaf[0].span, pred.leaf[0].negate) == (1, 0, 0)
    assert np.array_equal(mask, in_set("user_name", BY_ID[7])) and mask.any() and not mask.all()


def test_not_in_set_negates_the_leaf():
    mask, passes = plan_mask([("user_name", "NOT IN SET", "7")])
    assert passes[0][2]["set"] == 7 and passes[1][0].leaf[0].negate == 1
    assert np.array_equal(mask, ~in_set("user_name", BY_ID[7]))


def test_i32_set_carries_its_base_and_bits():
    mask, passes = plan_mask([("risk_level", "IN SET", "9")])
    member = passes[0][2]
    assert (member["set"], member["base"], member["n_bits"], member["column"]) == (9, 1, 4, pq.COL["risk_level"])
    assert np.array_equal(mask, in_set("risk_level", BY_ID[9]))
    mask, passes = plan_mask([("exit_code", "IN SET", "11")])
    assert passes[0][2]["base"] == (-3) & 0xFFFFFFFF
    assert np.array_equal(mask, in_set("exit_code", BY_ID[11])) and mask.any()


def test_i32_set_on_another_i32_column():
    """exit_code spans [INT_MIN, INT_MAX] in the rows: values below and above risk_level's range are no members"""
    mask, passes = plan_mask([("exit_code", "IN SET", "9")])
    assert passes[0][2]["column"] == pq.COL["exit_code"] and passes[0][2]["set"] == 9
    assert np.array_equal(mask, in_set("exit_code", BY_ID[9])) and mask.any()
    mask, _ = plan_mask([("user_id", "NOT IN SET", "9")])
    assert mask.all()


def test_two_sets_make_two_member_passes():
    chain = [("user_name", "IN SET", "7"), "OR", ("risk_level", "IN SET", "9"), "AND", ("sudo_used", "=", "true")]
    mask, passes = plan_mask(chain)
    assert [p[2]["set"] for p in passes[:-1]] == [7, 9] and passes[-1][2] is None
    want = in_set("user_name", BY_ID[7]) | (in_set("risk_level", BY_ID[9]) & (ROWS["sudo_used"] == 1))
    assert np.array_equal(mask, want)


def test_set_inside_a_sub_chain_and_beside_a_fragmented_in():
    odd = pq.in_list([u.decode() for u in USERS[1::2]])
    chain = [("risk_level", ">", "2"), "AND", [("user_name", "NOT IN SET", "7"), "OR", ("user_name", "IN", odd)]]
    mask, passes = plan_mask(chain)
    assert sorted(p[2]["set"] for p in passes[:-1]) == [0, 7]
    want = (ROWS["risk_level"] > 2) & (~in_set("user_name", BY_ID[7]) | (ROWS["user_name"] % 2 == 1))
    assert np.array_equal(mask, want)


def test_more_than_32_leaves_around_a_set():
    chain = []
    for k in range(40):
        chain += [("exit_code", "=", str(k)), "OR"]
    chain += [("user_name", "IN SET", "7")]
    mask, passes = plan_mask(chain)
    assert len(passes) > 2 and passes[0][2]["set"] == 7
    want = ((ROWS["exit_code"] >= 0) & (ROWS["exit_code"] < 40)) | in_set("user_name", BY_ID[7])
    assert np.array_equal(mask, want)


def test_empty_and_whole_sets_fold_to_constants():
    for chain, want in (([("user_name", "IN SET", "12")], False), ([("user_name", "NOT IN SET", "12")], True),
                        ([("user_name", "IN SET", "13")], True), ([("user_name", "NOT IN SET", "13")], False)):
        mask, passes = plan_mask(chain)
        assert len(passes) == 1 and passes[0][2] is None and passes[0][0].n_leaves == 0
        assert mask.all() == want and mask.any() == want


@pytest.mark.parametrize("chain, word", [
    ([("user_name", "IN SET", "8")], "does not exist"),                  # unknown id
    ([("user_name", "IN SET", "0")], "decimal id"),
    ([("user_name", "IN SET", "7x")], "decimal id"),
    ([("user_name", "IN SET", "")], "decimal id"),
    ([("risk_level", "IN SET", "14")], "stale"),
    ([("host_name", "IN SET", "7")], "another column"),                  # a string set on another string column
    ([("user_name", "IN SET", "15")], "another column"),
    ([("user_name", "IN SET", "9")], "another column"),                  # an i32 set on a string column
    ([("risk_level", "IN SET", "7")], "another column"),
    ([("command_id", "IN SET", "9")], "command_id"),
    ([("sudo_used", "NOT IN SET", "9")], "sudo_used"),
    ([("risk_level", "=", "1"), "AND", [("exit_code", "=", "0"), "OR", ("user_name", "NOT IN SET", "8")]], "does not exist"),
])
def test_refusals(chain, word):
    with pytest.raises(pq.PqpsError, match=word):
        pq.compile_plan_sets(SPEC, chain, sets=SETS)


def test_compilers_without_a_set_table_refuse_set_nodes():
    for op in ("IN SET", "NOT IN SET"):
        with pytest.raises(pq.PqpsError):
            pq.compile_plan_sets(SPEC, [("user_name", op, "7")])            # hipCompileWherePlan
        with pytest.raises(pq.PqpsError):
            pq.compile_where(SPEC, [("user_name", op, "7")])                 # hipCompileWhere
        with pytest.raises(pq.PqpsError):
            pq.compile_plan_sets(SPEC, [("user_name", op, "7")], sets=[])
    # and a chain without set nodes compiles the same with and without a table
    chain = [("risk_level", ">", "2"), "AND", ("user_name", "LIKE", "student1%")]
    a, b = pq.compile_plan_sets(SPEC, chain), pq.compile_plan_sets(SPEC, chain, sets=SETS)
    assert len(a) == len(b) and all(bytes(x[0]) == bytes(y[0]) and x[1] == y[1] for x, y in zip(a, b))


def test_set_operator_spellings():
    L = pq.lib()
    for op in (b"IN SET", b"NOT IN SET", b"IN", b"LIKE"):
        assert L.hipIsSetOperator(op) == 1
    for op in (b"in set", b"IN  SET", b"INSET", b"NOT IN SET ", b"="):
        assert L.hipIsSetOperator(op) == 0


# ---- hipCompileHaving ---------------------------------------------------------------------------------------------
U64, TOP = pq.KIND_U64, pq.TOP_BY
M63 = 1 << 63


def having(agg, kind, op, const):
    out = pq.Having()
    rc = pq.lib().hipCompileHaving(TOP[agg], kind, op.encode(), const.encode(), C.byref(out))
    return None if rc != 0 else (out.field, out.op, out.constant, out.value_signed)


def test_having_compiles():
    assert [having("count", -1, op, "3")[1] for op in ("=", "!=", "<", ">", "<=", ">=")] == [0, 1, 2, 3, 4, 5]
    assert having("count", -1, ">=", "3") == (0, 5, 3, 0)
    assert having("count", I32, "=", " +18446744073709551615") == (0, 0, 2**64 - 1, 0)
    assert having("sum", I32, "<", "-1") == (1, 2, 2**64 - 1, 1)
    assert having("sum", I32, "<", "-9223372036854775808") == (1, 2, M63, 1)
    assert having("sum", I32, ">", "9223372036854775807") == (1, 3, M63 - 1, 1)
    assert having("sum", U64, ">", "18446744073709551615") == (1, 3, 2**64 - 1, 0)
    assert having("min", I32, "<=", "-2147483648") == (2, 4, ((-2**31) & (2**64 - 1)) ^ M63, 0)
    assert having("max", I32, ">=", "2147483647") == (3, 5, (2**31 - 1) ^ M63, 0)
    assert having("max", I32, ">=", "0") == (3, 5, M63, 0)
    assert having("min", U64, "=", "5") == (2, 0, 5, 0)


@pytest.mark.parametrize("agg, kind, op, const", [
    ("count", -1, "=", "-1"), ("count", -1, "=", ""), ("count", -1, "=", " "), ("count", -1, "=", "3 "), ("count", -1, "=", "3x"),
    ("count", -1, "=", "0x10"), ("count", -1, "=", "18446744073709551616"), ("count", -1, "==", "3"), ("count", -1, "<>", "3"),
    ("count", -1, "", "3"), ("sum", I32, "<", "9223372036854775808"), ("sum", I32, "<", "-9223372036854775809"),
    ("sum", I32, "<", "--1"), ("sum", I32, "<", "+"), ("sum", U64, "<", "-1"), ("min", U64, "<", "-0"), ("sum", -1, "<", "1"),
    ("sum", pq.KIND_DICT, "<", "1"), ("max", pq.KIND_BOOL, "<", "1"), ("key", I32, "<", "1"),
])
def test_having_refusals(agg, kind, op, const):
    assert having(agg, kind, op, const) is None
