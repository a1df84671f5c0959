"""Set predicates (LIKE / NOT LIKE / IN / NOT IN) in engine/hip/hipPredicate.c, checked on the CPU.

What a set node selects is decided by the host compiler; the expected sets here come from Python alone (`re` for LIKE,
sets for IN).  A compiled plan is evaluated with the numpy model of the filter kernel (kernel_model.evaluate); the member
passes of a plan are computed here from the member description compile_plan_sets returns."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import kernel_model as km
import qpelib as q

pq = q.pq
N_ROWS = 2000


# ---- the table: dictionaries + 2 000 random rows ----------------------------------------------------------------
def _raw_dictionary():
    rng = random.Random(0x11CE)
    words = {b"", b"a", b"ab", b"abc", b"abcd", b"a%", b"a_c", b"a\\c", b"a\\", b"\\", b"%", b"_", b"%%", b"a%b%c", b"axbyc",
             b"abxc", b"ac", b"aXc", b"rm -rf /", b"sudo rm -rf /tmp", b"sudo ls", b"sudo ", b"sudo", b"sud", b"100%",
             b"50%_off", b"x_y", b"x\\_y", b"caf\xe9", b"\xe9", b"\xff\xfe", b"a\xffz", b"z", b"zz", b"zzz\xff"}
    alphabet = b"abc%_\\ x\xe9"
    while len(words) < 300:
        words.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 9))))
    return sorted(words)


RAW = _raw_dictionary()
HOSTS = list(pq.SYNTH_HOSTS)
USERS = list(pq.SYNTH_USERS_DICT)
SHELLS = list(pq.SYNTH_SHELLS)
BASES = list(pq.SYNTH_BASES)
TEXT = {"raw_command": RAW, "host_name": HOSTS, "user_name": USERS, "shell_type": SHELLS, "base_command": BASES,
        "timestamp": [pq.SYNTH_CONSTANTS["timestamp"]], "working_directory": [pq.SYNTH_CONSTANTS["working_directory"]]}


def _spec():
    s = pq.SchemaSpec()
    for name, w in (("command_id", 8), ("exit_code", 4), ("user_id", 4), ("risk_level", 4), ("sudo_used", 1)):
        s.set_numeric(name, w)
    for name, w in (("raw_command", 2), ("host_name", 1), ("user_name", 2), ("shell_type", 1), ("base_command", 1),
                    ("timestamp", 1), ("working_directory", 1)):
        s.set_dict(name, w, TEXT[name])
    return s


def _rows():
    rng = np.random.default_rng(0x5E7)
    a = {"command_id": rng.integers(0, 4000, N_ROWS).astype(np.uint64),
         "exit_code": rng.integers(-6, 300, N_ROWS).astype(np.int32),
         "user_id": rng.integers(1000, 3000, N_ROWS).astype(np.int32),
         "risk_level": rng.integers(0, 6, N_ROWS).astype(np.int32),
         "sudo_used": rng.integers(0, 2, N_ROWS).astype(np.uint8),
         "raw_command": rng.integers(0, len(RAW), N_ROWS).astype(np.uint16),
         "host_name": rng.integers(0, len(HOSTS), N_ROWS).astype(np.uint8),
         "user_name": rng.integers(0, len(USERS), N_ROWS).astype(np.uint16),
         "shell_type": rng.integers(0, len(SHELLS), N_ROWS).astype(np.uint8),
         "base_command": rng.integers(0, len(BASES), N_ROWS).astype(np.uint8),
         "timestamp": np.zeros(N_ROWS, dtype=np.uint8), "working_directory": np.zeros(N_ROWS, dtype=np.uint8)}
    a["command_id"][:4] = [0, 2**64 - 1, 2**63, 2**32]
    a["exit_code"][:4] = [-2**31, 2**31 - 1, -1, 0]
    return a


SPEC = _spec()
ROWS = _rows()


# ---- plans through the numpy model --------------------------------------------------------------------------------
def member_mask(member, arrays):
    """What pqps_member_flags computes for one member pass (include/pqps_hip.h)."""
    v = arrays[pq.COLUMNS[member["column"]]]
    if member["form"] == pq.MEMBER_BITMAP:
        assert v.dtype.itemsize < 8 and 0 < member["n_bits"] <= 2**32
        x = v.astype(np.int64) & 0xFFFFFFFF
        idx = (x - member["base"]) & 0xFFFFFFFF
        ok = idx < member["n_bits"]
        words = np.array(member["words"], dtype=np.uint32)
        assert len(words) == (member["n_bits"] + 31) // 32
        safe = np.where(ok, idx, 0)
        return ok & (((words[safe >> 5] >> (safe & 31).astype(np.uint32)) & 1) != 0)
    values = member["values"]
    assert values == sorted(set(values)), "the list is ascending and duplicate-free"
    x = (v.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) if v.dtype == np.int32 else v.astype(np.uint64)
    return np.isin(x, np.array(values, dtype=np.uint64))


def plan_mask(chain, arrays=ROWS, spec=SPEC):
    """-> (bool mask of the rows the compiled plan selects, the passes)."""
    passes = pq.compile_plan_sets(spec, chain)
    n = len(arrays["command_id"])
    flags = []
    for pred, ids, member in passes:
        if member is not None:
            assert pred.n_leaves == 0 and ids == []
            mask = member_mask(member, arrays)
        else:
            assert len(ids) <= pq.MAX_COLUMNS and pred.n_leaves <= pq.MAX_LEAVES
            assert all(i < pq.MAX_COLUMNS + len(flags) for i in ids), "a pass reads the flags of earlier passes only"
            mask = km.evaluate(pred, [flags[i - pq.MAX_COLUMNS] if i >= pq.MAX_COLUMNS else arrays[pq.COLUMNS[i]] for i in ids])
        if isinstance(mask, bool):
            mask = np.full(n, mask)
        flags.append(mask.astype(np.uint8))
    assert passes[-1][2] is None, "the last pass is a filter pass"
    return flags[-1].astype(bool), passes


def pred_bytes(pred):
    return C.string_at(C.byref(pred), C.sizeof(pred))


# ---- the same chains in plain Python --------------------------------------------------------------------------------
def like_regex(pattern: bytes):
    out, i = b"", 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"\\" and pattern[i + 1:i + 2] in (b"%", b"_", b"\\"):
            out += re.escape(pattern[i + 1:i + 2])
            i += 1
        elif c == b"%":
            out += b".*"
        elif c == b"_":
            out += b"."
        else:
            out += re.escape(c)                                  # (a lone or trailing backslash is itself)
        i += 1
    return re.compile(out, re.DOTALL)


_ITEMS = {}                                                      # IN value text -> the Python items it was built from


def IN(attr, items, negate=False):
    text = pq.in_list(items)
    _ITEMS[text] = list(items)
    return (attr, "NOT IN" if negate else "IN", text)


def leaf_mask(leaf, arrays):
    attr, op, value = leaf[:3]
    v = arrays[attr]
    neg = op.startswith("NOT ")
    if op in ("LIKE", "NOT LIKE"):
        rx = like_regex(value.encode("latin-1"))
        per_code = np.array([rx.fullmatch(t) is not None for t in TEXT[attr]])
        return per_code[v] != neg
    if op in ("IN", "NOT IN"):
        items = _ITEMS[value]
        if attr in TEXT:
            want = {t.encode("latin-1") if isinstance(t, str) else t for t in items}
            per_code = np.array([t in want for t in TEXT[attr]])
            return per_code[v] != neg
        if attr == "sudo_used":
            want = {1 if str(t).lower() in ("true", "1") else 0 for t in items}
        else:
            want = {int(t) for t in items}
        return np.array([int(x) in want for x in v]) != neg
    if attr in TEXT:
        lit = value.encode("latin-1")
        x = np.array([(t > lit) - (t < lit) for t in TEXT[attr]])[v]
        y = 0
    elif attr == "sudo_used":
        x, y = v.astype(np.int64), 1 if value.lower() in ("true", "1") else 0
    else:
        x, y = np.array([int(t) for t in v], dtype=object), int(value)
    return np.array({"=": x == y, "!=": x != y, "<": x < y, ">": x > y, "<=": x <= y, ">=": x >= y}[op], dtype=bool)


def chain_mask(chain, arrays=ROWS):
    """evaluateWhereClause: right-recursive, no precedence, nesting via lists."""
    items, ops = chain[0::2], chain[1::2]
    masks = [chain_mask(it, arrays) if isinstance(it, list) else leaf_mask(it, arrays) for it in items]
    acc = masks[-1]
    for m, op in zip(reversed(masks[:-1]), reversed(ops)):
        acc = (m | acc) if op == "OR" else (m & acc)
    return acc


def resolved_codes(attr, op, pattern):
    """The codes of `attr` the compiled `attr op pattern` selects: the plan evaluated on one row per dictionary entry."""
    n = len(TEXT[attr])
    arrays = {attr: np.arange(n, dtype=ROWS[attr].dtype), "command_id": np.zeros(n, dtype=np.uint64)}
    mask, passes = plan_mask([(attr, op, pattern)], arrays)
    return set(np.nonzero(mask)[0].tolist()), passes


# ---- LIKE against re ------------------------------------------------------------------------------------------------------
PATTERNS = ["", "%", "%%", "_", "__", "a%", "%a", "%a%", "a%b%c", "a_c", "a__", "_b%", "%_", "_%", "%_%", "a", "ab", "abc", "abcd",
            "abcde", "ab%", "abc%", "sudo %", "sudo%", "sud_", "sudo rm -rf /tmp", "%rm -rf%", "% %", "\\%", "\\_", "\\\\", "a\\%",
            "a\\_c", "a\\\\c", "a\\\\", "a\\", "\\", "%\\%", "%\\%%", "\\%\\%", "%\\_%", "x\\_y", "x_y", "x\\\\_y", "100\\%", "%\\\\%",
            "caf\xe9", "caf_", "\xe9%", "%\xe9", "\xff%", "\xff\xfe", "a\xff%", "%\xff%", "zzz\xff\xff%", "\xff\xff%", "zzzz%", "zz_",
            "_" * 12, "%" + "_" * 10 + "%", "abcdefghijklmnopqrstuvwxyz", "a%" * 8 + "a", "%a%b%", "%%a%%", "a%c", "a%%c", "_\\%", "\\a"]


@pytest.mark.parametrize("pattern", PATTERNS, ids=[repr(p) for p in PATTERNS])
def test_like_selects_what_re_matches(pattern):
    rx = like_regex(pattern.encode("latin-1"))
    want = {i for i, t in enumerate(RAW) if rx.fullmatch(t)}
    got, _ = resolved_codes("raw_command", "LIKE", pattern)
    assert got == want
    got_not, _ = resolved_codes("raw_command", "NOT LIKE", pattern)
    assert got_not == set(range(len(RAW))) - want


def test_like_patterns_cover_the_interesting_cases():
    hits = {p: sum(like_regex(p.encode("latin-1")).fullmatch(t) is not None for t in RAW) for p in PATTERNS}
    assert hits["%"] == len(RAW) and hits[""] == 1 and hits["\xff\xff%"] == 0 and hits["abcdefghijklmnopqrstuvwxyz"] == 0
    assert 0 < hits["%a%"] < len(RAW) and hits["\\%"] == 1 and hits["a\\"] == 1 and hits["x\\_y"] == 1 and hits["x_y"] >= 1
    assert RAW[-1] < b"\xff\xff", "a literal prefix that sorts past the last dictionary entry"


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def window_of(prefix: bytes):
    codes = [i for i, t in enumerate(RAW) if t.startswith(prefix)]
    assert codes == list(range(codes[0], codes[-1] + 1))
    return codes[0], codes[-1]


@pytest.mark.parametrize("pattern,prefix", [("sudo %", b"sudo "), ("a%", b"a"), ("ab%%", b"ab"), ("\\%%", b"%")])
def test_prefix_pattern_is_one_window_leaf(pattern, prefix):
    passes = pq.compile_plan_sets(SPEC, [("raw_command", "LIKE", pattern)])
    assert len(passes) == 1 and passes[0][2] is None
    pred, ids, _ = passes[0]
    lo, hi = window_of(prefix)
    assert pred.n_leaves == 1 and ids == [pq.COL["raw_command"]]
    assert (pred.leaf[0].lo, pred.leaf[0].span, pred.leaf[0].negate) == (lo, hi - lo, 0)


SCATTERED = {
    "shell_type": ["bash", "zsh"],
    "host_name": [HOSTS[1].decode(), HOSTS[5].decode(), HOSTS[9].decode(), HOSTS[14].decode()],
    "user_name": ["student1007", "student1300", "student2100", "student2999"],
    "risk_level": ["0", "2", "5"],
    "exit_code": ["-1", "1", "127", "130"],
    "command_id": ["3", "77", "1999"],
    "raw_command": [RAW[3].decode("latin-1"), RAW[100].decode("latin-1"), RAW[250].decode("latin-1")],
}


@pytest.mark.parametrize("attr", sorted(SCATTERED))
@pytest.mark.parametrize("negate", [False, True], ids=["in", "not_in"])
def test_in_of_few_values_is_the_or_chain(attr, negate):
    """2, 3 and 4 scattered values: one pass, byte for byte the predicate of the nested chain of = (or of != for NOT IN)."""
    items = SCATTERED[attr]
    for k in range(2, len(items) + 1):
        some = items[:k]
        ladder = []
        for v in some:
            ladder += [(attr, "!=" if negate else "=", v), "AND" if negate else "OR"]
        for shape in (lambda x: [x], lambda x: [("risk_level", ">", "1"), "AND", x, "OR", ("sudo_used", "=", "true")]):
            a = pq.compile_plan_sets(SPEC, shape(IN(attr, some, negate)))
            b = pq.compile_plan_sets(SPEC, shape(ladder[:-1]))
            assert len(a) == 1 and len(b) == 1 and a[0][1] == b[0][1]
            assert pred_bytes(a[0][0]) == pred_bytes(b[0][0])
        alone = pq.compile_plan_sets(SPEC, [IN(attr, some, negate)])[0][0]
        assert alone.n_leaves == k and all(alone.leaf[i].negate == int(negate) for i in range(k))
        # the same predicate through the single-pass entry point
        assert pred_bytes(pq.compile_where(SPEC, [IN(attr, some, negate)])[0]) == pred_bytes(pq.compile_where(SPEC, ladder[:-1])[0])


def test_shell_in_bash_zsh_is_the_handwritten_chain():
    spec = pq.synth_schema()
    a = pq.compile_where(spec, [("sudo_used", "=", "FALSE"), "AND", ("shell_type", "IN", "('bash','zsh')")])
    b = pq.compile_where(spec, [("sudo_used", "=", "FALSE"), "AND", [("shell_type", "=", "bash"), "OR", ("shell_type", "=", "zsh")]])
    assert pred_bytes(a[0]) == pred_bytes(b[0]) and a[1] == b[1]


FIVE = ["student1007", "student1300", "student1650", "student2100", "student2999"]


@pytest.mark.parametrize("negate", [False, True], ids=["in", "not_in"])
def test_five_scattered_values_are_a_member_pass_and_a_flag_leaf(negate):
    passes = pq.compile_plan_sets(SPEC, [IN("user_name", FIVE, negate)])
    assert len(passes) == 2
    member = passes[0][2]
    codes = sorted(USERS.index(v.encode()) for v in FIVE)
    assert member["column"] == pq.COL["user_name"] and member["form"] == pq.MEMBER_BITMAP
    assert member["base"] == codes[0] and member["n_bits"] == codes[-1] - codes[0] + 1
    pred, ids, none = passes[1]
    assert none is None and ids == [pq.MAX_COLUMNS] and pred.n_leaves == 1
    assert (pred.leaf[0].lo, pred.leaf[0].span, pred.leaf[0].negate) == (1, 0, int(negate))
    with pytest.raises(pq.PqpsError, match="member pass"):
        pq.compile_where(SPEC, [IN("user_name", FIVE, negate)])
    mask, _ = plan_mask([IN("user_name", FIVE, negate)])
    assert np.array_equal(mask, np.isin(ROWS["user_name"], codes) != negate)


@pytest.mark.parametrize("negate", [False, True], ids=["in", "not_in"])
def test_a_complement_of_few_runs_gives_windows(negate):
    out = {2, 5, 8, 11}                                          # the set has 5 runs, what it leaves out 4
    items = [h.decode() for i, h in enumerate(HOSTS) if i not in out]
    passes = pq.compile_plan_sets(SPEC, [IN("host_name", items, negate)])
    assert len(passes) == 1
    pred = passes[0][0]
    assert pred.n_leaves == 4
    assert sorted((pred.leaf[i].lo, pred.leaf[i].span, pred.leaf[i].negate) for i in range(4)) == [(c, 0, int(not negate)) for c in sorted(out)]
    mask, _ = plan_mask([IN("host_name", items, negate)])
    assert np.array_equal(mask, np.isin(ROWS["host_name"], sorted(out)) == negate)


def constant_of(chain):
    passes = pq.compile_plan_sets(SPEC, chain)
    assert len(passes) == 1 and passes[0][2] is None and passes[0][0].n_leaves == 0
    return passes[0][0].truth & 1


def test_empty_full_and_single_valued_sets_are_constants():
    assert constant_of([("host_name", "IN", "()")]) == 0 and constant_of([("host_name", "NOT IN", " ( ) ")]) == 1
    assert constant_of([("risk_level", "IN", "()")]) == 0 and constant_of([("command_id", "NOT IN", "()")]) == 1
    assert constant_of([IN("host_name", ["nowhere", "labpc-1"])]) == 0 and constant_of([IN("host_name", ["nowhere"], True)]) == 1
    everything = [h.decode() for h in HOSTS]
    assert constant_of([IN("host_name", everything + everything[:3])]) == 1 and constant_of([IN("host_name", everything, True)]) == 0
    assert constant_of([("raw_command", "LIKE", "%")]) == 1 and constant_of([("raw_command", "NOT LIKE", "%%")]) == 0
    assert constant_of([("raw_command", "LIKE", "\xff\xff%")]) == 0 and constant_of([("raw_command", "NOT LIKE", "zzzz_")]) == 1
    # a column with one value is decided on the host
    assert constant_of([("timestamp", "LIKE", "2025-%")]) == 1 and constant_of([("timestamp", "LIKE", "2026-%")]) == 0
    assert constant_of([("timestamp", "NOT LIKE", "%Z")]) == 0 and constant_of([IN("working_directory", ["/home/u", "/tmp"])]) == 1
    assert constant_of([IN("working_directory", ["/tmp"], True)]) == 1


@pytest.mark.parametrize("items,want", [([], None), (["true"], 1), (["TRUE", "1"], 1), (["false"], 0), (["0", "no"], 0), (["true", "false"], "both"),
                                        (["1", "0", "1"], "both")])
def test_sudo_used_in_never_needs_a_pass(items, want):
    for negate in (False, True):
        chain = [IN("sudo_used", items, negate)]
        passes = pq.compile_plan_sets(SPEC, chain)
        assert len(passes) == 1 and passes[0][2] is None and passes[0][0].n_leaves <= 1
        mask, _ = plan_mask(chain)
        expect = np.zeros(N_ROWS, bool) if want is None else np.ones(N_ROWS, bool) if want == "both" else ROWS["sudo_used"] == want
        assert np.array_equal(mask, expect != negate)


def test_numeric_sets_choose_bitmap_or_list():
    near = [str(v) for v in (1003, 1100, 1500, 1900, 2400, 2998)]
    far = [str(v) for v in (-2**31, -7, 0, 5, 130, 2**31 - 1)]
    ids = [str(v) for v in (0, 5, 77, 1999, 2**32, 2**63, 2**64 - 1)]
    m = pq.compile_plan_sets(SPEC, [IN("user_id", near)])[0][2]
    assert m["form"] == pq.MEMBER_BITMAP and m["base"] == 1003 and m["n_bits"] == 2998 - 1003 + 1
    m = pq.compile_plan_sets(SPEC, [IN("exit_code", far)])[0][2]
    assert m["form"] == pq.MEMBER_LIST and m["values"] == sorted(int(v) & 0xFFFFFFFF for v in far)
    m = pq.compile_plan_sets(SPEC, [IN("exit_code", ["-3", "-1", "1", "3", "5", "7"])])[0][2]
    assert m["form"] == pq.MEMBER_BITMAP and m["base"] == (-3) & 0xFFFFFFFF and m["n_bits"] == 11
    m = pq.compile_plan_sets(SPEC, [IN("command_id", ids)])[0][2]
    assert m["form"] == pq.MEMBER_LIST and m["values"] == sorted(int(v) for v in ids)
    for attr, items in (("user_id", near), ("exit_code", far), ("exit_code", ["-3", "-1", "1", "3", "5", "7"]), ("command_id", ids)):
        for negate in (False, True):
            chain = [IN(attr, items, negate)]
            assert np.array_equal(plan_mask(chain)[0], chain_mask(chain)), (attr, negate)


def test_list_items_quotes_blanks_and_duplicates():
    text = "( 'labpc-01' ,labpc-05,  'labpc-05', 'it''s, (not) a host' , labpc-09 )"
    _ITEMS[text] = ["labpc-01", "labpc-05", "labpc-09"]
    chain = [("host_name", "IN", text)]
    assert np.array_equal(plan_mask(chain)[0], chain_mask(chain))
    assert pq.in_list(["a", b"b\xe9", 7, True, "it's"]) == "('a', 'b\xe9', '7', 'true', 'it''s')"
    assert pq.like_escape("50%_off\\") == "50\\%\\_off\\\\"
    hit, _ = resolved_codes("raw_command", "LIKE", pq.like_escape("50%_off"))
    assert hit == {RAW.index(b"50%_off")}


# ---- planner interplay ------------------------------------------------------------------------------------------------------------------------
def test_thirty_comparisons_and_a_set_of_four_runs():
    rng = random.Random(7)
    chain = []
    for i in range(30):
        attr, op, val = rng.choice([("risk_level", ">", "2"), ("exit_code", "=", "0"), ("user_id", "<", "2000"), ("sudo_used", "=", "true"),
                                    ("shell_type", "!=", "zsh"), ("host_name", ">=", "labpc-05"), ("command_id", "<", "2000"),
                                    ("base_command", "<=", "cmd050"), ("exit_code", ">", str(rng.randint(0, 200)))])
        item = (attr, op, val)
        chain += [[item, "OR", ("risk_level", "=", str(i % 6))] if i % 7 == 3 else item, rng.choice(["AND", "OR"])]
    chain += [IN("user_name", SCATTERED["user_name"])]
    mask, passes = plan_mask(chain)
    assert len(passes) > 1 and all(m is None for _, _, m in passes), "more than 32 leaves: flag passes, no member pass"
    assert np.array_equal(mask, chain_mask(chain)) and 0 < mask.sum() < N_ROWS
    for k in (0, 12, 30):                                         # the set at other places of the chain (items sit at even places)
        moved = chain[:-2]
        moved[k:k] = [IN("user_name", SCATTERED["user_name"], k == 12), "OR" if k else "AND"]
        assert np.array_equal(plan_mask(moved)[0], chain_mask(moved))


def test_ten_member_nodes_in_one_chain():
    rng = random.Random(99)
    users = lambda: [USERS[i].decode() for i in rng.sample(range(len(USERS)), 40)]
    nodes = [IN("user_name", users()), IN("user_name", users(), True), IN("user_name", users()), IN("user_name", FIVE, True),
             IN("command_id", [str(v) for v in range(0, 4000, 9)]), IN("command_id", ["0", "5", "77", "1999", "2001", str(2**64 - 1)], True),
             ("raw_command", "LIKE", "%a%"), ("raw_command", "NOT LIKE", "%\\%%"),
             IN("exit_code", ["-2147483648", "-5", "0", "17", "130", "2147483647"]), IN("user_id", [str(v) for v in range(1000, 3000, 7)])]
    for node in nodes:
        assert pq.compile_plan_sets(SPEC, [node])[0][2] is not None, node[:2]
    chain = [nodes[0], "OR", [nodes[1], "AND", ("risk_level", ">", "1"), "AND", [nodes[2], "OR", nodes[3]]], "AND",
             nodes[4], "OR", ("shell_type", "=", "bash"), "AND", [nodes[5], "AND", nodes[6], "OR", ("host_name", "<", "labpc-04")], "OR",
             nodes[7], "AND", [[nodes[8], "OR", ("sudo_used", "=", "false")], "AND", ("exit_code", "!=", "0")], "OR",
             nodes[9], "AND", ("base_command", ">", "cmd020")]
    mask, passes = plan_mask(chain)
    assert sum(m is not None for _, _, m in passes) == 10
    assert np.array_equal(mask, chain_mask(chain)) and 0 < mask.sum() < N_ROWS
    flat = []
    for node in nodes:
        flat += [node, "AND" if len(flat) % 4 else "OR"]
    flat = flat[:-1]
    assert np.array_equal(plan_mask(flat)[0], chain_mask(flat))


def test_random_chains_with_sets():
    rng = random.Random(2024)
    leaves = [("risk_level", ">", "2"), ("exit_code", "=", "0"), ("sudo_used", "=", "true"), ("shell_type", "!=", "zsh"), ("host_name", "<", "labpc-07"),
              ("raw_command", "LIKE", "a%"), ("raw_command", "LIKE", "%c%"), ("raw_command", "NOT LIKE", "%_\\\\%"), ("raw_command", "LIKE", "_b%"),
              IN("host_name", ["labpc-02", "vm-ubuntu-01"]), IN("user_name", FIVE), IN("risk_level", ["1", "3", "5"], True),
              IN("command_id", [str(v) for v in range(1, 4000, 401)]), IN("sudo_used", ["true"]), IN("shell_type", ["sh", "fish", "zsh"], True),
              IN("base_command", ["cmd%03d" % i for i in range(0, 111, 2)]), ("timestamp", "LIKE", "2025%"), IN("user_id", [], True)]

    def build(depth):
        out = []
        for i in range(rng.randint(1, 5)):
            out += [build(depth - 1) if depth and rng.random() < 0.3 else rng.choice(leaves), rng.choice(["AND", "OR"])]
        return out[:-1]

    for _ in range(60):
        chain = build(2)
        assert np.array_equal(plan_mask(chain)[0], chain_mask(chain)), chain


# ---- refusals, and what stays as it was -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,message", [
    (("risk_level", "LIKE", "3%"), "string column"), (("sudo_used", "NOT LIKE", "t%"), "string column"), (("command_id", "LIKE", "%"), "string column"),
    (("host_name", "IN", "labpc-01, labpc-02"), "parenthesised"), (("host_name", "IN", "(labpc-01"), "parenthesised"),
    (("host_name", "NOT IN", "labpc-01)"), "parenthesised"), (("host_name", "IN", ""), "parenthesised"),
    (("host_name", "IN", "('labpc-01)"), "unterminated"), (("host_name", "IN", "('a', 'b''')x')"), "malformed"), (("risk_level", "IN", "(1, '2)"), "unterminated"),
    (("host_name", "IN", "(a,,b)"), "empty item"), (("host_name", "IN", "(a, )"), "empty item"), (("risk_level", "NOT IN", "(,1)"), "empty item"),
    (("command_id", "IN", "(" + ",".join(str(i) for i in range(65537)) + ")"), "65536"),
])
def test_refusals(leaf, message):
    for chain in ([leaf], [("risk_level", ">", "3"), "AND", [("sudo_used", "=", "true"), "OR", leaf]]):
        with pytest.raises(pq.PqpsError, match=message):
            pq.compile_plan_sets(SPEC, chain)
        with pytest.raises(pq.PqpsError, match=message):
            pq.compile_where(SPEC, chain)


def test_the_largest_list_is_accepted():
    chain = [("command_id", "IN", "(" + ",".join(str(i) for i in range(0, 2 * 65536, 2)) + ")")]
    mask, passes = plan_mask(chain)
    assert passes[0][2]["form"] == pq.MEMBER_LIST and len(passes[0][2]["values"]) == 65536
    assert np.array_equal(mask, (ROWS["command_id"] % np.uint64(2) == 0) & (ROWS["command_id"] < np.uint64(2 * 65536)))


@pytest.mark.parametrize("op", ["~", "==", "like", "in", "Like", "NOT  IN", "not in", "IN "])
def test_unknown_operators_are_still_never_true(op):
    for attr, value in (("raw_command", "%"), ("host_name", "('labpc-01')"), ("risk_level", "(3)")):
        assert constant_of([(attr, op, value)]) == 0
        mask, _ = plan_mask([("risk_level", ">", "3"), "OR", (attr, op, value)])
        assert np.array_equal(mask, ROWS["risk_level"] > 3)
    assert pq.lib().hipIsSetOperator(op.encode()) == 0 and pq.lib().hipIsSetOperator(b"NOT LIKE") == 1
