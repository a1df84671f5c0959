"""hipMergeDictionaries (engine/hip/hipPredicate.c), the dictionary merge of a batch INSERT, checked on the CPU against a Python
model: merged = sorted(set(old) | set(new)) in bytes (= strcmp) order, lut_old / lut_new the position of every input string in
it, identity exactly when every old string keeps its position -- and every refusal, each leaving the outputs as they were."""
import ctypes as C

import pytest

import qpelib as q

pq = q.pq

FIELD_BYTES = {"raw_command": 512, "base_command": 100, "shell_type": 20, "timestamp": 30, "working_directory": 200,
               "user_name": 50, "host_name": 100}
OLD = [b"delta", b"golf", b"kilo", b"papa"]


def model(old, new):
    merged = sorted(set(old) | set(new))
    lut_old = [merged.index(v) for v in old]
    return merged, lut_old, [merged.index(v) for v in new], lut_old == list(range(len(old)))


CASES = {
    "disjoint, interleaved": (OLD, [b"alpha", b"hotel", b"zulu"]),
    "equal lists": (OLD, list(OLD)),
    "a subset, nothing new": (OLD, [b"golf", b"papa"]),
    "new at rank 0": (OLD, [b"alpha"]),
    "new in the middle": (OLD, [b"hotel"]),
    "new at the end": (OLD, [b"zulu"]),
    "new at the end, next to a known one": (OLD, [b"papa", b"papa2", b"quebec"]),
    "rank 0, middle and end at once": (OLD, [b"alpha", b"delta", b"hotel", b"kilo", b"zulu"]),
    "a prefix of an old string sorts before it": (OLD, [b"gol", b"golf ", b"golfa"]),
    "bytes above 127 sort last": (OLD, [b"Zed", b"\xc3\xa9cole"]),
    "empty old list": ([], [b"alpha", b"bravo"]),
    "empty new list": (OLD, []),
    "both empty": ([], []),
    "one and one": ([b"only"], [b"only"]),
    "a second value for a single-valued column": ([b"only"], [b"first"]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_merge_matches_the_model(case):
    old, new = CASES[case]
    assert pq.merge_dictionaries(old, new) == model(old, new)


def test_identity_only_when_the_old_codes_stay():
    assert pq.merge_dictionaries(OLD, [b"zulu"])[3] is True
    assert pq.merge_dictionaries(OLD, [b"papa", b"zulu", b"zz"])[3] is True
    assert pq.merge_dictionaries(OLD, [])[3] is True
    assert pq.merge_dictionaries(OLD, [b"alpha"])[3] is False
    assert pq.merge_dictionaries(OLD, [b"oscar"])[3] is False      # only the last old string moves
    assert pq.merge_dictionaries([], [b"alpha"])[3] is True


def test_a_large_merge():
    old = sorted(b"student%d" % i for i in range(1000, 3000))
    new = sorted([b"student%dx" % i for i in range(1000, 3000, 7)] + [b"aaa", b"zzz"] + old[::5])
    assert pq.merge_dictionaries(old, new) == model(old, new)


def test_longest_string_that_fits():
    for name, size in FIELD_BYTES.items():
        v = b"y" * (size - 1)
        assert pq.merge_dictionaries([b"a"], [v], column=name) == model([b"a"], [v])
        assert pq.merge_dictionaries([v], [b"a"], column=name) == model([v], [b"a"])


def raw_merge(old, new, column="user_name", null=()):
    """hipMergeDictionaries itself over pre-filled outputs: -> (rc, output bytes after, output bytes before)."""
    a = (C.c_char_p * max(1, len(old)))(*old)
    b = (C.c_char_p * max(1, len(new)))(*new)
    room = max(1, len(old) + len(new))
    outs = {"merged": (C.c_char_p * room)(), "count": C.c_int(), "lut_old": (C.c_uint32 * room)(), "lut_new": (C.c_uint32 * room)(),
            "identity": C.c_int()}
    for o in outs.values():
        C.memset(C.byref(o), 0xA5, C.sizeof(o))
    before = [bytes(o) for o in outs.values()]
    col = column if isinstance(column, int) else pq.COL[column]

    def arg(name, pointer):
        if name in null:
            return None
        return pointer
    rc = pq.lib().hipMergeDictionaries(arg("old", a), len(old), arg("new", b), len(new), col, arg("merged", outs["merged"]),
                                       arg("count", C.byref(outs["count"])), arg("lut_old", outs["lut_old"]), arg("lut_new", outs["lut_new"]),
                                       arg("identity", C.byref(outs["identity"])))
    return rc, [bytes(o) for o in outs.values()], before


REFUSED = {
    "old list descending": dict(old=[b"b", b"a"], new=[b"c"]),
    "old list with a duplicate": dict(old=[b"a", b"a"], new=[b"c"]),
    "new list descending": dict(old=[b"a"], new=[b"d", b"c"]),
    "new list with a duplicate at its end": dict(old=[b"a"], new=[b"c", b"d", b"d"]),
    "empty string in the old list": dict(old=[b"", b"a"], new=[b"c"]),
    "empty string in the new list": dict(old=[b"a"], new=[b"", b"c"]),
    "empty string alone": dict(old=[], new=[b""]),
    "a numeric column": dict(old=[b"a"], new=[b"b"], column="risk_level"),
    "a column that does not exist": dict(old=[b"a"], new=[b"b"], column=12),
    "a negative column": dict(old=[b"a"], new=[b"b"], column=-1),
    **{f"{name}: new string too long": dict(old=[b"a"], new=[b"z" * size], column=name) for name, size in FIELD_BYTES.items()},
    **{f"{name}: old string too long": dict(old=[b"z" * size], new=[b"a"], column=name) for name, size in FIELD_BYTES.items()},
    **{f"NULL {what}": dict(old=[b"a"], new=[b"b"], null=(what,)) for what in ("old", "new", "merged", "count", "lut_old", "lut_new", "identity")},
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_leave_the_outputs_unset(case):
    rc, after, before = raw_merge(**REFUSED[case])
    assert rc == -1 and after == before


def test_negative_counts_refused():
    a = (C.c_char_p * 1)(b"a")
    out = (C.c_char_p * 4)()
    n, ident = C.c_int(7), C.c_int(7)
    lo, ln = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    assert pq.lib().hipMergeDictionaries(a, -1, a, 1, pq.COL["user_name"], out, C.byref(n), lo, ln, C.byref(ident)) == -1
    assert pq.lib().hipMergeDictionaries(a, 1, a, -1, pq.COL["user_name"], out, C.byref(n), lo, ln, C.byref(ident)) == -1
    assert n.value == 7 and ident.value == 7


def test_a_null_list_with_count_zero_is_legal():
    rc, after, _ = raw_merge([], [b"b"], null=("old",))
    assert rc == 0
    assert C.c_int.from_buffer_copy(after[1]).value == 1


def test_wrapper_raises():
    with pytest.raises(pq.PqpsError):
        pq.merge_dictionaries([b"b", b"a"], [])
    with pytest.raises(pq.PqpsError):
        pq.merge_dictionaries([b"a"], [b""])
