"""hipCompileAssignments (engine/hip/hipPredicate.c), the SET list of an UPDATE, checked on the CPU against expectations written
here: every value text typed by its column as the literal of `=` is, a string's presence and rank in its dictionary, and
every refusal -- each leaving the output as it was."""
import ctypes as C

import pytest

import qpelib as q

pq = q.pq

SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
HOSTS = [b"alpha", b"delta", b"omega"]
FIELD_BYTES = {"raw_command": 512, "base_command": 100, "shell_type": 20, "timestamp": 30, "working_directory": 200,
               "user_name": 50, "host_name": 100}


def make_spec():
    s = pq.SchemaSpec()
    for name, w in (("command_id", 8), ("exit_code", 4), ("user_id", 4), ("risk_level", 4), ("sudo_used", 1)):
        s.set_numeric(name, w)
    s.set_dict("shell_type", 1, SHELLS)
    s.set_dict("host_name", 1, HOSTS)
    for name in ("raw_command", "base_command", "timestamp", "working_directory", "user_name"):
        s.set_dict(name, 1, [b"only"])
    return s


SPEC = make_spec()


def one(column, value):
    (a,) = pq.compile_assignments(SPEC, {column: value})
    assert a[0] == pq.COL[column] and a[1] == pq.COLUMN_KIND[pq.COL[column]]
    return a[2:]


def test_numeric_typing():
    assert one("command_id", "18446744073709551615") == (2**64 - 1, True, 0)      # strtoull
    assert one("command_id", "42abc") == (42, True, 0)
    assert one("exit_code", "-7") == (-7, True, 0)                               # atoi, a negative value
    assert one("exit_code", "12junk") == (12, True, 0)
    assert one("risk_level", "junk") == (0, True, 0)
    assert one("user_id", 1030) == (1030, True, 0)
    assert one("risk_level", " 5") == (5, True, 0)


@pytest.mark.parametrize("text, want", [("TRUE", 1), ("true", 1), ("True", 1), ("1", 1), ("yes", 0), ("0", 0), ("false", 0),
                                        ("", 0), ("2", 0), (True, 1), (False, 0)])
def test_bool_typing(text, want):
    assert one("sudo_used", text) == (want, True, 0)


@pytest.mark.parametrize("text, present, rank", [
    (b"alpha", True, 0), (b"delta", True, 1), (b"omega", True, 2),                # present: first, middle, last
    (b"aaa", False, 0), (b"beta", False, 1), (b"delta ", False, 2), (b"zulu", False, 3),   # absent: first, middle, past the end
])
def test_string_presence_and_rank(text, present, rank):
    assert one("host_name", text) == (rank, present, rank)


def test_several_assignments_keep_their_order():
    got = pq.compile_assignments(SPEC, {"risk_level": 4, "shell_type": "ksh", "sudo_used": "TRUE", "command_id": "9"})
    assert got == [(pq.COL["risk_level"], pq.KIND_I32, 4, True, 0), (pq.COL["shell_type"], pq.KIND_DICT, 2, False, 2),
                   (pq.COL["sudo_used"], pq.KIND_BOOL, 1, True, 0), (pq.COL["command_id"], pq.KIND_U64, 9, True, 0)]


def test_twelve_assignments():
    every = {name: ("x" if pq.COLUMN_KIND[i] == pq.KIND_DICT else "3") for i, name in enumerate(pq.COLUMNS)}
    assert [a[0] for a in pq.compile_assignments(SPEC, every)] == list(range(12))


def test_longest_string_that_fits():
    for name, size in FIELD_BYTES.items():
        assert one(name, b"y" * (size - 1))[1] is False


def raw_compile(columns, values, n=None):
    """hipCompileAssignments itself over a pre-filled output: -> (rc, output bytes after, output bytes before)."""
    n = len(columns) if n is None else n
    names = (C.c_char_p * max(1, len(columns)))(*columns)
    texts = (C.c_char_p * max(1, len(values)))(*values)
    out = (pq.Assignment * pq.MAX_COLUMNS)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    rc = pq.lib().hipCompileAssignments(C.byref(SPEC.schema), names, texts, n, out)
    return rc, bytes(out), before


REFUSED = {
    "unknown column": ([b"risk"], [b"1"]),
    "unknown column after a good one": ([b"risk_level", b"nope"], [b"1", b"2"]),
    "same column twice": ([b"risk_level", b"user_id", b"risk_level"], [b"1", b"2", b"3"]),
    "no assignment": ([], []),
    "empty string": ([b"host_name"], [b""]),
    "command_id 0": ([b"command_id"], [b"0"]),
    "command_id that parses to 0": ([b"command_id"], [b"abc"]),
    **{f"{name} too long": ([name.encode()], [b"z" * size]) for name, size in FIELD_BYTES.items()},
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_leave_the_output_unset(case):
    columns, values = REFUSED[case]
    rc, after, before = raw_compile(columns, values)
    assert rc == -1 and after == before


def test_thirteen_assignments_refused():
    columns = [name.encode() for name in pq.COLUMNS] + [b"risk_level"]
    rc, after, before = raw_compile(columns, [b"1"] * 13)
    assert rc == -1 and after == before
    rc, after, before = raw_compile([b"risk_level"], [b"1"], n=-1)
    assert rc == -1 and after == before


def test_wrapper_raises():
    with pytest.raises(pq.PqpsError):
        pq.compile_assignments(SPEC, {"host_name": ""})
    with pytest.raises(pq.PqpsError):
        pq.compile_assignments(SPEC, {})
