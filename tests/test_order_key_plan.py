"""hipOrderKeyPlan (the packing rule of ORDER BY several columns; pure host code, no GPU) at its boundaries, and a numpy model of
the field arithmetic the kernels implement: the ascending order of (packed, row) is the lexsort of the raw keys with per-key
directions, and a value outside its domain stays inside its own field."""
import numpy as np
import pytest

import qpelib as q

pq = q.pq
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
U64, I32, BOOL, DICT = 0, 1, 2, 3                       # HIPKIND_* (include/hipPredicate.h)
I32_COLS = ("exit_code", "user_id", "risk_level")
DICT_COLS = ("raw_command", "base_command", "shell_type", "timestamp", "working_directory", "user_name", "host_name")


def ceil_log2(d):
    return 0 if d <= 1 else (d - 1).bit_length()


def plan(keys, counts=None, bounds=None):
    return pq.order_key_plan(keys, counts, bounds)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 65536, 65537, (1 << 20), (1 << 20) + 1])
def test_domain_bits_dictionary_and_range(d):
    """Domains 1, 2, 2^k and 2^k + 1, as a dictionary count and as an i32 range, beside a second key so that the field is kept."""
    p = plan(["user_name", "sudo_used"], {"user_name": d})
    if d == 1:                                          # a single-valued string column is no key: sudo_used alone is left
        assert p["form"] == pq.ORDER_ONE and [f["column"] for f in p["fields"]] == [pq.COL["sudo_used"]]
    else:
        assert p["form"] == pq.ORDER_PACK32 and p["total_bits"] == ceil_log2(d) + 1
        f0, f1 = p["fields"]
        assert (f0["kind"], f0["bits"], f0["base"], f0["shift"]) == (DICT, ceil_log2(d), 0, 1)
        assert (f1["kind"], f1["bits"], f1["base"], f1["shift"]) == (BOOL, 1, 0, 0)
    lo = -7
    p = plan(["exit_code", "sudo_used"], bounds={"exit_code": (lo, lo + d - 1)})
    f0 = p["fields"][0]
    assert p["form"] == pq.ORDER_PACK32 and len(p["fields"]) == 2       # a one-valued i32 column stays, with 0 bits
    assert (f0["kind"], f0["bits"], f0["base"], f0["shift"]) == (I32, ceil_log2(d), lo & 0xFFFFFFFF, 1)


def test_full_range_i32():
    p = plan(["user_id", "sudo_used"], bounds={"user_id": (INT32_MIN, INT32_MAX)})
    assert p["form"] == pq.ORDER_PACK64 and p["total_bits"] == 33
    assert p["fields"][0]["bits"] == 32 and p["fields"][0]["base"] == 0x80000000 and p["fields"][0]["shift"] == 1
    p = plan(["user_id", "exit_code"], bounds={"user_id": (INT32_MIN, INT32_MAX), "exit_code": (INT32_MIN, INT32_MAX)})
    assert p["form"] == pq.ORDER_PACK64 and p["total_bits"] == 64 and [f["shift"] for f in p["fields"]] == [32, 0]
    p = plan(["user_id"], bounds={"user_id": (0, 1 << 30)})             # 2^30 + 1 values: 31 bits
    assert p["fields"][0]["bits"] == 31
    p = plan(["user_id"], bounds={"user_id": (-1, INT32_MAX)})          # 2^31 + 1 values: 32 bits
    assert p["fields"][0]["bits"] == 32
    p = plan(["user_id", "sudo_used"], bounds={"user_id": (5, 4)})      # lo > hi: no rows, no bits
    assert p["fields"][0]["bits"] == 0


@pytest.mark.parametrize("t, form", [(32, "PACK32"), (33, "PACK64"), (64, "PACK64"), (65, "CHAIN")])
def test_total_bits_at_the_form_edges(t, form):
    """T exactly 32, 33, 64 and 65 out of an i32 range of t - 32 .. bits beside a full-range one, or of dictionaries."""
    want = getattr(pq, "ORDER_" + form)
    if t == 32:
        p = plan(["user_name", "host_name"], {"user_name": 1 << 16, "host_name": 1 << 16})
        shifts = [16, 0]
    else:
        rest = t - 32                                   # 1, 32 or 33 bits beside the 32 of user_id
        keys = ["user_id", "exit_code"] if rest <= 32 else ["user_id", "exit_code", "sudo_used"]
        span = min(rest, 32)
        exit_range = (0, (1 << span) - 1) if span < 32 else (INT32_MIN, INT32_MAX)
        p = plan(keys, bounds={"user_id": (INT32_MIN, INT32_MAX), "exit_code": exit_range})
        shifts = [span, 0] if rest <= 32 else None
    assert p["form"] == want and p["total_bits"] == t
    if want != pq.ORDER_CHAIN:
        assert [f["shift"] for f in p["fields"]] == shifts
    else:
        assert all(f["shift"] == 0 for f in p["fields"])


def test_keys_without_information():
    counts = {"user_name": 100, "shell_type": 1, "host_name": 7}
    p = plan(["user_name", ("user_name", True), "host_name"], counts)    # a repeated column: its first position counts
    assert p["form"] == pq.ORDER_PACK32 and [(f["column"], f["descending"]) for f in p["fields"]] == \
        [(pq.COL["user_name"], False), (pq.COL["host_name"], False)]
    p = plan([("user_name", True), "user_name"], counts)
    assert p["form"] == pq.ORDER_ONE and p["fields"][0]["descending"] is True
    p = plan(["shell_type", ("host_name", True)], counts)                # a single-valued column is dropped
    assert p["form"] == pq.ORDER_ONE and p["fields"][0]["column"] == pq.COL["host_name"] and p["fields"][0]["descending"]
    p = plan(["shell_type", "shell_type"], counts)
    assert p["form"] == pq.ORDER_ROWS and p["fields"] == [] and p["total_bits"] == 0
    p = plan(["shell_type"], {"shell_type": 0})                          # an empty dictionary
    assert p["form"] == pq.ORDER_ROWS


def test_command_id():
    p = plan([("command_id", True)])
    assert p["form"] == pq.ORDER_ONE and p["fields"][0]["kind"] == U64 and p["fields"][0]["bits"] == 64
    p = plan(["command_id", "command_id"])
    assert p["form"] == pq.ORDER_ONE
    p = plan(["shell_type", "command_id"], {"shell_type": 1})            # alone after the drop
    assert p["form"] == pq.ORDER_ONE
    for keys in (["sudo_used", "command_id"], ["command_id", "sudo_used"], ["user_id", ("command_id", True), "host_name"]):
        p = plan(keys, {"host_name": 3}, {"user_id": (0, 9)})
        assert p["form"] == pq.ORDER_CHAIN and len(p["fields"]) == len(keys)
    # nothing is refused for the size of a domain: 4 full-range-sized keys are a CHAIN
    p = plan(["user_id", "exit_code", "risk_level", "user_name"],
             {"user_name": 1 << 20}, {c: (INT32_MIN, INT32_MAX) for c in I32_COLS})
    assert p["form"] == pq.ORDER_CHAIN and p["total_bits"] == 116


def test_refusals(capfd):
    for keys in ([], ["user_id"] * 5, ["no_such_column"], ["user_id", "nope"]):
        with pytest.raises(pq.PqpsError):
            plan(keys)
    L = pq.lib()
    import ctypes as C
    names = (C.c_char_p * 2)(b"user_id", None)                           # a NULL column
    zeros = (C.c_int * 12)()
    out = pq.OrderKeyPlan()
    out.form = 77
    assert L.hipOrderKeyPlan(names, (C.c_int * 2)(), 2, zeros, zeros, zeros, C.byref(out)) == -1
    assert out.form == 77                                                # untouched
    assert L.hipOrderKeyPlan(None, (C.c_int * 2)(), 1, zeros, zeros, zeros, C.byref(out)) == -1
    assert "ORDER BY" in capfd.readouterr().err


# ---- the field arithmetic, modelled in numpy -----------------------------------------------------------------------------
def pack_model(values, fields):
    """values[j]: the raw column of field j as stored (u8 / u16 / u32 codes, i32 values); fields[j]: a dict of the plan.
    -> the packed word of every row, a Python-int array (object dtype, so that 64-bit words do not wrap silently)."""
    packed = np.zeros(len(values[0]), dtype=object)
    for v, f in zip(values, fields):
        mask = (1 << f["bits"]) - 1
        bins = (v.astype(np.int64) - f["base"]) & 0xFFFFFFFF             # value - base in 32-bit arithmetic
        field = np.minimum(bins, mask) ^ (mask if f["descending"] else 0)
        packed = packed | (field.astype(object) << f["shift"])
    return packed


def lexsort_order(raw, descending):
    """Rows by the raw keys (signed / unsigned as given), each key in its own direction, ties by row."""
    cols = [np.arange(len(raw[0]))]
    for v, d in reversed(list(zip(raw, descending))):
        cols.append(-v.astype(np.int64) if d else v.astype(np.int64))
    return np.lexsort(cols)


MODEL_CASES = [
    # (keys, dictionary counts, bounds)
    (["risk_level", "sudo_used"], {}, {"risk_level": (0, 5)}),
    (["user_name", "exit_code", "sudo_used", "shell_type"], {"user_name": 1000, "shell_type": 5}, {"exit_code": (-3, 255)}),
    (["user_id", "exit_code"], {}, {"user_id": (INT32_MIN, INT32_MAX), "exit_code": (INT32_MIN, INT32_MAX)}),
    (["host_name", "user_id"], {"host_name": 257}, {"user_id": (INT32_MAX - 4, INT32_MAX)}),
    (["exit_code", "timestamp"], {"timestamp": 1 << 20}, {"exit_code": (INT32_MIN, INT32_MIN + 4095)}),
]


def model_columns(rng, n, keys, counts, bounds):
    raw = []
    for c in keys:
        if c in counts:
            v = rng.integers(0, counts[c], size=n)
            v[:2] = (0, counts[c] - 1)
        elif c in bounds:
            lo, hi = bounds[c]
            v = rng.integers(lo, hi + 1, size=n) if hi - lo < (1 << 20) else rng.choice(
                np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi], np.int64), size=n)
            v[:2] = (lo, hi)
        else:
            v = rng.integers(0, 2, size=n)
        raw.append(v.astype(np.int64))
    return raw


@pytest.mark.parametrize("case", range(len(MODEL_CASES)))
def test_model_order_is_the_lexsort(case):
    keys, counts, bounds = MODEL_CASES[case]
    rng = np.random.default_rng(100 + case)
    n = 4000
    raw = model_columns(rng, n, keys, counts, bounds)
    for dirs in range(1 << len(keys)):
        desc = [bool(dirs >> j & 1) for j in range(len(keys))]
        p = plan(list(zip(keys, desc)), counts, bounds)
        assert p["form"] in (pq.ORDER_PACK32, pq.ORDER_PACK64)
        packed = pack_model(raw, p["fields"])
        assert max(packed) < (1 << p["total_bits"])
        got = sorted(range(n), key=lambda r: (packed[r], r))
        assert got == lexsort_order(raw, desc).tolist(), (keys, desc)


def test_model_out_of_domain_stays_in_its_field():
    counts, bounds = {"user_name": 100, "shell_type": 5}, {"exit_code": (10, 20)}
    keys = ["user_name", "exit_code", "shell_type"]
    for desc in ([False] * 3, [True] * 3, [False, True, False]):
        p = plan(list(zip(keys, desc)), counts, bounds)
        inside = [np.array([3], np.int64), np.array([15], np.int64), np.array([2], np.int64)]
        base = pack_model(inside, p["fields"])[0]
        for j, bad in ((0, 200), (0, 0xFFFF), (1, 9), (1, 26), (1, INT32_MIN), (1, INT32_MAX), (2, 255)):
            vals = [a.copy() for a in inside]
            vals[j][0] = bad
            word = pack_model(vals, p["fields"])[0]
            f = p["fields"][j]
            own = ((1 << f["bits"]) - 1) << f["shift"]
            assert (word ^ base) & ~own == 0, (desc, j, bad)            # no other field changed
            clamped = (1 << f["bits"]) - 1
            assert (word & own) >> f["shift"] == (0 if desc[j] else clamped), (desc, j, bad)
