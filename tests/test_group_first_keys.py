"""CPU: the word of "the first row of every group" and its model.  hipFirstKeyDecode (pure host code of the library) undoes
(img ^ x) << 32 | row for every kind and direction; tests/group_first_model.py's numpy model agrees with a row-by-row loop."""
import numpy as np
import pytest

import group_first_model as m

pq = m.q.pq
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ROWS = (0, 1, (1 << 32) - 2)
KEYS = {m.KIND_I32: (INT32_MIN, -1, 0, 1, INT32_MAX), m.KIND_DICT: (0, 1, 65535, 65536, (1 << 32) - 1), m.KIND_BOOL: (0, 1)}


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kind", sorted(KEYS))
def test_decode_round_trip(kind, descending):
    for key in KEYS[kind]:
        for row in ROWS:
            word = m.pack_word(kind, descending, key, row)
            assert word != m.EMPTY
            assert pq.first_key_decode(kind, descending, word) == (key, row), (kind, descending, key, row)
            assert m.unpack_word(kind, descending, word) == (key, row)


@pytest.mark.parametrize("descending", [False, True])
def test_decode_empty_and_wide(descending):
    for kind in KEYS:
        assert pq.first_key_decode(kind, descending, m.EMPTY) is None
    with pytest.raises(ValueError):
        pq.first_key_decode(m.KIND_U64, descending, 5)
    # the C function leaves its outputs alone for the empty word and takes NULL outputs
    import ctypes as C
    key, row = C.c_longlong(77), C.c_uint(88)
    assert pq.lib().hipFirstKeyDecode(m.KIND_I32, int(descending), m.EMPTY, C.byref(key), C.byref(row)) == 0
    assert (key.value, row.value) == (77, 88)
    assert pq.lib().hipFirstKeyDecode(m.KIND_I32, int(descending), 5, None, None) == 1


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kind", sorted(KEYS))
def test_word_order_is_the_answer_order(kind, descending):
    """Ascending unsigned order of the words == key order in the asked direction, then ascending row."""
    pairs = [(k, r) for k in KEYS[kind] for r in ROWS]
    by_word = sorted(pairs, key=lambda p: m.pack_word(kind, descending, *p))
    by_rule = sorted(sorted(pairs, key=lambda p: p[1]), key=lambda p: p[0], reverse=descending)
    assert by_word == by_rule


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("dtype", [np.int64, np.uint64])
def test_model_against_brute_force(dtype, grouped, descending):
    rng = np.random.default_rng([7, grouped, descending])
    n = 200
    rows = rng.integers(0, 120, size=n)                          # rows listed more than once
    pool = np.array([0, 1, 2, 3, (1 << 63) + 1, (1 << 64) - 1], np.uint64) if dtype == np.uint64 else np.array([-5, -1, 0, 0, 3, 9], np.int64)
    per_row = rng.choice(pool, size=120)                         # heavy ties; a row keeps its key
    keys = per_row[rows]
    groups = (rng.integers(0, 7, size=120)[rows]) if grouped else None
    slow = m.first_rows_slow(rows, keys, groups, descending)
    for model in (m.first_rows, m.first_rows_fast):
        g, r, k = model(rows, keys, groups, descending)
        assert g.tolist() == sorted(slow)
        assert [(int(a), int(b)) for a, b in zip(r, k)] == [slow[x] for x in sorted(slow)]
    assert len(slow) == (7 if grouped else 1)


def test_model_empty_and_words():
    g, r, k = m.first_rows([], np.array([], np.int64), None, False)
    assert len(g) == len(r) == len(k) == 0
    out = m.expected_words(4, m.KIND_I32, True, [5, 6, 7, 8], np.array([1, 9, 9, 2]), [0, 2, 2, 7], row_base=100)
    assert out.tolist() == [m.pack_word(m.KIND_I32, True, 1, 105), m.EMPTY, m.pack_word(m.KIND_I32, True, 9, 106), m.EMPTY]
    o, b = m.expected_wide(2, True, [3, 4, 5], np.array([7, 7, 1], np.uint64), [1, 1, 1])
    assert o.tolist() == [m.EMPTY, 3] and int(b[1]) == 7 ^ m.U64


def test_group_first_is_exported():
    """The library exports the form and the package wraps it."""
    L = pq.lib()
    for sym in ("executeQueryGroupFirstHIP", "freeGroupFirstResultHIP", "executeQuerySelectGroupFirstHIP", "pqps_filter_group_first",
                "pqps_group_first_list", "hipFirstKeyDecode"):
        assert hasattr(L, sym), sym
    for name in ("group_first", "select_group_first"):
        assert callable(getattr(pq.HipEngine, name, None))
    fields = [f for f, _ in pq.GroupFirstResult._fields_]
    assert fields[:6] == ["groupColumn", "groupKind", "orderColumn", "orderKind", "descending", "numGroups"]
    assert fields[-2:] == ["queryTime", "success"]
