"""tests/sparse_table.py without a device: the byte operations of a sparse table, laid over zero numpy buffers, unpack to the rows
its patches hold; the expected answers equal kernel_model.evaluate over all rows; moving the tail leaves nothing of the old one.

The table is small enough for full host arrays and large enough for the dense patch (two groups from row 458 752) and, after the
second move, for the first supergroup boundary (row 4 194 304)."""
import numpy as np

import kernel_model
import pack12_model as pm
import sparse_table as st
import test_gpu_packed12_eq as eq
from test_gpu_packed12 import predicate

SIZES = [700_001, 701_025, 4_194_304 + 8193]           # the tail moved twice: by one step, then past a supergroup boundary
EDGES = (10 * 65_536,)                                 # a "switch" row of the small table: the first group boundary behind the dense patch
CODE = st.CODE


def predicates():
    """(what, predicate, the background matches)"""
    return [("= and FALSE", predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "and", 2), False),
            ("= or TRUE", predicate([(0, CODE, 0, 0), (1, 1, 0, 0)], "or", 2), False),
            ("= or FALSE", predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "or", 2), True),
            ("= 0 and FALSE", predicate([(0, 0, 0, 0), (1, 0, 0, 0)], "and", 2), True),
            ("=", predicate([(0, CODE, 0, 0)], "one", 1), False),
            ("= 0", predicate([(0, 0, 0, 0)], "one", 1), True)]


def apply(buffers, ops):
    for op, kind, off, what in ops:
        if op == "zero":
            buffers[kind][off:off + what] = 0
        else:
            assert off + what.size <= buffers[kind].size
            buffers[kind][off:off + what.size] = what


def rows_of(buffers, n):
    """codes and booleans of rows [0, n) as each column kind holds them"""
    return {"u16": buffers["u16"].view(np.uint16)[:n], "u8": buffers["u8"][:n],
            "plane": np.unpackbits(buffers["plane"], bitorder="little")[:n], "p12": pm.unpack(buffers["p12"], n)}


def test_uploads_unpack_to_the_patches_and_answers_match_the_model():
    tab = st.SparseTable(st.KINDS, SIZES, EDGES)
    buffers = {k: np.zeros(tab.buffer_bytes(k), dtype=np.uint8) for k in st.KINDS}
    for n in SIZES:
        apply(buffers, tab.set_n(n))
        # the same patches, built into full host arrays here
        codes, sudo = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint8)
        names = []
        for p in tab.patches():
            assert p.first % st.STEP == 0 and len(p.codes) % st.STEP == 0 and p.first + p.rows <= n
            codes[p.first:p.first + p.rows], sudo[p.first:p.first + p.rows] = p.codes[:p.rows], p.sudo[:p.rows]
            names.append(p.name)
        assert names[:4] == ["start", "group edge", "quad edge", "dense"] and names[-1] == "tail"
        assert ("switch edge" in names) and (("supergroup edge" in names) == (n > st.SUPER))
        a, b = eq.table_positions(2 * st.TILE, CODE, seed=len("positions"))      # a constructor's window is a patch as it is
        assert np.array_equal(codes[:2 * st.TILE], a) and np.array_equal(sudo[:2 * st.TILE], b)
        assert codes[n - 1] == CODE and sudo[n - 1] == 0 and tab.patches()[-1].first == st.tail_first(n)
        assert np.all(codes[st.DENSE_FIRST:st.DENSE_FIRST + st.DENSE_ROWS] == CODE) and not sudo[st.DENSE_FIRST:st.DENSE_FIRST + st.DENSE_ROWS].any()
        fc, fs = tab.full_arrays()
        assert np.array_equal(fc, codes) and np.array_equal(fs, sudo)
        # what the buffers hold: those rows in every kind, and zero bytes from row n on (the packed fields of the last step among them)
        got = rows_of(buffers, n)
        assert np.array_equal(got["u16"], codes) and np.array_equal(got["p12"], codes)
        assert np.array_equal(got["u8"], sudo) and np.array_equal(got["plane"], sudo)
        padded = pm.padded_rows(n)
        assert not pm.unpack(buffers["p12"], padded)[n:].any() and not np.unpackbits(buffers["plane"], bitorder="little")[n:].any()
        assert not buffers["u16"].view(np.uint16)[n:].any() and not buffers["u8"][n:].any()
        buffer_rows = (SIZES[-1] + 4095) // 4096 * 4096             # whole tiles of the largest n
        assert buffer_rows >= padded and all(buffers[k].size * 8 == buffer_rows * st.EIGHTHS[k] for k in st.KINDS)
        # the expected answers against the model over all rows
        for what, pred, background in predicates():
            cols = [codes, sudo][:pred.n_columns]
            mask = kernel_model.evaluate(pred, cols)
            assert tab.background_matches(pred) == background, what
            assert tab.expected_count(pred) == int(mask.sum()), (n, what)
            if background:
                try:
                    tab.expected_ids(pred)
                except AssertionError:
                    continue
                raise AssertionError("an ID list over a matching background was not refused")
            want = np.nonzero(mask)[0].astype(np.uint32)
            ids = tab.expected_ids(pred)
            assert ids.dtype == np.uint32 and np.array_equal(ids, want), (n, what)
            cl = st.classes(ids, n, EDGES)
            assert set(cl) == {"start", "group edge", "supergroup edge", "dense", "tail", f"switch edge {EDGES[0]}"}
            assert all(v > 0 for k, v in cl.items() if k != "supergroup edge" or n > st.SUPER), (n, what, cl)
            assert cl["dense"] == st.DENSE_ROWS and (n > st.SUPER or cl["supergroup edge"] == 0)


def test_a_moved_tail_leaves_background_behind():
    """The old tail's rows are background again (or a fixed patch placed over them), in every kind; a smaller n is refused."""
    tab = st.SparseTable(st.KINDS, SIZES, EDGES)
    buffers = {k: np.zeros(tab.buffer_bytes(k), dtype=np.uint8) for k in st.KINDS}
    apply(buffers, tab.set_n(SIZES[0]))
    old = tab.patches()[-1]
    ops = tab.set_n(SIZES[1])
    assert [o[0] for o in ops[:len(st.KINDS)]] == ["zero"] * len(st.KINDS) and all(o[0] == "write" for o in ops[len(st.KINDS):])
    apply(buffers, ops)
    new = tab.patches()[-1]
    assert old.first < new.first < old.end                         # the two tails overlap: the order of the operations matters
    got = rows_of(buffers, SIZES[1])
    for k in st.KINDS:
        assert not got[k][old.first:new.first].any(), k
    try:
        tab.set_n(SIZES[0])
    except AssertionError:
        return
    raise AssertionError("a smaller n was not refused")


def test_sizes_at_the_switches_have_every_class():
    """The plan of the GPU test's sizes (no buffers: the plan alone): every class has a match at every size, for the AND form."""
    import test_gpu_size_regimes as sr
    tab = st.SparseTable(("p12", "plane"), sr.SIZES, sr.EDGES)
    pred = predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "and", 2)
    for n in sr.SIZES:
        ops = tab.set_n(n)
        assert sum(o[3].nbytes for o in ops if o[0] == "write") < 2 << 20      # a few KB per move (the first placement: the dense patch too)
        cl = st.classes(tab.expected_ids(pred), n, sr.EDGES)
        assert all(v > 0 for v in cl.values()) and len(cl) == 5 + sum(e <= n for e in sr.EDGES), (n, cl)
