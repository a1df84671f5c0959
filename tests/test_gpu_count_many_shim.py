"""pqps_filter_count_many called alone at the shim: every count compared, exactly, with numpy (count_many_model, the model of
the kernel the CPU suite checks against kernel_model).

One small table of every column form (8, 4, 2, 1 bytes, a bit plane, and enough 1-byte columns to fill all 12 slots) is
uploaded once, padded to PQPS_TILE_ROWS with rows that WOULD match, so that a prefix of it is a table of any smaller size
and the trimming of the partial last step is part of every case.  The counts buffer is pre-filled with a pattern: the call
writes every count itself.

  * n_rows 1, 1023, 1024, 1025, 4096 + 17 with K = 1, 2, 15, 16 queries
  * the smallest size at which a wave of the persistent grid (8 workgroups of 4 waves per CU) takes a second step, 1-byte
    columns; the same once with streaming loads (a child process: the shim reads PQPS_NT_LOADS once)
  * exactly 32 distinct leaves; 33 refused
  * one leaf used by 16 queries in both polarities; a query on the last column only; the OR form; a nested 6-step program
    whose jumps skip steps; both constants
  * widths 1 / 2 / 4 / 8 and a plane in one union; all 12 columns
  * windows that wrap; lo = 256 on a byte column
  * every row matching every query
  * every PQPS_EINVAL case
  * K = 1: the same count as pqps_filter_count of the predicate it was packed from
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import count_many_model as cm
import qpelib as q

pq = q.pq

EINVAL = -1
A, R = pq.ACCEPT, pq.REJECT
N_SMALL = 4096 + 17
SIZES = (1, 1023, 1024, 1025, N_SMALL)
SENTINEL = 0xABABABABABABABAB


def padded_rows(n_rows):
    return (n_rows + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS


class Table:
    """Host arrays and their device copies: name -> (array, device pointer, pqps width)."""

    def __init__(self, ctx, arrays):
        self.ctx, self.cols = ctx, {}
        for name, (a, width) in arrays.items():
            p = ctx.malloc(a.nbytes)
            ctx.upload(p, a.ctypes.data, a.nbytes)
            self.cols[name] = (a, p, width)
        self.counts = ctx.malloc(8 * pq.COUNT_MANY_MAX)

    def run(self, names, n_rows, prog, rc_only=False):
        """One call over the columns `names` (slot order).  -> the counts, checked against the model."""
        cols = pq.column_array([(self.cols[n][1], self.cols[n][2]) for n in names])
        fill = np.full(pq.COUNT_MANY_MAX, SENTINEL, dtype=np.uint64)
        self.ctx.upload(self.counts, fill.ctypes.data, fill.nbytes)
        rc = pq.lib().pqps_filter_count_many(self.ctx.h, cols, len(names), n_rows, C.byref(prog), self.counts, None)
        if rc_only:
            return rc
        pq.check(rc, "pqps_filter_count_many")
        self.ctx.sync()
        got = np.empty_like(fill)
        self.ctx.download(got.ctypes.data, self.counts, got.nbytes)
        want = cm.counts(prog, [self.values(n)[:n_rows] for n in names], n_rows)
        assert [int(x) for x in got[:prog.n_queries]] == want, (names, n_rows)
        assert all(int(x) == SENTINEL for x in got[prog.n_queries:]), "nothing behind the last query is written"
        return want

    def values(self, name):
        """The column as one value per row (a plane unpacked)."""
        a, _, width = self.cols[name]
        return np.unpackbits(a, bitorder="little") if width == pq.WIDTH_BITS else a

    def close(self):
        for _, p, _ in self.cols.values():
            self.ctx.free(p)
        self.ctx.free(self.counts)


def small_arrays():
    rng = np.random.default_rng(0xC0DE)
    n = padded_rows(N_SMALL)
    a8 = rng.integers(0, 40, n).astype(np.uint64)
    a8[:4] = [0, 2**64 - 1, 2**63, 2**32 + 5]
    b4 = rng.integers(-3, 7, n).astype(np.int32)
    b4[:4] = [-2**31, 2**31 - 1, -1, 0]
    c2 = rng.integers(0, 300, n).astype(np.uint16)
    c2[:2] = [0, 65535]
    d1 = rng.integers(0, 256, n).astype(np.uint8)
    e1 = (rng.random(n) < 0.3).astype(np.uint8)
    out = {"a8": (a8, 8), "b4": (b4, 4), "c2": (c2, 2), "d1": (d1, 1), "e1": (e1, 1),
           "ep": (np.packbits(e1, bitorder="little"), pq.WIDTH_BITS)}
    for i in range(7):
        out[f"g{i}"] = (rng.integers(0, 4 + i, n).astype(np.uint8), 1)
    return out


@pytest.fixture(scope="module")
def ctx():
    c = pq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    t = Table(ctx, small_arrays())
    yield t
    t.close()


# leaves over (b4, c2, d1, ep) in slot order, and sixteen programs over them
LEAVES4 = [(0, 2, 2**32 - 3), (0, (-1) & 0xFFFFFFFF, 2),         # 2 .. 2^32 - 1 unsigned: b4 >= 2 and every negative value; -1 <= b4 <= 1 (wraps)
           (1, 100, 99), (1, 7, 0),                              # 100 <= c2 <= 199, c2 == 7
           (2, 0, 127), (2, 200, 300),                           # d1 <= 127, d1 >= 200 (the window runs past 255)
           (3, 1, 0)]                                            # the plane's bit
PROGRAMS16 = [
    [(0, A, R)], [(0, R, A)], [(6, A, R)], [(6, R, A)],
    [(0, 1, R), (6, A, R)],                                      # AND
    [(0, A, 1), (6, A, R)],                                      # OR
    [(2, 1, 2), (4, A, 2), (5, A, R)],                           # (l2 AND l4) OR l5
    [(1, A, 1), (3, A, 2), (5, 3, R), (6, R, A)],                # l1 OR l3 OR (l5 AND NOT l6)
    True, False,
    [(6, 1, R), (4, 2, R), (2, A, R)],
    [(3, A, R)], [(5, R, A)],
    [(0, 1, 3), (1, 2, 3), (2, A, 3), (3, 4, R), (4, 5, R), (6, A, R)],   # six steps, jumps over steps
    [(4, R, 1), (5, R, A)],
    [(1, A, R)],
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 15, 16])
def test_sizes_and_query_counts(small, k):
    names = ["b4", "c2", "d1", "ep"]
    for n_rows in SIZES:
        # the last k programs, so that K = 1 is no constant and every K keeps all four columns in play
        used = PROGRAMS16[-k:] if k > 2 else [PROGRAMS16[13], PROGRAMS16[7]][:k]
        want = small.run(names, n_rows, cm.make_prog(LEAVES4, used, 4))
        assert n_rows < 1000 or any(0 < w < n_rows for w in want)


def big_case(ctx, expect_kernel):
    """Some waves of the grid take a second step, the last step is partial; two 1-byte columns."""
    cus = ctx.info()[1]
    n_rows = cus * 8 * 4 * 1024 + 1025
    rng = np.random.default_rng(7)
    n = padded_rows(n_rows)
    x = rng.integers(0, 5, n).astype(np.uint8)
    y = rng.integers(0, 3, n).astype(np.uint8)
    x[n_rows:] = 1                                               # the padding would match
    y[n_rows:] = 1
    t = Table(ctx, {"x": (x, 1), "y": (y, 1)})
    prog = cm.make_prog([(0, 1, 0), (0, 3, 1), (1, 1, 0)], [[(0, A, R)], [(1, 1, R), (2, A, R)], [(0, A, 1), (2, R, A)], True], 2)
    want = t.run(["x", "y"], n_rows, prog)
    assert want[3] == n_rows and 0 < want[0] < n_rows
    assert pq.lib().pqps_last_kernel().decode() == expect_kernel
    t.close()


@pytest.mark.gpu
def test_second_step_of_the_grid_stride_loop(ctx):
    big_case(ctx, "count_many_scan_kernel<NT=false>")


@pytest.mark.gpu
def test_second_step_with_streaming_loads():
    p = subprocess.run([sys.executable, __file__, "streaming"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


@pytest.mark.gpu
def test_thirty_two_leaves_and_one_more(small):
    leaves = [(0, v & 0xFFFFFFFF, 0) for v in range(-3, 7)] + [(1, 10 * v, 9) for v in range(12)] + [(2, 25 * v, 24) for v in range(10)]
    assert len(leaves) == 32
    queries = [[(2 * i, A, 1), (2 * i + 1, A, R)] for i in range(16)]        # every leaf is somebody's
    small.run(["b4", "c2", "d1"], N_SMALL, cm.make_prog(leaves, queries, 3))
    prog = cm.make_prog(leaves, queries, 3)
    prog.n_leaves = 33
    assert small.run(["b4", "c2", "d1"], N_SMALL, prog, rc_only=True) == EINVAL


@pytest.mark.gpu
def test_one_leaf_sixteen_queries_both_polarities(small):
    queries = [[(0, A, R)] if i % 2 == 0 else [(0, R, A)] for i in range(16)]
    want = small.run(["c2"], N_SMALL, cm.make_prog([(0, 100, 99)], queries, 1))
    assert want[0] + want[1] == N_SMALL and len(set(want)) == 2


@pytest.mark.gpu
def test_program_shapes(small):
    names = ["a8", "b4", "c2", "d1", "e1"]
    leaves = [(0, 10, 9), (1, 0, 3), (2, 0, 149), (3, 64, 63), (4, 1, 0), (4, 0, 0)]
    queries = [
        [(4, A, R)],                                             # the last column only
        [(0, A, 1), (1, A, 2), (2, A, 3), (3, A, R)],            # the OR form
        [(0, 1, 2), (1, A, 2), (2, 3, 4), (3, A, 4), (4, 5, R), (5, A, R)],   # (0 AND 1) OR (2 AND 3) OR (4 AND 5): never both of the last
        [(0, 2, 1), (1, 2, R), (2, 5, 3), (3, 4, R), (4, A, 5), (5, A, R)],   # jumps over one and two steps
        True, False,
    ]
    want = small.run(names, N_SMALL, cm.make_prog(leaves, queries, 5))
    assert want[4] == N_SMALL and want[5] == 0
    for n_rows in (1, 1025):
        small.run(names, n_rows, cm.make_prog(leaves, queries, 5))


@pytest.mark.gpu
def test_every_width_and_all_twelve_columns(small):
    names = ["a8", "b4", "c2", "d1", "ep"]
    leaves = [(0, 2**63, 2**63 - 1), (0, 5, 10), (1, (-3) & 0xFFFFFFFF, 3), (2, 65535, 0), (2, 0, 9), (3, 250, 5), (4, 0, 0)]
    queries = [[(i, A, R)] for i in range(7)] + [[(1, 1, R), (2, A, 2), (4, A, R)]]
    small.run(names, N_SMALL, cm.make_prog(leaves, queries, 5))
    names = ["a8", "b4", "c2", "d1", "ep"] + [f"g{i}" for i in range(7)]
    assert len(names) == pq.MAX_COLUMNS
    leaves = [(0, 0, 19), (1, 0, 2), (2, 0, 99), (3, 0, 99), (4, 1, 0)] + [(5 + i, 1, 1) for i in range(7)]
    queries = [[(i, A, R)] for i in range(12)] + [[(11, 1, R), (0, A, R)], [(5, A, 1), (11, R, A)]]
    for n_rows in (1023, N_SMALL):
        small.run(names, n_rows, cm.make_prog(leaves, queries, 12))


@pytest.mark.gpu
def test_edge_windows(small):
    names = ["a8", "b4", "d1"]
    leaves = [(0, 2**64 - 1, 1),                                 # wraps in 64 bits: 2^64 - 1 and 0
              (0, 2**32 + 5, 0),
              (1, 2**31 - 1, 1),                                 # INT_MAX and INT_MIN
              (1, (-1) & 0xFFFFFFFF, 1),                         # wraps in 32 bits: -1 and 0
              (2, 250, 10),                                      # runs past 255: 250 .. 255 only, 0 .. 4 are no hits in 32-bit arithmetic
              (2, 256, 0), (2, 256, 2**32 - 1 - 256),            # lo = 256 on a byte column: nothing
              (2, 0, 255)]                                       # everything
    want = small.run(names, N_SMALL, cm.make_prog(leaves, [[(i, A, R)] for i in range(8)], 3))
    a8, b4, d1 = (small.values(n)[:N_SMALL] for n in names)
    assert want[0] == int(((a8 == 2**64 - 1) | (a8 == 0)).sum()) and want[1] == 1
    assert want[2] == int(((b4 == 2**31 - 1) | (b4 == -2**31)).sum()) and want[3] == int(((b4 == -1) | (b4 == 0)).sum())
    assert want[4] == int((d1 >= 250).sum()) and want[5] == 0 and want[6] == 0 and want[7] == N_SMALL


@pytest.mark.gpu
def test_every_row_matches_every_query(small):
    leaves = [(0, 0, 2**32 - 1), (1, 0, 65535), (2, 0, 1)]
    queries = [[(i % 3, A, R)] for i in range(14)] + [[(0, 1, R), (1, 2, R), (2, A, R)], True]
    for n_rows in (1, 1024, N_SMALL):
        assert small.run(["b4", "c2", "ep"], n_rows, cm.make_prog(leaves, queries, 3)) == [n_rows] * 16


@pytest.mark.gpu
def test_einval(small):
    names = ["b4", "c2"]
    good = lambda: cm.make_prog([(0, 1, 1), (1, 5, 5)], [[(0, 1, R), (1, A, R)], True], 2)

    def refused(change, names=names, n_cols=None):
        prog = good()
        change(prog)
        cols = pq.column_array([(small.cols[n][1], small.cols[n][2]) for n in names])
        rc = pq.lib().pqps_filter_count_many(small.ctx.h, cols, len(names) if n_cols is None else n_cols, 100, C.byref(prog), small.counts, None)
        assert rc == EINVAL, pq.lib().pqps_last_error()

    assert small.run(names, 100, good(), rc_only=True) == 0
    refused(lambda p: setattr(p, "n_queries", 0))
    refused(lambda p: setattr(p, "n_queries", 17))
    refused(lambda p: setattr(p, "n_leaves", 33))
    refused(lambda p: setattr(p, "n_columns", 3))
    refused(lambda p: setattr(p.leaf[1], "column", 2))                            # column slot out of range
    refused(lambda p: (setattr(p.leaf[0], "column", 1), setattr(p.leaf[1], "column", 0)))   # not sorted by column
    refused(lambda p: setattr(p.leaf[0], "negate", 1))
    refused(lambda p: p.query[0].leaf.__setitem__(1, 2))                          # leaf slot out of range
    refused(lambda p: p.query[0].on_true.__setitem__(0, 0))                       # onto itself
    refused(lambda p: p.query[0].on_false.__setitem__(1, 0))                      # backwards
    refused(lambda p: p.query[0].on_true.__setitem__(0, 2))                       # past the last step
    refused(lambda p: setattr(p.query[0], "n_steps", 7))
    refused(lambda p: setattr(p.query[1], "constant", 2))
    L, h = pq.lib(), small.ctx.h
    cols = pq.column_array([(small.cols[n][1], small.cols[n][2]) for n in names])
    prog = good()
    assert L.pqps_filter_count_many(None, cols, 2, 100, C.byref(prog), small.counts, None) == EINVAL
    assert L.pqps_filter_count_many(h, None, 2, 100, C.byref(prog), small.counts, None) == EINVAL
    assert L.pqps_filter_count_many(h, cols, 2, 100, None, small.counts, None) == EINVAL
    assert L.pqps_filter_count_many(h, cols, 2, 100, C.byref(prog), None, None) == EINVAL
    for width, ptr in ((pq.WIDTH_P12, small.cols["c2"][1]), (3, small.cols["c2"][1]), (2, small.cols["c2"][1] + 2), (2, None)):
        bad = pq.column_array([(small.cols["b4"][1], 4), (ptr, width)])          # a packed column, a width, an alignment, no data
        assert L.pqps_filter_count_many(h, bad, 2, 100, C.byref(prog), small.counts, None) == EINVAL
    small.ctx.sync()


@pytest.mark.gpu
def test_one_query_counts_what_filter_count_counts(small):
    spec = pq.SchemaSpec()
    for name, w in (("command_id", 8), ("exit_code", 4), ("user_id", 4), ("risk_level", 4), ("sudo_used", 1)):
        spec.set_numeric(name, w)
    held = {"risk_level": "b4", "sudo_used": "e1", "command_id": "a8"}
    for chain in ([("risk_level", ">", "3"), "AND", ("sudo_used", "=", "1")], [("risk_level", "<=", "3")],
                  [("command_id", "<", "20"), "OR", [("risk_level", "!=", "0"), "AND", ("sudo_used", "=", "0")]]):
        pred, ids = pq.compile_where(spec, chain)
        (batch, batch_ids), = pq.count_many_pack([(pred, ids)])[0]
        for n_rows in (1025, N_SMALL):
            fused = small.run([held[pq.COLUMNS[i]] for i in batch_ids], n_rows, batch)
            cols = pq.column_array([(small.cols[held[pq.COLUMNS[i]]][1], small.cols[held[pq.COLUMNS[i]]][2]) for i in ids])
            pq.check(pq.lib().pqps_filter_count(small.ctx.h, cols, len(ids), n_rows, C.byref(pred), small.counts, None), "pqps_filter_count")
            small.ctx.sync()
            one = C.c_uint64()
            small.ctx.download(C.byref(one), small.counts, 8)
            assert fused == [one.value]


@pytest.mark.gpu
def test_the_timing_recorder_sees_one_record_per_call(small):
    small.ctx.set_timing(True)
    try:
        small.run(["b4", "c2", "d1", "ep"], N_SMALL, cm.make_prog(LEAVES4, PROGRAMS16, 4))
        scan_ms, query_ms, launches = small.ctx.kernel_time()
    finally:
        small.ctx.set_timing(False)
    assert launches == 1 and 0 < scan_ms <= query_ms


def test_program_tables_are_well_formed():
    """CPU: the shared programs jump forwards only and use every leaf, so the GPU cases test what they say."""
    assert len(PROGRAMS16) == 16
    used = set()
    for steps in PROGRAMS16:
        if isinstance(steps, bool):
            continue
        assert 1 <= len(steps) <= pq.TT_LEAVES
        for s, (k, t, f) in enumerate(steps):
            used.add(k)
            assert all(x in (A, R) or s < x < len(steps) for x in (t, f))
    assert used == set(range(len(LEAVES4)))
    assert [c for c, _, _ in LEAVES4] == sorted(c for c, _, _ in LEAVES4)


if __name__ == "__main__":
    assert sys.argv[1] == "streaming" and os.environ.get("PQPS_NT_LOADS") == "1"
    context = pq.Context(0)
    big_case(context, "count_many_scan_kernel<NT=true>")
    context.close()
    print("OK")
