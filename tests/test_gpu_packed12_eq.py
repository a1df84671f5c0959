"""The raw-dword equality of the shapes with a 12-bit packed column (context option "eq12"): (P) and (P,B) as ID list and COUNT(*).

A step whose packed column holds no row with the wanted code is decided on the column's raw dwords (csrc/packed12_eq.hpp) and
leaves no match; a step with a candidate takes the extracting path.  Everything is checked at the shim (pqps_filter_scan /
pqps_filter_count) against kernel_model.evaluate on the u16 codes, ID for ID and in order, with "eq12" 0 against 1 and "steps" 0
against 1 (one or two steps per wave).

Rows of a step: row = 1024 step + 512 chunk + 8 lane + field; a wave of a two-step kernel takes steps 2 w and 2 w + 1 of its tile of
8.  The tables are constructed: no row carries the code except the rows placed here, with one-bit neighbours of the code in the
fields beside them (fields 2 and 5 straddle two dwords of the chunk's three)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_model
import qpelib as q
import test_gpu_bit_plane as bp
from test_gpu_packed12 import P, B, packed_copy, predicate

pq = q.pq
pytestmark = pytest.mark.gpu

STEP = 1024
CODE = 1030
SIZES = [1, 1025, 2049, 8193, 65537, 73729]
NT_SIZES = [1, 2049, 73729]
# the evaluator variant (EV in pqps_last_kernel()) the equality takes at these sizes: the kernels that have the raw-dword test.
# A launch that fell back to another variant would pass every comparison without running it.
EQ_EV = {("ids", 1): 1, ("count", 1): 1, ("ids", 2): 2, ("count", 2): 0}     # (COUNT of (P,B): the ballot kernel, which has no such test)


def row_of(step, chunk, lane, field):
    return STEP * step + 512 * chunk + 8 * lane + field


def blank(n, code, seed):
    """codes without `code`, sudo_used at random"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4096, n).astype(np.uint16)
    codes[codes == code] = (code + 1) & 0xFFF
    sudo = (rng.random(n) < 0.4).astype(np.uint8)
    return codes, sudo


def put(codes, sudo, row, value, flag=None):
    if 0 <= row < len(codes):
        codes[row] = value
        if flag is not None:
            sudo[row] = flag


def steps_of(n):
    """the steps a table gets placed rows in: its first two tiles, and its last three steps (full or partial)"""
    steps = (n + STEP - 1) // STEP
    return sorted(set(range(min(steps, 16))) | set(range(max(steps - 3, 0), steps)))


def table_positions(n, code, seed):
    """The code at every field of both chunks of every step of steps_of(n) (so: in a wave's first and in its second step), a
    one-bit neighbour of the code in the field before and in the field after; over the steps every bit takes its turn."""
    codes, sudo = blank(n, code, seed)
    for s in steps_of(n):
        for chunk in (0, 1):
            for f in range(8):
                lane = 8 * f + chunk + 2 * (s % 4)
                b = (s + f) % 12
                r = row_of(s, chunk, lane, f)
                put(codes, sudo, r, code, 0)
                if f > 0:
                    put(codes, sudo, r - 1, code ^ (1 << b))
                if f < 7:
                    put(codes, sudo, r + 1, code ^ (1 << ((b + 6) % 12)))
    put(codes, sudo, n - 1, code, 0)                                # the table's last row
    return codes, sudo


def table_straddle(n, code, seed):
    """Fields 2 and 5: per step and chunk, lane b + 24 (field == 5) has the code there and the code with bit b flipped on both
    sides (b = 0 .. 11); lanes 48 .. 63 have only the flipped code in the straddling field, the code nowhere."""
    codes, sudo = blank(n, code, seed)
    for s in steps_of(n):
        for chunk in (0, 1):
            for f in (2, 5):
                for b in range(12):
                    r = row_of(s, chunk, b + 12 * (s % 2) + 24 * (f == 5), f)
                    put(codes, sudo, r, code, 0)
                    put(codes, sudo, r - 1, code ^ (1 << b))
                    put(codes, sudo, r + 1, code ^ (1 << b))
                for lane in range(48, 64):
                    put(codes, sudo, row_of(s, chunk, lane, f), code ^ (1 << ((lane + s) % 12)))
    return codes, sudo


def table_decoys(n, code, seed):
    """(P,B): decoys = the code with sudo_used TRUE.  Wave 0 of tile 0: step 0 has decoys only, step 1 a match with a decoy in the
    same lane and chunk and one in the other chunk.  Wave 1: the match in the first step, decoys only in the second.  Wave 2:
    decoys only in the first step, matches in the second.  The same in tile 1 with first and second steps swapped, and around
    the table's end."""
    codes, sudo = blank(n, code, seed)
    steps = (n + STEP - 1) // STEP

    def only_decoys(s):
        put(codes, sudo, row_of(s, 0, 9, 2), code, 1)
        put(codes, sudo, row_of(s, 1, 63, 7), code, 1)
        put(codes, sudo, row_of(s, 0, 0, 0), code, 1)

    def match_and_decoys(s):
        put(codes, sudo, row_of(s, 0, 5, 3), code, 0)
        put(codes, sudo, row_of(s, 0, 5, 4), code, 1)                # same lane, same chunk
        put(codes, sudo, row_of(s, 1, 5, 3), code, 1)                # the other chunk
        put(codes, sudo, row_of(s, 1, 40, 5), code, 0)

    for base in (0, 9):                                              # tile 0 as described; from step 9 on the roles are swapped
        for k, what in enumerate((only_decoys, match_and_decoys, match_and_decoys, only_decoys, only_decoys, match_and_decoys)):
            what(base + k)
    for k, what in enumerate((match_and_decoys, only_decoys, match_and_decoys)):
        if steps - 1 - k >= 0:
            what(steps - 1 - k)
    put(codes, sudo, n - 1, code, 1)                                 # a decoy in the table's last row
    return codes, sudo


def table_every_step(n, code, seed):
    """Every step has a candidate, and only one: ONE row with the code, sudo_used FALSE -- a match the raw-dword test must not miss,
    with no other field of the wave to cover for it.  Step s has it in field s % 8 of chunk (s / 8) % 2: from 16 steps on every
    field of both chunks has had its turn, the straddling fields 2 and 5 among them."""
    codes, sudo = blank(n, code, seed)
    for s in range((n + STEP - 1) // STEP):
        put(codes, sudo, row_of(s, (s // 8) % 2, (7 * s) % 64, s % 8), code, 0)
    put(codes, sudo, 0, code, 0)
    return codes, sudo


def table_random(n, code, seed):
    """codes 0 and 4095 (and the rows past a partial last step, which read as code 0) among all-zero and all-one neighbours"""
    rng = np.random.default_rng(seed)
    codes = rng.choice(np.array([0, 4095, 1, 4094, 2048, 2047, code], dtype=np.uint16), n, p=[0.3, 0.3, 0.1, 0.1, 0.08, 0.08, 0.04])
    sudo = (rng.random(n) < 0.4).astype(np.uint8)
    return codes, sudo


def s1(code):
    return [(0, code, 0, 0), (1, 0, 0, 0)]


def predicates(shape, code):
    """[(what, predicate, may be empty)]: the equality the raw-dword test takes, and the forms that keep the extracting path"""
    if len(shape) == 1:
        return [("=", predicate([(0, code, 0, 0)], "one", 1), False)]
    return [("= and FALSE", predicate(s1(code), "and", 2), False)]


def old_path_predicates(shape, code):
    two = len(shape) == 2
    nc = len(shape)
    tail = [(1, 0, 0, 0)] if two else []
    form = "and" if two else "one"
    out = [
        ("!=", predicate([(0, code, 0, 1)] + tail, form, nc)),
        ("<=", predicate([(0, 0, code, 0)] + tail, form, nc)),
        ("window", predicate([(0, code - 3 if code >= 3 else 0, 6, 0)] + tail, form, nc)),
        ("two leaves", predicate([(0, code, 0, 0), (0, 0, 1638, 0)] + tail, "and", nc)),
        ("lo 4096", predicate([(0, 4096, 0, 0)] + tail, form, nc)),
        ("lo 5000", predicate([(0, 5000, 0, 0)] + tail, form, nc)),
    ]
    if two:
        out.append(("or", predicate(s1(code), "or", nc)))
    return out


def check_table(ctx, n, shape, codes, sudo, preds, nt=False, tag=""):
    """IDs and COUNT of every predicate under eq12 0 / 1 x steps 0 / 1 (and the defaults): exact, and all alike."""
    L = pq.lib()
    out, dev = bp.Out(ctx, n), bp.Dev(ctx)
    try:
        cols = [(packed_copy(dev, codes, n), pq.WIDTH_P12)] + ([(dev.plane(sudo, n), pq.WIDTH_BITS)] if len(shape) == 2 else [])
        carr = pq.column_array(cols)
        for what, pred, may_be_empty in preds:
            want = np.nonzero(kernel_model.evaluate(pred, [codes, sudo][:len(shape)]))[0].astype(np.uint32)
            assert may_be_empty or len(want) > 0, (tag, what)
            for eq12, steps in ((-1, -1), (0, 0), (1, 0), (0, 1), (1, 1)):
                ctx.set_option("eq12", eq12)
                ctx.set_option("steps", steps)
                where = f"{tag} n={n} shape={shape} {what} eq12={eq12} steps={steps}"
                pq.check(L.pqps_filter_scan(ctx.h, carr, len(shape), n, 0, C.byref(pred), out.ids, out.cap, out.count, None), where)
                k = L.pqps_last_kernel().decode()
                got = out.ids_value()
                assert len(got) == len(want) and np.array_equal(got, want), (where, k, len(got), len(want))
                assert "W0=P12" in k and ("NT=true" if nt else "NT=false") in k and (steps < 0 or ("S=2" if steps else "S=1") in k), (where, k)
                assert not what.startswith("=") or f"EV={EQ_EV['ids', len(shape)]}>" in k, (where, k)
                # " eq12" behind the name: the launch was told to test its steps on the raw dwords -- the equality unless the option is 0,
                # and no other form ever
                assert k.endswith(" eq12") == (what.startswith("=") and eq12 != 0), (where, k)
                pq.check(L.pqps_filter_count(ctx.h, carr, len(shape), n, C.byref(pred), out.count, None), where)
                k = L.pqps_last_kernel().decode()
                assert out.count_value() == len(want), (where, k)
                assert "W0=P12" in k and (steps < 0 or ("S=2" if steps else "S=1") in k), (where, k)
                assert not what.startswith("=") or f"EV={EQ_EV['count', len(shape)]}>" in k, (where, k)
                assert k.endswith(" eq12") == (what.startswith("=") and eq12 != 0 and len(shape) == 1), (where, k)
    finally:
        ctx.set_option("eq12", -1)
        ctx.set_option("steps", -1)
        dev.free()
        out.free()


def check_sizes(sizes, nt=False):
    ctx = pq.Context(0)
    try:
        for n in sizes:
            for shape in ((P,), (P, B)):
                eq = [(w, p, n < STEP) for w, p, _ in predicates(shape, CODE)]     # (a one-row table has no room for every plan)
                for name, make in (("positions", table_positions), ("straddle", table_straddle), ("every step", table_every_step)) + (
                        (("decoys", table_decoys),) if len(shape) == 2 else ()):
                    codes, sudo = make(n, CODE, seed=n % 1000 + len(name))
                    # (the decoys' plan has its first match in step 1: a table without a full second step may have none)
                    check_table(ctx, n, shape, codes, sudo, [(w, p, e or (name == "decoys" and n < 2 * STEP)) for w, p, e in eq], nt=nt, tag=name)
                # the forms that keep the extracting path, on the table with the most going on
                codes, sudo = table_positions(n, CODE, seed=n % 1000 + 1)
                check_table(ctx, n, shape, codes, sudo, [(w, p, True) for w, p in old_path_predicates(shape, CODE)], nt=nt, tag="old path")
                # codes 0 and 4095: the field's extremes, among all-zero and all-one neighbours; lo 4096 / 5000: no row
                codes, sudo = table_random(n, CODE, seed=n % 1000 + 2)
                for code in (0, 4095):
                    check_table(ctx, n, shape, codes, sudo, [(w, p, True) for w, p, _ in predicates(shape, code)], nt=nt, tag=f"code {code}")
                    codes2, sudo2 = table_positions(n, code, seed=n % 1000 + 3)
                    check_table(ctx, n, shape, codes2, sudo2, [(w, p, n < STEP) for w, p, _ in predicates(shape, code)], nt=nt, tag=f"positions of {code}")
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_raw_dword_equality(n):
    """1025 / 2049: the partial last step is a wave's second / first step; 8193, 65537, 73729: a tile, a group, a group and a tile
    have just ended."""
    check_sizes([n])


def test_no_row_for_codes_the_column_cannot_hold():
    ctx = pq.Context(0)
    try:
        n = 8193
        codes, sudo = table_random(n, CODE, seed=5)
        for shape in ((P,), (P, B)):
            preds = [(w, p) for w, p in old_path_predicates(shape, CODE) if w.startswith("lo ")]
            for what, pred in preds:
                assert not kernel_model.evaluate(pred, [codes, sudo][:len(shape)]).any()
            check_table(ctx, n, shape, codes, sudo, [(w, p, True) for w, p in preds], tag="no row")
    finally:
        ctx.close()


def test_raw_dword_equality_streaming_loads():
    """The `nt` instantiations (the default from 256 MB of columns on), forced at test sizes in a process of their own."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_packed12_eq as t; t.check_sizes(%r, nt=True); print('OK')"
            % (str(q.ROOT / "tests"), NT_SIZES))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
