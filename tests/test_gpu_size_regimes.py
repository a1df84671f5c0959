"""The plain scan's defaults on both sides of every table size at which they switch, on sparse tables (tests/sparse_table.py).

What a launch of pqps_filter_scan / pqps_filter_count, the query stream and the exchange chooses from the table's size
(csrc/pqps_hip.hip), restated here:

  decision                                                                  one side                    the other
  ID scans get a 16-bit list area (run_filter, kListAreaBelowGroups)        n <= 268 369 920 (4095 groups)  n >= 268 369 921
  the S1 shapes (2,1,0) (2,B,0) (P,B,0) as ID list take EV 2, else EV 0     n <= 268 435 455            n >= 268 435 456
  (valu_chain_default)
  expanders all behind the last tile, else among the tiles with the         n <= 536 805 376 (8191 groups)  n >= 536 805 377
  default lags (expand_lag, kInterleaveFromGroups)
  the query stream uses two lanes, else lane 0 only (one_lane_table)        n <= 536 870 911            n >= 536 870 912
  plain loads, else `nt` loads and a one-shot grid (is_streaming)           columns read <= 256 MB      more: every size above
                                                                            (P,B,0): n <= 165 191 050   n >= 165 191 051

Between 268 369 921 and 268 435 455 rows an EV 2 launch runs WITHOUT a list area: the first decision counts groups, the second rows.

Each shape gets ONE allocation at the largest n: zero bytes (code 0, sudo_used FALSE), plus patches of constructed rows at the table's
start, around the first group, quad-of-groups and supergroup boundary, a dense patch of two whole groups (every row matches: 16-bit
lists where there is a list area, bit masks and the ranking expansion where not), around the last supergroup boundary, around the
rows 268 369 920 / 268 435 456 / 536 805 376 / 536 870 912, and the table's last three steps with a match in row n - 1.  The sizes
are taken in ascending order; the tail moves.  Expected IDs: kernel_model.evaluate on the placed rows -- exact, ID for ID, in order.

Per shape, size and predicate the launches run with the context's options at their defaults, then "steps" 0 and 1, then "list16" 0
and 1.  The list-area and the lag decision cannot be read back: both "list16" settings next to the default must give the same
list, and the sizes one group either side of 4096 and 8192 groups run with nothing forced.  pqps_last_kernel() must name the
instance the table above says -- a launch that fell back to another instance would pass every comparison without running the one meant.

(P,B,0) also takes the 256 MB edge of its 1.625 bytes per row: 165 191 049 and 165 191 050 rows read n * 13 / 8 <= 2^28 bytes and take
plain loads, 165 191 051 rows are the first with `nt` loads.  The other shapes' footprint edges stay with PQPS_NT_LOADS.

Not covered here: MODE_FLAGS at these sizes (test_dense_answer_above_600m_rows), dense backgrounds as ID lists, the engine level."""
import ctypes as C
import time

import numpy as np
import pytest

import qpelib as q
import sparse_table as st
import test_gpu_bit_plane as bp
from test_gpu_packed12 import predicate

pq = q.pq
pytestmark = pytest.mark.gpu

GROUP = 65536
LIST_AREA_BELOW_GROUPS, INTERLEAVE_FROM_GROUPS = 4096, 8192                     # kListAreaBelowGroups, kInterleaveFromGroups
EV2_BELOW_ROWS = 268_435_456                                                     # valu_chain_default
ONE_LANE_FROM_ROWS = 536_870_912                                                 # one_lane_table
STREAMING_ABOVE_BYTES = 256 << 20                                                # kStreamingFootprint
EDGES = ((LIST_AREA_BELOW_GROUPS - 1) * GROUP, EV2_BELOW_ROWS, (INTERLEAVE_FROM_GROUPS - 1) * GROUP, ONE_LANE_FROM_ROWS)
# one row or one group either side of each switch; at the EV edge the partial last step as a wave's second step (+ 1025), as its
# first (+ 2049), and a tile just ended (+ 8193)
SIZES = [268_369_920, 268_369_921, 268_435_455, 268_435_456, 268_435_456 + 1025, 268_435_456 + 2049, 268_435_456 + 8193,
         536_805_376, 536_805_377, 536_870_911, 536_870_912, 536_870_912 + 1025]
assert EDGES == (SIZES[0], SIZES[3], SIZES[7], SIZES[10])
FOOTPRINT_SIZES = {"(P,B,0)": [165_191_049, 165_191_050, 165_191_051]}            # n * 13 / 8 bytes either side of kStreamingFootprint
ID_CAP = 1 << 20
CODE = st.CODE

# shape -> (column kinds, widths for pqps_column, names in pqps_last_kernel())
SHAPES = {
    "(P,B,0)": (("p12", "plane"), (pq.WIDTH_P12, pq.WIDTH_BITS), ("P12", "B")),
    "(2,B,0)": (("u16", "plane"), (2, pq.WIDTH_BITS), ("2", "B")),
    "(2,1,0)": (("u16", "u8"), (2, 1), ("2", "1")),
    "(P,0,0)": (("p12",), (pq.WIDTH_P12,), ("P12", "0")),                       # the control: one leaf, EV 1 on both sides of every switch
}
SETTINGS = [(), (("steps", 0),), (("steps", 1),), (("list16", 0),), (("list16", 1),)]


def predicates(shape):
    """[(what, predicate, form, modes)].  The S1 form; its OR form -- for ID lists with the boolean leaf turned to TRUE, so that the
    background does not match, for COUNT also as it stands (the background matches); for COUNT the AND form the background matches.
    The control has one leaf: equality alone (one leaf has no OR form of its own: its truth table is the equality's)."""
    if len(SHAPES[shape][0]) == 1:
        return [("=", predicate([(0, CODE, 0, 0)], "one", 1), "and", ("ids", "count")),
                ("= 0", predicate([(0, 0, 0, 0)], "one", 1), "and", ("count",))]
    return [("= and FALSE", predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "and", 2), "and", ("ids", "count")),
            ("= or TRUE", predicate([(0, CODE, 0, 0), (1, 1, 0, 0)], "or", 2), "or", ("ids", "count")),
            ("= or FALSE", predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "or", 2), "or", ("count",)),
            ("= 0 and FALSE", predicate([(0, 0, 0, 0), (1, 0, 0, 0)], "and", 2), "and", ("count",))]


def expected_kernel(shape, mode, form, n, steps_opt=-1):
    """The instance pick_eval documents for this launch, as pqps_last_kernel() spells it."""
    kinds, _, names = SHAPES[shape]
    packed, one = kinds[0] == "p12", len(kinds) == 1
    ev = 1 if one else (2 if mode == "ids" and n < EV2_BELOW_ROWS else 0)
    s = 2 if packed and steps_opt != 0 else 1                                    # chain_steps(): 2 for the packed shapes, 1 for the u16 ones
    nt = n * sum(st.EIGHTHS[k] for k in kinds) // 8 > STREAMING_ABOVE_BYTES
    eq12 = packed and form == "and" and (ev == 1 or (ev == 2 and mode == "ids"))
    return (f"eval_chain_kernel<{'MODE_IDS' if mode == 'ids' else 'MODE_COUNT'}, W0={names[0]}, W1={names[1]}, W2=0, S={s}, "
            f"NT={'true' if nt else 'false'}, EV={ev}>" + (" eq12" if eq12 else ""))


def check_size(ctx, tab, out, shape, n):
    """Every predicate x setting at one n.  -> (kernel of the default S1 ID launch, its expected IDs)"""
    L = pq.lib()
    carr = pq.column_array(list(zip(tab.ptrs, SHAPES[shape][1])))
    nc = len(tab.ptrs)
    seen = None
    for what, pred, form, modes in predicates(shape):
        want = tab.plan.expected_ids(pred) if "ids" in modes else None
        count = tab.plan.expected_count(pred)
        if want is not None:
            assert 0 < len(want) == count <= ID_CAP
            cl = st.classes(want, n, EDGES)
            assert all(v > 0 for v in cl.values()) and cl["dense"] == st.DENSE_ROWS, (shape, n, what, cl)     # (an empty class: a bug of this test)
        else:
            assert tab.plan.background_matches(pred) and count > n - (1 << 20)
        default_ids = None
        for setting in SETTINGS:
            steps_opt = dict(setting).get("steps", -1)
            for name, value in setting:
                ctx.set_option(name, value)
            try:
                where = f"{shape} n={n} {what} {setting}"
                if want is not None:
                    pq.check(L.pqps_filter_scan(ctx.h, carr, nc, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), where)
                    k = L.pqps_last_kernel().decode()
                    got = out.ids_value()
                    assert len(got) == len(want), (where, k, len(got), len(want))
                    if not np.array_equal(got, want):
                        bad = np.nonzero(got != want)[0]
                        raise AssertionError((where, k, len(bad), "first difference at", int(bad[0]), got[bad[:8]].tolist(), want[bad[:8]].tolist()))
                    assert k == expected_kernel(shape, "ids", form, n, steps_opt), (where, k)
                    if default_ids is None:
                        default_ids = got
                        seen = seen or (k, len(want))
                    assert np.array_equal(got, default_ids), where
                pq.check(L.pqps_filter_count(ctx.h, carr, nc, n, C.byref(pred), out.count, None), where)
                k = L.pqps_last_kernel().decode()
                assert out.count_value() == count, (where, k, out.count_value(), count)
                assert k == expected_kernel(shape, "count", form, n, steps_opt), (where, k)
            finally:
                for name, _ in setting:
                    ctx.set_option(name, -1)
    return seen


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scan_defaults_either_side_of_every_switch(shape):
    ctx = pq.Context(0)
    tab, out = None, None
    try:
        out = bp.Out(ctx, ID_CAP - 8)
        sizes = FOOTPRINT_SIZES.get(shape, []) + SIZES
        tab = st.DeviceTable(ctx, SHAPES[shape][0], sizes, EDGES)
        assert tab.bytes_allocated() <= 1.7e9
        for n in sizes:
            t0 = time.perf_counter()
            tab.set_n(n)
            kernel, ids = check_size(ctx, tab, out, shape, n)
            print(f"size-regimes {shape} n={n} ids={ids} {time.perf_counter() - t0:.3f} s  {kernel}")
    finally:
        for name in ("steps", "list16"):
            ctx.set_option(name, -1)
        if tab:
            tab.free()
        if out:
            out.free()
        ctx.close()


def test_query_stream_lanes_either_side_of_536m_rows():
    """A query stream of depth 4 over the (P,B,0) table at 536 870 911 and 536 870 912 rows: eight S1 ID queries back to back (slots
    0 - 3 twice; each query with buffers and an id_base of its own, so that no answer can stand in for another), then four COUNTs,
    one of each form; every answer is the expected one.  pqps_qstream_lane hands consecutive slots two different lane contexts at
    the smaller size and the same one at the larger (one_lane_table).

    The `dense` hint (pqps_qstream_hint_answer: the last answers held a quarter of the rows or more) would send ID queries to lane 0
    at the smaller size too; nothing here gives the hint, and the answers stay far below a quarter of the rows, so a caller that
    hints from its answers -- the engine -- would not engage it either."""
    L = pq.lib()
    shape = "(P,B,0)"
    sizes = [ONE_LANE_FROM_ROWS - 1, ONE_LANE_FROM_ROWS]
    depth = 4
    ctx = pq.Context(0)
    tab, qs, outs = None, C.c_void_p(), []
    try:
        tab = st.DeviceTable(ctx, SHAPES[shape][0], sizes, EDGES)
        outs = [bp.Out(ctx, ID_CAP - 8) for _ in range(8)]
        pq.check(L.pqps_qstream_create(ctx.h, depth, C.byref(qs)), "pqps_qstream_create")
        carr = pq.column_array(list(zip(tab.ptrs, SHAPES[shape][1])))
        what, s1, form, _ = predicates(shape)[0]
        assert what == "= and FALSE"
        for n in sizes:
            tab.set_n(n)
            want = tab.plan.expected_ids(s1)
            assert 0 < len(want) < n // 4
            kernels = []
            for i, o in enumerate(outs):
                pq.check(L.pqps_qstream_scan_slot(qs, i % depth, carr, 2, n, 1000 * i, C.byref(s1), o.ids, o.cap, o.count, None), f"n={n} query {i}")
                kernels.append(L.pqps_last_kernel().decode())
            for slot in range(depth):
                pq.check(L.pqps_qstream_wait(qs, slot), f"n={n} wait {slot}")
            for i, o in enumerate(outs):
                got = o.ids_value()
                assert len(got) == len(want) and np.array_equal(got, want + np.uint32(1000 * i)), (n, i, kernels[i])
                assert kernels[i] == expected_kernel(shape, "ids", form, n), (n, i, kernels[i])
            counts = predicates(shape)
            for i in range(depth):
                what, pred, form, _ = counts[i % len(counts)]
                pq.check(L.pqps_qstream_count_slot(qs, i, carr, 2, n, C.byref(pred), outs[i].count, None), f"n={n} count {i}")
                assert L.pqps_last_kernel().decode() == expected_kernel(shape, "count", form, n), (n, i)
            for i in range(depth):
                what, pred, form, _ = counts[i % len(counts)]
                pq.check(L.pqps_qstream_wait(qs, i), f"n={n} wait {i}")
                assert outs[i].count_value() == tab.plan.expected_count(pred), (n, i, what)
            lanes = []
            for slot in range(depth):
                lane_ctx, lane_stream = C.c_void_p(), C.c_void_p()
                pq.check(L.pqps_qstream_lane(qs, slot, n, None, C.byref(lane_ctx), C.byref(lane_stream)), "pqps_qstream_lane")
                pq.check(L.pqps_qstream_mark(qs, slot), "pqps_qstream_mark")
                lanes.append(lane_ctx.value)
            assert all(lanes) and ctx.h.value not in lanes
            if n < ONE_LANE_FROM_ROWS:
                assert lanes[0] != lanes[1] and lanes[0] == lanes[2] and lanes[1] == lanes[3], (n, lanes)
            else:
                assert len(set(lanes)) == 1, (n, lanes)
            pq.check(L.pqps_qstream_sync(qs), "pqps_qstream_sync")
            print(f"size-regimes qstream n={n} lanes={len(set(lanes))} ids={len(want)}")
    finally:
        if qs:
            L.pqps_qstream_destroy(qs)
        for o in outs:
            o.free()
        if tab:
            tab.free()
        ctx.close()
