"""While a context records timings (Context.set_timing(True)) the query stream and the exchange do not run a query on one
of their scan lanes: it runs on the PARENT context and the caller's stream, so that the recorded events mean what
pqps_ctx_kernel_time documents.  Both take that decision in one place (ScanLanes::route in csrc/pqps_hip.hip); this file is
the test of its timed arm, which nothing else in tests/ reaches, and of going back and forth between the two arms.

One ID query and one COUNT(*) per predicate through pqps_qstream_scan / pqps_qstream_count and through
pqps_exchange_select / pqps_exchange_count (world of 1, tests/loopback's library as the RCCL library), with timing off,
on, and off again.  Every phase must give the counts and ID checksums NumPy gives for the same predicate over
pqps_synth_generate_host's rows, and the timed phase must record as many launches as it did before the lanes were shared."""
import ctypes as C

import numpy as np
import pytest

import qpelib as q
import test_gpu_group_count as grp

pq = q.pq
pytestmark = pytest.mark.gpu

LOOPBACK = q.ROOT / "tests" / "loopback" / "libloopback_rccl.so"
CHAINS = {name: grp.SYNTH_CHAINS[name] for name in ("s1", "risk_gt1")}
# 1 025 rows: one step of 1 024 rows and a partial one.  65 537 rows: one row past a scan group (kGroupSteps * kStepRows =
# 64 * 1 024 rows in filter_kernels.hpp), so the launch has two groups and expander workgroups run behind another group's tiles.
SIZES = (1025, 64 * 1024 + 1)
# Launches pqps_ctx_kernel_time reports for the timed phase: measured on the commit before the lanes were shared (parent
# of this file's first commit), same sequence, both sizes.  Each ID query is one record (one launch), each COUNT(*) one
# (scan + reduction): 2 predicates x (stream scan + stream count + exchange select + exchange count).
TIMED_LAUNCHES = 8


def numpy_answer(host, name):
    """(count, (sum of ids, sum of ids[i] * (2 i + 1)) mod 2^64) of the named predicate, by NumPy over the host rows."""
    a = host.arr
    if name == "s1":
        mask = (a["sudo_used"] == 0) & (a["user_name"] == pq.SYNTH_USERS_DICT.index(b"student1030"))
    else:
        assert name == "risk_gt1"
        mask = a["risk_level"] > 1
    ids = np.flatnonzero(mask).astype(np.uint64)
    weights = 2 * np.arange(len(ids), dtype=np.uint64) + 1
    return len(ids), (int(ids.sum(dtype=np.uint64)), int((ids * weights).sum(dtype=np.uint64)))


def read_u64(ctx, dptr):
    v = C.c_uint64()
    ctx.download(C.byref(v), dptr, 8)
    return int(v.value)


@pytest.mark.parametrize("n", SIZES)
def test_timing_moves_queries_to_the_parent_context_and_back(n):
    assert LOOPBACK.exists(), "build it first: make -C tests/loopback (python __graft_entry__.py does)"
    L = pq.lib()
    host = q.HostSynth(n)
    want = {name: numpy_answer(host, name) for name in CHAINS}
    assert want["risk_gt1"][0] > n // 4                              # (a dense answer; s1 is the sparse one)
    ctx = pq.Context(0)
    dev = pq.SyntheticTable(ctx, n)
    ids_dev, cnt_ids, cnt_count = ctx.malloc(4 * (n + 16)), ctx.malloc(64), ctx.malloc(64)
    qs, xh = C.c_void_p(), C.c_void_p()
    pq.check(L.pqps_qstream_create(ctx.h, 4, C.byref(qs)), "pqps_qstream_create")
    ident = C.create_string_buffer(128)
    path = str(LOOPBACK).encode()
    pq.check(L.pqps_exchange_unique_id(path, ident), "pqps_exchange_unique_id")
    pq.check(L.pqps_exchange_create(ctx.h, path, ident, 1, 0, n + 16, 4, C.byref(xh)), "pqps_exchange_create")

    def phase():
        """-> {predicate: (stream count, stream ID count, stream checksum, exchange count, exchange ID count, exchange checksum)}"""
        got = {}
        for name, chain in CHAINS.items():
            pred, cols, nc, _ = dev.bind(chain)
            pq.check(L.pqps_qstream_scan(qs, cols, nc, n, 0, C.byref(pred), ids_dev, n + 16, cnt_ids, None), "pqps_qstream_scan")
            pq.check(L.pqps_qstream_count(qs, cols, nc, n, C.byref(pred), cnt_count, None), "pqps_qstream_count")
            pq.check(L.pqps_qstream_sync(qs), "pqps_qstream_sync")
            ctx.sync()                                              # (timed: the queries ran on the context's own stream)
            k = read_u64(ctx, cnt_ids)
            stream = (read_u64(ctx, cnt_count), k, ctx.ids_checksum(ids_dev, min(k, n + 16)))
            pq.check(L.pqps_exchange_select(xh, cols, nc, n, 0, C.byref(pred), 0, None), "pqps_exchange_select")
            pq.check(L.pqps_exchange_count(xh, cols, nc, n, C.byref(pred), 1, None), "pqps_exchange_count")
            merged, local, totals = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 2)()
            pq.check(L.pqps_exchange_result(xh, 0, C.byref(merged), C.byref(local), totals), "pqps_exchange_result")
            assert int(totals[0]) == int(totals[1]) == int(local.value)
            listed = (int(totals[0]), ctx.ids_checksum(merged.value, int(totals[0])))
            pq.check(L.pqps_exchange_result(xh, 1, None, C.byref(local), totals), "pqps_exchange_result")
            assert int(totals[0]) == int(local.value)
            pq.check(L.pqps_exchange_sync(xh), "pqps_exchange_sync")
            got[name] = stream + (int(totals[0]),) + listed
        return got

    try:
        phases, launches = [], []
        for timed in (False, True, False):
            ctx.set_timing(timed)
            phases.append(phase())
            launches.append(ctx.kernel_time()[2])
        print(f"n={n} launches per phase (off, on, off): {launches}")
        for got in phases:
            for name, (k, sums) in want.items():
                assert got[name] == (k, k, sums, k, k, sums), (n, name, got[name], k, sums)
        assert phases[0] == phases[1] == phases[2]
        assert launches == [0, TIMED_LAUNCHES, 0], launches
    finally:
        L.pqps_exchange_destroy(xh)
        L.pqps_qstream_destroy(qs)
        for p in (ids_dev, cnt_ids, cnt_count):
            ctx.free(p)
        dev.free()
        ctx.close()
