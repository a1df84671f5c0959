"""ORDER BY column [DESC] LIMIT K (HipEngine.order_ids) against COUNT(*) and the ungrouped aggregate of the same WHERE, on a
synthetic table: device time through the engine's own kernel timing (hipEngineKernelTiming: events on the dispatch packets
of the queries' launches), and end-to-end wall time against today's route of an ordered answer -- select_columnar of the
key column, then a host sort (numpy lexsort by key and row).

    python scripts/order_bench.py [--rows 100000000] [--queries 20] [--out results/order_bench.json]

The device time of the fused path covers the scan and its reduction rounds (one recorded query each).  On the list and
full-sort paths the timing records the selection only, so their us_device reads "selection only"; their wall time is the
whole query.  ms_engine: the C call's own queryTime (best of --wall-queries), ms_wall_python: order_ids including its
Python list of row numbers, ms_wall_host_route: the route above (best of --wall-queries)."""
import argparse
import ctypes as C
import importlib.util
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
DENSE = [("risk_level", ">", "1")]
SHAPES = [
    # name, WHERE, order column, DESC, limit, path
    ("S1 ORDER BY command_id DESC LIMIT 20", S1, "command_id", True, 20, "fused"),
    ("risk_level > 1 ORDER BY command_id DESC LIMIT 20", DENSE, "command_id", True, 20, "fused"),
    ("risk_level > 1 ORDER BY user_name LIMIT 1024", DENSE, "user_name", False, 1024, "fused"),
    ("ORDER BY exit_code DESC LIMIT 20", None, "exit_code", True, 20, "fused"),
    ("S1 ORDER BY user_id", S1, "user_id", False, None, "full sort"),
    ("risk_level > 1 ORDER BY risk_level DESC LIMIT 0", DENSE, "risk_level", True, 0, "full sort"),
]


def timed(eng, fn, k):
    """(device us per query, recorded launches per query) over k calls."""
    L = pq.lib()
    assert L.hipEngineKernelTiming(eng.e, 1) == 0
    for _ in range(k):
        fn()
    scan, query, n = C.c_double(), C.c_double(), C.c_int()
    assert L.hipEngineKernelTime(eng.e, C.byref(scan), C.byref(query), C.byref(n)) == 0
    assert L.hipEngineKernelTiming(eng.e, 0) == 0
    return query.value * 1e3 / k, n.value / k


def wall(fn, k):
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    return (time.perf_counter() - t0) * 1e3 / k


def engine_ms(eng, chain, column, desc, limit):
    """The C call's own queryTime (issue to row numbers in host memory), without the Python list of order_ids."""
    L = pq.lib()
    wl = pq.WhereList(chain)
    ids, matches, qt = C.POINTER(C.c_uint)(), C.c_longlong(), C.c_double()
    n = L.executeQueryOrderIdsHIP(eng.e, wl.ptr, column.encode(), desc, int(limit or 0), C.byref(ids), C.byref(matches), C.byref(qt))
    assert n >= 0
    L.free(ids)
    return qt.value * 1e3


def host_route(eng, chain, column, desc, limit):
    """Today's route: every matching key to the host, then a host sort by (key, row) -- the row is command_id in the
    synthetic table."""
    out = eng.select_columnar([column, "command_id"], chain, text=False)
    key, rows = out["values"][0], out["values"][1].astype(np.int64)
    eng.free_columnar(out)
    k = key.astype(np.int64) if key.dtype != np.uint64 else key
    if desc:
        k = ~k if k.dtype == np.uint64 else -k
    order = rows[np.lexsort((rows, k))]
    return order[:limit] if limit else order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--wall-queries", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indexes into SHAPES (default: all)")
    args = ap.parse_args()
    eng = pq.HipEngine.synthetic(args.rows)
    results = []
    pick = [int(i) for i in args.shapes.split(",")] if args.shapes else range(len(SHAPES))
    for name, chain, column, desc, limit, path in (SHAPES[i] for i in pick):
        count = eng.count(chain or [])
        ids, matches = eng.order_ids(column, chain, desc, limit)          # warm-up
        assert matches == count, name
        kernel = pq.lib().pqps_last_kernel().decode()
        us_count, _ = timed(eng, lambda: eng.count(chain or []), args.queries)
        us_agg, _ = timed(eng, lambda: eng.aggregate("risk_level", None, chain), args.queries)
        us_order, launches = timed(eng, lambda: eng.order_ids(column, chain, desc, limit), args.queries)
        ms_order = wall(lambda: eng.order_ids(column, chain, desc, limit), args.wall_queries)
        ms_engine = min(engine_ms(eng, chain, column, desc, limit) for _ in range(args.wall_queries))
        r = dict(shape=name, path=path, rows=args.rows, matches=count, returned=len(ids), us_count=round(us_count, 1),
                 us_aggregate=round(us_agg, 1), us_device=round(us_order, 1) if path == "fused" else "selection only",
                 ratio_to_aggregate=round(us_order / us_agg, 3) if path == "fused" else None,
                 recorded_per_query=launches, ms_engine=round(ms_engine, 3), ms_wall_python=round(ms_order, 3), kernel=kernel)
        if count > 1_000_000 or path != "fused":
            want = host_route(eng, chain, column, desc, limit)
            assert want.tolist() == ids, name
            r["ms_wall_host_route"] = round(min(wall(lambda: host_route(eng, chain, column, desc, limit), 1)
                                                for _ in range(args.wall_queries)), 3)
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
