"""Device time of COUNT(DISTINCT value column) (HipEngine.count_distinct) against COUNT(*) and the ungrouped aggregate of the
same WHERE, through the engine's own kernel timing (hipEngineKernelTiming: events on the dispatch packets of the queries'
launches), on a synthetic table; and, for the dense shapes, end-to-end time against today's route of such an answer --
select_columnar of the value (and group) column and a host-side np.unique.

    python scripts/distinct_bench.py [--rows 100000000] [--queries 20] [--wall-queries 3] [--shapes I,J] [--out F]

Per shape: us per query of each, the ratio to the aggregate, the kernel (pqps_last_kernel).  On the fused path the
recorded time runs from the scan's start to the end of the popcount pass.  On the sort path the timing records the
selection only, so us_distinct reads "selection only"; ms_engine is the C call's own queryTime (best of --wall-queries),
the whole query including the sort and the downloads."""
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
RISK = [("risk_level", ">", "1")]
SHAPES = [
    # name, WHERE, value column, group column, path, host route
    ("S1 distinct user_name", S1, "user_name", None, "fused", False),
    ("risk_level > 1 distinct host_name", RISK, "host_name", None, "fused", True),
    ("distinct user_name by host_name", None, "user_name", "host_name", "fused", True),
    ("risk_level > 1 distinct base_command by user_name", RISK, "base_command", "user_name", "fused", True),
    ("S1 distinct command_id", S1, "command_id", None, "sort", False),
    ("risk_level > 1 distinct command_id", RISK, "command_id", None, "sort", True),
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


def engine_ms(eng, chain, value, column):
    """The C call's own queryTime (issue to distinct counts in host memory)."""
    L = pq.lib()
    wl = pq.WhereList(chain)
    res = L.executeQueryCountDistinctHIP(eng.e, value.encode(), column.encode() if column else None, wl.ptr)
    try:
        assert res and res.contents.success
        return res.contents.queryTime * 1e3
    finally:
        L.freeDistinctResultHIP(res)


def host_route(eng, chain, value, column):
    """Today's route: every matching cell of the value (and group) column to the host, then np.unique (of (group << 32 |
    value - min) with a group column: the shapes' values are dictionary codes)."""
    out = eng.select_columnar([value] + ([column] if column else []), chain, text=False)
    vals = out["values"][0]
    if column is None:
        d = [(None, len(np.unique(vals)))]
    else:
        v = vals.astype(np.int64)
        pairs = np.unique((out["values"][1].astype(np.int64) << 32) | (v - v.min()))
        keys, counts = np.unique(pairs >> 32, return_counts=True)
        d = list(zip(keys.tolist(), counts.tolist()))
    eng.free_columnar(out)
    return d


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
    for name, chain, value, column, path, route in (SHAPES[i] for i in pick):
        count = eng.count(chain or [])
        got, total = eng.count_distinct_total(value, column, chain)          # warm-up (first use: bounds, scratch)
        assert total == count, name
        kernel = pq.lib().pqps_last_kernel().decode()
        us_count, _ = timed(eng, lambda: eng.count(chain or []), args.queries)
        us_agg, _ = timed(eng, lambda: eng.aggregate("risk_level", None, chain), args.queries)
        us_dist, launches = timed(eng, lambda: eng.count_distinct(value, column, chain), args.queries)
        ms_engine = min(engine_ms(eng, chain, value, column) for _ in range(args.wall_queries))
        r = dict(shape=name, path=path, rows=args.rows, matches=count, groups=len(got), distinct=sum(d for _, d in got),
                 us_count=round(us_count, 1), us_aggregate=round(us_agg, 1),
                 us_distinct=round(us_dist, 1) if path == "fused" else "selection only",
                 ratio_to_aggregate=round(us_dist / us_agg, 3) if path == "fused" else None,
                 recorded_per_query=launches, ms_engine=round(ms_engine, 3), kernel=kernel)
        if route:
            want = host_route(eng, chain, value, column)
            assert [d for _, d in want] == [d for _, d in got], name
            r["ms_wall_host_route"] = round(min(wall(lambda: host_route(eng, chain, value, column), 1) for _ in range(args.wall_queries)), 3)
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
