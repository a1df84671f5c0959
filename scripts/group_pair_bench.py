"""Device time of GROUP BY two columns (HipEngine.group_pair) against COUNT(*) and the one-column form (group_count, or
aggregate with a value) by the wider of the two columns over the same WHERE, through the engine's own kernel timing
(hipEngineKernelTiming: events on the dispatch packets of the queries' launches), on a synthetic table; and end-to-end time
against today's route of such an answer -- select_columnar of the columns and a host-side np.unique.

    python scripts/group_pair_bench.py [--rows 100000000] [--queries 20] [--wall-queries 3] [--shapes I,J] [--out F]

Per shape: us per query of each, the ratio to the one-column form next to the ratio of the bytes the two read per matching
step (predicate columns + group columns + value), the kernel (pqps_last_kernel).  On the sort path the timing records the
selection only, so us_pair reads "selection only"; ms_engine is the C call's own queryTime (best of --wall-queries), the
whole query including the sort, the run reduction and the download."""
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
# bytes per row of the synthetic table's columns as the fused scans read them (sudo_used: its bit plane)
WIDTH = dict(user_name=2, host_name=1, shell_type=1, base_command=1, sudo_used=0.125, risk_level=4, exit_code=4, command_id=8)
SHAPES = [
    # name, WHERE, (A, B), value, the wider column, path
    ("host_name x shell_type", None, ("host_name", "shell_type"), None, "host_name", "LDS count"),
    ("risk_level > 1: host_name x shell_type", RISK, ("host_name", "shell_type"), None, "host_name", "LDS count"),
    ("risk_level > 1: host_name x shell_type, exit_code", RISK, ("host_name", "shell_type"), "exit_code", "host_name", "LDS value"),
    ("user_name x host_name", None, ("user_name", "host_name"), None, "user_name", "global count"),
    ("S1: user_name x base_command", S1, ("user_name", "base_command"), None, "user_name", "sort"),
    ("risk_level > 1: user_name x base_command", RISK, ("user_name", "base_command"), None, "user_name", "sort"),
]


def where_columns(chain):
    return sorted({leaf[0] for leaf in (chain or []) if isinstance(leaf, tuple)})


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


def host_route(eng, chain, pair, value):
    """Today's route: every matching cell of the columns to the host, then np.unique of (A << 32 | B) and reduceat."""
    out = eng.select_columnar(list(pair) + ([value] if value else []), chain, text=False)
    key = (out["values"][0].astype(np.int64) << 32) | out["values"][1].astype(np.int64)
    if value is None:
        counts = np.unique(key, return_counts=True)[1]
        sums = None
    else:
        order = np.argsort(key, kind="stable")
        starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]]) if len(key) else np.zeros(0, np.int64)
        counts = np.diff(np.append(starts, len(key)))
        sums = np.add.reduceat(out["values"][2].astype(np.int64)[order], starts) if len(key) else np.zeros(0, np.int64)
    eng.free_columnar(out)
    return counts.tolist(), None if sums is None else sums.tolist()


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
    for name, chain, pair, value, wider, path in (SHAPES[i] for i in pick):
        count = eng.count(chain or [])
        got, total, _ = eng.group_pair_total(pair, value, chain)             # warm-up (first use: bounds, scratch)
        assert total == count, name
        kernel = pq.lib().pqps_last_kernel().decode()
        one = (lambda: eng.group_count(wider, chain)) if value is None else (lambda: eng.aggregate(value, wider, chain))
        one()
        one_kernel = pq.lib().pqps_last_kernel().decode()
        us_count, _ = timed(eng, lambda: eng.count(chain or []), args.queries)
        us_one, _ = timed(eng, one, args.queries)
        us_pair, launches = timed(eng, lambda: eng.group_pair(pair, value, chain), args.queries)
        ms_engine = min(eng.group_pair_total(pair, value, chain)[2] for _ in range(args.wall_queries)) * 1e3
        pred = sum(WIDTH[c] for c in where_columns(chain))
        b_one = pred + WIDTH[wider] + (WIDTH[value] if value else 0)
        b_pair = pred + WIDTH[pair[0]] + WIDTH[pair[1]] + (WIDTH[value] if value else 0)
        fused = path != "sort"
        r = dict(shape=name, path=path, rows=args.rows, matches=count, pairs=len(got),
                 us_count=round(us_count, 1), us_one_column=round(us_one, 1), us_pair=round(us_pair, 1) if fused else "selection only",
                 ratio_to_one_column=round(us_pair / us_one, 3) if fused else None, byte_ratio=round(b_pair / b_one, 3),
                 recorded_per_query=launches, ms_engine=round(ms_engine, 3), kernel=kernel, one_column_kernel=one_kernel)
        counts, sums = host_route(eng, chain, pair, value)
        assert counts == [g[1] for g in got] and (sums is None or sums == [g[2] for g in got]), name
        r["ms_wall_host_route"] = round(min(wall(lambda: host_route(eng, chain, pair, value), 1) for _ in range(args.wall_queries)), 3)
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
