"""Device time of COUNT / SUM / MIN / MAX of a value column (HipEngine.aggregate) against COUNT(*) of the same WHERE, through
the engine's own kernel timing (hipEngineKernelTiming: events on the dispatch packets of the queries' launches), on a
synthetic table.

    python scripts/aggregate_bench.py [--rows 100000000] [--queries 50] [--out results/aggregate_bench.json]

Per shape: us per query of each, their ratio, and the fraction of 8 TB/s over the bytes the aggregate reads -- the
predicate columns whole, the value column and the group column only in the 1024-row steps that hold a match (estimated
from the count as 1 - (1 - p)^1024 of the steps for an answer of p of the rows spread evenly)."""
import argparse
import ctypes as C
import importlib.util
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
SHAPES = [
    # name, WHERE, value column, group column, predicate bytes per row (sudo_used is read from its bit plane)
    ("SUM/MAX(risk_level) over S1", S1, "risk_level", None, 2.125),
    ("SUM/MAX(risk_level) over risk_level > 1", [("risk_level", ">", "1")], "risk_level", None, 4.0),
    ("MAX(command_id) by user_name", None, "command_id", "user_name", 0.0),
    ("SUM(exit_code) by host_name", None, "exit_code", "host_name", 0.0),
]
COLUMN_BYTES = {"user_name": 2, "risk_level": 4, "host_name": 1, "command_id": 8, "exit_code": 4}


def timed(eng, fn, k):
    L = pq.lib()
    assert L.hipEngineKernelTiming(eng.e, 1) == 0
    for _ in range(k):
        fn()
    scan, query, n = C.c_double(), C.c_double(), C.c_int()
    assert L.hipEngineKernelTime(eng.e, C.byref(scan), C.byref(query), C.byref(n)) == 0
    assert L.hipEngineKernelTiming(eng.e, 0) == 0
    assert n.value == k, (n.value, k)
    return query.value * 1e3 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = pq.HipEngine.synthetic(args.rows)
    results = []
    for name, chain, value, column, pred_bytes in SHAPES:
        count = eng.count(chain or [])
        groups = eng.aggregate(value, column, chain)                # warm-up (first use: scratch, bounds)
        assert sum(g[1] for g in groups) == count, name
        kernel = pq.lib().pqps_last_kernel().decode()
        us_count = timed(eng, lambda: eng.count(chain or []), args.queries)
        us_agg = timed(eng, lambda: eng.aggregate(value, column, chain), args.queries)
        p = count / args.rows
        steps_hit = 1.0 - (1.0 - p) ** 1024
        # (a column that is also a predicate column is read once)
        extra = sum(COLUMN_BYTES[c] for c in (value, column) if c and not (chain and c in str(chain)))
        read = args.rows * (pred_bytes + extra * steps_hit)
        r = dict(shape=name, rows=args.rows, matches=count, groups=len(groups), us_count=round(us_count, 1),
                 us_aggregate=round(us_agg, 1), ratio=round(us_agg / us_count, 3), bytes_read=int(read),
                 frac_8tbs=round(read / (us_agg * 1e-6) / 8e12, 3), kernel=kernel)
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
