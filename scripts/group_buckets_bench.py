"""Device time of GROUP BY buckets (HipEngine.group_buckets) beside the whole-value form on the same column and WHERE
(HipEngine.group_count, or HipEngine.aggregate with a value column), in the same process, through the engine's own kernel
timing (hipEngineKernelTiming: events on the dispatch packets of the queries' launches).

    python scripts/group_buckets_bench.py [--rows 100000000] [--ts-rows 20000000] [--ts-values 1000000] [--queries 50]
                                          [--out results/group_buckets_bench.json]

Two tables: the synthetic one (its timestamp is single-valued, so the shapes are user_id WIDTH 16 and WIDTH 1 and user_name
PREFIX 9, under the WHEREs of scripts/group_bench.py), and one over caller-supplied columns whose timestamp dictionary holds
--ts-values generated ISO-8601 strings, bucketed by hour (PREFIX 13) and by day (PREFIX 10) -- group_count refuses that
column, so its baseline is COUNT(*) of the same WHERE.  Per shape: us per query of COUNT(*), of the whole-value form and of
the bucketed form, and the ratio of the last two.  What the figures should show: the bounds search does not change the order
of magnitude of the grouped scan."""
import argparse
import ctypes as C
import importlib.util
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
WHERES = [("S1", S1), ("risk_level > 2", [("risk_level", ">", "2")]), ("risk_level > 1", [("risk_level", ">", "1")]), ("no WHERE", None)]
# column, prefix, width, value column
SYNTH_SHAPES = [("user_id", None, 16, None), ("user_id", None, 1, None), ("user_name", 9, None, None),
                ("user_id", None, 16, "risk_level"), ("user_name", 9, None, "risk_level")]
STR_COLUMNS = ["raw_command", "base_command", "shell_type", "timestamp", "working_directory", "user_name", "host_name"]


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


def measure(eng, table, rows, wname, chain, column, prefix, width, value, queries, whole_value=True):
    count = eng.count(chain or [])
    bucketed = lambda: eng.group_buckets(column, prefix=prefix, width=width, value_column=value, chain=chain)
    whole = (lambda: eng.aggregate(value, column, chain)) if value else (lambda: eng.group_count(column, chain))
    got = bucketed()                                             # warm-up (first use: scratch, bounds)
    assert sum(g[1] for g in got) == count, (wname, column)
    us_count = timed(eng, lambda: eng.count(chain or []), queries)
    us_bucket = timed(eng, bucketed, queries)
    kernel = pq.lib().pqps_last_kernel().decode()
    us_whole = groups = None
    if whole_value:
        groups = len(whole())
        us_whole = timed(eng, whole, queries)
    r = dict(table=table, rows=rows, where=wname, column=column, prefix=prefix, width=width, value=value, matches=count,
             buckets=len(got), groups=groups, us_count=round(us_count, 1), us_whole_value=us_whole and round(us_whole, 1),
             us_buckets=round(us_bucket, 1), ratio=us_whole and round(us_bucket / us_whole, 3), kernel=kernel)
    print(json.dumps(r), flush=True)
    return r


def timestamp_table(n, n_values, seed=13):
    """from_columns input: n rows over a dictionary of n_values ascending ISO-8601 timestamps, about 3.6 s apart (some 1 000 hours, 42 days)"""
    rng = np.random.default_rng(seed)
    ms = np.datetime64("2026-01-10T00:00:00.000") + (np.arange(n_values, dtype=np.int64) * 3_600 + rng.integers(0, 3_600, n_values)).astype("timedelta64[ms]")
    stamps = [(s + "Z").encode() for s in np.datetime_as_string(ms, unit="ms").tolist()]
    cols = {name: (None, [b"x"]) for name in STR_COLUMNS}
    cols.update(command_id=np.arange(n, dtype=np.uint64), exit_code=rng.integers(0, 3, size=n).astype(np.int32),
                user_id=rng.integers(1000, 3000, size=n).astype(np.int32), risk_level=rng.integers(1, 6, size=n).astype(np.int32),
                sudo_used=(rng.random(n) < 0.3).astype(np.uint8), timestamp=(rng.integers(0, n_values, size=n).astype(np.uint32), stamps))
    return cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--ts-rows", type=int, default=20_000_000)
    ap.add_argument("--ts-values", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    eng = pq.HipEngine.synthetic(args.rows)
    for wname, chain in WHERES:
        for column, prefix, width, value in SYNTH_SHAPES:
            results.append(measure(eng, "synthetic", args.rows, wname, chain, column, prefix, width, value, args.queries))
    eng.close()
    eng = pq.HipEngine.from_columns(args.ts_rows, timestamp_table(args.ts_rows, args.ts_values))
    for wname, chain in WHERES[1:]:
        for prefix in (13, 10):
            for value in (None, "risk_level"):
                results.append(measure(eng, "timestamps", args.ts_rows, wname, chain, "timestamp", prefix, None, value, args.queries,
                                       whole_value=False))
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
