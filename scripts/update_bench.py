"""UPDATE SET ... WHERE on a synthetic engine without host rows.

    python scripts/update_bench.py [--rows 100000000] [--queries 30] [--out results/update_bench.json]

(a) the fused route: `SET risk_level = <v> WHERE sudo_used = FALSE AND user_name = 'student1030'` (bench.py's S1), ONE
    pqps_filter_assign per shard;
(b) COUNT of the same WHERE on the same engine;
(c) the flags route of the same statement: the WHERE with `user_id IN (six scattered ids, 1030 among them)` in front, a member
    pass, so that the rows are the same and the plan has two passes (pqps_member_flags, pqps_filter_flags, pqps_assign_flags).
The value alternates between two values call by call, so every UPDATE changes every row it selects.  Every figure is host
time around a finished engine call, the three series alternated call by call, medians reported; the model is the
predicate's bytes per row plus 4 x width bytes per matched 4-row chunk, at 8 TB/s."""
import argparse
import importlib.util
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
TWO_PASS = [("user_id", "IN", pq.in_list([1030, 1033, 1037, 1041, 1046, 1052])), "AND"] + S1
PREDICATE_BYTES = 2.125                                          # the 2-byte user_name code + the sudo_used plane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = pq.HipEngine.synthetic(args.rows)
    assert len(pq.compile_plan(pq.synth_schema(), S1)) == 1 and len(pq.compile_plan(pq.synth_schema(), TWO_PASS)) == 2
    matches = eng.count(S1)
    assert eng.count(TWO_PASS) == matches
    turn = [0]

    def value():
        turn[0] += 1
        return 4 + turn[0] % 2

    def fused():
        assert eng.update({"risk_level": value()}, S1) == matches

    def count():
        assert eng.count(S1) == matches

    def flags():
        assert eng.update({"risk_level": value()}, TWO_PASS) == matches

    series = [fused, count, flags]
    for f in series:
        f()
    times = [[] for _ in series]
    for _ in range(args.queries):
        for i, f in enumerate(series):
            t0 = time.perf_counter()
            f()
            times[i].append((time.perf_counter() - t0) * 1e6)
    eng.close()
    med = [statistics.median(t) for t in times]
    model_us = (args.rows * PREDICATE_BYTES + matches * 16) / 8e12 * 1e6      # at most one 16-byte chunk per matching row
    res = dict(rows=args.rows, matches=matches, us_update_fused=med[0], us_count=med[1], us_update_flags=med[2], model_us=model_us,
               spread_us=[(min(t), max(t)) for t in times])
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
