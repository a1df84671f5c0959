"""Time of exact percentiles (HipEngine.quantiles) against the two yardsticks that existed before them, in one process.

    python scripts/quantile_bench.py [--rows 100000000] [--reps 7] [--out results/quantile_bench.json]

Per shape (a value column, a group column or none, a WHERE, the fractions), alternating repetition by repetition and between
TWO copies of the table (different seeds), so that no query finds the bytes of the one before it in a cache:
  (q) quantiles(value, fractions, group, WHERE)   one counting scan per pass, the tables summed on the host between passes
  (a) aggregate(value, group, WHERE)              ONE fused scan over the same columns (numeric value columns only)
  (b) order_ids(value, WHERE) without LIMIT       today's route to a percentile, for the ungrouped shapes: a device radix
                                                  sort of the selection and its download (the index on the host not counted)
Every figure is the engine's own wall clock of the call (queryTime of the C result: locks, launches, waits, downloads), in
microseconds: the minimum and the median over --reps repetitions (at least five) after one warm-up each.  q_over_a_per_pass is
median(q) / (passes x median(a)); the spread is (max - min) / median of each form."""
import argparse
import ctypes as C
import importlib.util
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

RISK_GT2 = [("risk_level", ">", "2")]
MEDIAN, P50_95_99 = [500_000], [500_000, 950_000, 990_000]
# (name, value column, group column, WHERE, fractions)
SHAPES = [
    ("median user_id", "user_id", None, None, MEDIAN),
    ("median user_id, risk_level > 2", "user_id", None, RISK_GT2, MEDIAN),
    ("p50/p95/p99 timestamp per user_name", "timestamp", "user_name", None, P50_95_99),
    ("p50/p95/p99 user_id per user_name", "user_id", "user_name", None, P50_95_99),
    ("median command_id", "command_id", None, None, MEDIAN),
    ("median risk_level per host_name", "risk_level", "host_name", None, MEDIAN),
    ("skew: median risk_level, risk_level = 3", "risk_level", None, [("risk_level", "=", "3")], MEDIAN),
]


def quantiles_us(eng, value, group, chain, ppm):
    groups, info = eng.quantiles_result(value, ppm, group, chain)
    return info["seconds"] * 1e6, info["passes"], groups


def aggregate_us(eng, value, group, chain):
    wl = pq.WhereList(chain)
    res = pq.lib().executeQueryAggregateHIP(eng.e, value.encode(), group.encode() if group else None, wl.ptr)
    assert res and res.contents.success
    us = res.contents.queryTime * 1e6
    pq.lib().freeAggregateResultHIP(res)
    return us


def order_ids_us(eng, value, chain):
    """The sort and its download, without turning 10^8 ids into a Python list."""
    wl = pq.WhereList(chain)
    ids, matches, qt = C.POINTER(C.c_uint)(), C.c_longlong(), C.c_double()
    n = pq.lib().executeQueryOrderIdsHIP(eng.e, wl.ptr, value.encode(), False, 0, C.byref(ids), C.byref(matches), C.byref(qt))
    assert n >= 0
    pq.lib().free(ids)
    return qt.value * 1e6


def summary(samples):
    med = statistics.median(samples)
    return dict(min=round(min(samples), 1), median=round(med, 1), spread=round((max(samples) - min(samples)) / med, 3) if med else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least five repetitions"
    engines = [pq.HipEngine.synthetic(args.rows, seed=0x5EED), pq.HipEngine.synthetic(args.rows, seed=0x5EED + 1)]
    numeric = {"user_id", "command_id", "risk_level", "exit_code"}
    results = []
    for name, value, group, chain, ppm in SHAPES:
        forms = {"q": lambda e: quantiles_us(e, value, group, chain, ppm)[0]}
        if value in numeric:
            forms["a"] = lambda e: aggregate_us(e, value, group, chain)
        if group is None:
            forms["b"] = lambda e: order_ids_us(e, value, chain)
        passes, answers = [], []
        for eng in engines:                                              # warm-up: scratch, bounds, and what the answer is
            _, p, groups = quantiles_us(eng, value, group, chain, ppm)
            kernel = pq.lib().pqps_last_kernel().decode()                # the last pass's
            passes.append(p)
            answers.append(len(groups))
            if value in numeric and groups:                              # the median lies between aggregate's minimum and maximum
                agg = eng.aggregate(value, group, chain)
                assert [(k, n) for k, n, _ in groups] == [(k, c) for k, c, _, _, _ in agg]
                assert all(lo <= v[0] <= hi for (_, _, v), (_, _, _, lo, hi) in zip(groups, agg))
            for f, fn in forms.items():
                if f != "q":
                    fn(eng)
        samples = {f: [] for f in forms}
        for rep in range(args.reps):                                     # alternate the forms and the table copies
            for f, fn in forms.items():
                samples[f].append(fn(engines[rep % 2]))
        s = {f: summary(v) for f, v in samples.items()}
        r = dict(shape=name, rows=args.rows, value=value, group=group, fractions=ppm, passes=passes[0], groups=answers[0], last_kernel=kernel,
                 us_quantiles=s["q"], us_aggregate=s.get("a"), us_order_ids=s.get("b"))
        if "a" in s and passes[0]:
            r["q_over_a_per_pass"] = round(s["q"]["median"] / (passes[0] * s["a"]["median"]), 3)
        if "b" in s:
            r["q_over_b"] = round(s["q"]["median"] / s["b"]["median"], 4)
            # faster than the sort by more than the run-to-run spread of the two measurements
            r["faster_than_sort"] = max(samples["q"]) < min(samples["b"])
        results.append(r)
        print(json.dumps(r), flush=True)
    for eng in engines:
        eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
