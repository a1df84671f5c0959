"""K COUNT(*) clauses asked as ONE HipEngine.count_many call against the same K clauses as K COUNT tickets kept in flight on
the engine's lanes (executeQueryCountAsyncHIP: the form bench.py times), on synthetic tables.

    python scripts/count_many_bench.py [--rows 100000000] [--regions 9] [--calls 6] [--out results/count_many_bench.json]

Two engines over two copies of the table are alternated call by call (the physical placement of one copy is not the answer),
every form is warmed up, a region is `calls` calls, and the figure is the median over `regions` regions; all forms run in one
process.  Per family and K in {1, 2, 4, 8, 16}:
  us_kernel       device time of the call's launches (hipEngineKernelTiming: scan + the one-workgroup reduction)
  us_many         wall time of count_many
  us_tickets      wall time of the K tickets, issued up to the engine's lanes at a time, then awaited
  per clause      each of the three divided by K, and us_many / us_tickets
Families: `s1` K variations of `sudo_used = FALSE AND user_name = ...` (2.125 B/row in the union: the plane and the u16
codes); `s1_risk` the same with a risk_level comparison (6.125 B/row); `six` K clauses over six different columns
(risk_level, exit_code, user_id, host_name, shell_type, base_command: 15 B/row from K = 6 on)."""
import argparse
import ctypes as C
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

KS = (1, 2, 4, 8, 16)
WIDTH = {"sudo_used": 0.125, "user_name": 2, "risk_level": 4, "exit_code": 4, "user_id": 4, "host_name": 1, "shell_type": 1, "base_command": 1}


def s1(i):
    return [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", f"student{1030 + 7 * i}")]


def s1_risk(i):
    return s1(i) + ["AND", ("risk_level", ">=", str(1 + i % 5))]


def six(i):
    k = i // 6
    return [[("risk_level", ">", str(1 + k))], [("exit_code", "=", str(k))], [("user_id", "<", str(1100 + 300 * k))],
            [("host_name", "=", "labpc-%02d" % (3 + k))], [("shell_type", "=", ("zsh", "bash", "fish")[k])],
            [("base_command", "=", "cmd%03d" % (17 + k))]][i % 6]


FAMILIES = {"s1": s1, "s1_risk": s1_risk, "six": six}


def union_bytes(chains):
    columns = {item[0] for chain in chains for item in chain[0::2]}
    return sum(WIDTH[c] for c in columns)


def tickets(eng, chains, lanes):
    out = []
    for at in range(0, len(chains), lanes):
        held = [eng.select_async(chain, count_only=True) for chain in chains[at:at + lanes]]
        for tk in held:
            out.append(eng.await_ticket(tk)[0])
        for tk in held:
            eng.release_ticket(tk)
    return out


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def kernel_us(eng, fn):
    L = pq.lib()
    assert L.hipEngineKernelTiming(eng.e, 1) == 0
    fn()
    scan, query, n = C.c_double(), C.c_double(), C.c_int()
    assert L.hipEngineKernelTime(eng.e, C.byref(scan), C.byref(query), C.byref(n)) == 0
    assert L.hipEngineKernelTiming(eng.e, 0) == 0
    return query.value * 1e3, n.value


def median_of_regions(engines, regions, calls, measure):
    """measure(engine) -> us of one call; a region = `calls` calls on alternating engines; -> median over the regions' means"""
    means = []
    for _ in range(regions):
        means.append(statistics.fmean(measure(engines[c % len(engines)]) for c in range(calls)))
    return statistics.median(means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    engines = [pq.HipEngine.synthetic(args.rows), pq.HipEngine.synthetic(args.rows)]
    lanes = pq.lib().hipEngineLanes(engines[0].e)
    results = []
    for family, make in FAMILIES.items():
        for k in KS:
            chains = [make(i) for i in range(k)]
            want = [engines[0].count(chain) for chain in chains]
            for eng in engines:                                  # warm-up, and the three forms agree
                assert eng.count_many(chains) == want and tickets(eng, chains, lanes) == want, (family, k)
            launches = []

            def device(eng):
                us, n = kernel_us(eng, lambda: eng.count_many(chains))
                launches.append(n)
                return us

            us_kernel = median_of_regions(engines, args.regions, args.calls, device)
            us_many = median_of_regions(engines, args.regions, args.calls, lambda eng: wall_us(lambda: eng.count_many(chains)))
            us_tickets = median_of_regions(engines, args.regions, args.calls, lambda eng: wall_us(lambda: tickets(eng, chains, lanes)))
            read = args.rows * union_bytes(chains)
            r = dict(family=family, k=k, rows=args.rows, lanes=lanes, launches=max(launches), union_bytes_per_row=union_bytes(chains),
                     us_kernel=round(us_kernel, 1), us_many=round(us_many, 1), us_tickets=round(us_tickets, 1),
                     us_kernel_per_clause=round(us_kernel / k, 2), us_many_per_clause=round(us_many / k, 2),
                     us_tickets_per_clause=round(us_tickets / k, 2), many_over_tickets=round(us_many / us_tickets, 3),
                     kernel_frac_8tbs=round(read / (us_kernel * 1e-6) / 8e12, 3))
            results.append(r)
            print(json.dumps(r), flush=True)
    for eng in engines:
        eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
