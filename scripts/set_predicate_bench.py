"""Set predicates (LIKE / IN) on the device and on the host.

    python scripts/set_predicate_bench.py [--rows 100000000] [--queries 30] [--csv-rows 1000000] [--out results/set_predicate_bench.json]

(a) COUNT of `shell_type IN ('bash','zsh')` against the hand-written OR chain -- the same compiled predicate -- with the
    run-to-run spread measured on the OR chain itself (two series of it, alternated with the IN series).
(b) `user_name IN (200 scattered)`: the member pass alone at the shim, plane and byte output, against its traffic model
    (2 B/row read + 1/8 or 1 B/row written, at 8 TB/s); the engine's COUNT of it; and the same query as an OR chain of 200
    `=` leaves (seven passes).
(c) `raw_command LIKE '%...%'` on a CSV engine: host compile time per distinct string (hipCompileWherePlan on the engine's
    dictionary sizes, through HipEngine.count of a pattern, minus the COUNT of a pattern-free WHERE).
Every figure is host time around a finished call (the engine's COUNT, or a shim call and a synchronise), the series of a
comparison alternated call by call, medians reported."""
import argparse
import ctypes as C
import importlib.util
import json
import pathlib
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)


def alternated(fns, k):
    """Each of `fns` k times, in turn (so that no series owns a warm cache or a quiet moment) -> median us per call each."""
    times = [[] for _ in fns]
    for f in fns:
        f()
    for _ in range(k):
        for i, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            times[i].append((time.perf_counter() - t0) * 1e6)
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def part_a(eng, k):
    in_chain = [("shell_type", "IN", "('bash','zsh')")]
    or_chain = [("shell_type", "=", "bash"), "OR", ("shell_type", "=", "zsh")]
    assert eng.count(in_chain) == eng.count(or_chain)
    med, _ = alternated([lambda: eng.count(or_chain), lambda: eng.count(in_chain), lambda: eng.count(or_chain)], k)
    return dict(us_or=med[0], us_in=med[1], us_or_again=med[2], spread_us=abs(med[0] - med[2]),
                within_spread=abs(med[1] - (med[0] + med[2]) / 2) <= max(abs(med[0] - med[2]), 0.02 * med[0]))


def part_b(eng, rows, k):
    users = [pq.SYNTH_USERS_DICT[i] for i in range(3, pq.SYNTH_USERS, 10)]
    in_chain = [("user_name", "IN", pq.in_list(users))]
    or_chain = []
    for u in users:
        or_chain += [("user_name", "=", u.decode()), "OR"]
    or_chain = or_chain[:-1]
    want = eng.count(in_chain)
    assert want == eng.count(or_chain)
    med, _ = alternated([lambda: eng.count(in_chain), lambda: eng.count(or_chain)], max(3, k // 3))
    out = dict(values=len(users), matches=want, us_engine_in=med[0], us_engine_or_chain=med[1], or_chain_passes=len(pq.compile_plan(pq.synth_schema(), or_chain)))
    # the member pass alone, both output forms
    ctx = pq.Context(0)
    tab = pq.SyntheticTable(ctx, rows, columns=["user_name"])
    member = pq.compile_plan_sets(tab.schema, in_chain)[0][2]
    words = (C.c_uint32 * len(member["words"]))(*member["words"])
    set_dev, out_dev, cnt_dev = ctx.malloc(4 * len(words)), ctx.malloc(rows + 8192), ctx.malloc(64)
    ctx.upload(set_dev, words, 4 * len(words))
    col = pq.Column(tab.ptr["user_name"], 2, 0)

    def run(form):
        pq.check(pq.lib().pqps_member_flags(ctx.h, C.byref(col), rows, member["form"], member["base"], member["n_bits"], set_dev, None, 0,
                                            form, out_dev, cnt_dev, None))
        ctx.sync()

    med, _ = alternated([lambda: run(pq.MEMBER_PLANE), lambda: run(pq.MEMBER_BYTES)], k)
    for name, us, wr in (("plane", med[0], 0.125), ("bytes", med[1], 1.0)):
        model_us = rows * (2 + wr) / 8e12 * 1e6
        out[name] = dict(us=us, model_us=model_us, fraction_of_8TBs=model_us / us)
    tab.free()
    ctx.close()
    return out


def part_c(csv_rows):
    with tempfile.TemporaryDirectory() as d:
        csv = pathlib.Path(d) / "commands.csv"
        subprocess.run([sys.executable, str(ROOT / "scripts" / "make_csv.py"), str(csv_rows), str(csv)], check=True)
        eng = pq.HipEngine(csv, [])
        distinct = eng.count_distinct("raw_command")[0][1]
        plain = [("risk_level", ">", "9")]
        like = [("raw_command", "LIKE", "%rm -rf%")]
        eng.count(like)
        med, _ = alternated([lambda: eng.count(plain), lambda: eng.count(like)], 9)
        eng.close()
    return dict(rows=csv_rows, distinct_strings=distinct, us_count_plain=med[0], us_count_like=med[1],
                ns_per_distinct_string=(med[1] - med[0]) * 1e3 / max(distinct, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--csv-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = pq.HipEngine.synthetic(args.rows)
    res = dict(rows=args.rows, a=part_a(eng, args.queries), b=part_b(eng, args.rows, args.queries))
    eng.close()
    if args.csv_rows:
        res["c"] = part_c(args.csv_rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
