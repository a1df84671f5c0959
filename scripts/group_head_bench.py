"""The two forms of "the first n rows of every group" (HipEngine.group_head) against each other, and the rounds form against
group_first, on the synthetic table grouped by user_name and ordered by user_id.

    python scripts/group_head_bench.py [--rows 100000000] [--queries 20] [--rounds 5] [--route-rows 10000000]
                                       [--out results/group_head_bench.json]

Per selection (no WHERE, S1, risk_level > 2) and n = 1, 2, 4, 8, 16, 32, 64, in one process, the forms alternating round by
round after a warm-up; each round times --queries queries, the figures are the median over the rounds and the spread:
  rounds   PQPS_HEAD_ROUNDS unset: n scans issued back to back (only for n <= PQPS_HEAD_ROUNDS_MAX of the build)
  sort     PQPS_HEAD_ROUNDS=0: the selection, one chain sort, the flag pass and the compaction
`engine_us` is the C call's own queryTime (lock to result, no Python decoding), the figure BOTH forms have: the radix sort's
launches are not taken by the engine's timing recorder, so the sort form has no complete device time.  `device_us` is the
recorder's figure (hipEngineKernelTiming), given for the rounds form and for group_first, whose launches it does record.
  per-round cost   (device_us of n rounds - device_us of 1 round) / (n - 1) over device_us of group_first, same process
  old route        group_head at n = 5 against order_ids without a limit plus the host pick, wall clock, --route-rows rows"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pqps_amd", ROOT / "parallel-query-processing-system_amd" / "__init__.py")
pq = importlib.util.module_from_spec(spec)
sys.modules["pqps_amd"] = pq
spec.loader.exec_module(pq)

S1 = [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")]
WHERES = [("no WHERE", None), ("S1", S1), ("risk_level > 2", [("risk_level", ">", "2")])]
GROUP, ORDER = "user_name", "user_id"
NS = (1, 2, 4, 8, 16, 32, 64)


def head_call(eng, n, wl):
    """One executeQueryGroupHeadHIP: (its queryTime in µs, rows in the answer) -- nothing decoded."""
    res = pq.lib().executeQueryGroupHeadHIP(eng.e, GROUP.encode(), ORDER.encode(), False, n, wl.ptr)
    r = res.contents
    assert r.success
    out = r.queryTime * 1e6, int(r.offsets[r.numGroups])
    pq.lib().freeGroupHeadResultHIP(res)
    return out


def force(form):
    if form == "sort":
        os.environ["PQPS_HEAD_ROUNDS"] = "0"
    else:
        os.environ.pop("PQPS_HEAD_ROUNDS", None)


def device_us(eng, fn, k):
    """Device time per query through the engine's recorder, whatever number of launches a query makes."""
    L = pq.lib()
    assert L.hipEngineKernelTiming(eng.e, 1) == 0
    for _ in range(k):
        fn()
    scan, query, n = C.c_double(), C.c_double(), C.c_int()
    assert L.hipEngineKernelTime(eng.e, C.byref(scan), C.byref(query), C.byref(n)) == 0
    assert L.hipEngineKernelTiming(eng.e, 0) == 0
    assert n.value > 0 and n.value % k == 0, (n.value, k)
    return query.value * 1e3 / k


def summary(samples):
    return dict(median=round(statistics.median(samples), 1), lo=round(min(samples), 1), hi=round(max(samples), 1))


def bench_forms(eng, rows, args, results):
    for wname, chain in WHERES:
        wl = pq.WhereList(chain)
        matches = eng.count(chain or [])
        for n in NS:
            forms = ["rounds", "sort"] if n <= pq.HEAD_ROUNDS_MAX else ["sort"]
            answer = {}
            for form in forms:                                          # warm-up, and both forms give the same answer
                force(form)
                answer[form] = eng.group_head_result(GROUP, ORDER, n, chain)[2]["rows"]
                head_call(eng, n, wl)
            assert len({tuple(a) for a in answer.values()}) == 1, (wname, n)
            engine = {f: [] for f in forms}
            device = []
            for _ in range(args.rounds):
                for form in forms:
                    force(form)
                    engine[form].append(statistics.mean(head_call(eng, n, wl)[0] for _ in range(args.queries)))
                force("rounds")
                if "rounds" in forms:
                    device.append(device_us(eng, lambda: head_call(eng, n, wl), args.queries))
            r = dict(rows=rows, where=wname, matches=matches, n=n, answer_rows=len(answer[forms[0]]),
                     engine_us={f: summary(v) for f, v in engine.items()}, device_us_rounds=summary(device) if device else None)
            if len(forms) == 2:
                r["rounds_over_sort"] = round(r["engine_us"]["rounds"]["median"] / r["engine_us"]["sort"]["median"], 3)
            results.append(r)
            print(json.dumps(r), flush=True)
        # the cost of a round r >= 1 against group_first, this project's own unchanged kernel, in the same process
        force("rounds")
        top = pq.HEAD_ROUNDS_MAX
        eng.group_first(GROUP, ORDER, chain)
        first, one, many = [], [], []
        for _ in range(args.rounds):
            first.append(device_us(eng, lambda: eng.group_first(GROUP, ORDER, chain), args.queries))
            one.append(device_us(eng, lambda: head_call(eng, 1, wl), args.queries))
            many.append(device_us(eng, lambda: head_call(eng, top, wl), args.queries))
        per_round = (statistics.median(many) - statistics.median(one)) / (top - 1)
        r = dict(rows=rows, where=wname, matches=matches, device_us_group_first=summary(first), device_us_one_round=summary(one),
                 device_us_top_rounds=summary(many), top=top, device_us_per_later_round=round(per_round, 1),
                 later_round_over_group_first=round(per_round / statistics.median(first), 3))
        results.append(r)
        print(json.dumps(r), flush=True)


def old_route(eng, chain, n):
    """order_ids without a limit and the group codes of those rows in that order (select_ordered: the sort runs twice, no call
    returns both), then the first n rows of every group picked on the host."""
    ids, _ = eng.order_ids(ORDER, chain, False, None)
    cells = eng.select_ordered([GROUP], chain, ORDER, False, None, text=False)
    codes = np.asarray(cells["values"][0])
    eng.free_columnar(cells)
    by = np.argsort(codes, kind="stable")                               # groups in key order, the order inside them kept
    sorted_codes = codes[by]
    starts = np.flatnonzero(np.r_[True, sorted_codes[1:] != sorted_codes[:-1]])
    rank = np.arange(len(by)) - np.repeat(starts, np.diff(np.r_[starts, len(by)]))
    return np.asarray(ids)[by[rank < n]].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--route-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5, "medians of at least five rounds"
    results = []
    eng = pq.HipEngine.synthetic(args.rows)
    bench_forms(eng, args.rows, args, results)
    eng.close()
    if args.route_rows:
        force("rounds")
        eng = pq.HipEngine.synthetic(args.route_rows)
        for wname, chain in WHERES[1:]:
            new, old = [], []
            want = eng.group_head_result(GROUP, ORDER, 5, chain)[2]["rows"]
            assert old_route(eng, chain, 5) == want, wname
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                eng.group_head(GROUP, ORDER, 5, chain)
                t1 = time.perf_counter()
                old_route(eng, chain, 5)
                t2 = time.perf_counter()
                new.append((t1 - t0) * 1e6)
                old.append((t2 - t1) * 1e6)
            r = dict(rows=args.route_rows, where=wname, n=5, wall_us_group_head=summary(new), wall_us_order_ids_and_host_pick=summary(old))
            results.append(r)
            print(json.dumps(r), flush=True)
        eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
