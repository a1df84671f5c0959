"""ORDER BY several columns (HipEngine.order_ids_by) on a synthetic table, in the pattern of scripts/order_bench.py.

    python scripts/order_multi_bench.py [--rows 100000000] [--queries 20] [--out results/order_multi_bench.json]
    python scripts/order_multi_bench.py --ab OTHER/libpqps_hip.so [--rows 100000000]

Default mode: two-key and four-key shapes, 32-bit and 64-bit packed keys, sparse and dense, through the fused scan, the list
path (a WHERE with a member pass) and the full sort.  `form` is what hipOrderKeyPlan makes of the key list on this table and
`kernel` the scan that ran.  us_device: the engine's own kernel timing (hipEngineKernelTiming; the fused path records the
scan and its rounds, the other paths the selection only), ms_engine: the C call's queryTime (best of --wall-queries),
ms_wall_host_route: select_columnar of the key columns and a numpy lexsort by (keys, row).

--ab: the one comparison with a bound.  pqps_filter_topk of ANOTHER build of the library (the parent commit's)
against this build's pqps_filter_topk_multi with ONE field on the same column -- user_name over risk_level > 1, K = 20 and
K = 1024 -- in one process, on one table, launches interleaved, device time from the events on the dispatch packets.  Both
build the same keys in the same order, so both do the same LDS work and read the same bytes."""
import argparse
import ctypes as C
import importlib.util
import json
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
DENSE = [("risk_level", ">", "1")]
NAMES = pq.in_list(["student%d" % u for u in range(1000, 3000, 250)])     # 8 scattered names: a member pass, so the list path
LIST_SPARSE = [("user_name", "IN", NAMES)]
LIST_DENSE = [("risk_level", ">", "1"), "AND", ("user_name", "NOT IN", NAMES)]
# bits on the synthetic table: user_name 11, user_id 11, exit_code 8, base_command 7, host_name 4, risk_level 3, shell_type 2,
# sudo_used 1; timestamp is single-valued and drops out.  No two of them pass 32 bits: PACK64 needs four keys here.
KEYS_A = [("risk_level", True), ("user_name", False)]                                                  # 14 bits: PACK32
KEYS_B = [("shell_type", False), ("risk_level", True), ("sudo_used", False), ("user_name", False)]     # 17 bits: PACK32
KEYS_C = [("risk_level", True), ("timestamp", True)]                                                   # one key left
KEYS_W = [("user_name", False), ("user_id", True), ("exit_code", False), ("base_command", True)]       # 37 bits: PACK64
SHAPES = [
    # name, WHERE, keys, limit, path
    ("S1 risk,user LIMIT 20", S1, KEYS_A, 20, "fused"),
    ("S1 user,uid,exit,base LIMIT 20", S1, KEYS_W, 20, "fused"),
    ("dense risk,user LIMIT 20", DENSE, KEYS_A, 20, "fused"),
    ("dense shell,risk,sudo,user LIMIT 1024", DENSE, KEYS_B, 1024, "fused"),
    ("dense user,uid,exit,base LIMIT 20", DENSE, KEYS_W, 20, "fused"),
    ("dense user,uid,exit,base LIMIT 512", DENSE, KEYS_W, 512, "fused"),
    ("dense risk,timestamp LIMIT 20", DENSE, KEYS_C, 20, "fused"),
    ("IN-list risk,user LIMIT 20", LIST_SPARSE, KEYS_A, 20, "list"),
    ("IN-list user,uid,exit,base LIMIT 20", LIST_SPARSE, KEYS_W, 20, "list"),
    ("dense NOT-IN risk,user LIMIT 20", LIST_DENSE, KEYS_A, 20, "list"),
    ("dense NOT-IN user,uid,exit,base LIMIT 20", LIST_DENSE, KEYS_W, 20, "list"),
    ("S1 risk,user", S1, KEYS_A, None, "full sort"),
    ("S1 user,uid,exit,base", S1, KEYS_W, None, "full sort"),
    ("dense risk,user", DENSE, KEYS_A, None, "full sort"),
    ("dense user,uid,exit,base", DENSE, KEYS_W, None, "full sort"),
]


# the synthetic table as hipOrderKeyPlan needs it (tests/qpelib.py's HostSynth shows the same domains)
SYNTH_COUNTS = dict(user_name=2000, base_command=111, host_name=16, shell_type=4, timestamp=1, raw_command=1, working_directory=1)
SYNTH_BOUNDS = dict(user_id=(1000, 2999), exit_code=(0, 130), risk_level=(1, 5))


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


def engine_call(eng, chain, keys, limit):
    """One executeQueryOrderIdsByHIP without the Python list: (rows as numpy, ms of the call's own queryTime)."""
    L = pq.lib()
    wl = pq.WhereList(chain)
    arr, n_keys = pq.order_keys(keys)
    ids, matches, qt = C.POINTER(C.c_uint)(), C.c_longlong(), C.c_double()
    n = L.executeQueryOrderIdsByHIP(eng.e, wl.ptr, arr, n_keys, int(limit or 0), C.byref(ids), C.byref(matches), C.byref(qt))
    assert n >= 0
    rows = np.ctypeslib.as_array(ids, shape=(max(n, 1),))[:n].copy()
    L.free(ids)
    return rows, int(matches.value), qt.value * 1e3


def host_route(eng, chain, keys, limit):
    """The route without the engine's ORDER BY: every matching key to the host, then a numpy lexsort by (keys, row) -- the row
    is command_id in the synthetic table; the codes select_columnar returns are ranks in strcmp order."""
    names = [c for c, _ in keys]
    out = eng.select_columnar(names + ["command_id"], chain, text=False)
    rows = out["values"][-1].astype(np.int64)
    cols = [rows]
    for (c, desc), v in reversed(list(zip(keys, out["values"][:-1]))):
        k = v.astype(np.int64)
        cols.append(-k if desc else k)
    eng.free_columnar(out)
    order = rows[np.lexsort(cols)]
    return order[:limit] if limit else order


def run_shapes(args):
    eng = pq.HipEngine.synthetic(args.rows)
    results = []
    pick = [int(i) for i in args.shapes.split(",")] if args.shapes else range(len(SHAPES))
    for name, chain, keys, limit, path in (SHAPES[i] for i in pick):
        rows, matches, _ = engine_call(eng, chain, keys, limit)              # warm-up
        kernel = pq.lib().pqps_last_kernel().decode()                        # the scan the query launched last
        assert matches == eng.count(chain or []), name
        us_dev, launches = timed(eng, lambda: engine_call(eng, chain, keys, limit), args.queries)
        ms_engine = min(engine_call(eng, chain, keys, limit)[2] for _ in range(args.wall_queries))
        plan = pq.order_key_plan(keys, SYNTH_COUNTS, SYNTH_BOUNDS)
        form = ("rows", "one key", "PACK32", "PACK64", "CHAIN")[plan["form"]]
        r = dict(shape=name, path=path, form=form, bits=plan["total_bits"] if plan["form"] >= 2 else None, keys=keys, rows=args.rows, matches=matches, returned=len(rows),
                 us_device=round(us_dev, 1) if path == "fused" else "selection only", recorded_per_query=launches,
                 ms_engine=round(ms_engine, 3), kernel=kernel)
        if not args.no_host_route:
            t = []
            for _ in range(args.wall_queries):
                t0 = time.perf_counter()
                want = host_route(eng, chain, keys, limit)
                t.append((time.perf_counter() - t0) * 1e3)
            r["ms_wall_host_route"] = round(min(t), 3)
            r["same_rows_as_host_route"] = bool(np.array_equal(want, rows))
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


def run_ab(args):
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    new = pq.lib()
    old = C.CDLL(str(pathlib.Path(args.ab).resolve()))
    old.pqps_last_error.restype = C.c_char_p
    old.pqps_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    old.pqps_ctx_sync.argtypes = [vp, vp]
    old.pqps_ctx_set_timing.argtypes = [vp, C.c_int]
    old.pqps_ctx_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    old.pqps_topk_scratch_bytes.restype = u64
    old.pqps_topk_scratch_bytes.argtypes = [vp, u64, u32, C.c_int, C.c_int]
    old.pqps_filter_topk.argtypes = [vp, C.POINTER(pq.Column), u32, u64, C.POINTER(pq.Predicate), C.POINTER(pq.Column), C.c_int, C.c_int,
                                     u32, u32, vp, u64, vp, vp, vp]
    ctx = pq.Context(0)
    n = args.rows
    table = pq.SyntheticTable(ctx, n, seed=0x5EED, columns=["risk_level", "user_name"])
    pred, cols, nc, _ = table.bind(DENSE)
    key = pq.Column(table.ptr["user_name"], table.width["user_name"], 0)
    bits = 8 * table.width["user_name"]
    h_old = vp()
    assert old.pqps_ctx_create(0, C.byref(h_old)) == 0, old.pqps_last_error()
    out_new, out_old, cnt = ctx.malloc(16 * 1024), ctx.malloc(16 * 1024), ctx.malloc(64)
    results = []
    for k in (20, 1024):
        need = max(new.pqps_topk_scratch_bytes(ctx.h, n, k, 0, 1), old.pqps_topk_scratch_bytes(h_old, n, k, 0, 1))
        scratch = ctx.malloc(need)

        def run_old():
            assert old.pqps_filter_topk(h_old, cols, nc, n, C.byref(pred), C.byref(key), 0, 0, 0, k, scratch, need, out_old, cnt, None) == 0

        def run_new():
            assert pq.filter_topk_multi(ctx, cols, nc, n, pred, [(key, 0, bits, 0, 0)], 0, k, scratch, need, out_new, cnt) == 0

        builds = (("parent pqps_filter_topk", old, h_old, run_old), ("pqps_filter_topk_multi x1", new, ctx.h, run_new))
        times = {b[0]: [] for b in builds}
        for _, L, h, run in builds:                                      # warm-up: code objects, scratch
            for _ in range(2):
                run()
            L.pqps_ctx_sync(h, None)
        a, b = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        ctx.download(a.ctypes.data, out_old, 8 * k)
        ctx.download(b.ctypes.data, out_new, 8 * k)
        assert np.array_equal(a, b), "the two builds' keys differ"
        for _ in range(args.rounds):
            for name, L, h, run in builds:
                L.pqps_ctx_set_timing(h, 1)
                for _ in range(args.reps):
                    run()
                ev, tot, m = C.c_double(), C.c_double(), C.c_int()
                L.pqps_ctx_kernel_time(h, C.byref(ev), C.byref(tot), C.byref(m))
                L.pqps_ctx_set_timing(h, 0)
                times[name].append(tot.value / m.value * 1e3)
        med = {name: statistics.median(t) for name, t in times.items()}
        names = [b[0] for b in builds]
        r = dict(rows=n, k=k, us={name: round(med[name], 1) for name in names},
                 spread={name: [round(min(times[name]), 1), round(max(times[name]), 1)] for name in names},
                 ratio_new_to_parent=round(med[names[1]] / med[names[0]], 4))
        results.append(r)
        print(json.dumps(r), flush=True)
        ctx.sync()
        ctx.free(scratch)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--wall-queries", type=int, default=3)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indexes into SHAPES (default: all)")
    ap.add_argument("--ab", default=None, help="another build of libpqps_hip.so: run the one-field A/B instead of the shapes")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    (run_ab if args.ab else run_shapes)(args)


if __name__ == "__main__":
    main()
