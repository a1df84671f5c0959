"""The top-N groups (HipEngine.group_top) on a table with a wide column, and the routes under it at the shim.

    python scripts/group_top_bench.py [--rows 50000000] [--queries 5] [--spans 100000,1000000,10000000] [--out results/group_top_bench.json]

The synthetic table has no wide column, so one is made: from_columns with user_id over `span` values, once uniform and once
with one value owning 30 % of the rows; risk_level uniform over 1 .. 5 (risk_level > 3: 40 % of the rows), exit_code uniform
over 10 000 values (exit_code = 7: 0.01 %).  Per table:

  engine     group_top("user_id", by="count", limit=20) with no WHERE, at 40 % and at 0.01 %: ms per query over --queries
             calls (the C call's queryTime, which ends after the download and the host ordering)
  host       what the parent commit can do: select_columnar(["user_id"]) + numpy.unique, wall ms, three times
  routes     at the shim, on one context over the same columns, host clock around calls that end in a synchronise; the
             variants ALTERNATE -- one call of each per round, --queries rounds after a warm-up round:
             wide    pqps_filter_group_wide + pqps_bins_compact + the download of the runs, front on / front off
                     (pqps_ctx_set_option "wide_front"), and the download alone
             list    pqps_filter_scan, then pqps_group_wide_list + pqps_bins_compact + download
             sort    pqps_filter_scan, then pqps_group_sort + download
Every time is reported as [min, median, max] of its calls, so that the spread stands beside every difference.  Every route's
runs are compared with each other before a time is reported."""
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

WHERES = {"none": None, "40%": [("risk_level", ">", "3")], "0.01%": [("exit_code", "=", "7")]}


def columns(n, span, skewed, seed=1):
    rng = np.random.default_rng([seed, n, span, int(skewed)])
    user = rng.integers(0, span, n, dtype=np.int64)
    if skewed:
        user[rng.random(n) < 0.3] = span // 3
    user[0], user[n - 1] = 0, span - 1
    one = lambda text: (None, [text])
    return {"command_id": np.arange(n, dtype=np.uint64), "exit_code": rng.integers(0, 10_000, n).astype(np.int32),
            "risk_level": rng.integers(1, 6, n).astype(np.int32), "user_id": user.astype(np.int32),
            "sudo_used": np.zeros(n, np.uint8), "shell_type": one(b"bash"), "base_command": one(b"ls"), "host_name": one(b"h"),
            "user_name": one(b"u"), "timestamp": one(b"t"), "raw_command": one(b"ls"), "working_directory": one(b"/")}


def spread(ms):
    """[min, median, max] of a list of times."""
    return [min(ms), statistics.median(ms), max(ms)]


def once(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def engine_part(cols, n, k):
    eng = pq.HipEngine.from_columns(n, cols)
    out = {}
    try:
        for name, chain in WHERES.items():
            eng.group_top_result("user_id", None, "count", True, 20, chain)          # warm: code objects, the cached bounds
            res = [eng.group_top_result("user_id", None, "count", True, 20, chain) for _ in range(k)]
            out[name] = {"ms_engine": spread([r["seconds"] * 1e3 for r in res]), "matches": res[0]["total"], "groups": res[0]["groups_total"],
                         "top": res[0]["rows"][:3]}

            def host():
                got = eng.select_columnar(["user_id"], chain, text=False)
                try:
                    values, counts = np.unique(got["values"][0] if got["numRecords"] else np.zeros(0, np.int32), return_counts=True)
                finally:
                    eng.free_columnar(got)
                order = np.lexsort((values, -counts))[:20]
                return [(str(int(values[i])), int(counts[i])) for i in order]
            timed = [once(host) for _ in range(3)]
            top = timed[-1][1]
            out[name]["ms_host_unique"] = spread([ms for ms, _ in timed])
            out[name]["same_top"] = top == res[0]["rows"]
    finally:
        eng.close()
    return out


def shim_part(cols, n, span, k):
    ctx = pq.Context(0)
    L = pq.lib()
    pad = (n + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS
    dev = {}
    for name in ("user_id", "risk_level", "exit_code"):
        a = np.zeros(pad, np.int32)
        a[:n] = cols[name]
        dev[name] = ctx.malloc(a.nbytes)
        ctx.upload(dev[name], a.ctypes.data, a.nbytes)
    ctx.sync()
    schema = pq.SchemaSpec()
    for name in dev:
        schema.set_numeric(name, 4)
    gcol = pq.Column(dev["user_id"], 4, 0)
    bins = ctx.malloc(4 * span)
    ids, cnt = ctx.malloc(4 * n), ctx.malloc(64)
    out = {}

    def fetch(runs_dev, n_runs):
        host = np.zeros(max(1, 2 * n_runs.value), np.uint64)
        if n_runs.value:
            ctx.download(host.ctypes.data, runs_dev, 16 * n_runs.value)
            ctx.free(runs_dev)
        return host[:2 * n_runs.value]

    for name, chain in WHERES.items():
        pred, cids = pq.compile_where(schema, chain)
        pcols = pq.column_array([(dev[pq.COLUMNS[i]], 4) for i in cids]) if cids else pq.column_array([(dev["user_id"], 4)])
        nc = len(cids)

        def wide(download=True):
            runs_dev, n_runs = C.c_void_p(), C.c_uint64()
            pq.check(L.pqps_filter_group_wide(ctx.h, pcols, nc, n, C.byref(pred), None, C.byref(gcol), 0, span, bins, None), "wide")
            pq.check(L.pqps_bins_compact(ctx.h, bins, span, 0, C.byref(runs_dev), C.byref(n_runs), None), "compact")
            if download:
                return fetch(runs_dev, n_runs)
            if n_runs.value:
                ctx.free(runs_dev)
            return n_runs.value

        def selection():
            pq.check(L.pqps_filter_scan(ctx.h, pcols, nc, n, 0, C.byref(pred), ids, n, cnt, None), "scan")
            ctx.sync()
            m = C.c_uint64()
            ctx.download(C.byref(m), cnt, 8)
            return m.value

        def listed():
            m = selection()
            runs_dev, n_runs = C.c_void_p(), C.c_uint64()
            pq.check(L.pqps_group_wide_list(ctx.h, None, C.byref(gcol), n, ids, cnt, m, 0, 0, span, bins, None), "list")
            pq.check(L.pqps_bins_compact(ctx.h, bins, span, 0, C.byref(runs_dev), C.byref(n_runs), None), "compact")
            return fetch(runs_dev, n_runs)

        def sort():
            m = selection()
            runs_dev, n_runs = C.c_void_p(), C.c_uint64()
            pq.check(L.pqps_group_sort(ctx.h, C.byref(gcol), 0, span, None, n, ids, m, 0, C.byref(runs_dev), C.byref(n_runs), None), "sort")
            return fetch(runs_dev, n_runs)

        ref = wide()
        variants = (("wide_front_on", wide, -1), ("wide_front_off", wide, 0), ("wide_no_download", lambda: wide(False), -1),
                    ("list_wide", listed, -1), ("sort", sort, -1), ("selection", selection, -1))
        times = {label: [] for label, _, _ in variants}
        for rnd in range(k + 1):                                 # round 0 warms every variant up
            for label, fn, front in variants:
                ctx.set_option("wide_front", front)
                ms, got = once(fn)
                if rnd:
                    times[label].append(ms)
                elif not isinstance(got, int):
                    assert np.array_equal(got, ref), (name, label)
        ctx.set_option("wide_front", -1)
        row = {"ms_" + label: spread(ms) for label, ms in times.items()}
        row["runs"] = len(ref) // 2
        row["download_share"] = 1.0 - row["ms_wide_no_download"][1] / row["ms_wide_front_on"][1]
        out[name] = row
    for p in list(dev.values()) + [bins, ids, cnt]:
        ctx.free(p)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--queries", type=int, default=5)
    ap.add_argument("--spans", default="100000,1000000,10000000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    for span in [int(s) for s in a.spans.split(",")]:
        for skewed in (False, True):
            cols = columns(a.rows, span, skewed)
            r = {"rows": a.rows, "span": span, "skewed": skewed, "engine": engine_part(cols, a.rows, a.queries),
                 "shim": shim_part(cols, a.rows, span, a.queries)}
            results.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        path = pathlib.Path(a.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
