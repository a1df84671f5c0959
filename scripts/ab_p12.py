#!/usr/bin/env python3
"""Same-process A/B of the S1 scan over the u16 user_name column against its 12-bit packed copy (PQPS_WIDTH_P12).

    python scripts/ab_p12.py --rows 100000000 --libs head=parallel-query-processing-system_amd/libpqps_hip.so

The same codes go in as a u16 column and as a packed copy; both are scanned with the plane of sudo_used behind them --
(2,B,0) against (P,B,0) -- as ID list and as COUNT(*), by every build / setting named in --libs, launches interleaved,
device time from the HIP events on the dispatch.  `--copies 2` (the default) alternates two tables, so nothing a launch
reads was left in the Infinity Cache by the launch before it.

    --libs name=path[@VAR=value ...],...

A build reads its environment switches once, at its first launch: `@VAR=value` sets them in the process environment for that
build's warm-up launches, so several settings of ONE switch can be compared in one process on one table -- each from a copy of
the library file of its own (a path loaded twice is one library).  PQPS_NT_LOADS is read by every build, PQPS_VALU_CHAIN by
development builds (make libpqps_hip_dev.so).

    python scripts/ab_p12.py --rows 100000000 --steps-ab --libs head=parallel-query-processing-system_amd/libpqps_hip.so

Steps per wave are a context option ("steps": 0 = one step per wave, 1 = the shape's chain_steps()): `--steps-ab` runs the two
packed shapes -- (P,B,0) with S1, (P,0,0) with `user_name = "student1030"` -- as ID list and as COUNT(*) on two contexts of
the FIRST build in --libs, one with the option 0 and one with 1, over the same buffers, launches interleaved.

    python scripts/ab_p12.py --rows 100000000 --eq12-ab --libs head=parallel-query-processing-system_amd/libpqps_hip.so

The same for the context option "eq12" (0 = every step extracts the packed column's values, 1 = steps are first tested on the raw
dwords): the packed column's equality with and without the raw-dword test, in one build."""
import argparse
import ctypes as C
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import bench  # noqa: E402
import ab_libs  # noqa: E402

S1 = bench.QUERIES["S1"][0]
ONE = [("user_name", "=", "student1030")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--libs", required=True)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--steps-ab", action="store_true", help="the first build, context option 'steps' 0 against 1, shapes (P,B,0) and (P,0,0)")
    ap.add_argument("--eq12-ab", action="store_true", help="the first build, context option 'eq12' 0 against 1, shapes (P,B,0) and (P,0,0)")
    args = ap.parse_args()
    option_ab = "steps" if args.steps_ab else "eq12" if args.eq12_ab else None
    pq, _ = bench.load_pkg()
    ctx = pq.Context(0)
    n = args.rows
    padded = (n + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS
    u16, p12, p12_alone = ("u16", "p12", None) if not option_ab else (None, "(P,B,0)", "(P,0,0)")
    shapes = {name: [] for name in (u16, p12, p12_alone) if name}      # name -> column arrays, one per table copy
    preds, n_cols, bytes_per_row = {}, {u16: 2, p12: 2, p12_alone: 1}, {u16: 2.125, p12: 1.625, p12_alone: 1.5}
    for _ in range(max(1, args.copies)):
        t = pq.SyntheticTable(ctx, n, seed=0x5EED, columns=["user_name", "sudo_used"])
        pred, ids = pq.compile_where(t.schema, S1)
        assert [pq.COLUMNS[i] for i in ids] == ["user_name", "sudo_used"], ids
        pred_one, ids = pq.compile_where(t.schema, ONE)
        assert [pq.COLUMNS[i] for i in ids] == ["user_name"], ids
        preds = {u16: pred, p12: pred, p12_alone: pred_one}
        plane, packed = ctx.malloc(padded // 8), ctx.malloc(padded // 2 * 3)
        pq.check(pq.lib().pqps_pack_bits(ctx.h, t.ptr["sudo_used"], n, plane, 0, padded // 8, None), "pqps_pack_bits")
        ctx.pack12(t.ptr["user_name"], n, packed, 0, padded)
        ctx.sync()
        if u16:
            shapes[u16].append(pq.column_array([(t.ptr["user_name"], 2), (plane, pq.WIDTH_BITS)]))
        shapes[p12].append(pq.column_array([(packed, pq.WIDTH_P12), (plane, pq.WIDTH_BITS)]))
        if p12_alone:
            shapes[p12_alone].append(pq.column_array([(packed, pq.WIDTH_P12)]))
    ids_dev, cnt = ctx.malloc(4 * max(n // 2, 1024)), ctx.malloc(64)
    turn = [0]

    def run(L, h, shape, mode):
        cols = shapes[shape][turn[0] % len(shapes[shape])]
        turn[0] += 1
        if mode == "ids":
            rc = L.pqps_filter_scan(h, cols, n_cols[shape], n, 0, C.byref(preds[shape]), ids_dev, n // 2, cnt, None)
        else:
            rc = L.pqps_filter_count(h, cols, n_cols[shape], n, C.byref(preds[shape]), cnt, None)
        if rc != 0:
            sys.exit(L.pqps_last_error().decode())

    builds = []
    specs = args.libs.split(",")
    if option_ab:                                                    # one build, two contexts: the option off and on
        names = ("S=1", "S=2") if args.steps_ab else ("eq12=0", "eq12=1")
        specs = [(name, specs[0].split("=", 1)[1], v) for name, v in zip(names, (0, 1))]
    else:
        specs = [tuple(spec.split("=", 1)) + (None,) for spec in specs]
    for name, rest, value in specs:
        path, *env = rest.split("@")
        L = ab_libs.bind(ROOT / path, pq)
        L.pqps_last_kernel.restype = C.c_char_p
        h = C.c_void_p()
        if L.pqps_ctx_create(0, C.byref(h)) != 0:
            sys.exit(f"{name}: {L.pqps_last_error().decode()}")
        if value is not None and L.pqps_ctx_set_option(h, option_ab.encode(), value) != 0:
            sys.exit(f"{name}: {L.pqps_last_error().decode()}")
        for kv in env:                                               # read once, by this build's first launches below
            k, v = kv.split("=")
            os.environ[k] = v
        kernels = {}
        for shape in shapes:
            for mode in ("ids", "count"):
                for _ in range(2):
                    run(L, h, shape, mode)
                kernels[shape, mode] = L.pqps_last_kernel().decode()
        L.pqps_ctx_sync(h, None)
        for kv in env:
            del os.environ[kv.split("=")[0]]
        builds.append((name, L, h, kernels))
    print(f"rows={n:,}  copies={args.copies}  rounds={args.rounds} x reps={args.reps}", flush=True)
    for mode in ("ids", "count"):
        times = {(b[0], s): [] for b in builds for s in shapes}
        matches = {}
        for _ in range(args.rounds):
            for name, L, h, _k in builds:
                for shape in shapes:
                    L.pqps_ctx_set_timing(h, 1)
                    for _ in range(args.reps):
                        run(L, h, shape, mode)
                    ev, tot, k = C.c_double(), C.c_double(), C.c_int()
                    L.pqps_ctx_kernel_time(h, C.byref(ev), C.byref(tot), C.byref(k))
                    L.pqps_ctx_set_timing(h, 0)
                    times[name, shape].append(tot.value / k.value * 1e3)
                    m = C.c_uint64()
                    ctx.download(C.byref(m), cnt, 8)
                    matches[shape] = m.value
        for shape in shapes:
            for name, _L, _h, kernels in builds:
                t = times[name, shape]
                med = statistics.median(t)
                byts = n * bytes_per_row[shape] + (4 * matches[shape] if mode == "ids" else 8)
                print(f"{shape}/{mode} {name:>10}: {med:6.1f} us [{min(t):.1f}..{max(t):.1f}]  {byts / (med * 1e-6) / 8e12:.3f} of 8 TB/s"
                      f"  ({matches[shape]:,} matches)  {kernels[shape, mode]}", flush=True)


if __name__ == "__main__":
    main()
