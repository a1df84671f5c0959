"""Batch INSERT on a synthetic engine without host rows.

    python scripts/insert_bench.py [--rows 100000000] [--launches 20] [--batch 65536] [--new-names 64] [--out results/insert_bench.json]

(a) the remap pass alone, at the shim, on a 2-byte code column of --rows rows with a 2 064-entry table (the synthetic user_name
    dictionary + 64 names): pqps_remap_codes in place in the LDS form and in the global form, and a 1 -> 2 byte widening of a
    1-byte column -- beside pqps_bump_codes on the same 2-byte column, which is what ONE new string costs without the batch
    path.  Each figure: --launches back-to-back launches between two stream synchronisations, host time / launches; bytes/s
    over (src_width + dst_width) x rows.
(b) a batch of --batch rows that brings --new-names new user names through executeQueryInsertColumnsHIP (three batches in a
    row, each with names of its own), beside executeQueryInsertHIP row by row: 256 rows, 8 of them with a new name, reported
    PER ROW (a per-row figure, not a measured run of --batch rows).
A library without the batch path (the parent commit) runs the pqps_bump_codes and executeQueryInsertHIP parts alone."""
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


def have_batch_path():
    try:
        return hasattr(pq.lib(), "pqps_remap_codes")
    except AttributeError:
        return False


def timed(ctx, launches, f):
    f()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        f()
    ctx.sync()
    return (time.perf_counter() - t0) / launches * 1e6


def remap_pass(rows, launches, batch_path):
    L = pq.lib()
    L.pqps_bump_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
    ctx = pq.Context(0)
    rng = np.random.default_rng(7)
    padded = (rows + 4095) // 4096 * 4096
    wide = np.zeros(padded, dtype=np.uint16)
    wide[:rows] = rng.integers(0, 2000, rows, dtype=np.uint16)
    narrow = np.zeros(padded, dtype=np.uint8)
    narrow[:rows] = rng.integers(0, 16, rows, dtype=np.uint8)
    wide_dev, bump_dev, narrow_dev, out_dev = (ctx.malloc(padded * 2), ctx.malloc(padded * 2), ctx.malloc(padded), ctx.malloc(padded * 2))
    ctx.upload(wide_dev, wide.ctypes.data, wide.nbytes)
    ctx.upload(bump_dev, wide.ctypes.data, wide.nbytes)
    ctx.upload(narrow_dev, narrow.ctypes.data, narrow.nbytes)
    res = {}
    us = timed(ctx, launches, lambda: pq.check(L.pqps_bump_codes(ctx.h, bump_dev, 2, rows, 1000, None)))
    res["bump_codes_2B"] = dict(us=us, bytes_per_s=rows * 4 / us * 1e6)
    if batch_path:
        # a table that keeps every code below 2 000 below 2 064: launch after launch stays in range
        lut = (np.arange(max(2064, pq.REMAP_LDS_CODES), dtype=np.uint32) * 7) % 2000
        lut_dev = ctx.malloc(lut.nbytes)
        ctx.upload(lut_dev, lut.ctypes.data, lut.nbytes)
        small = np.arange(16, dtype=np.uint32) * 3
        small_dev = ctx.malloc(small.nbytes)
        ctx.upload(small_dev, small.ctypes.data, small.nbytes)
        for count in (2064, pq.REMAP_LDS_CODES):                   # (a table longer than 2 064 entries is read in its first 2 064)
            for name, form in (("remap_2B_in_place_lds", pq.REMAP_LDS), ("remap_2B_in_place_global", pq.REMAP_GLOBAL)):
                us = timed(ctx, launches, lambda: pq.remap_codes(ctx, wide_dev, 2, wide_dev, 2, rows, lut_dev, count, form))
                res[name + ("" if count == 2064 else "_%d" % count)] = dict(us=us, bytes_per_s=rows * 4 / us * 1e6)
        for name, form in (("widen_1B_to_2B_lds", pq.REMAP_LDS), ("widen_1B_to_2B_global", pq.REMAP_GLOBAL)):
            us = timed(ctx, launches, lambda: pq.remap_codes(ctx, narrow_dev, 1, out_dev, 2, rows, small_dev, 16, form))
            res[name] = dict(us=us, bytes_per_s=rows * 3 / us * 1e6)
        ctx.free(lut_dev)
        ctx.free(small_dev)
    for p in (wide_dev, bump_dev, narrow_dev, out_dev):
        ctx.free(p)
    ctx.close()
    return res


def batch_columns(B, first_id, names, rng):
    """B synthetic-looking rows; user names drawn from `names` (bytes)."""
    values = sorted(set(names))
    rank = {v: i for i, v in enumerate(values)}
    picks = rng.integers(0, len(names), B)
    cols = {
        "command_id": np.arange(first_id, first_id + B, dtype=np.uint64),
        "exit_code": rng.integers(0, 3, B).astype(np.int32),
        "user_id": rng.integers(1000, 3000, B).astype(np.int32),
        "risk_level": rng.integers(1, 6, B).astype(np.int32),
        "sudo_used": (rng.random(B) < 0.1).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, B).astype(np.uint8), pq.SYNTH_SHELLS),
        "user_name": (np.array([rank[names[i]] for i in picks], dtype=np.uint16), values),
        "host_name": (rng.integers(0, 16, B).astype(np.uint8), pq.SYNTH_HOSTS),
        "base_command": (rng.integers(0, 111, B).astype(np.uint8), pq.SYNTH_BASES),
    }
    for name, value in pq.SYNTH_CONSTANTS.items():
        cols[name] = (None, [value])
    return cols


def one_record(command_id, user_name):
    r = pq.Record()
    r.command_id, r.raw_command, r.base_command, r.shell_type, r.exit_code = command_id, pq.SYNTH_CONSTANTS["raw_command"], b"cmd005", b"bash", 0
    r.timestamp, r.sudo_used, r.working_directory = pq.SYNTH_CONSTANTS["timestamp"], False, pq.SYNTH_CONSTANTS["working_directory"]
    r.user_id, r.user_name, r.host_name, r.risk_level = 1030, user_name, b"labpc-01", 2
    return r


def engine_part(rows, B, new_names, batch_path):
    res = {}
    rng = np.random.default_rng(11)
    eng = pq.HipEngine.synthetic(rows)
    # row by row: 256 rows, every 32nd with a name the table has not seen
    known, fresh = [], []
    for i in range(256):
        new = i % 32 == 5
        r = one_record(10**12 + i, b"student1500_row%d" % i if new else b"student1030")
        t0 = time.perf_counter()
        ok = pq.lib().executeQueryInsertHIP(eng.e, b"commands", C.byref(r))
        (fresh if new else known).append((time.perf_counter() - t0) * 1e6)
        assert ok
    res["insert_row_by_row"] = dict(rows=256, new_names=len(fresh), us_per_row=(sum(known) + sum(fresh)) / 256,
                                    us_per_known_row=statistics.median(known), us_per_new_name_row=statistics.median(fresh))
    if batch_path:
        times = []
        for k in range(3):
            names = [b"student%d" % (1000 + i) for i in range(0, 2000, 3)] + [b"student1%03d_batch%d" % (i * 13, k) for i in range(new_names)]
            cols = batch_columns(B, 2 * 10**12 + k * B, names, rng)
            t0 = time.perf_counter()
            assert eng.insert_columns(B, cols) == B
            times.append((time.perf_counter() - t0) * 1e6)
        res["insert_batch"] = dict(rows=B, new_names=new_names, us=times, us_median=statistics.median(times),
                                   us_per_row=statistics.median(times) / B)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65_536)
    ap.add_argument("--new-names", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch_path = have_batch_path()
    res = dict(rows=args.rows, batch_path=batch_path)
    res.update(remap_pass(args.rows, args.launches, batch_path))
    res.update(engine_part(args.rows, args.batch, args.new_names, batch_path))
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
