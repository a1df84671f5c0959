"""Value sets -- IN (SELECT ... [HAVING]) with the set kept on the device -- against the older route.

    python scripts/value_set_bench.py [--rows 100000000] [--column-rows 20000000] [--span 1000000] [--rounds 7] [--out FILE]

(a) the synthetic table: a set of user_name without HAVING, with HAVING COUNT and with HAVING SUM; an outer COUNT and an outer
    ID query over each.  The older route is timed beside it, its answers compared for equality first: group_count / aggregate,
    the keys picked in Python, an IN ( ... ) text, the same outer query (the host parses the text and builds the bitmap).
(b) a from_columns table whose user_id spans --span values: the same with sets of user_id (the wide bins with HAVING, the
    global presence bitmap without).  The older route is select_columnar + numpy there (group_count refuses more than 65 536
    bins) and stops where the set has more than 65 536 members (PQPS_MEMBER_MAX_ITEMS): reported as null.
(c) pqps_bins_having alone at the shim against its traffic model: the bytes it reads per bin (4 for u32 counts; 8 for COUNT of
    valued bins; 16 for SUM / MIN / MAX) plus the bitmap it writes, at 8 TB/s.
Every figure is host time around a finished call, in ms; the series of one comparison alternate call by call after a warm-up;
medians with (min-max)."""
import argparse
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

OPS = {">=": lambda a, b: a >= b, ">": lambda a, b: a > b, "<": lambda a, b: a < b}


def alternated(fns, k):
    """Each of `fns` once as a warm-up, then k times in turn -> [median, min, max] ms each."""
    times = [[] for _ in fns]
    for f in fns:
        f()
    for _ in range(k):
        for i, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            times[i].append((time.perf_counter() - t0) * 1e3)
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def old_route_keys(eng, column, chain, having, wide):
    """The members by the older route: the grouped answer on the host, the keys picked in Python."""
    if wide:                                                              # group_count refuses: the rows themselves
        cols = [column] + ([having[1]] if having and having[1] else [])
        res = eng.select_columnar(cols, chain, text=False)
        try:
            if res["numRecords"] == 0:
                return []
            keys = res["values"][0]
            if having is None:
                return np.unique(keys).tolist()
            uniq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
            x = cnt if having[0] == "count" else np.bincount(inv, weights=res["values"][1].astype(np.float64)).astype(np.int64)
            return uniq[OPS[having[2]](x, int(having[3]))].tolist()
        finally:
            eng.free_columnar(res)
    if having is None or having[0] == "count":
        groups = eng.group_count(column, chain)
        return [k for k, c in groups if having is None or OPS[having[2]](c, int(having[3]))]
    return [k for k, c, s, lo, hi in eng.aggregate(having[1], column, chain) if OPS[having[2]](s, int(having[3]))]


def compare(eng, column, chain, having, outer_extra, rounds, wide=False):
    """One set: creation, the outer COUNT and ID query over it, and the same three by the older route."""
    made = []

    def create():
        made.append(eng.value_set(column, chain, having))

    def old_create():
        keys = old_route_keys(eng, column, chain, having, wide)
        return None if len(keys) > pq.MEMBER_MAX_ITEMS else [(column, "IN", pq.in_list(keys))]

    old_item = old_create()
    create()
    vs = made[0]
    out = dict(column=column, having=having, members=vs.members, rows=vs.rows, old_route_possible=old_item is not None)
    new_chain = [vs.item()] + outer_extra
    if old_item is not None:
        old_chain = old_item + outer_extra
        assert eng.count(new_chain) == eng.count(old_chain) and eng.select_ids(new_chain) == eng.select_ids(old_chain), "answers differ"
        out["matches"] = eng.count(new_chain)
        out["outer_count_ms"], out["old_outer_count_ms"] = alternated([lambda: eng.count(new_chain), lambda: eng.count(old_chain)], rounds)
        out["outer_ids_ms"], out["old_outer_ids_ms"] = alternated([lambda: eng.select_ids(new_chain), lambda: eng.select_ids(old_chain)], rounds)
        out["create_ms"], out["old_create_ms"] = alternated([create, old_create], rounds)
    else:
        out["matches"] = eng.count(new_chain)
        out["outer_count_ms"], out["outer_ids_ms"] = alternated([lambda: eng.count(new_chain), lambda: eng.select_ids(new_chain)], rounds)
        out["create_ms"], out["old_keys_ms"] = alternated([create, lambda: old_route_keys(eng, column, chain, having, wide)], max(3, rounds // 2))
    for s in made:
        s.free()
    return out


def part_a(rows, rounds):
    eng = pq.HipEngine.synthetic(rows)
    inner = [("risk_level", "=", "5")]
    per_user = rows / pq.SYNTH_USERS
    out = [compare(eng, "user_name", inner, having, ["AND", ("sudo_used", "=", "FALSE"), "AND", ("risk_level", "=", "4")], rounds)
           for having in (None, ("count", None, ">=", str(max(1, int(per_user * 0.011)))), ("sum", "exit_code", ">", "0"))]
    eng.close()
    return out


def column_table(n, span, seed=11):
    rng = np.random.default_rng(seed)
    return {
        "command_id": np.arange(1, n + 1, dtype=np.uint64), "exit_code": rng.integers(0, 256, n).astype(np.int32),
        "risk_level": rng.integers(1, 6, n).astype(np.int32), "user_id": rng.integers(1000, 1000 + span, n).astype(np.int32),
        "sudo_used": (rng.random(n) < 0.3).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, n).astype(np.uint8), [b"bash", b"fish", b"sh", b"zsh"]),
        "base_command": (rng.integers(0, 8, n).astype(np.uint8), [b"cat", b"cd", b"grep", b"ls", b"make", b"rm", b"ssh", b"vim"]),
        "host_name": (rng.integers(0, 16, n).astype(np.uint8), [b"host-%02d" % i for i in range(16)]),
        "user_name": (rng.integers(0, 256, n).astype(np.uint8), [b"user-%03d" % i for i in range(256)]),
        "timestamp": (None, [b"2025-01-01T00:00:00.000Z"]), "raw_command": (None, [b"ls -la"]), "working_directory": (None, [b"/home/u"]),
    }


def part_b(n, span, rounds):
    eng = pq.HipEngine.from_columns(n, column_table(n, span))
    inner = [("risk_level", "=", "5"), "AND", ("sudo_used", "=", "TRUE")]
    per_value = n * 0.2 * 0.3 / span
    out = [compare(eng, "user_id", inner, having, ["AND", ("shell_type", "=", "zsh"), "AND", ("risk_level", "=", "1")], max(3, rounds // 2), wide=True)
           for having in (None, ("count", None, ">=", str(int(per_value * 4) + 1)), ("sum", "exit_code", ">", str(int(per_value * 128 * 4))))]
    eng.close()
    return out


def part_c(rounds):
    ctx = pq.Context(0)
    out = []
    for n in (65_536, 1_000_000, 8_000_000):
        rng = np.random.default_rng(n)
        fields = np.ascontiguousarray(np.stack([rng.integers(0, 9, n), rng.integers(-1000, 1000, n), rng.integers(0, 1 << 62, n),
                                                rng.integers(0, 1 << 62, n)]).astype(np.int64).view(np.uint64))
        counts = fields[0].astype(np.uint32)
        bins_v, bins_c = ctx.malloc(fields.nbytes), ctx.malloc(counts.nbytes)
        bitmap, members = ctx.malloc((n + 63) // 64 * 8), ctx.malloc(8)
        ctx.upload(bins_v, fields.ctypes.data, fields.nbytes)
        ctx.upload(bins_c, counts.ctypes.data, counts.nbytes)

        def run(bins, valued, field):
            pq.check(pq.lib().pqps_bins_having(ctx.h, bins, n, valued, field, 5, 3, 1, bitmap, members, None))
            ctx.sync()

        cases = (("u32 counts", bins_c, 0, 0, 4), ("valued COUNT", bins_v, 1, 0, 8), ("valued SUM", bins_v, 1, 1, 16), ("valued MAX", bins_v, 1, 3, 16))
        meds = alternated([lambda b=b, v=v, f=f: run(b, v, f) for _, b, v, f, _ in cases], rounds * 3)
        for (name, _, _, _, per_bin), med in zip(cases, meds):
            model_us = n * (per_bin + 0.125) / 8e12 * 1e6
            out.append(dict(n_bins=n, layout=name, bytes_per_bin=per_bin, us=[round(x * 1e3, 2) for x in med], model_us=round(model_us, 3),
                            fraction_of_8TBs=round(model_us / (med[0] * 1e3), 4)))
        for p in (bins_v, bins_c, bitmap, members):
            ctx.free(p)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--column-rows", type=int, default=20_000_000)
    ap.add_argument("--span", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(rows=args.rows, column_rows=args.column_rows, span=args.span, rounds=args.rounds)
    res["kernel"] = part_c(args.rounds)
    if args.rows:
        res["synthetic"] = part_a(args.rows, args.rounds)
    if args.column_rows:
        res["columns"] = part_b(args.column_rows, args.span, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
