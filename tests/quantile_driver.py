"""Exact percentiles through the engine (HipEngine.quantiles) over the table of tests/shard_matrix.py, against
tests/quantile_model.py over tests/column_model.py: the case list and the driver.  No expected answer comes from an engine.

    python tests/quantile_driver.py run <devices>        every WHERE route x every value column x the groups
    python tests/quantile_driver.py history <devices>    writers, and the percentiles of the new state after each

<devices> is the PQPS_DEVICES value the engines are created under ("0,0,0": three shards on one card).  Both print the number
of cases and OK, or exit non-zero with the first case that differs.  tests/test_gpu_quantiles.py runs both in this process
for one shard and starts a child per layout of several.

The table (shard_matrix.table(), 5 123 rows) has what a radix select can get wrong: command_id over the whole u64 range
(six passes, values either side of 2^32 and 2^63), exit_code from INT32_MIN to INT32_MAX (32 bits, three passes), a unique
timestamp of 5 123 values (13 bits: two passes; as a GROUP column more than 4096 groups), two single-valued string columns
without a buffer, user names that live in one shard only, and ties that span every shard boundary.  Routes: fused scans, a
WHERE of two passes, a member pass (NOT IN: the list form), index probes with rows listed twice, nothing, exactly one row, an
IN SET, and the rows either side of a shard boundary (a median whose neighbours sit on different shards)."""
import os
import sys

import numpy as np

import column_model as cm
import quantile_model as qm
import qpelib as q
import shard_matrix as sm

pq = q.pq
N = sm.N
SIX = [0, 1, 500_000, 950_000, 999_999, 1_000_000]
SIXTEEN = [0, 62_500, 125_000, 250_000, 333_333, 400_000, 499_999, 500_000, 500_001, 600_000, 700_000, 800_000, 900_000, 990_000, 999_999, 1_000_000]
FRACTIONS = [SIX, [500_000], SIXTEEN, [950_000, 0, 500_000, 950_000, 1, 500_000]]     # .., one, sixteen, repeats in no order
GROUPS = (None, "risk_level", "user_name")
WORDS_KNOB = "PQPS_QUANTILE_WORDS"               # lowers the words one launch counts: groups in batches (read per query)
SMALL_CAP = str(1 << 16)                         # 256 groups of 8 bits per launch, 16 of them with 16 slots each


def boundary_chains(n_shards):
    """The two and the four rows around the first shard boundary (of the three-shard layout on one shard)."""
    b = sm.starts(N, n_shards if n_shards > 1 else 3)[1]
    return {"across_2": sm.rows_between(b - 1, b), "across_4": sm.rows_between(b - 2, b + 1)}


def routes(n_shards):
    out = {name: chain for name, (chain, _, _, _) in sm.ROUTES.items()}
    out["one_row"] = [("timestamp", "=", sm.stamp(N - 1 - 1234).decode())]
    out.update(boundary_chains(n_shards))
    return out


def case(tag, eng, model, ids, value, group, ppm, chain):
    return (tag + (value, group, tuple(ppm)), lambda: eng.quantiles(value, ppm, group, chain),
            lambda: qm.column_expected(model, ids, value, ppm, group))


def cross_checks(eng, model, ids, chain, group):
    """p = 0 and p = 10^6 are aggregate's minimum and maximum, n is group_count's count, the keys and their order are its keys."""
    out = []
    for value in ("exit_code", "command_id"):
        def engine_says(value=value):
            got = eng.quantiles(value, [0, 1_000_000], group, chain)
            return [(k, n, v[0], v[1]) for k, n, v in got]
        out.append((("min/max", value, group), engine_says, lambda value=value: [(k, c, lo, hi) for k, c, _, lo, hi in eng.aggregate(value, group, chain)]))
    if group:
        out.append((("keys", group), lambda: [(k, n) for k, n, _ in eng.quantiles("risk_level", [500_000], group, chain)],
                    lambda: model.group_count(group, ids)))
    return out


def cases(eng, model, indexes, n_shards, names=None):
    todo, turn = [], 0
    made = {}
    for name, chain in routes(n_shards).items():
        if names is not None and name not in names:
            continue
        ids = model.select_ids(chain, indexes)
        for value in pq.COLUMNS:
            for group in GROUPS:
                todo.append(case((name,), eng, model, ids, value, group, FRACTIONS[turn % len(FRACTIONS)], chain))
                turn += 1
        for group in GROUPS:
            todo += [((name,) + what, e, m) for what, e, m in cross_checks(eng, model, ids, chain, group)]
        made[name] = ids
    assert names is not None or (made["nothing"] == [] and len(made["one_row"]) == 1 and len(made["across_2"]) == 2 and len(made["across_4"]) == 4)
    return todo


def set_cases(eng, model, indexes):
    """An IN SET: the members of a value set the engine keeps on the device, the model's as an IN list."""
    inner = [("risk_level", ">=", "4"), "AND", ("shell_type", "=", "fish")]
    vs = eng.value_set("user_name", inner)
    keys, _ = model.value_set("user_name", model.scan_rows(inner))
    assert 10 < len(keys) < 290 and vs.members == len(keys)
    chain = [vs.item(), "AND", ("exit_code", "<=", "1")]
    ids = model.select_ids(cm.resolve_sets(chain, {str(vs.id): keys}), indexes)
    assert len(ids) > 100
    todo = [case(("in_set",), eng, model, ids, value, group, SIX, chain)
            for value, group in (("timestamp", None), ("command_id", "user_name"), ("exit_code", "risk_level"), ("user_name", "host_name"))]
    return todo, vs


def batch_cases(eng, model, indexes):
    """GROUP BY timestamp: 5 123 groups; under the lowered cap they run in batches of consecutive bins."""
    todo = []
    for name in ("none", "probe", "member"):
        chain = sm.ROUTES[name][0]
        ids = model.select_ids(chain, indexes)
        for value, ppm in (("command_id", [500_000]), ("user_name", SIX), ("exit_code", SIXTEEN)):
            todo.append(case(("batches", name), eng, model, ids, value, "timestamp", ppm, chain))
    return todo


def special_names(n_shards):
    """User names whose rows all sit on one shard (the last one among them)."""
    return [sm.only_name(k, s).decode() for k in sm.LAYOUTS for s in range(k)] if n_shards in sm.LAYOUTS else []


def run(devices):
    n_shards = len(devices.split(","))
    columns, count = sm.table(), 0
    saved = os.environ.pop(WORDS_KNOB, None)
    try:
        for config, indexes in sm.INDEX_CONFIGS.items():
            model = cm.ColumnModel(columns, n_shards)
            eng = pq.HipEngine.from_columns(N, columns, indexes)
            try:
                assert eng.shards() == model.shard_rows, (eng.shards(), model.shard_rows)
                count += sm.compare(eng, cases(eng, model, indexes, n_shards), config)
                todo, vs = set_cases(eng, model, indexes)
                count += sm.compare(eng, todo, config)
                vs.free()
                for name in special_names(n_shards):                 # the group of a shard's own name is in the per-group answer
                    got = dict((k, (n, v)) for k, n, v in eng.quantiles("timestamp", [500_000], "user_name"))
                    assert got[name][0] == 3, (name, got[name])
                full = eng.quantiles_result("command_id", [500_000], "timestamp")[1]["passes"]
                os.environ[WORDS_KNOB] = SMALL_CAP
                count += sm.compare(eng, batch_cases(eng, model, indexes), config)
                batched = eng.quantiles_result("command_id", [500_000], "timestamp")[1]["passes"]
                assert batched > 4 * full, (full, batched)              # the same passes, each in batches of 256 groups
                del os.environ[WORDS_KNOB]
            finally:
                eng.close()
    finally:
        os.environ.pop(WORDS_KNOB, None)
        if saved is not None:
            os.environ[WORDS_KNOB] = saved
    print("CASES", count, "OK", flush=True)
    return count


HISTORY_NAMES = ("none", "fused", "member", "or_probes", "one_value")


def history(devices):
    """insert_rows with a new smallest string and an i32 below the old minimum, an UPDATE of the value columns, a DELETE:
    after each the percentiles are the model's over the new state -- bounds and dictionaries moved under cached plans."""
    n_shards = len(devices.split(","))
    columns = sm.table()
    model = cm.ColumnModel(columns, n_shards)
    eng = pq.HipEngine.from_columns(N, columns, sm.INDEXES)
    count = 0

    def check(note):
        eng.n = eng.e.contents.num_records
        assert eng.n == model.n and eng.shards() == model.shard_rows, (note, eng.n, eng.shards(), model.shard_rows)
        return sm.compare(eng, cases(eng, model, sm.INDEXES, n_shards, HISTORY_NAMES), note)

    try:
        count += check("start")                                       # the i32 bounds are cached from here on
        row = sm.one_row(7_000_001, user_name=b"aaa-first", user_id=5, risk_level=-3, timestamp=b"1999-01-01T00:00:00.000Z")
        assert model.insert_one(row) is True
        r = pq.Record()
        for column, value in row.items():
            setattr(r, column, value)
        assert eng.insert_rows([r]) == 1
        assert model.m["user_name"][1][0] == b"aaa-first" and int(model.m["user_id"].min()) == 5 and int(model.m["risk_level"].min()) == -3
        count += check("insert_rows")
        chain = sm.ROUTES["band_ends"][0]
        assignments = {"user_id": 2_000_000_000, "exit_code": -7, "user_name": "zzz-last"}
        assert sm.engine_step(eng, "UPDATE", (assignments, chain)) == sm.model_step(model, "UPDATE", (assignments, chain)) > 100
        count += check("update")
        gone = [("risk_level", ">=", "4")]
        assert sm.engine_step(eng, "DELETE", (gone,)) == sm.model_step(model, "DELETE", (gone,)) > 1000
        count += check("delete")
    finally:
        eng.close()
    print("CASES", count, "OK", flush=True)
    return count


def main(argv):
    what, devices = argv[1], argv[2]
    os.environ["PQPS_DEVICES"] = devices                            # read when an engine is created
    if what == "run":
        run(devices)
    elif what == "history":
        history(devices)
    else:
        raise SystemExit(f"quantile_driver: unknown command {what!r}")


if __name__ == "__main__":
    main(sys.argv)
