"""Every query form over three and five shards on one card (tests/shard_matrix.py), and on the CPU everything that makes its
table and its model a reference: the properties of the table against the partitions of both layouts, the two model
functions the matrix adds (ColumnModel.group_first / order_ids_by) against row-by-row loops, every route's plan and probes,
the forms of the three key lists, and the number of cases -- which the GPU tests then demand of the driver's output, so a
case that silently drops out fails them."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import column_model as cm
import qpelib as q
import shard_matrix as sm
import test_gpu_order_by as ob

pq = q.pq
N = sm.N
PARTITION = {3: [1708, 1708, 1707], 5: [1025, 1025, 1025, 1024, 1024]}
# cases of `run` per layout: 15 routes x 84 forms and the tickets, under two index configurations; of `history`: 2 routes x 22
# forms and the tickets, at the start and after each of its 7 writers that change the table
RUN_CASES = {3: 2 * (15 * 84 + 1), 5: 2 * (15 * 84 + 1)}
HISTORY_CASES = 8 * (2 * 22 + 1)


@functools.lru_cache(maxsize=None)
def model_of(k):
    return cm.ColumnModel(sm.table(), k)


def shards_holding(rows, k):
    """The shards of the k-shard layout that hold any of the rows: counted row by row against the partition."""
    first = sm.starts(N, k)
    held = [0] * k
    for r in rows:
        s = next(s for s in range(k) if first[s] <= r < first[s + 1])
        held[s] += 1
    return held


def route_rows(k, name, indexes=sm.INDEXES):
    return model_of(k).select_ids(sm.ROUTES[name][0], indexes)


# ---- the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_partition_and_bands(k):
    model = model_of(k)
    assert N == 5123 and model.shard_rows == PARTITION[k] == cm.partition(N, k)
    assert all(rows % pq.TILE_ROWS for rows in PARTITION[k])                       # a partial last tile in every shard
    assert set(sm.starts(N, 3)[1:-1]).isdisjoint(sm.starts(N, 5)[1:-1])            # the boundaries in different places
    assert np.array_equal(model.m["user_id"], 1000 + np.arange(N) // 256)
    held = {name: shards_holding(model.scan_rows(sm.ROUTES[name][0]).tolist(), k) for name in sm.ROUTES}
    assert sum(c > 0 for c in held["band_inside"]) == 1
    across = [c > 0 for c in held[f"band_across_{k}"]]
    assert sum(across) == 2 and across.index(True) + 1 == len(across) - 1 - across[::-1].index(True)   # two neighbours
    for name in ("band_ends", "ends_fused"):                                        # shards with rows but no match, in the middle
        assert held[name][0] and held[name][-1] and not any(held[name][1:-1]) and all(PARTITION[k][1:-1]), name
    assert held["band_all"] == PARTITION[k] == held["none"]
    assert held["nothing"] == [0] * k


@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_extremes_sit_in_the_chosen_shards(k):
    m, first = model_of(k).m, sm.starts(N, k)
    middle, last = range(first[1], first[-2]), range(first[-2], N)
    ids = m["command_id"]
    assert len(set(ids.tolist())) == N and ids.dtype == np.uint64
    assert (np.diff(ids.astype(object)) < 0).sum() > 1000 and (np.diff(ids.astype(object)) > 0).sum() > 1000      # not monotone
    assert (1 << 63) in ids.tolist() and (ids > np.uint64(1 << 63)).sum() > 500 and (ids < np.uint64(1 << 63)).sum() > 500
    assert int(np.argmin(ids)) in last and int(np.argmax(ids)) in middle and int(ids.max()) == sm.M64
    for column in ("exit_code", "risk_level"):
        v = m[column]
        assert np.flatnonzero(v == v.min()).tolist() == [sm.MIN_ROW] and sm.MIN_ROW in middle, column
        assert np.flatnonzero(v == v.max()).tolist() == [sm.MAX_ROW] and sm.MAX_ROW in last, column
    assert (int(m["exit_code"].min()), int(m["exit_code"].max())) == (sm.INT32_MIN, sm.INT32_MAX)
    # increasing and decreasing with the row: a LIMIT answer comes from the first shard alone, or from the last
    assert (np.diff(m["user_id"]) >= 0).all() and (np.diff(m["timestamp"][0].astype(np.int64)) < 0).all()
    model, every = model_of(k), list(range(N))
    for column, desc, where in (("user_id", False, 0), ("user_id", True, k - 1), ("timestamp", False, k - 1), ("timestamp", True, 0)):
        held = shards_holding(model.order_ids(column, every, desc, 20)[0], k)
        assert held[where] == 20 and sum(held) == 20, (column, desc)


@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_dictionary_values_by_shard(k):
    m = model_of(k).m
    codes, words = m["user_name"]
    assert len(words) == 300 and codes.dtype == np.uint16 and words == sorted(words)
    assert sorted(sm.COMMON) != sm.COMMON                                           # byte order is not insertion order
    assert words.index(b"student10") < words.index(b"student2")
    held = {w: shards_holding(np.flatnonzero(codes == i).tolist(), k) for i, w in enumerate(words)}
    assert sum(all(h) for h in held.values()) >= 100                                # values present in every shard
    for s in range(k):                                                              # a value present in shard s only
        assert [c > 0 for c in held[sm.only_name(k, s)]] == [t == s for t in range(k)], s
    skip = held[sm.skip_name(k)]
    assert skip[0] and skip[2] and not skip[1]
    assert len(m["host_name"][1]) == 256 and len(words) * 256 > cm.GROUP_MAX_BINS                      # the sparse pair form
    assert len(m["shell_type"][1]) * (int(m["risk_level"].max()) - int(m["risk_level"].min()) + 1) <= cm.GROUP_MAX_BINS
    assert m["raw_command"][0] is None and m["working_directory"][0] is None


@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_ties_span_every_boundary(k):
    risk = model_of(k).m["risk_level"]
    runs = np.flatnonzero(risk == sm.TIE).tolist()
    assert runs == [r for b in sm.boundaries() for r in range(b - 4, b + 4)]
    for b in sm.starts(N, k)[1:-1]:                                                 # four rows of the tie on either side
        assert shards_holding(range(b - 4, b + 4), k).count(4) == 2
    # ORDER BY risk_level DESC: behind the maximum the tie's rows in row order, through every shard
    order = model_of(k).order_ids("risk_level", list(range(N)), True, 1 + len(runs))[0]
    assert order == [sm.MAX_ROW] + runs and all(shards_holding(runs, k))


@pytest.mark.parametrize("probe_bool", [False, True])
@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_limit_edges_are_the_matches_of_one_shard(k, probe_bool):
    model = model_of(k)
    for config, indexes in sm.INDEX_CONFIGS.items():
        for name in sm.ROUTES:
            ids = model.select_ids(sm.ROUTES[name][0], indexes, probe_bool)
            held = shards_holding(ids, k)
            assert held == sm.shard_counts(ids, model.shard_rows)
            c = next((c for c in reversed(held) if c), 1)
            assert sm.limits_of(ids, model.shard_rows) == [1, max(1, c - 1), c, c + 1, len(ids) + 7, None], (name, config)
    ids = model.select_ids(sm.ROUTES["fused"][0], ())
    assert 2 < sm.limits_of(ids, model.shard_rows)[2] < len(ids)


# ---- the two model functions -----------------------------------------------------------------------------------------------------
def small_model():
    """The first 1025 rows of the table."""
    cut = 1025
    return cm.ColumnModel({c: (v[:cut] if isinstance(v, np.ndarray) else (None if v[0] is None else v[0][:cut], v[1])) for c, v in sm.table().items()})


def candidates(model):
    out = [model.select_ids(sm.ROUTES[name][0], sm.INDEXES) for name in ("none", "probe", "or_probes", "nothing", "fused", "band_across_5")]
    assert len(set(out[2])) < len(out[2]) and out[1] != sorted(out[1]) and out[3] == []        # rows twice, probe order, no row
    return out


def test_group_first_of_the_model_row_by_row():
    model = small_model()
    assert model.n == 1025
    for ids in candidates(model):
        for group in ("user_name", "risk_level", "sudo_used", "raw_command", None):
            for column in ("risk_level", "command_id", "user_name", "exit_code", "timestamp", "working_directory"):
                for desc in (False, True):
                    best = {}
                    for r in ids:
                        g = model.cell(r, group) if group else None
                        key = ob.cell_key(column, model.cell(r, column))
                        if g not in best:
                            best[g] = (key, r)
                            continue
                        bk, br = best[g]
                        if (key > bk if desc else key < bk) or (key == bk and r < br):
                            best[g] = (key, r)
                    order = sorted(best, key=lambda g: cm.grp.key_order(group, g)) if group else list(best)
                    want = [(g, best[g][1], model.cell(best[g][1], column)) for g in order]
                    assert model.group_first(group, column, ids, desc) == (want, len(ids)), (group, column, desc)


def test_order_ids_by_of_the_model_row_by_row():
    model = small_model()
    key_lists = list(sm.KEY_LISTS.values()) + [["user_id", ("timestamp", True)], [("sudo_used", True), "raw_command", ("host_name", True), "command_id"]]
    for ids in candidates(model):
        for keys in key_lists:
            pairs = [(k, False) if isinstance(k, str) else k for k in keys]
            images = {c: [ob.cell_key(c, t) for t in model.cells(c)] for c, _ in pairs}

            def before(x, y):
                """Row x against row y, key by key from the first, then by the row."""
                for c, desc in pairs:
                    a, b = images[c][x], images[c][y]
                    if a != b:
                        return (1 if a < b else -1) if desc else (-1 if a < b else 1)
                return -1 if x < y else 1 if x > y else 0

            order = []
            for r in ids:                                                           # insertion, one row at a time
                at = len(order)
                while at and before(r, order[at - 1]) < 0:
                    at -= 1
                order.insert(at, r)
            for limit in (1, 20, None):
                assert model.order_ids_by(keys, ids, limit) == (order[:limit] if limit else order, len(ids)), (keys, limit)


# ---- the routes, the key lists, the cases ----------------------------------------------------------------------------------------
def test_every_route_takes_its_plan():
    model = model_of(3)
    for name, (chain, plan, n_probes, n_probes_bool) in sm.ROUTES.items():
        got = sm.passes(model.m, chain)
        assert got == plan, (name, got)
        assert sm.probes(chain, sm.INDEXES) == n_probes and sm.probes(chain, sm.INDEXES, True) == n_probes_bool and sm.probes(chain, ()) == 0, name
        ids, scan = model.select_ids(chain, sm.INDEXES), model.scan_rows(chain).tolist()
        assert sorted(set(ids)) == scan and model.select_ids(chain, ()) == scan, name
        if n_probes == 0:
            assert ids == scan, name
    assert len(list(cm.leaves_of(sm.ROUTES["wide"][0]))) > 32
    probe, both = route_rows(3, "probe"), route_rows(3, "or_probes")
    assert probe != sorted(probe) and len(set(probe)) == len(probe)                 # probe order
    assert len(both) - len(set(both)) > 100                                         # the reference's duplicates
    plane = model.select_ids(sm.ROUTES["plane"][0], sm.INDEXES, True)
    assert plane != sorted(plane) and sorted(plane) == route_rows(3, "plane")       # with BOOL indexes probed: probe order
    member = [p for p in pq.compile_plan_sets(sm.spec_of(model.m), sm.ROUTES["member"][0]) if p[2] is not None]
    assert len(member) == 1 and member[0][2]["column"] == pq.COL["user_name"]
    assert all(len(route_rows(3, name)) > 0 for name in sm.ROUTES if name != "nothing")


def test_key_lists_take_the_planned_forms():
    model = model_of(3)
    assert set(sm.KEY_LISTS) == {pq.ORDER_PACK32, pq.ORDER_PACK64, pq.ORDER_CHAIN}
    for form, keys in sm.KEY_LISTS.items():
        assert sm.key_form(model, keys) == form, keys
    chain = sm.KEY_LISTS[pq.ORDER_CHAIN]
    assert [c for c, _ in chain] == ["exit_code", "risk_level", "command_id"]       # two i32 keys (one of full range) and command_id
    # most rows tie on the first key and many on the second: the comparison reaches the last key
    every = list(range(N))
    order = model.order_ids_by(chain, every)[0]
    assert order != model.order_ids_by(chain[:2], every)[0] and order != model.order_ids_by(chain[:1], every)[0]


@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_case_counts(k):
    model = model_of(k)
    per_config = [len(sm.cases(model, indexes)) for indexes in sm.INDEX_CONFIGS.values()]
    assert sum(per_config) == RUN_CASES[k]
    assert sum(len(sm.cases(model, sm.INDEXES, families=(f,))) for f in sm.FAMILIES) == per_config[0]
    whats = [what for what, _, _ in sm.cases(model, sm.INDEXES)]
    assert len(set(map(repr, whats))) >= len(whats) - 3 * len(sm.ROUTES) * 6        # (LIMIT values may coincide, nothing else)
    assert len(sm.ROUTES) == 15 and len(sm.cases(model, sm.INDEXES, routes=sm.HISTORY_ROUTES, full=False)) * 8 == HISTORY_CASES


@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_history_reaches_its_states_on_the_model(k):
    """The history without an engine: its own assertions (an empty shard in the middle, at the end, the matchless middle of
    the UPDATE, growth, the refusals) hold on the model and every case has a model answer."""
    h = sm.history(",".join("0" * k), dry=True)
    assert h.count == HISTORY_CASES
    writers = [entry[0] for entry in h.log]
    assert writers == ["DELETE", "UPDATE", "UPDATE", "batch INSERT", "DELETE", "INSERT", "INSERT", "DELETE", "batch INSERT"]
    assert [entry for entry in h.log if entry[0] in ("UPDATE", "INSERT")][1][-1] is None and h.log[6][-1] is None       # the refusals
    assert h.log[0][2] == [PARTITION[k][0], 0] + PARTITION[k][2:]
    assert h.log[4][2][-1] == 0 and h.log[4][2][1] == 0 and h.log[7][2] == [0] * k and h.model.shard_rows == [0] * (k - 1) + [1500]


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
_stopped = []                                                    # a child that ended by a signal or a timeout: nothing more is started


def devices_of(k):
    two_cards = pq.lib().pqps_device_count() >= 2
    return ",".join(str(s % 2 if two_cards else 0) for s in range(k))


def drive(what, k, want, timeout, **env):
    assert not _stopped, f"not started: an earlier child ended abnormally ({_stopped[0]})"
    devices = devices_of(k)
    try:
        p = subprocess.run([sys.executable, str(q.ROOT / "tests" / "shard_matrix.py"), what, devices], capture_output=True, text=True,
                           timeout=timeout, env=dict(os.environ, PQPS_DEVICES=devices, **env), cwd=str(q.ROOT / "tests"))
    except subprocess.TimeoutExpired:
        _stopped.append(f"{what} {devices}: timeout")
        raise
    if p.returncode < 0 or "illegal memory access" in p.stderr:
        _stopped.append(f"{what} {devices}: exit {p.returncode}")
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.split()[-3:] == ["CASES", str(want), "OK"], p.stdout[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_matrix(k):
    drive("run", k, RUN_CASES[k], 600)


@pytest.mark.gpu
@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_history(k):
    drive("history", k, HISTORY_CASES, 600)


@pytest.mark.gpu
def test_matrix_with_bool_indexes_probed():
    model = model_of(3)
    want = sum(len(sm.cases(model, indexes, True)) for indexes in sm.INDEX_CONFIGS.values())
    assert want == RUN_CASES[3]
    drive("run", 3, want, 600, PQPS_PROBE_BOOL="1")
