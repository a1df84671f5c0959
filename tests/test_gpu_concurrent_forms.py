"""Every query form under concurrent readers and a writer (tests/concurrent_matrix.py): on the GPU its two commands over one
and three shards and on a single lane; on the CPU everything that makes the driver a checker -- the window of states a call
can have seen against a brute-force schedule, the recorded history, both commands against a ModelEngine with the counts the
GPU tests demand of the driver's output, and two engines that are wrong on purpose (a stale grouped answer, answers handed to
the wrong thread), which the driver must report."""
import itertools
import os
import subprocess
import sys

import pytest

import column_model as cm
import concurrent_matrix as cx
import qpelib as q
import shard_matrix as sm
import test_gpu_many_shards as ms

pq = q.pq
READ_CALLS = cx.READERS * cx.READ_CASES                                             # 6 x 177
ONE_LANE_CALLS = cx.READERS * (cx.READ_CASES - 1)                                   # without the tickets case
EXACT_CHECKS = cx.STATES * cx.WRITER_READERS * cx.GATE + cx.WRITER_READERS * cx.HISTORY_CASES


def test_the_counts():
    assert (cx.READ_CASES, READ_CALLS, ONE_LANE_CALLS, cx.HISTORY_CASES, cx.STATES, EXACT_CHECKS) == (177, 1062, 1056, 45, 10, 975)
    assert cx.READERS > 4 and set(cx.READ_ROUTES) <= set(sm.ROUTES) and set(sm.HISTORY_ROUTES) <= set(cx.READ_ROUTES)
    plans = {name: sm.ROUTES[name][1:] for name in cx.READ_ROUTES}
    assert plans["wide"][0] == (2, 0) and plans["member"][0] == (1, 1) and plans["probe"][1] == 1 and plans["or_probes"][1] == 2


# ---- the window ----------------------------------------------------------------------------------------------------------------
def test_states_seen_by_hand():
    for (g0, g1), want in {
        (0, 0): [0], (4, 4): [2], (18, 18): [9],                                    # even and equal: one state
        (1, 1): [0, 1], (5, 5): [2, 3],                                             # inside one write
        (3, 4): [1, 2], (1, 2): [0, 1],                                             # began inside a write that then ended
        (4, 5): [2, 3], (0, 1): [0, 1],                                             # a write began meanwhile
        (2, 4): [1, 2], (2, 8): [1, 2, 3, 4], (3, 9): [1, 2, 3, 4, 5], (1, 6): [0, 1, 2, 3], (0, 18): list(range(10)),
    }.items():
        assert cx.states_seen(g0, g1) == want, (g0, g1)


def test_states_seen_against_a_schedule():
    """Three writer steps as their events in time: gen = 2k + 1, the table changes, gen = 2k + 2.  A call reads gen at some
    moment, sees the table at the same or a later one, and reads gen again at that or a later one: every (g0, g1) must give
    exactly the states that some such call can see."""
    steps = 3
    events = [e for k in range(steps) for e in (("gen", 2 * k + 1), ("state", k + 1), ("gen", 2 * k + 2))]
    gen, state, moments = 0, 0, [(0, 0)]
    for kind, value in events:
        gen, state = (value, state) if kind == "gen" else (gen, value)
        moments.append((gen, state))
    seen = {}
    for a, b, c in itertools.combinations_with_replacement(range(len(moments)), 3):
        seen.setdefault((moments[a][0], moments[c][0]), set()).add(moments[b][1])
    assert len(seen) == sum(range(1, 2 * steps + 2)) and (0, 2 * steps) in seen
    for (g0, g1), states in seen.items():
        assert cx.states_seen(g0, g1) == sorted(states), (g0, g1)


# ---- the recorded history --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3))
def test_recorded_history(k):
    steps, want, final = cx.record(",".join("0" * k))
    assert [kind for kind, _, _ in steps] == ["DELETE", "UPDATE", "UPDATE", "batch INSERT", "DELETE", "INSERT", "INSERT", "DELETE", "batch INSERT"]
    assert set(kind for kind, _, _ in steps) == set(sm.WRITERS)
    assert [predicted is None for _, _, predicted in steps] == [False, False, True, False, False, False, True, False, False]
    assert steps[5][2] is True and all(isinstance(steps[s][2], int) and steps[s][2] > 0 for s in (0, 1, 3, 4, 7, 8))
    assert len(want) == cx.STATES and want[0] == cx.model_answers(cm.ColumnModel(sm.table(), k), sm.HISTORY_ROUTES)
    assert want[-1] == cx.model_answers(final, sm.HISTORY_ROUTES) and final.n == 1500
    for s in range(len(steps)):                                                     # a refused step changes nothing, any other does
        assert (want[s + 1] == want[s]) == (steps[s][2] is None), s
    assert want[0][-1][0] == cx.TICKETS_CASE and sum("group" in what for what, _ in want[0]) == 3


# ---- the driver without a device ---------------------------------------------------------------------------------------------------
def dry(capsys, command, devices, engine, lanes="4", monkeypatch=None):
    """The command in this process; -> (exit status, what it printed)."""
    monkeypatch.setenv("PQPS_ENGINE_LANES", lanes)
    status = 0
    try:
        command(devices, engine)
    except SystemExit as e:
        status = e.code
    return status, capsys.readouterr().out


@pytest.mark.parametrize("lanes", ("4", "1"))
def test_dry_readers(capsys, monkeypatch, lanes):
    status, out = dry(capsys, cx.readers, "0,0,0", "dry", lanes, monkeypatch)
    calls = cx.DRY_READERS * (cx.READ_CASES - (lanes == "1"))
    assert status == 0 and out.split()[-3:] == ["CASES", str(calls), "OK"], out[-2000:]


@pytest.mark.parametrize("k", (1, 3))
def test_dry_writers(capsys, monkeypatch, k):
    status, out = dry(capsys, cx.writers, ",".join("0" * k), "dry", monkeypatch=monkeypatch)
    assert status == 0, out[-2000:]
    exact, ambiguous = parse_writers(out)
    assert exact >= cx.STATES * cx.DRY_READERS * cx.DRY_GATE + cx.DRY_READERS * cx.HISTORY_CASES and ambiguous >= 0


def test_a_stale_grouped_answer_is_reported(capsys, monkeypatch):
    status, out = dry(capsys, cx.writers, "0,0,0", "stale", monkeypatch=monkeypatch)
    assert status == 1 and "OK" not in out.split()[-1:], out[-500:]
    first = out[out.index("DIFFERENT"):].splitlines()[0]
    assert "'group'" in first and "'states': [" in first, first


def test_answers_handed_to_the_wrong_thread_are_reported(capsys, monkeypatch):
    status, out = dry(capsys, cx.readers, "0,0,0", "swapped", monkeypatch=monkeypatch)
    assert status == 1 and "OK" not in out.split()[-1:], out[-500:]
    first = out[out.index("DIFFERENT"):].splitlines()[0]
    assert "'group'" in first and "'thread'" in first, first


def parse_writers(out):
    words = out.split()[-7:]
    assert words[0] == "EXACT" and words[2] == "AMBIGUOUS" and words[4:] == ["STATES", str(cx.STATES), "OK"], out[-1000:]
    return int(words[1]), int(words[3])


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
_stopped = []                                                    # a child that ended by a signal or a timeout: nothing more is started


def drive(what, devices, **env):
    assert not _stopped, f"not started: an earlier child ended abnormally ({_stopped[0]})"
    try:
        p = subprocess.run([sys.executable, str(q.ROOT / "tests" / "concurrent_matrix.py"), what, devices], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, PQPS_DEVICES=devices, **env), cwd=str(q.ROOT / "tests"))
    except subprocess.TimeoutExpired:
        _stopped.append(f"{what} {devices}: timeout")
        raise
    if p.returncode < 0 or "illegal memory access" in p.stderr:
        _stopped.append(f"{what} {devices}: exit {p.returncode}")
    assert p.returncode == 0, (devices, p.stdout[-3000:], p.stderr[-3000:])
    print(p.stdout[-600:])
    return p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
def test_readers(k):
    out = drive("readers", ms.devices_of(k), PQPS_ENGINE_LANES="4")
    assert out.split()[-3:] == ["CASES", str(READ_CALLS), "OK"], out[-1000:]


@pytest.mark.gpu
def test_readers_on_one_lane():
    out = drive("readers", "0", PQPS_ENGINE_LANES="1")
    assert out.split()[-3:] == ["CASES", str(ONE_LANE_CALLS), "OK"], out[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
def test_writers(k):
    exact, _ = parse_writers(drive("writers", ms.devices_of(k), PQPS_ENGINE_LANES="4"))
    assert exact >= EXACT_CHECKS
