"""Value sets and the top-N groups under concurrent readers and a writer (tests/concurrent_sets.py): on the GPU its three
commands over both tables, over one and three shards and on a single lane; on the CPU everything that makes the driver a
checker -- ColumnModel.value_set against the plain-dict members_of and ColumnModel.group_top against group_top_matrix's
expectation, the numpy evaluation of a chain with sets against chain_true row by row, the pinned case lists, the epochs of the
recorded histories, the rule for what a set may answer against a brute-force schedule, every command against a SetEngine, and
four engines that are wrong on purpose (a set that outlives its writer, a registry slot handed out twice, a 65th set, a slot
that is not given back), which the driver must report."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import column_model as cm
import concurrent_matrix as cx
import concurrent_sets as cs
import group_top_matrix as gm
import qpelib as q
import shard_matrix as sm
import test_gpu_many_shards as ms
import test_gpu_value_sets as vsets

pq = q.pq
TABLES = {name: make() for name, make in cs.TABLES.items()}
READ_CASES = {(name, lanes): len(cs.read_cases(t, lanes)) for name, t in TABLES.items() for lanes in (4, 1)}
WRITER_CASES = {name: len(cs.writer_cases(t)) for name, t in TABLES.items()}
STATES, EPOCHS = {"matrix": 10, "wide": 6}, {"matrix": 8, "wide": 5}


def exact_checks(table, readers, gate):
    """The least the writers command can print: per reader GATE EXACT cases in every state and GATE EXACT set answers in every
    epoch, and the final pass of every case."""
    return STATES[table] * readers * gate + EPOCHS[table] * readers * gate + readers * WRITER_CASES[table]


def test_the_counts():
    assert READ_CASES == {("matrix", 4): 249, ("matrix", 1): 248, ("wide", 4): 167, ("wide", 1): 166}
    assert {name: (len(cs.top_cases(t)), len(cs.outer_cases(t)), len(cs.lifecycle_cases(t))) for name, t in TABLES.items()} == \
        {"matrix": (160, 72, 16), "wide": (80, 72, 14)}
    assert WRITER_CASES == {"matrix": 25, "wide": 13} and all(len(t.shared) == 8 and len(t.writer_specs) == 4 for t in TABLES.values())
    assert (cs.READERS, cs.READERS * cs.CAP_TRIES, cs.MAX_SETS) == (6, 96, 64)
    assert (exact_checks("matrix", cs.WRITER_READERS, cs.GATE), exact_checks("wide", cs.WRITER_READERS, cs.GATE)) == (845, 505)
    # at most 4 private sets a thread (a lifecycle holds at most 2, the tickets case 1) and the shared ones: the cap is never hit
    assert all(len(specs) <= 2 for t in TABLES.values() for specs, _ in t.private) and cs.READERS * 4 + 8 < 40 <= cs.MAX_SETS
    for t in TABLES.values():
        kinds = [(having[0] if having else None, column in cm.STRINGS) for _, column, _, having in t.shared]
        assert {(None, True), (None, False), ("count", True), ("sum", True), ("min", False)} <= set(kinds)
        assert any(leaf[1] == "IN SET" for _, _, chain, _ in t.shared for leaf in cm.leaves_of(chain))


@pytest.mark.parametrize("name", list(TABLES))
def test_the_routes_are_what_their_names_say(name):
    t = TABLES[name]
    model = cm.ColumnModel(t.columns())
    for where, chain in t.wheres.items():
        passes, probes = t.plans[where]
        assert (sm.passes(model.m, chain) if chain else (1, 0)) == passes and sm.probes(chain, t.indexes) == probes, where
    assert [t.plans[w] for w in ("fused", "wide", "or_probes")] == [((1, 0), 0), ((2, 0), 0), ((1, 0), 2)]
    spans = {c: (len(model.m[c][1]) if c in cm.STRINGS else int(model.m[c].max()) - int(model.m[c].min()) + 1) for c, _ in t.top}
    if name == "matrix":
        assert 290 < spans["user_name"] <= 65536 and spans["timestamp"] == sm.N and spans["risk_level"] == 10
        assert spans["exit_code"] == 1 << 32 and 4 * spans["exit_code"] > cs.TOP_BINS_BUDGET          # the sort route
        ref = cs.SetEngine(t, 1)
        assert [cs.make(ref, ("a",) + spec, {})[1] for spec in t.refused] == ["refused", "refused"]
    else:
        assert spans == {"user_name": 70_000, "exit_code": 100_001}                                 # above 65 536 bins, within the budget
        assert all(65536 < n and 32 * n <= cs.TOP_BINS_BUDGET and n <= cs.MEMBER_MAX_BITS for n in spans.values())


# ---- the model -------------------------------------------------------------------------------------------------------------------
def matrix_states():
    """The matrix table as it is, after the history's second step (an UPDATE with a new string), and empty."""
    states = []
    sm.history("0,0,0", dry=True, recorder=lambda model, step: states.append(cm.ColumnModel(model.m, 3)))
    assert len(states) == 10 and states[8].n == 0 and states[2].n < states[0].n
    return [states[0], states[2], states[8]]


def middle(values):
    return sorted(values)[len(values) // 2] if values else 0


@pytest.fixture(scope="module")
def states():
    return matrix_states()


@pytest.mark.parametrize("s", (0, 1, 2), ids=("untouched", "after_an_update", "empty"))
def test_value_set_equals_the_plain_dict_members(states, s):
    model = states[s]
    checked = 0
    for column in ("user_name", "risk_level"):
        cells = [vsets.sp.field(r, column) for r in model.records()[:model.n]] if model.n else []
        for chain in (None, sm.ROUTES["fused"][0]):
            rows = model.scan_rows(chain).tolist()
            keys, n = model.value_set(column, rows, None)
            assert n == len(rows) and keys == [vsets.text(v) for v in sorted(vsets.members_of(cells, None, rows, None))]
            for agg, vcol in (("count", None), ("sum", "exit_code"), ("sum", "command_id"), ("min", "exit_code"), ("max", "command_id")):
                values = model.numbers(vcol) if vcol else None
                per = {}
                for r in rows:
                    per.setdefault(cells[r], []).append(values[r] if vcol else 0)
                constant = middle([vsets.aggregate_of(agg, xs, vcol) for xs in per.values()])     # an aggregate some group has
                for op in vsets.OPS:
                    having = (agg, vcol, op, str(constant))
                    want = vsets.members_of(cells, values, rows, having)
                    keys, n = model.value_set(column, rows, having)
                    assert (keys, n) == ([vsets.text(v) for v in sorted(want)], len(rows)), (column, chain, having)
                    checked += 1
                    if model.n and op in ("<=", ">="):
                        assert want, (column, having)
    assert checked == 2 * 2 * 5 * 6
    if model.n == 0:
        assert model.value_set("user_name", [], ("count", None, "<", "5")) == ([], 0)       # a value without inner rows is no member


def test_sums_wrap_and_compare_as_the_header_says():
    model = cm.ColumnModel(sm.table())
    rows = model.scan_rows(None)
    ids = model.m["command_id"]
    wrapped = [int(ids[model.codes("shell_type") == k].sum(dtype=np.uint64)) for k in range(4)]
    plain = [sum(int(x) for x in ids[model.codes("shell_type") == k]) for k in range(4)]
    assert all(p > cm.M64 and w == p & cm.M64 for p, w in zip(plain, wrapped))                # every sum wraps
    for k in range(4):
        keys, _ = model.value_set("shell_type", rows, ("sum", "command_id", "=", str(wrapped[k])))
        assert keys == [sm.SHELLS[k].decode()]
    # the i32 sum is signed: exit_code holds INT_MIN and INT_MAX on this table
    negative, _ = model.value_set("user_name", rows, ("sum", "exit_code", "<", "0"))
    assert negative == [model.cell(sm.MIN_ROW, "user_name")]


def test_group_top_equals_the_matrix_expectation():
    cols = gm.table(2_000, 300)
    run = gm.Run.__new__(gm.Run)                                   # the model's side of a Run: no engine
    run.indexes, run.model = list(gm.INDEXES), cm.ColumnModel(cols)
    run.reset()
    checked = 0
    for column in ("user_name", "exit_code", "risk_level", "sudo_used"):
        for value in (None, "risk_level", "command_id"):
            for where in gm.WHERES:
                for by in gm.orders(value):
                    for descending in (False, True):
                        for limit in (1, 10, 0):
                            got = run.model.group_top(column, value, run.rows(where), by, descending, limit)
                            assert got == run.expected(column, value, where, by, descending, limit), (column, value, where, by, descending, limit)
                            checked += 1
    assert checked == 4 * (2 + 5 + 5) * len(gm.WHERES) * 2 * 3
    assert run.model.group_top("user_name", None, run.rows("none"), "count", True, None)["groups_total"] == len(set(run.model.cells("user_name")))


def test_a_chain_with_sets_is_the_in_list_chain_row_by_row():
    """member_mask (numpy) against python_mask (chain_true) over the same resolved chain, and the index walk over it."""
    t = TABLES["matrix"]
    ref = cs.SetEngine(t, 1)
    shared, _ = cs.make_shared(t, ref)
    model = ref.model
    chains = list(t.chains.values()) + [[cs.S(name, column, negate)] for name, column, _, _ in t.shared for negate in (False, True)]
    for chain in chains:
        plain = ref.resolved(cs.bind(chain, shared))
        assert cm.has_member_leaf(plain) and not any(leaf[1] in cm.VALUE_SET_OPERATORS for leaf in cm.leaves_of(plain))
        mask = model.mask(plain)
        assert np.array_equal(mask, model.python_mask(plain)), chain
        ids = model.select_ids(plain, t.indexes)
        assert sorted(set(ids)) == np.flatnonzero(mask).tolist() or sm.probes(plain, t.indexes), chain
        assert all(mask[r] for r in ids)
    said = dict((name, (vs.members, vs.rows)) for name, vs in shared.items())
    assert said["nobody"] == (0, 0) and said["shells"] == (4, sm.N) and 0 < said["hosts"][0] < 256 and 0 < said["often"][0] and 0 < said["names"][0]


# ---- the recorded histories and the epoch ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return {(name, k): cs.record(",".join("0" * k), TABLES[name]) for name in TABLES for k in (1, 3)}


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("name", list(TABLES))
def test_recorded_history_and_its_epochs(recorded, name, k):
    steps, want, final = recorded[name, k]
    kinds, refused = [kind for kind, _, _ in steps], [predicted is None for _, _, predicted in steps]
    if name == "matrix":
        assert kinds == ["DELETE", "UPDATE", "UPDATE", "batch INSERT", "DELETE", "INSERT", "INSERT", "DELETE", "batch INSERT"]
        assert refused == [False, False, True, False, False, False, True, False, False]
        assert cs.epochs_of(steps) == [0, 1, 2, 2, 3, 4, 5, 5, 6, 7]
        empty, n_final = 8, 1500
    else:
        assert kinds == ["UPDATE", "batch INSERT", "DELETE", "UPDATE", "DELETE"] and refused == [False, False, False, True, False]
        assert cs.epochs_of(steps) == [0, 1, 2, 3, 3, 4]
        empty, n_final = 5, 0
    # the rule: a successful step makes sets stale; the refused ones of these histories are refused before a dictionary changes
    # -- each brings a second value to a column without a buffer, which is looked for before anything is entered
    assert [cs.makes_stale(kind, predicted) for kind, _, predicted in steps] == [not r for r in refused]
    for (kind, args, _), r in zip(steps, refused):
        if r:
            row = args[0]
            assert cm.as_bytes(row["raw_command"]) != sm.RAW and kind in ("UPDATE", "INSERT")
    assert len(want) == STATES[name] and cs.epochs_of(steps)[-1] + 1 == EPOCHS[name] and final.n == n_final
    for s in range(len(steps)):                                                     # a refused step changes nothing, any other does
        assert (want[s + 1] == want[s]) == refused[s], s
    assert [what for what, _ in want[0]["cases"]][-1] == cs.TICKETS_CASE and len(want[0]["cases"]) == WRITER_CASES[name]
    # the empty table: a set has no members and no rows, IN SET selects nothing and NOT IN SET everything, which is nothing
    t = TABLES[name]
    assert want[empty]["sets"] == [(0, 0, [])] * 4
    for j, spec in enumerate(t.writer_specs):
        forms = [form for form, _ in t.writer_forms(spec[1])]
        assert forms == ["count", "keys", "ids", "top", "count"]
        assert want[empty]["uses"][j] == [0, [], [], {"rows": [], "total": 0, "groups_total": 0}, 0]
        assert want[0]["uses"][j][0] > 0 and want[0]["uses"][j][1] and want[0]["sets"][j][0] > 0
    if name == "wide":                                                              # what the steps are there for
        exits, names = [w["sets"][1] for w in want], [w["sets"][0] for w in want]
        assert str(cs.WIDE_NEW_EXIT) not in exits[0][2] and exits[1][2][-1] == str(cs.WIDE_NEW_EXIT)
        assert cs.HOT in names[2][2] and cs.HOT not in names[3][2] and names[3] == names[4]


# ---- what a set may answer -----------------------------------------------------------------------------------------------------------
def test_allowed_by_hand():
    epoch = [0, 1, 1, 2]                                                            # step 2 is refused
    assert cs.allowed([0], [0], epoch) == ([(0, 0)], False)
    assert cs.allowed([1], [0], epoch) == ([], True)                                # made before the write, asked after: refused
    assert cs.allowed([0, 1], [0], epoch) == ([(0, 0)], True)                       # asked across the write: either
    assert cs.allowed([2], [1], epoch) == ([(2, 1)], False)                         # a refused step in between: the set lives
    assert cs.allowed([1, 2], [1, 2], epoch) == ([(1, 1), (2, 1), (2, 2)], False)
    assert cs.allowed([3], [0, 1], epoch) == ([], True)
    assert cs.allowed([1], [0, 1], epoch) == ([(1, 1)], True)                       # made across the write: which side decides


def test_allowed_against_a_schedule():
    """Four writer steps as their events in time -- successful, refused, refused but stale-making (an UPDATE that had entered
    a string), successful -- gen = 2k + 1, the table and the epoch change at one moment, gen = 2k + 2.  A set is made at every
    moment and asked at every later one, each call reading gen before and after.  For what the driver observes -- the two
    windows and what the set said of itself -- allowed() must give exactly the outcomes that some such pair of calls has."""
    kinds = ("ok", "refused", "refused, stale", "ok")
    tables, epoch = [0], [0]                                                        # per state: which table it is, its epoch
    for kind in kinds:
        tables.append(tables[-1] + (kind == "ok"))
        epoch.append(epoch[-1] + (kind != "refused"))
    events = [e for k in range(len(kinds)) for e in (("gen", 2 * k + 1), ("state", k + 1), ("gen", 2 * k + 2))]
    gen, state, moments = 0, 0, [(0, 0)]
    for kind, value in events:
        gen, state = (value, state) if kind == "gen" else (gen, value)
        moments.append((gen, state))
    outcomes = {}
    for a, b, c, d, e, f in itertools.combinations_with_replacement(range(len(moments)), 6):
        made_in, asked_in = moments[b][1], moments[e][1]
        observed = (moments[a][0], moments[c][0], tables[made_in], moments[d][0], moments[f][0])
        outcome = "refused" if epoch[asked_in] != epoch[made_in] else (tables[asked_in], tables[made_in])
        outcomes.setdefault(observed, set()).add(outcome)
    assert len(outcomes) > 200
    for (c0, c1, said, u0, u1), real in outcomes.items():
        candidates = [s for s in cx.states_seen(c0, c1) if tables[s] == said]
        pairs, refusal = cs.allowed(cx.states_seen(u0, u1), candidates, epoch)
        assert {(tables[s], tables[c]) for s, c in pairs} | ({"refused"} if refusal else set()) == real, (c0, c1, said, u0, u1)


# ---- the driver without a device ---------------------------------------------------------------------------------------------------
def dry(capsys, monkeypatch, command, *args, lanes="4"):
    """The command in this process; -> (exit status, what it printed)."""
    monkeypatch.setenv("PQPS_ENGINE_LANES", lanes)
    status = 0
    try:
        command(*args)
    except SystemExit as e:
        status = e.code
    return status, capsys.readouterr().out


def parse_writers(out, table):
    words = out.split()[-9:]
    assert words[0::2] == ["EXACT", "STALE", "AMBIGUOUS", "STATES", "OK"] and words[7] == str(STATES[table]), out[-1000:]
    return int(words[1]), int(words[3])


@pytest.mark.parametrize("lanes", ("4", "1"))
@pytest.mark.parametrize("k", (1, 3))
def test_dry_readers(capsys, monkeypatch, k, lanes):
    status, out = dry(capsys, monkeypatch, cs.readers, ",".join("0" * k), "matrix", "dry", lanes=lanes)
    assert status == 0 and out.split()[-3:] == ["CASES", str(cs.DRY_READERS * READ_CASES["matrix", int(lanes)]), "OK"], out[-2000:]


def test_dry_readers_of_the_wide_table(capsys, monkeypatch):
    status, out = dry(capsys, monkeypatch, cs.readers, "0,0,0", "wide", "dry")
    assert status == 0 and out.split()[-3:] == ["CASES", str(cs.DRY_READERS * READ_CASES["wide", 4]), "OK"], out[-2000:]


@pytest.mark.parametrize("k", (1, 3))
def test_dry_cap(capsys, monkeypatch, k):
    status, out = dry(capsys, monkeypatch, cs.cap, ",".join("0" * k), "dry")
    assert status == 0 and out.split()[-7:] == ["MADE", "64", "REFUSED", "32", "AGAIN", "64", "OK"], out[-2000:]


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("name", list(TABLES))
def test_dry_writers(capsys, monkeypatch, name, k):
    status, out = dry(capsys, monkeypatch, cs.writers, ",".join("0" * k), name, "dry")
    assert status == 0, out[-2000:]
    exact, stale = parse_writers(out, name)
    assert exact >= exact_checks(name, cs.DRY_READERS, cs.DRY_GATE) and stale >= cs.DRY_READERS * (EPOCHS[name] - 1)


def first_line(status, out):
    assert status == 1 and "OK" not in out.split()[-1:], out[-500:]
    return out[out.index("DIFFERENT"):].splitlines()[0]


def test_a_set_that_outlives_its_writer_is_reported(capsys, monkeypatch):
    first = first_line(*dry(capsys, monkeypatch, cs.writers, "0,0,0", "matrix", "stale_set"))
    assert "('set', 'asked'" in first and "'states': [" in first and "'made_in': [" in first, first


def test_a_slot_handed_out_twice_is_reported(capsys, monkeypatch):
    first = first_line(*dry(capsys, monkeypatch, cs.readers, "0,0,0", "matrix", "crossed_set"))
    assert ("('lifecycle'" in first or "('tickets'" in first) and "'thread'" in first, first


@pytest.mark.parametrize("engine, what", (("leaky_cap", "('cap', 'made')"), ("leaky_free", "('cap', 'again')")))
def test_a_leaky_cap_is_reported(capsys, monkeypatch, engine, what):
    first = first_line(*dry(capsys, monkeypatch, cs.cap, "0", engine))
    assert what in first, first


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
_stopped = []                                                    # a child that ended by a signal or a timeout: nothing more is started


def drive(*command, **env):
    assert not _stopped, f"not started: an earlier child ended abnormally ({_stopped[0]})"
    devices = command[1]
    try:
        p = subprocess.run([sys.executable, str(q.ROOT / "tests" / "concurrent_sets.py"), *command], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, PQPS_DEVICES=devices, **env), cwd=str(q.ROOT / "tests"))
    except subprocess.TimeoutExpired:
        _stopped.append(f"{command}: timeout")
        raise
    if p.returncode < 0 or "illegal memory access" in p.stderr:
        _stopped.append(f"{command}: exit {p.returncode}")
    assert p.returncode == 0, (command, p.stdout[-3000:], p.stderr[-3000:])
    print(p.stdout[-800:])
    return p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
def test_readers(k):
    out = drive("readers", ms.devices_of(k), "matrix", PQPS_ENGINE_LANES="4")
    assert out.split()[-3:] == ["CASES", str(cs.READERS * READ_CASES["matrix", 4]), "OK"], out[-1000:]


@pytest.mark.gpu
def test_readers_on_one_lane():
    out = drive("readers", "0", "matrix", PQPS_ENGINE_LANES="1")
    assert out.split()[-3:] == ["CASES", str(cs.READERS * READ_CASES["matrix", 1]), "OK"], out[-1000:]


@pytest.mark.gpu
def test_readers_of_the_wide_table():
    out = drive("readers", "0", "wide", PQPS_ENGINE_LANES="4")
    assert out.split()[-3:] == ["CASES", str(cs.READERS * READ_CASES["wide", 4]), "OK"], out[-1000:]


@pytest.mark.gpu
def test_cap():
    out = drive("cap", "0", PQPS_ENGINE_LANES="4")
    assert out.split()[-7:] == ["MADE", "64", "REFUSED", "32", "AGAIN", "64", "OK"], out[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("name", list(TABLES))
def test_writers(name, k):
    exact, stale = parse_writers(drive("writers", ms.devices_of(k), name, PQPS_ENGINE_LANES="4"), name)
    assert exact >= exact_checks(name, cs.WRITER_READERS, cs.GATE) and stale >= cs.WRITER_READERS * (EPOCHS[name] - 1)
