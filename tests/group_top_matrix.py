"""The top-N groups (HipEngine.group_top_result) against tests/group_top_model.py: the tables, the WHERE forms, the checks.

tests/test_gpu_group_top.py runs the checks in its own process over one shard; test_over_three_shards starts this file as a
child, once per check, because an engine reads PQPS_DEVICES when it is created:

    python tests/group_top_matrix.py run <devices> <check>     one of SHARD_CHECKS under PQPS_DEVICES=<devices> ("0,0,0": three shards)

Prints the number of engine answers compared and OK, or fails with the first that differs.  The rows of a WHERE come from
ColumnModel.select_ids (the oracle's scan, or its index walk with the probes' duplicates); no expected answer comes from an
engine."""
import os
import sys

import numpy as np

import column_model as cm
import group_top_model as gtm
import qpelib as q
import shard_matrix as sm
import test_gpu_insert_batch as ib

pq = q.pq
N = 150_000
USERS = 70_000                                                   # a dictionary of 4-byte codes: past the 65 536 bins of group_count
EXIT_LO, EXIT_HI = -50_000, 50_000                               # exit_code spans 100 001 values
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1
HOSTS = [b"host-%03d" % i for i in range(256)]
SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
BASES = [b"cat", b"cd", b"grep", b"ls", b"make", b"rm", b"ssh", b"vim"]
STAMP, RAW, DIR = b"2025-01-01T00:00:00.000Z", b"ls -la", b"/home/u"
INDEXES = ib.INDEXES
LIMITS = (1, 10, "all", "all+1", 0)
COMPARED = [0]


def user_words(count):
    return [b"user-%06d" % i for i in range(count)]


def table(n=N, users=USERS, extremes=False, seed=7):
    """The columns from_columns takes.  user_name: `users` strings, one of which owns a fifth of the rows, most of the others
    one to four rows (many groups share a count).  exit_code: [EXIT_LO, EXIT_HI] with both ends, or with `extremes` INT_MIN and
    INT_MAX too.  command_id: every fifth at or above 2^63."""
    rng = np.random.default_rng([seed, n, users])
    row = np.arange(n)
    names = rng.integers(0, users, n)
    names[rng.random(n) < 0.2] = users // 3
    if n >= 2:
        names[0], names[n - 1] = 0, users - 1
    exit_code = rng.integers(EXIT_LO, EXIT_HI + 1, n)
    exit_code[rng.random(n) < 0.1] = -7
    if n >= 4:
        exit_code[1], exit_code[n - 2] = EXIT_LO, EXIT_HI
        if extremes:
            exit_code[2], exit_code[n - 3] = INT32_MIN, INT32_MAX
    command_id = 1000 + 7 * rng.permutation(n).astype(np.uint64)
    command_id[row % 5 == 3] += np.uint64(1 << 63)
    code_dt = cm.code_dtype(users)
    return {
        "command_id": command_id, "exit_code": exit_code.astype(np.int32), "risk_level": rng.integers(1, 6, n).astype(np.int32),
        "user_id": (1000 + row // 4096).astype(np.int32), "sudo_used": (rng.random(n) < 0.3).astype(np.uint8),
        "shell_type": (rng.integers(0, 4, n).astype(np.uint8), list(SHELLS)),
        "base_command": (rng.integers(0, 8, n).astype(np.uint8), list(BASES)),
        "host_name": (rng.integers(0, 256, n).astype(np.uint8), list(HOSTS)),
        "user_name": (names.astype(code_dt), user_words(users)),
        "timestamp": (None, [STAMP]), "raw_command": (None, [RAW]), "working_directory": (None, [DIR]),
    }


def wide_chain(last_op="="):
    chain = []
    for i in range(40):
        chain += [("host_name", "=", HOSTS[6 * i + 1].decode()), "OR"]
    return chain + [("base_command", last_op, "make")]


# name: (chain, (scan passes, member passes), index probes under INDEXES).  "several_passes" and "member" list fewer rows than
# either wide column has bins, "dense_passes" more: all of them take the wide bins over the list.
WHERES = {
    "none": (None, (1, 0), 0),
    "one_pass": ([("shell_type", "=", "zsh"), "AND", ("base_command", "!=", "rm")], (1, 0), 0),
    "several_passes": (wide_chain(), (2, 0), 0),
    "dense_passes": (wide_chain("!="), (2, 0), 0),
    "member": ([("host_name", "IN", pq.in_list([HOSTS[i].decode() for i in (0, 40, 80, 120, 160, 200, 240)])), "AND", ("sudo_used", "=", "FALSE")], (1, 1), 0),
    "probes": ([("risk_level", ">=", "4"), "OR", ("user_id", "<=", "1003")], (1, 0), 2),
    "rare": ([("user_id", "=", "1002"), "AND", ("base_command", "=", "vim")], (1, 0), 1),
    "nothing": ([("risk_level", "=", "77")], (1, 0), 1),
}


class Run:
    """An engine and the model of the same columns; the rows of a WHERE and the folds over them are computed once."""

    def __init__(self, cols, indexes=(), n_shards=None):
        self.indexes = list(indexes)
        self.eng = pq.HipEngine.from_columns(cm.rows_of(cols), cols, self.indexes)
        self.model = cm.ColumnModel(cols, n_shards or max(1, len(self.eng.shards())))
        self.reset()

    def reset(self):
        self.ids, self.folds = {}, {}

    def rows(self, where):
        if where not in self.ids:
            self.ids[where] = np.asarray(self.model.select_ids(WHERES[where][0], self.indexes), dtype=np.int64)
        return self.ids[where]

    def fold(self, column, value, where):
        key = (column, value, where)
        if key not in self.folds:
            m = self.model
            f = gtm.fold(m.codes(column), m.m[value] if value else None, self.rows(where), value == "command_id")
            v = m.m[column]
            if isinstance(v, np.ndarray):
                f["text"] = ["true" if k else "false" for k in f["key"].tolist()] if column == "sudo_used" else [str(k) for k in f["key"].tolist()]
            else:
                f["text"] = [v[1][k].decode("latin-1") for k in f["key"].tolist()]
            self.folds[key] = f
        return self.folds[key]

    def expected(self, column, value, where, by, descending, limit):
        f = self.fold(column, value, where)
        idx = gtm.order(f["key"], f[by], descending, limit).tolist()
        fields = [f["text"], f["count"].tolist()] + ([f["sum"].tolist(), f["min"].tolist(), f["max"].tolist()] if value else [])
        return {"rows": [tuple(a[i] for a in fields) for i in idx], "total": len(self.rows(where)), "groups_total": len(f["key"])}

    def check(self, column, value, where, by, descending, limit):
        groups = len(self.fold(column, value, where)["key"])
        lim = groups if limit == "all" else groups + 1 if limit == "all+1" else limit
        got = self.eng.group_top_result(column, value, by, descending, lim, WHERES[where][0])
        got.pop("seconds")
        want = self.expected(column, value, where, by, descending, lim)
        if got != want:
            bad = next((i for i, (a, b) in enumerate(zip(got["rows"], want["rows"])) if a != b), None)
            raise AssertionError(f"group_top({column}, {value}, by={by}, desc={descending}, limit={lim}, where={where}): total {got['total']} / "
                                 f"{want['total']}, groups {got['groups_total']} / {want['groups_total']}, listed {len(got['rows'])} / "
                                 f"{len(want['rows'])}, first difference at {bad}: {got['rows'][bad] if bad is not None else None} / "
                                 f"{want['rows'][bad] if bad is not None else None}")
        COMPARED[0] += 1
        return got

    def close(self):
        self.eng.close()


def orders(value):
    return gtm.BY if value else ("key", "count")


def check_answers(run, column, value, where="none", limits=LIMITS):
    """Every order in both directions at every limit."""
    for by in orders(value):
        for descending in (False, True):
            for limit in limits:
                run.check(column, value, where, by, descending, limit)


def check_wheres(run, column, value, wheres):
    """Each WHERE form: the 10 largest groups, every group in key order, and with a value the smallest sums and every group
    by its maximum."""
    for where in wheres:
        got = run.check(column, value, where, "count", True, 10)
        run.check(column, value, where, "key", False, 0)
        if value:
            run.check(column, value, where, "sum", False, 7)
            run.check(column, value, where, "max", True, "all")
        if where == "nothing":
            assert got == {"rows": [], "total": 0, "groups_total": 0}


def check_plans(model):
    """The WHERE forms take the routes their names say (hipCompileWherePlan over the model's dictionaries)."""
    for name, (chain, want, probes) in WHERES.items():
        if chain is not None:
            assert sm.passes(model.m, chain) == want, (name, sm.passes(model.m, chain))
        assert sm.probes(chain, INDEXES) == probes, name


def check_ties(run):
    """Many groups share a count, and the hot name stands alone: the ties are what the key rule orders."""
    f = run.fold("user_name", None, "none")
    counts = f["count"]
    assert len(counts) > 50_000 and np.count_nonzero(counts == 1) > 10_000 and np.count_nonzero(counts == 2) > 10_000
    assert counts.max() > 0.19 * N and np.count_nonzero(counts == counts.max()) == 1
    top = run.check("user_name", None, "none", "count", True, 10)["rows"]
    assert top[0][0] == "user-%06d" % (USERS // 3) and top[0][1] == counts.max()
    low = run.check("user_name", None, "none", "count", False, 10)["rows"]
    assert [c for _, c in low] == [1] * 10 and [t for t, _ in low] == sorted(t for t, _ in low)


def check_equivalences(run, wheres=("none", "one_pass", "probes")):
    """For every column group_count takes: group_top(by="key", limit=0) is group_count / aggregate exactly."""
    for column in ("shell_type", "base_command", "host_name", "sudo_used", "risk_level", "user_id", "timestamp", "raw_command",
                   "working_directory"):
        for where in wheres:
            chain = WHERES[where][0]
            assert run.eng.group_top(column, None, "key", False, 0, chain) == run.eng.group_count(column, chain), (column, where)
            assert run.eng.group_top(column, None, "key", True, 0, chain) == run.eng.group_count(column, chain)[::-1], (column, where)
            for value in ("risk_level", "command_id"):
                assert run.eng.group_top(column, value, "key", False, 0, chain) == run.eng.aggregate(value, column, chain), (column, value, where)
            COMPARED[0] += 4
            run.check(column, "exit_code", where, "sum", True, 3)


MAIN_COLUMNS = ("user_name", "exit_code")


def check_main(indexes=(), columns=MAIN_COLUMNS, limits=LIMITS, equivalences=True):
    """The wide columns of the 150 000-row table: every answer with no WHERE (an engine without indexes), every WHERE form."""
    run = Run(table(), indexes)
    try:
        check_plans(run.model)
        wheres = [w for w in WHERES if indexes or WHERES[w][2] == 0 or w == "nothing"]
        for column in columns:
            with_refused = None
            try:
                run.eng.group_count(column)
            except pq.PqpsError as e:
                with_refused = e
            assert with_refused is not None, f"group_count({column}) must keep refusing more than 65 536 bins"
            for value in (None, "risk_level", "command_id"):
                if not indexes:
                    check_answers(run, column, value, limits=limits)
                check_wheres(run, column, value, wheres)
        if not indexes and "user_name" in columns:
            check_ties(run)
        if equivalences:
            check_equivalences(run, ("none", "one_pass") + (("probes",) if indexes else ()))
        if indexes:
            ids = run.rows("probes")
            assert len(set(ids.tolist())) < len(ids), "the probed WHERE must list some row twice"
    finally:
        run.close()


def check_extremes(indexes=()):
    """exit_code holds INT_MIN and INT_MAX: 2^32 bins, past the budget -- the sort route, over a list for every WHERE."""
    run = Run(table(20_000, 300, extremes=True), indexes)
    try:
        for value in (None, "risk_level", "command_id"):
            check_answers(run, "exit_code", value)
            check_wheres(run, "exit_code", value, [w for w in WHERES if indexes or WHERES[w][2] == 0 or w == "nothing"])
        keys = [t for t, _ in run.eng.group_top("exit_code", None, "key", False, 0)]
        assert keys[0] == str(INT32_MIN) and keys[-1] == str(INT32_MAX)
        check_answers(run, "user_name", "command_id", limits=(1, "all"))      # 300 names: the dense bins, ordered on the host
    finally:
        run.close()


def check_empty_table():
    cols = table(0, 5)
    run = Run(cols)
    try:
        for column in ("user_name", "exit_code", "sudo_used"):
            for value in (None, "risk_level"):
                for by in orders(value):
                    got = run.eng.group_top_result(column, value, by, True, 10, None)
                    got.pop("seconds")
                    assert got == {"rows": [], "total": 0, "groups_total": 0}, (column, value, by)
                    COMPARED[0] += 1
    finally:
        run.close()


def check_writers():
    """A batch INSERT whose new strings take user_name from below 65 536 strings to above it, then a DELETE, then an UPDATE:
    the model's answer after each."""
    start = 65_000
    run = Run(table(100_000, start, seed=11))
    L = pq.lib()

    def ask():
        run.reset()
        for value in (None, "command_id"):
            for where in ("none", "one_pass", "member"):
                run.check("user_name", value, where, "count", True, 10)
                run.check("user_name", value, where, "key", True, 25)
            run.check("user_name", value, "none", "key", False, 0)

    try:
        assert run.eng.group_count("user_name")                  # 65 000 strings: still a column group_count takes
        ask()
        B = 3000
        new = [b"user-%06d-new" % (i * 20) for i in range(1500)]  # sort between the old ones: every code above the first moves
        words = sorted(set(user_words(start)[:100]) | set(new))
        rng = np.random.default_rng(12)
        batch = table(B, 5, seed=13)
        batch["user_name"] = (rng.integers(0, len(words), B).astype(np.uint16), words)
        batch["user_name"][0][:len(words)] = np.arange(len(words))
        batch["command_id"] = np.arange(10_000_000, 10_000_000 + B, dtype=np.uint64)
        assert run.model.insert_batch(batch) == B and run.eng.insert_columns(B, batch) == B
        assert len(run.model.m["user_name"][1]) == start + 1500 > 65_536
        try:
            run.eng.group_count("user_name")
            raise AssertionError("group_count must refuse the widened dictionary")
        except pq.PqpsError:
            pass
        ask()
        chain = [("risk_level", ">=", "4"), "OR", ("shell_type", "=", "fish")]
        want = run.model.delete(chain)
        rs = L.executeQueryDeleteHIP(run.eng.e, b"commands", pq.WhereList(chain).ptr)
        assert rs.contents.success and rs.contents.numRecords == want > 30_000
        L.freeResultSet(rs)
        ask()
        chain = [("base_command", "=", "vim")]
        want = run.model.update({"user_name": "user-000777-renamed", "risk_level": 9}, chain)
        assert want is not None and run.eng.update({"user_name": "user-000777-renamed", "risk_level": 9}, chain) == want > 1000
        ask()
        run.check("user_name", "risk_level", "none", "max", True, 3)
    finally:
        run.close()


# What a child process of test_over_three_shards runs, one check per process: every WHERE form on each wide column without
# indexes (check_wheres lists every group by key and by MAX) and with them, the equivalences, the sort route, the empty table
# and the writers.
SHARD_CHECKS = {
    "user_name": lambda: check_main((), ("user_name",), limits=(10,), equivalences=False),
    "exit_code": lambda: check_main((), ("exit_code",), limits=(10,), equivalences=False),
    "indexed": lambda: check_main(INDEXES),
    "extremes": check_extremes,
    "empty_and_writers": lambda: (check_empty_table(), check_writers()),
}


if __name__ == "__main__":
    assert sys.argv[1] == "run" and os.environ.get("PQPS_DEVICES") == sys.argv[2], "python group_top_matrix.py run <devices> <check> under PQPS_DEVICES=<devices>"
    shards = len(sys.argv[2].split(","))
    probe = pq.HipEngine.from_columns(4096, table(4096, 300))
    assert len(probe.shards()) == shards, (probe.shards(), shards)
    probe.close()
    SHARD_CHECKS[sys.argv[3]]()
    print(f"shards={shards} compared={COMPARED[0]}")
    print("OK")
