"""Value sets and the top-N groups from several host threads at once, with and without a writer, against tests/column_model.py.

tests/concurrent_matrix.py asks the older query forms from threads; this driver does the same for the two newest ones and for
the state they share between callers (include/executeEngine-hip.h, "VALUE SETS" and "THE TOP N GROUPS"): the registry of sets
that hangs off the table (made by readers, several at once; freed under the table's exclusive lock; made stale, all at once,
by every successful writer), the bitmaps an outer query reads without owning them, the per-query bins and bitmaps allocated on
the table's own context while other lanes have kernels running, and the cached i32 ranges that size the wide bins and the
bitmaps.  It keeps concurrent_matrix's conventions -- Verdict, states_seen, single_pass, one barrier, seeded orders per thread,
DIFFERENT and exit status 1 on the first difference -- and its rule that no expected answer comes from an engine: every case
is a function of (engine, shared sets), and what it must return is what the same function returns for a SetEngine, which is a
ColumnModel under one lock; the main thread evaluates it before any thread starts.

    python tests/concurrent_sets.py readers <devices> <table> [engine]
        READERS threads.  The main thread makes the table's SHARED sets (checked against the model) and then every thread walks
        every case once, in the order random.Random(t).shuffle gives: the top-N groups over every route of the table ("top"),
        outer queries and keys() over the shared sets ("outer", "keys"), private sets made, asked and freed -- the free takes
        the table's exclusive lock while the other threads have queries in flight ("lifecycle") -- and, with more than one
        lane, a set made, used and refused its free under three held tickets ("tickets").  Prints CASES <calls> OK.
    python tests/concurrent_sets.py cap <devices> [engine]
        READERS threads leave one barrier and each try CAP_TRIES sets of risk_level, freeing none: exactly HIP_MAX_VALUE_SETS
        attempts succeed, under distinct ids, each answering as the model does; the threads then free theirs while asking the
        ones not freed yet; then 64 more fit and the 65th does not.  Prints MADE 64 REFUSED 32 AGAIN 64 OK.
    python tests/concurrent_sets.py writers <devices> <table> [engine]
        The table's writer history, recorded on the model first (record()), replayed by one writer thread under WRITER_READERS
        readers with concurrent_matrix's gen counter and gate.  A reader alternates a top-N case, which must be the model's
        answer for one of the states its call can have seen, with one step of a set's life: it makes a set, asks it until an
        EXACT call sees it refused, frees it and makes the next.  What a set may answer is allowed() below.  Prints
        EXACT <n> STALE <k> AMBIGUOUS <m> STATES <s> OK.

<table> is "matrix" (shard_matrix.table(), 5 123 rows: the dense bins, the sort route over exit_code's full range, the two
refused set domains) or "wide" (group_top_matrix.table(40_000, 70_000): the wide bins of 4 and 32 bytes, a bitmap of 100 001
bits); both are in the suite at these sizes already.

THE EPOCH.  epoch(s) is the number of steps up to state s that make sets stale.  The header's rule: every successful writer
does, and so does an UPDATE that had put a new string into a dictionary before it was refused.  The refused steps of both
histories are refused BEFORE any dictionary changes -- an UPDATE that brings a second value to a column without a buffer fails
updateNeedsRebuildHIP, which looks at every assignment before updateInsertStringsHIP touches one (so the new user_name of the
wide history's refused UPDATE is not entered either), and the refused single INSERT fails the first pass of
appendRowDeviceTableHIP -- so here exactly the successful steps count (makes_stale; tests/test_gpu_concurrent_sets.py pins
the flags of both histories).

Every command prints the wall time of one single-threaded pass of its case list and of the threaded part (readers: also the
thread-seconds spent per kind of case); nothing depends on a time.  Run as a program, the interpreter's switch interval is set
to 0.5 ms: a thread that comes back from the engine then waits that long, not 5 ms, for one that is building an answer.

[engine] is left out on a GPU.  "dry" puts a SetEngine in the engine's place, with DRY_READERS threads and DRY_GATE; "stale_set",
"crossed_set", "leaky_cap" and "leaky_free" are SetEngines that are wrong on purpose, which the driver has to report."""
import os
import random
import sys
import threading
import time

import numpy as np

import column_model as cm
import concurrent_matrix as cx
import group_top_matrix as gm
import shard_matrix as sm

pq = sm.pq
READERS = cx.READERS
WRITER_READERS, GATE = cx.WRITER_READERS, 8
DRY_READERS, DRY_GATE = cx.DRY_READERS, cx.DRY_GATE
MAX_SETS = 64                                                    # HIP_MAX_VALUE_SETS
CAP_TRIES = 16
MEMBER_MAX_BITS = 1 << 27                                        # PQPS_MEMBER_MAX_BITS: the widest bitmap of a set without HAVING
TOP_BINS_BUDGET = 256 << 20                                      # HIP_TOP_BINS_BUDGET
WIDE_N, WIDE_USERS = 40_000, 70_000
_tickets_mutex = threading.Lock()


def S(name, attribute, negate=False):
    """The chain item that tests `attribute` against the set a case knows as `name` (bind() puts the id in)."""
    return (attribute, "NOT IN SET" if negate else "IN SET", "$" + name)


def bind(chain, sets):
    """The chain with every $name replaced by the id of sets[name]."""
    if chain is None:
        return None
    out = []
    for k, item in enumerate(chain):
        if k % 2 == 0 and isinstance(item, list):
            out.append(bind(item, sets))
        elif k % 2 == 0 and item[1] in cm.VALUE_SET_OPERATORS and item[2].startswith("$"):
            out.append((item[0], item[1], str(sets[item[2][1:]].id)))
        else:
            out.append(item)
    return out


def strip(res):
    res = dict(res)
    res.pop("seconds", None)
    return res


# ---- the two tables ------------------------------------------------------------------------------------------------------------
class Table:
    """What the commands need to know of a table: its columns, its WHERE routes, its sets, its forms, its history."""


def matrix():
    t = Table()
    t.name, t.n, t.indexes, t.columns = "matrix", sm.N, sm.INDEXES, sm.table
    # (chain, scan passes + member passes, index probes): None, fused, two passes, two probes
    t.wheres = {w: sm.ROUTES[w][0] for w in ("none", "fused", "wide", "or_probes")}
    t.plans = {w: sm.ROUTES[w][1:3] for w in t.wheres}
    # the dense bins (about 300 codes, 5 123 codes, a handful of i32 values) and the sort route (2^32 bins: past the budget)
    t.top = (("user_name", "exit_code"), ("timestamp", "exit_code"), ("risk_level", "exit_code"), ("exit_code", "command_id"))
    t.group, t.big, t.number, t.other_number = "user_name", "user_name", "risk_level", "exit_code"
    t.member = sm.ROUTES["member"][0][0]                            # user_name NOT IN (seven names): a member pass
    t.tickets = [(sm.ROUTES[r][0], count_only) for r, count_only in sm.TICKETS]
    t.refused = (("exit_code", None, None), ("exit_code", None, ("sum", "risk_level", ">", "0")))     # 2^32 values: no bitmap, no bins
    t.cells_of = lambda chain: chain
    t.history = sm.history
    return finish(t)


def wide():
    t = Table()
    t.name, t.n, t.indexes, t.columns = "wide", WIDE_N, gm.INDEXES, lambda: gm.table(WIDE_N, WIDE_USERS)
    t.wheres = {"none": None, "fused": gm.WHERES["one_pass"][0], "wide": gm.WHERES["several_passes"][0], "or_probes": gm.WHERES["probes"][0]}
    t.plans = {"none": ((1, 0), 0), "fused": gm.WHERES["one_pass"][1:], "wide": gm.WHERES["several_passes"][1:], "or_probes": gm.WHERES["probes"][1:]}
    t.top = (("user_name", "exit_code"), ("exit_code", "command_id"))       # 70 000 and 100 001 bins: 4 B each, 32 B with a value
    t.group, t.big, t.number, t.other_number = "host_name", "user_name", "exit_code", "risk_level"
    t.member = gm.WHERES["member"][0][0]
    t.tickets = [(gm.WHERES["one_pass"][0], False), (gm.WHERES["rare"][0], False), (gm.WHERES["probes"][0], True)]
    t.refused = ()
    # the cells of one band of 4 096 rows: turning 160 000 cells into Python strings, with the table held shared meanwhile, is
    # seconds per call once six threads take turns in the interpreter.  (The band is an index probe: the sets are the re-filter.)
    t.cells_of = lambda chain: [("user_id", "=", "1002"), "AND", chain]
    t.history = wide_history
    return finish(t)


def finish(t):
    big, number = t.big, t.number
    few = ("sudo_used", "=", "TRUE")
    # name, column B, the inner chain, HAVING
    t.shared = [
        ("names", big, t.wheres["fused"], None),                                         # no HAVING, a string column
        ("numbers", number, [few], None),                                                # no HAVING, an i32 column
        ("often", big, None, ("count", None, ">=", "3" if t.name == "wide" else "20")),  # HAVING COUNT
        ("summed", big, None, ("sum", "exit_code", ">", "2")),                           # HAVING SUM(exit_code)
        ("lowest", number, [("shell_type", "!=", "sh")], ("min", "command_id", "<", str(1 << 63))),  # HAVING MIN of the u64 column
        ("hosts", "host_name", [S("names", big), "AND", few], ("count", None, ">", "5")),   # an inner chain that names an earlier set
        ("shells", "shell_type", None, ("count", None, ">=", "0")),                      # the whole dictionary: folds to TRUE
        ("nobody", big, [("risk_level", "=", "77")], None),                              # the empty set: folds to FALSE
    ]
    t.forms = {
        "count": lambda e, c: e.count(c),
        "ids": lambda e, c: e.select_ids(c),
        "cells": lambda e, c: sm.columnar_rows(lambda: e.select_columnar(sm.CELLS, t.cells_of(c)), e)[0],
        "group": lambda e, c: e.group_count(t.group, c),
        "aggregate": lambda e, c: e.aggregate("exit_code", "shell_type", c),
        "top": lambda e, c: strip(e.group_top_result(big, "exit_code", "sum", True, 10, c)),
        "order": lambda e, c: e.order_ids("risk_level", c, True, 20),
        "distinct": lambda e, c: e.count_distinct("host_name", None, c),
    }
    # chains over several sets, a set beside a LIKE / IN member pass, an i32 set asked of another i32 column
    t.chains = {
        "member": [t.member, "AND", S("often", big)],
        "nested": [("risk_level", ">", "1"), "AND", [S("often", big), "OR", S("summed", big, True)]],
        "cross": [S("numbers", t.other_number, True), "OR", S("hosts", "host_name")],
        "folds": [S("shells", "shell_type"), "AND", [S("nobody", big), "OR", S("lowest", number)]],
    }
    # private sets: (sets made in order, [(form, chain)] asked of them); "$a", "$b" are the case's own
    a_forms = (("count", "ids"), ("group", "top"), ("aggregate", "order"), ("cells", "distinct"))
    t.private = []
    for k, (column, chain, having) in enumerate((
            (big, t.wheres["fused"], None), (number, None, None), (big, [few], ("count", None, ">", "1")),
            (big, t.wheres["wide"], ("max", "exit_code", ">=", "1")), (number, t.wheres["fused"], ("sum", "risk_level", ">", "30")),
            ("host_name", [t.member], ("count", None, ">=", "4")))):
        for pair in (a_forms[k % 4], a_forms[(k + 1) % 4]):
            t.private.append(([("a", column, chain, having)], [(pair[0], [S("a", column)]), (pair[1], [few, "AND", S("a", column, True)])]))
    t.private.append(([("a", big, [few], None), ("b", "host_name", [S("a", big, True)], ("count", None, ">", "2"))],
                      [("count", [S("a", big), "AND", S("b", "host_name")]), ("ids", [S("b", "host_name", True)])]))
    t.private.append(([("a", "shell_type", [S("often", big)], None)], [("group", [S("a", "shell_type"), "AND", S("names", big)]), ("count", [S("a", "shell_type", True)])]))
    for spec in t.refused:
        t.private.append(([("a",) + spec], []))
    t.ticket_set = ("a", big, t.wheres["fused"], ("count", None, ">=", "2"))
    # the writers' sets: a string column whose codes move, the i32 column whose range a writer widens; [(form, chain)] of each
    t.writer_specs = [("a", big, t.wheres["fused"], None), ("a", number, None, None), ("a", big, None, ("count", None, ">=", "2")),
                      ("a", number, [few], ("sum", "risk_level", ">", "4"))]
    t.writer_forms = lambda column: [("count", [S("a", column)]), ("keys", None), ("ids", [few, "AND", S("a", column, True)]),
                                     ("top", [S("a", column)]), ("count", [S("a", column, True)])]
    return t


TABLES = {"matrix": matrix, "wide": wide}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def limit_of(limit):
    return None if limit == "all" else limit


def top_cases(t, full=True):
    """The top-N groups: every route of the table.  With no WHERE every order in both directions at the limits 1 and 10 and in
    one direction with every group listed; under the fused, the two-pass and the two-probe WHERE one of each.  full=False: what a writer's readers loop over."""
    out = []

    def add(column, value, by, descending, limit, where):
        chain = t.wheres[where]
        out.append((("top", column, value, by, descending, limit, where),
                    lambda eng, shared: strip(eng.group_top_result(column, value, by, descending, limit_of(limit), chain))))

    for column, value_column in t.top:
        if not full:
            for where in t.wheres:
                add(column, value_column, "count", True, 10, where)
            add(column, value_column, "sum", False, "all", "none")
            add(column, None, "key", True, 1, "fused")
            continue
        for value in (value_column, None):
            orders = ("key", "count", "sum") if value else ("key", "count")
            for by, all_descending in zip(orders, (False, True, False)):
                for descending in (False, True):
                    for limit in (1, 10) + (("all",) if descending == all_descending else ()):   # (every group of a wide column is 70 000 rows of answer)
                        add(column, value, by, descending, limit, "none")
            for where in ("fused", "wide", "or_probes"):
                for by, descending, limit in zip(orders, (True, False, False), (10, "all", 1)):
                    add(column, value, by, descending, limit, where)
    return out


def ask_form(t, eng, form, chain, sets):
    """One reader form over a chain (or keys() of the set "a"); a refusal, COUNT's -1 included, is "refused"."""
    if form == "keys":
        return sm.ask(sets["a"].keys)
    got = sm.ask(lambda: t.forms[form](eng, bind(chain, sets)))
    return "refused" if form == "count" and got == -1 else got


def outer_cases(t):
    """The shared sets from outside: IN SET and NOT IN SET of each under COUNT and one more form, the chains of several sets
    under every form, and every set's keys."""
    out, forms = [], list(t.forms)
    for k, (name, column, _, _) in enumerate(t.shared):
        for negate in (False, True):
            for form in ("count", forms[1 + (2 * k + negate) % (len(forms) - 1)]):
                out.append((("outer", name, "NOT IN SET" if negate else "IN SET", form),
                            lambda eng, shared, form=form, chain=[S(name, column, negate)]: ask_form(t, eng, form, chain, shared)))
        out.append((("keys", name), lambda eng, shared, name=name: sm.ask(shared[name].keys)))
    for name, chain in t.chains.items():
        for form in forms:
            out.append((("outer", name, form), lambda eng, shared, form=form, chain=chain: ask_form(t, eng, form, chain, shared)))
    return out


def make(eng, spec, sets):
    """One set: -> (the set or None, what it says of itself: (members, rows, keys() or "refused"), or "refused")."""
    _, column, chain, having = spec
    try:
        vs = eng.value_set(column, bind(chain, sets), having)
    except pq.PqpsError:
        return None, "refused"
    return vs, (vs.members, vs.rows, sm.ask(vs.keys))


def lifecycle(t, eng, shared, specs, asks):
    """Private sets made in order, asked, freed in reverse order (each free waits like a writer), and asked once more."""
    sets, made, out = dict(shared), [], []
    try:
        for spec in specs:
            vs, says = make(eng, spec, sets)
            out.append(says)
            if vs is not None:
                made.append(vs)
                sets[spec[0]] = vs
        for form, chain in asks:
            out.append(ask_form(t, eng, form, chain, sets))
    finally:
        for vs in reversed(made):
            vs.free()
    return out + [eng.count([vs.item()]) for vs in made]           # freed: -1


def lifecycle_cases(t):
    return [(("lifecycle", k, tuple(spec[1] for spec in specs), tuple(form for form, _ in asks)),
             lambda eng, shared, specs=specs, asks=asks: lifecycle(t, eng, shared, specs, asks))
            for k, (specs, asks) in enumerate(t.private)]


def tickets_in_flight(eng, tickets, while_held):
    """shard_matrix.tickets_in_flight for any list of (chain, count only)."""
    if not isinstance(eng, pq.HipEngine):
        return eng.tickets(tickets, while_held)
    held = [eng.select_async(chain, count_only) for chain, count_only in tickets]
    out, ctx = [], pq.Context(0)
    try:
        assert all(held)
        while_held()
        for tk, (_, count_only) in reversed(list(zip(held, tickets))):
            n, res = eng.await_ticket(tk)
            assert n >= 0
            if count_only:
                out.append(int(n))
                continue
            got = np.zeros(max(n, 1), dtype=np.uint32)
            if n:
                ctx.download(got.ctypes.data, res.ids_dev, 4 * n)
            out.append(got[:n].tolist())
    finally:
        for tk in held:
            if tk:
                eng.release_ticket(tk)
        ctx.close()
    return out[::-1]


def held_tickets(t, eng):
    """Three tickets held under the mutex and, while they are: a set is made (a reader: legal), asked, and refused its free
    (which waits like a writer), after which it still answers; one top-N query goes past a writer that waits for the tickets.
    The set is freed once the tickets are released.  All of it is ONE answer: it must come from one state."""
    with _tickets_mutex:
        extra, made = [], []

        def while_held():
            vs, says = make(eng, t.ticket_set, {})
            made.append(vs)
            sets = {"a": vs}
            extra.append(says)
            extra.append(ask_form(t, eng, "count", [S("a", t.big)], sets))
            try:
                vs.free()
                extra.append("freed under a ticket")
            except pq.PqpsError:
                extra.append("free refused")
            extra.append(ask_form(t, eng, "ids", [S("a", t.big, True), "AND", ("sudo_used", "=", "TRUE")], sets))
            extra.append(strip(eng.group_top_result(t.top[0][0], t.top[0][1], "count", True, 10, t.wheres["fused"])))

        answers = tickets_in_flight(eng, t.tickets, while_held)
        for vs in made:
            if vs is not None:
                vs.free()
        return answers, extra


TICKETS_CASE = ("tickets", "set")


def tickets_case(t):
    return (TICKETS_CASE, lambda eng, shared: held_tickets(t, eng))


def read_cases(t, lanes):
    return top_cases(t) + outer_cases(t) + lifecycle_cases(t) + ([tickets_case(t)] if lanes > 1 else [])


def kind_of(what):
    """For the times a command prints: the kind of a case, the top-N cases that list every group and the outer forms apart."""
    return what[0] + (" all" if what[0] == "top" and what[5] == "all" else " " + what[-1] if what[0] == "outer" else "")


def make_shared(t, eng):
    """The shared sets, made by the calling thread: -> ({name: set}, [what each says of itself])."""
    shared, said = {}, []
    for spec in t.shared:
        vs, says = make(eng, spec, shared)
        assert vs is not None, spec
        shared[spec[0]] = vs
        said.append((("shared", spec[0]), says))
    return shared, said


# ---- an engine without a device ------------------------------------------------------------------------------------------------
class ModelSet:
    def __init__(self, engine, ident, column, keys, rows):
        self.engine, self.id, self.column, self.members, self.rows = engine, ident, column, len(keys), rows

    def item(self, attribute=None, negate=False):
        return (attribute or self.column, "NOT IN SET" if negate else "IN SET", str(self.id))

    def keys(self):
        return self.engine.keys_of(self.id)

    def free(self):
        self.engine.free_set(self.id)


class SetEngine(cx.ModelEngine):
    """concurrent_matrix.ModelEngine over either table, with value sets and the top-N groups: a registry of at most MAX_SETS
    sets that are not freed, each the key texts ColumnModel.value_set gave, all of them made stale by a successful writer;
    a chain that names one is the chain resolve_sets makes of it."""

    def __init__(self, t, n_shards, model=None):
        self.t = t
        self.model = model or cm.ColumnModel(t.columns(), n_shards)
        self.lock = threading.RLock()
        self.sets, self.next_id, self.holder = {}, 1, None

    def resolved(self, chain):
        named = {}
        for leaf in cm.leaves_of(chain):
            if leaf[1] in cm.VALUE_SET_OPERATORS:
                entry = self.sets.get(int(leaf[2]))
                if entry is None or entry["stale"]:
                    raise pq.PqpsError(f"value set {leaf[2]}: stale, freed or unknown")
                named[leaf[2]] = entry["keys"]
        return cm.resolve_sets(chain, named) if named else chain

    def rows(self, model, chain):
        return model.select_ids(self.resolved(chain), self.t.indexes, cx.probe_bool())

    def count(self, chain):
        def fold(m):
            try:
                return len(m.scan_rows(self.resolved(chain)))
            except pq.PqpsError:
                return -1
        return self.answer("count", fold)

    def group_top_result(self, column, value_column=None, by="count", descending=True, limit=10, chain=None):
        return self.answer("top", lambda m: dict(m.group_top(column, value_column, self.rows(m, chain), by, descending, limit), seconds=0.0))

    # ---- the sets ----
    def domain_refused(self, m, column, having):
        """The header's routes: without HAVING the bitmap takes MEMBER_MAX_BITS values; with it, above 65 536 bins, the bins
        (4 B, 32 B with a value) must fit TOP_BINS_BUDGET."""
        if column in cm.STRINGS:
            span = len(m.m[column][1])
        elif m.n == 0:
            return False
        else:
            span = int(m.m[column].max()) - int(m.m[column].min()) + 1
        if having is None:
            return span > MEMBER_MAX_BITS
        return span > cm.GROUP_MAX_BINS and span * (32 if having[1] else 4) > TOP_BINS_BUDGET

    def room(self):
        return len(self.sets) < MAX_SETS

    def build(self, m, column, chain, having):
        if self.domain_refused(m, column, having) or not self.room():
            raise pq.PqpsError(f"value_set({column!r}) refused")
        keys, rows = m.value_set(column, m.scan_rows(self.resolved(chain)), having)
        return self.register(column, keys, rows)

    def register(self, column, keys, rows):
        ident, self.next_id = self.next_id, self.next_id + 1
        self.sets[ident] = dict(column=column, keys=keys, stale=False, maker=threading.get_ident())
        return ModelSet(self, ident, column, keys, rows)

    def value_set(self, column, chain=None, having=None):
        return self.answer("value_set", lambda m: self.build(m, column, chain, having))

    def keys_of(self, ident):
        with self.lock:
            entry = self.sets.get(ident)
            if entry is None or entry["stale"]:
                raise pq.PqpsError(f"value set {ident}: stale or freed")
            return list(entry["keys"])

    def free_set(self, ident):
        if self.holder == threading.get_ident():
            raise pq.PqpsError(f"value set {ident}: free refused under a ticket")
        with self.lock:
            self.sets.pop(ident, None)

    def stale_all(self):
        for entry in self.sets.values():
            entry["stale"] = True

    def write(self, kind, args):
        got = super().write(kind, args)
        if got != "refused":                                         # (makes_stale: no refused step of these histories does)
            self.stale_all()
        return got

    def tickets(self, tickets, while_held):
        """The lock is kept while the tickets are, so whatever their holder asks meanwhile sees the state the tickets saw."""
        with self.lock:
            out = [len(self.model.scan_rows(chain)) if count_only else self.rows(self.model, chain) for chain, count_only in tickets]
            self.holder = threading.get_ident()
            try:
                while_held()
            finally:
                self.holder = None
            return out


class StaleSetEngine(SetEngine):
    """Wrong on purpose: a writer does not make the sets stale -- outer queries keep answering from the members a set had."""

    def stale_all(self):
        pass


class CrossedSetEngine(SetEngine):
    """Wrong on purpose: a creation returns the id of the set another thread made last -- one registry slot handed out twice."""

    def register(self, column, keys, rows):
        own = super().register(column, keys, rows)
        me = threading.get_ident()
        others = [ident for ident, entry in self.sets.items() if entry["maker"] != me]
        if others:
            own.id = others[-1]
        return own


class LeakyCapEngine(SetEngine):
    """Wrong on purpose: a 65th set is admitted."""

    def room(self):
        return len(self.sets) < MAX_SETS + 1


class LeakyFreeEngine(SetEngine):
    """Wrong on purpose: a freed set answers no more, but its slot is not given back."""

    def free_set(self, ident):
        with self.lock:
            if ident in self.sets:
                self.sets[-ident] = self.sets.pop(ident)


ENGINES = {"dry": SetEngine, "stale_set": StaleSetEngine, "crossed_set": CrossedSetEngine, "leaky_cap": LeakyCapEngine, "leaky_free": LeakyFreeEngine}


def make_engine(kind, t, n_shards):
    if kind is not None:
        return ENGINES[kind](t, n_shards)
    if t.name == "matrix":
        return cx.make_engine(None, n_shards)
    return pq.HipEngine.from_columns(t.n, t.columns(), t.indexes)


def answers(cases, ref, shared):
    return [(what, fn(ref, shared)) for what, fn in cases]


def bound(cases, eng, shared):
    """single_pass's calls: each case as a call without arguments."""
    return [(what, lambda fn=fn: fn(eng, shared)) for what, fn in cases]


# ---- readers ----------------------------------------------------------------------------------------------------------------------
def readers(devices, table, engine=None):
    n_shards = len(devices.split(","))
    lanes = int(os.environ.setdefault("PQPS_ENGINE_LANES", "4"))
    n_threads = DRY_READERS if engine else READERS
    t = TABLES[table]()
    cases = read_cases(t, lanes)
    ref = SetEngine(t, n_shards)
    ref_shared, want_shared = make_shared(t, ref)
    want = answers(cases, ref, ref_shared)
    eng = make_engine(engine, t, n_shards)
    try:
        assert eng.shards() == ref.model.shard_rows, (eng.shards(), ref.model.shard_rows)
        verdict, asked, spent = cx.Verdict(), [0] * n_threads, [{} for _ in range(n_threads)]
        shared, said = make_shared(t, eng)
        for (what, got), (_, wanted) in zip(said, want_shared):
            if got != wanted:
                verdict.differs(thread="main", what=what, got=got, want=wanted)
                verdict.end()
        calls = bound(cases, eng, shared)
        single = cx.single_pass(calls, want, verdict)
        barrier = threading.Barrier(n_threads)

        def walk(th):
            order = list(range(len(calls)))
            random.Random(th).shuffle(order)
            barrier.wait()
            for position, i in enumerate(order):
                if verdict.stop.is_set():
                    return
                t1 = time.perf_counter()
                got = calls[i][1]()
                asked[th] += 1
                spent[th][kind_of(want[i][0])] = spent[th].get(kind_of(want[i][0]), 0.0) + time.perf_counter() - t1
                if got != want[i][1]:
                    return verdict.differs(thread=th, position=position, what=want[i][0], got=got, want=want[i][1])

        threads = [verdict.guard(th, lambda th=th: walk(th)) for th in range(n_threads)]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        threaded = time.perf_counter() - t0
        if verdict.first is None:                                     # the shared sets are what they were, and go
            for (what, _), (_, wanted) in zip(said, want_shared):
                vs = shared[what[1]]
                got = (vs.members, vs.rows, sm.ask(vs.keys))
                if got != wanted:
                    verdict.differs(thread="main", what=what, got=got, want=wanted)
                    break
                vs.free()
    finally:
        eng.close()
    verdict.end()
    assert sum(asked) == n_threads * len(calls), asked
    print(f"TIMES one pass of {len(calls)} cases from one thread {single:.2f} s, {n_threads} threads x {len(calls)} cases {threaded:.2f} s, "
          f"{lanes} lane(s), table {table}; thread-seconds by kind of case "
          f"{ {kind: round(sum(sp.get(kind, 0.0) for sp in spent), 2) for kind in sorted(set().union(*spent))} }", flush=True)
    print("CASES", sum(asked), "OK", flush=True)


# ---- the cap ----------------------------------------------------------------------------------------------------------------------
def cap_chain(i):
    return [("risk_level", "<=", str(1 + i % 5))]


def cap(devices, engine=None):
    n_shards = len(devices.split(","))
    os.environ.setdefault("PQPS_ENGINE_LANES", "4")
    t = TABLES["matrix"]()
    ref = SetEngine(t, n_shards)
    want = []
    for i in range(5):                                                # what a set of cap_chain(i) answers, by i % 5
        vs = ref.value_set("risk_level", cap_chain(i))
        want.append((vs.members, vs.rows, ref.count([vs.item()])))
        vs.free()
    assert len(set(want)) == 5 and READERS * CAP_TRIES == MAX_SETS + 32
    eng = make_engine(engine, t, n_shards)
    try:
        verdict = cx.Verdict()
        made, refused = [[] for _ in range(READERS)], [0] * READERS
        freeing = [0] * READERS                                       # thread th is about to free, or has freed, its sets [0, freeing[th])
        barrier, filled = threading.Barrier(READERS, timeout=300), threading.Barrier(READERS, timeout=300)   # (a thread that raised breaks them)

        def says(vs):
            return (vs.members, vs.rows, eng.count([vs.item()]))

        def fill(th):
            barrier.wait()
            for i in range(CAP_TRIES):
                try:
                    made[th].append((i, eng.value_set("risk_level", cap_chain(i))))
                except pq.PqpsError:
                    refused[th] += 1
                    continue
                i, vs = made[th][-1]
                if says(vs) != want[i % 5]:
                    verdict.differs(thread=th, what=("cap", "made", i), got=says(vs), want=want[i % 5])
            filled.wait()
            # the registry is full and stays so until the first free: every set of every thread is there, once
            everyone = [vs for m in made for _, vs in m]
            if len(everyone) != MAX_SETS or sum(refused) != 32 or len({vs.id for vs in everyone}) != len(everyone):
                return verdict.differs(thread=th, what=("cap", "made"), got=(len(everyone), sum(refused), len({vs.id for vs in everyone})), want=(MAX_SETS, 32, MAX_SETS))
            filled.wait()
            rng = random.Random(th)
            for k, (i, vs) in enumerate(made[th]):
                other = rng.randrange(READERS)
                if made[other]:
                    j = rng.randrange(len(made[other]))
                    oi, ovs = made[other][j]
                    got = says(ovs)
                    if got != want[oi % 5] and not (got[2] == -1 and freeing[other] > j):
                        return verdict.differs(thread=th, what=("cap", "another thread's set", other, j), got=got, want=want[oi % 5])
                if says(made[th][-1][1]) != want[made[th][-1][0] % 5]:
                    return verdict.differs(thread=th, what=("cap", "a set not freed yet", k), got=says(made[th][-1][1]), want=want[made[th][-1][0] % 5])
                freeing[th] = k + 1
                vs.free()
                if eng.count([vs.item()]) != -1:
                    return verdict.differs(thread=th, what=("cap", "freed", k), got=eng.count([vs.item()]), want=-1)

        threads = [verdict.guard(th, lambda th=th: fill(th)) for th in range(READERS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        verdict.end()
        again, extra = [], None
        for i in range(MAX_SETS):                                     # no slot leaked
            try:
                again.append(eng.value_set("risk_level", cap_chain(i)))
            except pq.PqpsError:
                break
            if says(again[-1]) != want[i % 5]:
                verdict.differs(thread="main", what=("cap", "again", i), got=says(again[-1]), want=want[i % 5])
                verdict.end()
        try:
            extra = eng.value_set("risk_level", cap_chain(0))
        except pq.PqpsError:
            pass
        if len(again) != MAX_SETS or extra is not None or len({vs.id for vs in again}) != MAX_SETS:
            verdict.differs(thread="main", what=("cap", "again"), got=(len(again), extra is not None), want=(MAX_SETS, False))
        n_made, n_refused = sum(map(len, made)), sum(refused)
    finally:
        eng.close()
    verdict.end()
    print("MADE", n_made, "REFUSED", n_refused, "AGAIN", len(again), "OK", flush=True)


# ---- writers ----------------------------------------------------------------------------------------------------------------------
class WideHistory(sm.History):
    """shard_matrix.History over the wide table (the model's side alone: the replay asks the engine)."""

    def __init__(self, t, n_shards, recorder):
        self.model = cm.ColumnModel(t.columns(), n_shards)
        self.eng, self.probe_bool = None, cx.probe_bool()
        self.log, self.count, self.recorder = [], 0, recorder
        recorder(self.model, None)


HOT = "user-%06d" % (WIDE_USERS // 3)
WIDE_NEW_EXIT = gm.EXIT_HI + 30_000


def wide_history(devices, dry=True, recorder=None):
    assert dry and recorder
    h = WideHistory(TABLES["wide"](), len(devices.split(",")), recorder)
    model = h.model
    # 1. exit_code of a few rows past its range: the cached range is dropped, the wide bins and the bitmaps over exit_code grow
    few = [("user_id", "=", "1003"), "AND", ("base_command", "=", "vim"), "AND", ("shell_type", "=", "zsh")]
    assert 0 < h.update({"exit_code": str(WIDE_NEW_EXIT)}, few) < 400
    assert int(model.m["exit_code"].max()) == WIDE_NEW_EXIT
    # 2. a batch whose user_name dictionary brings names that sort in front of user-000000: every code moves
    B = 2000
    words = sorted([b"a-new-%03d" % i for i in range(60)] + gm.user_words(WIDE_USERS)[:40])
    batch = gm.table(B, 5, seed=13)
    codes = np.random.default_rng(14).integers(0, len(words), B).astype(np.uint16)
    codes[:len(words)] = np.arange(len(words))
    batch["user_name"] = (codes, words)
    batch["command_id"] = np.arange(20_000_000, 20_000_000 + B, dtype=np.uint64)
    assert h.batch(batch) == B and model.m["user_name"][1][59] == b"a-new-059" and len(model.m["user_name"][1]) == WIDE_USERS + 60
    # 3. the rows of the name that owns a fifth of the table: the hot bin of the wide bins' front goes
    assert h.delete([("user_name", "=", HOT)]) > WIDE_N // 6
    # 4. refused: a second value for a column without a buffer -- and the new user_name beside it is not entered either
    assert h.update({"user_name": "zzz-never-entered", "raw_command": "a second raw command"}, few) is None
    assert len(model.m["user_name"][1]) == WIDE_USERS + 60
    # 5. everything
    assert h.delete([("user_id", ">=", "0")]) > 0 and model.n == 0
    return h


def makes_stale(kind, predicted):
    """Whether the step makes the engine's sets stale (the module's header: THE EPOCH)."""
    return predicted is not None


def epochs_of(steps):
    out = [0]
    for kind, _, predicted in steps:
        out.append(out[-1] + makes_stale(kind, predicted))
    return out


def allowed(seen, candidates, epoch):
    """What an outer query or keys() may return for a set whose creation fits the states `candidates`, when the call can have
    seen the states `seen`: -> ([(s, c)]: the model's answer in state s with the members of state c, whether a refusal)."""
    pairs = [(s, c) for s in seen for c in candidates if c <= s and epoch[s] == epoch[c]]
    return pairs, any(epoch[s] > epoch[c] for s in seen for c in candidates)


def writer_cases(t):
    return top_cases(t, full=False) + [tickets_case(t)]


def state_wants(t, ref, cases):
    """What the model says in the state it is in: the cases, every writer spec's set and what each form says of it."""
    out = dict(cases=answers(cases, ref, {}), sets=[], uses=[])
    for spec in t.writer_specs:
        vs, says = make(ref, spec, {})
        out["sets"].append(says)
        out["uses"].append([ask_form(t, ref, form, chain, {"a": vs}) for form, chain in t.writer_forms(spec[1])])
        vs.free()
    return out


def record(devices, t):
    """The table's history on the model alone: -> (steps, want, the model in its last state); want[s] = state_wants after s steps."""
    steps, want, cases = [], [], writer_cases(t)
    n_shards = len(devices.split(","))

    def recorder(model, step):
        if step is not None:
            steps.append(step)
        want.append(state_wants(t, SetEngine(t, n_shards, model), cases))

    h = t.history(devices, dry=True, recorder=recorder)
    assert len(want) == len(steps) + 1
    return steps, want, h.model


def writers(devices, table, engine=None):
    n_shards = len(devices.split(","))
    os.environ.setdefault("PQPS_ENGINE_LANES", "4")
    n_readers, gate = (DRY_READERS, DRY_GATE) if engine else (WRITER_READERS, GATE)
    t = TABLES[table]()
    cases = writer_cases(t)
    steps, want, final_model = record(devices, t)
    last, epoch = len(steps), epochs_of(steps)
    n_states, n_epochs = last + 1, epoch[-1] + 1
    specs = t.writer_specs
    eng = make_engine(engine, t, n_shards)
    try:
        assert eng.shards() == cm.partition(t.n, n_shards), eng.shards()
        for column in ("user_id", "risk_level", "exit_code"):        # the i32 ranges cached before the first writer
            assert eng.group_top_result(column)["rows"]
        calls = bound(cases, eng, {})
        verdict = cx.Verdict()
        single = cx.single_pass(calls, want[0]["cases"], verdict)
        gen = [0]                                                     # written by the writer alone
        finishing = threading.Event()
        exact = [[0] * n_states for _ in range(n_readers)]            # EXACT checks of the cases, per state
        valid = [[0] * n_epochs for _ in range(n_readers)]            # EXACT answers of a live set, per epoch
        stale = [[0] * n_epochs for _ in range(n_readers)]            # EXACT refusals of a stale set, per epoch they were seen in
        made_exact, ambiguous = [0] * n_readers, [0] * n_readers
        live = [None] * n_readers                                     # the epoch in which reader r's set was made, EXACTly
        barrier = threading.Barrier(n_readers + 1)

        def gate_passed(state, sets_too):
            while True:
                if all(exact[r][state] >= gate and (not sets_too or (valid[r][epoch[state]] >= gate and live[r] == epoch[state])) for r in range(n_readers)):
                    return True
                if verdict.stop.is_set():
                    return False
                time.sleep(0.001)

        def write():
            barrier.wait()
            for k, (kind, args, predicted) in enumerate(steps):
                if not gate_passed(k, makes_stale(kind, predicted)) or verdict.stop.is_set():
                    return
                gen[0] = 2 * k + 1
                got = sm.engine_step(eng, kind, args)
                gen[0] = 2 * k + 2
                if got != ("refused" if predicted is None else predicted):
                    return verdict.differs(thread="writer", step=k + 1, what=kind, got=got, want=predicted)
            if gate_passed(last, True):
                finishing.set()

        def read(r):
            order = list(range(len(calls)))
            random.Random(r).shuffle(order)
            barrier.wait()
            position, final_pass, mine, n_made, n_asked = 0, None, None, r, r
            try:
                while not verdict.stop.is_set():
                    # ---- one case
                    i = order[position % len(order)]
                    position += 1
                    if final_pass is None and finishing.is_set():
                        final_pass = set()
                    g0 = gen[0]
                    got = calls[i][1]()
                    g1 = gen[0]
                    seen = cx.states_seen(g0, g1)
                    if not any(got == want[s]["cases"][i][1] for s in seen):
                        return verdict.differs(thread=r, position=position - 1, what=cases[i][0], g0=g0, g1=g1, states=seen, got=got,
                                               want=[want[s]["cases"][i][1] for s in seen])
                    if g0 == g1 and g0 % 2 == 0:
                        exact[r][g0 // 2] += 1
                        if final_pass is not None:
                            assert g0 == 2 * last, g0
                            final_pass.add(i)
                            if len(final_pass) == len(order):
                                return
                    else:
                        ambiguous[r] += 1
                    # ---- one step of a set's life
                    if mine is None:
                        j = n_made % len(specs)
                        n_made += 1
                        g0 = gen[0]
                        vs, says = make(eng, specs[j], {})
                        g1 = gen[0]
                        seen, one = cx.states_seen(g0, g1), g0 == g1 and g0 % 2 == 0
                        what = ("set", "made", j, specs[j][1])
                        if vs is None:
                            return verdict.differs(thread=r, what=what, g0=g0, g1=g1, states=seen, got=says, want=[want[s]["sets"][j] for s in seen])
                        if says[2] == "refused":                      # a writer between the creation and its keys()
                            candidates = [s for s in seen if want[s]["sets"][j][:2] == says[:2]]
                            if not candidates or not allowed(seen, candidates, epoch)[1]:
                                vs.free()
                                return verdict.differs(thread=r, what=what, g0=g0, g1=g1, states=seen, got=says, want=[want[s]["sets"][j] for s in seen])
                            ambiguous[r] += 1
                            vs.free()
                            continue
                        candidates = [s for s in seen if want[s]["sets"][j] == says]
                        if not candidates:
                            vs.free()
                            return verdict.differs(thread=r, what=what, g0=g0, g1=g1, states=seen, got=says, want=[want[s]["sets"][j] for s in seen])
                        mine = dict(vs=vs, j=j, candidates=candidates, exact=one, forms=t.writer_forms(specs[j][1]))
                        if one:
                            made_exact[r] += 1
                            live[r] = epoch[seen[0]]
                        else:
                            ambiguous[r] += 1
                        continue
                    f = n_asked % len(mine["forms"])
                    n_asked += 1
                    form, chain = mine["forms"][f]
                    g0 = gen[0]
                    got = ask_form(t, eng, form, chain, {"a": mine["vs"]})
                    g1 = gen[0]
                    seen, one = cx.states_seen(g0, g1), g0 == g1 and g0 % 2 == 0
                    pairs, refusal = allowed(seen, mine["candidates"], epoch)
                    what = ("set", "asked", mine["j"], specs[mine["j"]][1], form)
                    if got == "refused":
                        if not refusal:
                            return verdict.differs(thread=r, what=what, g0=g0, g1=g1, states=seen, made_in=mine["candidates"], got=got,
                                                   want=[want[c]["uses"][mine["j"]][f] for _, c in pairs])
                        if not one:
                            ambiguous[r] += 1                         # kept, and asked again: the refusal is counted when it is EXACT
                            continue
                        stale[r][epoch[seen[0]]] += 1
                    else:
                        if not any(got == want[c]["uses"][mine["j"]][f] for _, c in pairs):
                            return verdict.differs(thread=r, what=what, g0=g0, g1=g1, states=seen, made_in=mine["candidates"], got=got,
                                                   want=[want[c]["uses"][mine["j"]][f] for _, c in pairs] + (["refused"] if refusal else []))
                        if one:
                            valid[r][epoch[seen[0]]] += 1
                        else:
                            ambiguous[r] += 1
                        if mine["exact"]:
                            continue                                  # kept across the next write on purpose
                    live[r] = None
                    mine["vs"].free()
                    mine = None
            finally:
                live[r] = None
                if mine is not None:
                    mine["vs"].free()

        threads = [verdict.guard("writer", write)] + [verdict.guard(r, lambda r=r: read(r)) for r in range(n_readers)]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        threaded = time.perf_counter() - t0
        verdict.end()
        assert gen[0] == 2 * last
        assert cx.rows_of_engine(eng) == final_model.n and eng.shards() == final_model.shard_rows, (cx.rows_of_engine(eng), eng.shards())
        final = state_wants(t, eng, cases)                            # a final pass from one thread: the cases, the sets, their forms
        if final != want[last]:
            verdict.differs(thread="main", what=("final",), got=final, want=want[last])
            verdict.end()
    finally:
        eng.close()
    assert all(e[s] >= gate for e in exact for s in range(n_states)) and all(e[last] >= gate + len(calls) for e in exact), exact
    assert all(v[e] >= gate for v in valid for e in range(n_epochs)), valid
    assert all(s[e] >= 1 for s in stale for e in range(1, n_epochs)) and all(s[0] == 0 for s in stale), stale
    n_exact, n_stale = sum(map(sum, exact)) + sum(map(sum, valid)) + sum(made_exact), sum(map(sum, stale))
    print(f"TIMES one pass of {len(calls)} cases from one thread {single:.2f} s, the writer and {n_readers} readers {threaded:.2f} s, table {table}; "
          f"EXACT case checks per state {[sum(e[s] for e in exact) for s in range(n_states)]}, EXACT set answers per epoch "
          f"{[sum(v[e] for v in valid) for e in range(n_epochs)]}, sets made EXACTly {sum(made_exact)}", flush=True)
    print("EXACT", n_exact, "STALE", n_stale, "AMBIGUOUS", sum(ambiguous), "STATES", n_states, "OK", flush=True)


def main(argv):
    what, devices, rest = argv[1], argv[2], argv[3:]
    sys.setswitchinterval(0.0005)                                   # threads that come back from the engine do not wait 5 ms for the interpreter
    os.environ["PQPS_DEVICES"] = devices                            # read when an engine is created
    table = rest.pop(0) if what in ("readers", "writers") and rest else None
    engine = rest.pop(0) if rest else None
    if what not in ("readers", "writers", "cap") or rest or engine not in (None, *ENGINES) or (what != "cap" and table not in TABLES):
        raise SystemExit(f"concurrent_sets: unknown command {argv[1:]!r}")
    if what == "cap":
        cap(devices, engine)
    else:
        (readers if what == "readers" else writers)(devices, table, engine)


if __name__ == "__main__":
    main(sys.argv)
