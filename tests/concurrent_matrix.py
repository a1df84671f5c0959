"""Every query form from several host threads at once, with and without a writer, against tests/column_model.py.

tests/shard_matrix.py asks every form of one engine from one thread.  The engine is built for several callers (include/
executeEngine-hip.h, "asynchronous queries"): a query takes the table's shared lock and then a lane with a context, a stream
and scratch of its own (query_open; grow_group_parts and sort_tmp grow that scratch by freeing it), issues one launch per shard
under the issue lock (fused_issue), allocates on the table's own context while other lanes have kernels running (shard_reduce,
order_topk), reads the i32 ranges all readers share (column_bounds), and queues behind a writer that replaces column buffers,
widens dictionaries and drops those ranges.  Here the table, the routes, the cases and the model are shard_matrix's, and the
callers are threads.  No expected answer comes from an engine: the main thread evaluates the model before any thread starts
(the model and its caches are not thread-safe).

    python tests/concurrent_matrix.py readers <devices> [engine]
        READERS threads; thread t asks every case of READ_ROUTES once, in the order random.Random(t).shuffle gives, all of
        them released by one barrier.  With PQPS_ENGINE_LANES=1 in the environment (default: 4, set here) the tickets case is
        left out -- one thread cannot hold three tickets of one lane -- and every query queues on the single lane.
        Prints CASES <calls> OK.
    python tests/concurrent_matrix.py writers <devices> [engine]
        The writer history of shard_matrix.history, recorded on the model first (record()), replayed by one writer thread
        while WRITER_READERS threads walk the 45 cases of HISTORY_ROUTES over and over.  The writer sets gen = 2k + 1 just
        before the engine call of step k + 1 and gen = 2k + 2 just after it; a reader reads gen before and after its call,
        and the answer must be the model's for one of the states the call can have seen (states_seen).  A check whose two
        readings are the same even number is EXACT (one state), any other AMBIGUOUS (the call overlapped a write); none is
        dropped.  Only the writer is gated: before each step, and once more after the last, it waits until every reader has
        made GATE EXACT checks in the current state; the readers never pause, so a write lands while their calls are in flight
        or queued behind it.  Then every reader makes one more EXACT pass of all 45 cases and stops.
        Prints EXACT <n> AMBIGUOUS <m> STATES 10 OK.

The tickets case holds three of the four lanes in one thread.  Tickets held by several threads may add up to all lanes, and the
next request then waits PQPS_LANE_WAIT_MS and is refused (the header says so), so one Python mutex lets one thread at a time
hold tickets.  While it holds them that thread asks one grouped form: the "a holder may take more" path, on the lane the other
threads keep taking and giving back, past a writer that waits for the tickets.  The three answers and the grouped one are
checked as ONE answer, so all four must come from the same state: no writer gets in between a holder's tickets.

Both print the wall time of one single-threaded pass of their case list and of the threaded part; nothing depends on a time.
Both exit 1 with DIFFERENT and the first answer that differs.

[engine] is left out on a GPU.  "dry" puts a ModelEngine in its place -- the same methods answered by a ColumnModel of its own
under one lock -- with DRY_READERS threads and DRY_GATE, so that the recording, the replay, the gate and the bookkeeping run
on the CPU in seconds.  "stale" and "swapped" are two wrong ModelEngines the checker has to catch (StaleEngine,
SwappedEngine): tests/test_gpu_concurrent_forms.py."""
import os
import random
import sys
import threading
import time
import traceback

import column_model as cm
import shard_matrix as sm

pq = sm.pq
READ_ROUTES = ("none", "fused", "plane", "wide", "member", "probe", "or_probes", "nothing")
READERS = 6                                                      # more threads than lanes: they queue for lanes as well
WRITER_READERS, GATE = 5, 15
DRY_READERS, DRY_GATE = 2, 3
READ_CASES = len(READ_ROUTES) * 22 + 1
HISTORY_CASES = len(sm.HISTORY_ROUTES) * 22 + 1
STATES = 10                                                      # the untouched table and one per writer entry of the history
TICKET_GROUP = ("user_name", sm.ROUTES["fused"][0])
TICKETS_CASE = ("tickets", "group", TICKET_GROUP[0])
_tickets_mutex = threading.Lock()


def states_seen(g0, g1):
    """The states a call can have seen that began after `gen` read g0 and ended before it read g1: state s is the table after
    s writer steps; gen = 2s says step s is complete and step s + 1 not begun, gen = 2s + 1 that step s + 1 is under way."""
    return list(range(g0 // 2, (g1 + 1) // 2 + 1))


def probe_bool():
    return os.environ.get("PQPS_PROBE_BOOL") == "1"


# ---- an engine without a device ------------------------------------------------------------------------------------------------
class ModelEngine:
    """HipEngine's query and writer methods answered by a ColumnModel of its own, every call under one lock."""

    def __init__(self, n_shards):
        self.model = cm.ColumnModel(sm.table(), n_shards)
        self.lock = threading.RLock()                                # (entered again by the grouped form of a ticket holder)

    def rows(self, model, chain):
        return model.select_ids(chain, sm.INDEXES, probe_bool())

    def answer(self, form, fold):
        """`fold(model)` is the answer of the state the model is in."""
        with self.lock:
            return fold(self.model)

    def writer(self, kind, args):
        with self.lock:
            return self.write(kind, args)

    def write(self, kind, args):
        want = sm.model_step(self.model, kind, args)
        return "refused" if want is None else want

    def shards(self):
        return list(self.model.shard_rows)

    def close(self):
        pass

    def free_columnar(self, res):
        pass

    def select_ids(self, chain):
        return self.answer("ids", lambda m: self.rows(m, chain))

    def count(self, chain):
        return self.answer("count", lambda m: len(m.scan_rows(chain)))

    def select_columnar(self, columns, chain):
        return self.answer("cells", lambda m: dict(rows=m.project(self.rows(m, chain), columns)))

    def group_count(self, column, chain=None):
        return self.answer("group_count", lambda m: m.group_count(column, self.rows(m, chain)))

    def aggregate(self, value_column, group_column=None, chain=None):
        return self.answer("aggregate", lambda m: m.aggregate(value_column, group_column, self.rows(m, chain)))

    def count_distinct(self, value_column, group_column=None, chain=None):
        return self.answer("distinct", lambda m: m.count_distinct(value_column, group_column, self.rows(m, chain)))

    def group_pair(self, group_columns, value_column=None, chain=None):
        return self.answer("pair", lambda m: m.group_pair(group_columns, value_column, self.rows(m, chain)))

    def group_buckets(self, column, prefix=None, width=None, value_column=None, chain=None):
        return self.answer("buckets", lambda m: m.group_buckets(column, prefix, width, value_column, self.rows(m, chain)))

    def order_ids(self, order_column, chain=None, descending=False, limit=None):
        return self.answer("order", lambda m: m.order_ids(order_column, self.rows(m, chain), descending, limit))

    def order_ids_by(self, keys, chain=None, limit=None):
        return self.answer("order_by", lambda m: m.order_ids_by(keys, self.rows(m, chain), limit))

    def select_ordered(self, columns, chain, order_column, descending=False, limit=None):
        def fold(m):
            order, matches = m.order_ids(order_column, self.rows(m, chain), descending, limit)
            return dict(rows=m.project(order, columns), matches=matches)
        return self.answer("select_ordered", fold)

    def select_ordered_by(self, columns, chain, keys, limit=None):
        def fold(m):
            order, matches = m.order_ids_by(keys, self.rows(m, chain), limit)
            return dict(rows=m.project(order, columns), matches=matches)
        return self.answer("select_ordered_by", fold)

    def group_first(self, group_column, order_column, chain=None, descending=False):
        return self.answer("first", lambda m: m.group_first(group_column, order_column, self.rows(m, chain), descending))

    def select_group_first(self, columns, chain, group_column, order_column, descending=False):
        def fold(m):
            groups, total = m.group_first(group_column, order_column, self.rows(m, chain), descending)
            return dict(rows=m.project([r for _, r, _ in groups], columns), matches=total)
        return self.answer("select_group_first", fold)

    def tickets_in_flight(self, while_held=None):
        """The lock is kept while the tickets are: a writer waits until every ticket is released, so whatever their holder asks
        meanwhile sees the state the tickets saw."""
        with self.lock:
            out = self.answer("tickets", lambda m: [len(m.scan_rows(sm.ROUTES[r][0])) if count_only else self.rows(m, sm.ROUTES[r][0])
                                                    for r, count_only in sm.TICKETS])
            if while_held:
                while_held()
            return out


class StaleEngine(ModelEngine):
    """Wrong on purpose: group_count is answered from the table as it was before the last write that changed it -- a range or
    a buffer that outlived its writer."""

    def __init__(self, n_shards):
        super().__init__(n_shards)
        self.before = None

    def write(self, kind, args):
        before = cm.ColumnModel(self.model.m)
        got = super().write(kind, args)
        if got != "refused":
            self.before = before
        return got

    def answer(self, form, fold):
        with self.lock:
            return fold(self.before if form == "group_count" and self.before is not None else self.model)


class SwappedEngine(ModelEngine):
    """Wrong on purpose: every group_count is computed from the right state and handed to the wrong caller -- each thread
    gets the answer another thread got last (two queries on one lane's scratch)."""

    def __init__(self, n_shards):
        super().__init__(n_shards)
        self.last = {}

    def answer(self, form, fold):
        with self.lock:
            own = fold(self.model)
            if form != "group_count":
                return own
            me = threading.get_ident()
            others = [got for thread, got in self.last.items() if thread != me]
            self.last[me] = own
            return others[-1] if others else own


ENGINES = {"dry": ModelEngine, "stale": StaleEngine, "swapped": SwappedEngine}


def make_engine(kind, n_shards):
    if kind is None:
        return pq.HipEngine.from_columns(sm.N, sm.table(), sm.INDEXES)
    return ENGINES[kind](n_shards)


def rows_of_engine(eng):
    return eng.e.contents.num_records if isinstance(eng, pq.HipEngine) else eng.model.n


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def held_tickets(eng):
    """The tickets case of this driver: three tickets held under the mutex and, while they are, one grouped form."""
    with _tickets_mutex:
        extra = []
        answers = sm.tickets_in_flight(eng, lambda: extra.append(sm.ask(lambda: eng.group_count(*TICKET_GROUP))))
        return answers, extra[0]


def model_answers(model, routes):
    """[(what, the model's answer)] of every case for the state the model is in (main thread only)."""
    out = []
    for what, _, model_says in sm.cases(model, sm.INDEXES, probe_bool(), routes=routes, full=False):
        if what == ("tickets",):
            group = model.group_count(TICKET_GROUP[0], model.select_ids(TICKET_GROUP[1], sm.INDEXES, probe_bool()))
            out.append((TICKETS_CASE, (model_says(), group)))
        else:
            out.append((what, model_says()))
    return out


def engine_calls(eng, routes):
    """[(what, the call that asks the engine)] in model_answers' order (cases() needs no model for the engine's side)."""
    return [(TICKETS_CASE, lambda: held_tickets(eng)) if what == ("tickets",) else (what, engine_says)
            for what, engine_says, _ in sm.cases(None, sm.INDEXES, probe_bool(), routes=routes, full=False, eng=eng)]


class Verdict:
    """The first difference of any thread; `stop` ends the others."""

    def __init__(self):
        self.stop, self.lock, self.first = threading.Event(), threading.Lock(), None

    def differs(self, **found):
        with self.lock:
            if self.first is None:
                self.first = found
        self.stop.set()

    def guard(self, thread, body):
        """A thread's body: whatever it raises is a difference too."""
        def run():
            try:
                body()
            except BaseException:                                    # noqa: BLE001
                self.differs(thread=thread, what="raised", got=traceback.format_exc(), want=None)
        return threading.Thread(target=run, name=str(thread))

    def end(self):
        if self.first is not None:
            f = dict(self.first)
            got, want = f.pop("got"), f.pop("want")
            what = f.pop("what")
            print("DIFFERENT", what, f, "\n got ", (got if what == "raised" else repr(got))[:3000], "\n want", repr(want)[:1500], flush=True)
            sys.exit(1)


def single_pass(calls, want, verdict):
    """Every case once from this thread; -> seconds."""
    t0 = time.perf_counter()
    for (what, call), (what_too, answer) in zip(calls, want):
        got = sm.ask(call)
        assert what == what_too, (what, what_too)
        if got != answer:
            verdict.differs(thread="main", what=what, got=got, want=answer)
            verdict.end()
    return time.perf_counter() - t0


# ---- readers ----------------------------------------------------------------------------------------------------------------------
def readers(devices, engine=None):
    n_shards = len(devices.split(","))
    lanes = int(os.environ.setdefault("PQPS_ENGINE_LANES", "4"))   # read when an engine is created
    n_threads = DRY_READERS if engine else READERS
    model = cm.ColumnModel(sm.table(), n_shards)
    want = model_answers(model, READ_ROUTES)
    assert len(want) == READ_CASES == 177, len(want)
    eng = make_engine(engine, n_shards)
    try:
        assert eng.shards() == model.shard_rows, (eng.shards(), model.shard_rows)
        calls = engine_calls(eng, READ_ROUTES)
        if lanes == 1:
            calls, want = calls[:-1], want[:-1]
            assert len(want) == 176 and TICKETS_CASE not in [what for what, _ in want]
        verdict, asked = Verdict(), [0] * n_threads
        single = single_pass(calls, want, verdict)
        barrier = threading.Barrier(n_threads)

        def walk(t):
            order = list(range(len(calls)))
            random.Random(t).shuffle(order)
            barrier.wait()
            for position, i in enumerate(order):
                if verdict.stop.is_set():
                    return
                got = sm.ask(calls[i][1])
                asked[t] += 1
                if got != want[i][1]:
                    return verdict.differs(thread=t, position=position, what=want[i][0], got=got, want=want[i][1])

        threads = [verdict.guard(t, lambda t=t: walk(t)) for t in range(n_threads)]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        threaded = time.perf_counter() - t0
    finally:
        eng.close()
    verdict.end()
    assert sum(asked) == n_threads * len(calls), asked
    print(f"TIMES one pass of {len(calls)} cases from one thread {single:.2f} s, {n_threads} threads x {len(calls)} cases {threaded:.2f} s, "
          f"{lanes} lane(s)", flush=True)
    print("CASES", sum(asked), "OK", flush=True)


# ---- writers ----------------------------------------------------------------------------------------------------------------------
def record(devices):
    """The history on the model alone: -> (steps, want, the model in its last state); steps[k] = (kind, arguments, the
    model's predicted return), want[s] = model_answers after s steps."""
    steps, want = [], []

    def recorder(model, step):
        if step is not None:
            steps.append(step)
        want.append(model_answers(model, sm.HISTORY_ROUTES))

    h = sm.history(devices, dry=True, recorder=recorder)
    assert len(steps) == STATES - 1 and len(want) == STATES and all(len(w) == HISTORY_CASES == 45 for w in want)
    assert all([what for what, _ in w] == [what for what, _ in want[0]] for w in want)
    return steps, want, h.model


def writers(devices, engine=None):
    n_shards = len(devices.split(","))
    os.environ.setdefault("PQPS_ENGINE_LANES", "4")
    n_readers, gate = (DRY_READERS, DRY_GATE) if engine else (WRITER_READERS, GATE)
    steps, want, final_model = record(devices)
    last = len(steps)
    eng = make_engine(engine, n_shards)
    try:
        assert eng.shards() == cm.partition(sm.N, n_shards), eng.shards()
        for column in ("user_id", "risk_level"):                      # the i32 ranges cached before the first writer
            assert eng.group_count(column)
        calls = engine_calls(eng, sm.HISTORY_ROUTES)
        verdict = Verdict()
        single = single_pass(calls, want[0], verdict)
        gen = [0]                                                     # written by the writer alone
        finishing = threading.Event()
        exact = [[0] * STATES for _ in range(n_readers)]
        ambiguous = [0] * n_readers
        barrier = threading.Barrier(n_readers + 1)

        def gate_passed(state):
            while min(exact[r][state] for r in range(n_readers)) < gate:
                if verdict.stop.is_set():
                    return False
                time.sleep(0.001)
            return True

        def write():
            barrier.wait()
            for k, (kind, args, predicted) in enumerate(steps):
                if not gate_passed(k) or verdict.stop.is_set():
                    return
                gen[0] = 2 * k + 1
                got = sm.engine_step(eng, kind, args)
                gen[0] = 2 * k + 2
                if got != ("refused" if predicted is None else predicted):
                    return verdict.differs(thread="writer", step=k + 1, what=kind, got=got, want=predicted)
            if gate_passed(last):
                finishing.set()

        def read(r):
            order = list(range(len(calls)))
            random.Random(r).shuffle(order)
            barrier.wait()
            position, final_pass = 0, None
            while not verdict.stop.is_set():
                i = order[position % len(order)]
                position += 1
                if final_pass is None and finishing.is_set():
                    final_pass = set()
                g0 = gen[0]
                got = sm.ask(calls[i][1])
                g1 = gen[0]
                seen = states_seen(g0, g1)
                if not any(got == want[s][i][1] for s in seen):
                    return verdict.differs(thread=r, position=position - 1, what=want[0][i][0], g0=g0, g1=g1, states=seen, got=got,
                                           want=[want[s][i][1] for s in seen])
                if g0 == g1 and g0 % 2 == 0:
                    exact[r][g0 // 2] += 1
                    if final_pass is not None:
                        assert g0 == 2 * last, g0
                        final_pass.add(i)
                        if len(final_pass) == len(order):
                            return
                else:
                    ambiguous[r] += 1

        threads = [verdict.guard("writer", write)] + [verdict.guard(r, lambda r=r: read(r)) for r in range(n_readers)]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        threaded = time.perf_counter() - t0
        verdict.end()
        assert gen[0] == 2 * last
        assert rows_of_engine(eng) == final_model.n and eng.shards() == final_model.shard_rows, (rows_of_engine(eng), eng.shards())
        assert sm.compare(eng, sm.cases(final_model, sm.INDEXES, probe_bool(), routes=sm.HISTORY_ROUTES, full=False, eng=eng), "final") == 45
    finally:
        eng.close()
    n_exact, per_state = sum(map(sum, exact)), [sum(e[s] for e in exact) for s in range(STATES)]
    assert all(e[s] >= gate for e in exact for s in range(STATES)) and all(e[last] >= gate + len(calls) for e in exact), exact
    assert n_exact >= STATES * n_readers * gate + n_readers * len(calls), n_exact
    print(f"TIMES one pass of {len(calls)} cases from one thread {single:.2f} s, the writer and {n_readers} readers {threaded:.2f} s; "
          f"EXACT checks per state {per_state}", flush=True)
    print("EXACT", n_exact, "AMBIGUOUS", sum(ambiguous), "STATES", STATES, "OK", flush=True)


def main(argv):
    what, devices, engine = argv[1], argv[2], (argv[3] if len(argv) > 3 else None)
    os.environ["PQPS_DEVICES"] = devices                            # read when an engine is created
    if what not in ("readers", "writers") or engine not in (None, *ENGINES):
        raise SystemExit(f"concurrent_matrix: unknown command {argv[1:]!r}")
    (readers if what == "readers" else writers)(devices, engine)


if __name__ == "__main__":
    main(sys.argv)
