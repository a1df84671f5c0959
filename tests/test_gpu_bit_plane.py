"""Boolean columns read from a bit plane (PQPS_WIDTH_BITS: row r = bit r & 7 of byte r >> 3, LSB first).

The engine keeps a plane of sudo_used beside its byte column and hands the plane to its scans; every answer must stay
what the byte column gives.  Shim level: every width shape with a plane as its last column (and the shapes that take
the generic kernel: a plane first, four columns, more than six comparisons, a lone plane), AND / OR / tree forms, every
window a bool leaf can carry, IDs / COUNT(*) / DELETE flags, row counts that end mid-byte, mid-step and mid-tile, plain
and streaming loads.  Engine level: the oracle's answers after INSERTs and a DELETE, on a PQPS_DEVICES engine and on
ranks over the loopback exchange.  Plus the pack kernel against numpy.packbits and the entry points that refuse a plane."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import kernel_model
import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

B = "B"                                                   # a bit-plane column in a shape
DT = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}
SIZES = [1, 7, 1023, 1025, 4097, 10**6 + 13]
SHAPES = [(8, B), (4, B), (2, B), (1, B), (8, 4, B), (8, 2, B), (8, 1, B), (4, 4, B), (4, 2, B), (4, 1, B), (2, 2, B),
          (2, 1, B), (1, 1, B),
          (B,), (B, 4), (4, 2, 1, B), (2, B, 1)]          # generic kernel: a lone plane, a plane first, four columns, a plane mid-shape
LEAF_WINDOWS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 0xFFFFFFFE), (0xFFFFFFFF, 1)]   # (lo, span) over x in {0, 1}
EINVAL = -1


def plane_bytes(n):
    """Readable extent of a plane: n rounded up to whole 4096-row tiles (what the engine allocates), in bytes."""
    return max((n + pq.TILE_ROWS - 1) // pq.TILE_ROWS, 1) * pq.TILE_ROWS // 8


class Dev:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def column(self, a, pad_rows):
        nbytes = max(pad_rows, a.size, 1) * a.dtype.itemsize
        p = self.ctx.malloc(nbytes)
        self.ctx.memset(p, 0, nbytes)
        if a.size:
            self.ctx.upload(p, a.ctypes.data, a.nbytes)
        self.ptrs.append(p)
        return p

    def plane(self, bools, n):
        """The plane of `bools` made by the product's pack kernel (garbage in the padding first: the kernel clears it)."""
        nb = plane_bytes(n)
        src = self.column(np.ascontiguousarray(bools, dtype=np.uint8), nb * 8)
        p = self.ctx.malloc(nb)
        self.ctx.memset(p, 0xA5, nb)
        pq.check(pq.lib().pqps_pack_bits(self.ctx.h, src, n, p, 0, nb, None), "pqps_pack_bits")
        self.ptrs.append(p)
        return p

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


class Out:
    def __init__(self, ctx, n):
        self.ctx, self.cap = ctx, n + 8
        self.ids, self.count, self.flags = ctx.malloc(self.cap * 4), ctx.malloc(64), ctx.malloc(max(n, 1) + 64)

    def count_value(self):
        self.ctx.sync()
        k = C.c_uint64()
        self.ctx.download(C.byref(k), self.count, 8)
        return k.value

    def ids_value(self):
        k = self.count_value()
        a = np.zeros(max(k, 1), dtype=np.uint32)
        if k:
            self.ctx.download(a.ctypes.data, self.ids, 4 * min(k, self.cap))
        return a[:k]

    def free(self):
        for p in (self.ids, self.count, self.flags):
            self.ctx.free(p)


def make_pred(rng, n_cols, bool_slots, form):
    pred = pq.Predicate()
    leaves = []
    for c in range(n_cols):
        per = 1 if form == "one" or n_cols >= 3 else 2
        if form == "wide":
            per = 8 if c == 0 else 1
        for _ in range(per):
            if c in bool_slots:
                lo, span = LEAF_WINDOWS[int(rng.integers(0, len(LEAF_WINDOWS)))]
            else:
                lo, span = int(rng.integers(0, 5)), int(rng.integers(0, 3))
            leaves.append((c, int(rng.integers(0, 2)), lo, span))
        if form == "one":
            break
    k = len(leaves)
    pred.n_leaves, pred.n_columns = k, n_cols
    for i, (c, neg, lo, span) in enumerate(leaves):
        pred.leaf[i].column, pred.leaf[i].negate, pred.leaf[i].lo, pred.leaf[i].span = c, neg, lo, span
    if k > pq.TT_LEAVES:                                   # an OR of all leaves as a jump program
        for s in range(k):
            pred.order[s] = s
            pred.on_true[s] = pq.ACCEPT
            pred.on_false[s] = s + 1 if s + 1 < k else pq.REJECT
        return pred
    for i in range(k):
        pred.on_true[i], pred.on_false[i], pred.order[i] = pq.ACCEPT, pq.REJECT, i
    rows = 1 << k
    if form in ("and", "one"):
        pred.truth = 1 << (rows - 1)
    elif form == "or":
        pred.truth = ((1 << rows) - 1) & ~1
    else:
        pred.truth = int(rng.integers(1, 1 << min(rows, 62))) | (1 << (rows - 1))
    return pred


def check_shapes(sizes, shapes=SHAPES, seed=77):
    ctx = pq.Context(0)
    L = pq.lib()
    rng = np.random.default_rng(seed)
    try:
        for n in sizes:
            out = Out(ctx, n)
            pad = plane_bytes(n) * 8
            for shape in shapes:
                dev = Dev(ctx)
                arrays, cols, bool_slots = [], [], set()
                for slot, w in enumerate(shape):
                    if w == B:
                        a = (rng.random(n) < 0.4).astype(np.uint8)
                        cols.append((dev.plane(a, n), pq.WIDTH_BITS))
                        bool_slots.add(slot)
                    else:
                        a = rng.integers(0, 7, n).astype(DT[w])
                        cols.append((dev.column(a, pad), w))
                    arrays.append(a)
                carr = pq.column_array(cols)
                forms = ["and", "or", "tree", "one"] + (["wide"] if len(shape) <= 3 else [])
                for form in forms:
                    pred = make_pred(rng, len(shape), bool_slots, form)
                    want = np.nonzero(kernel_model.evaluate(pred, arrays))[0].astype(np.uint32)
                    what = f"n={n} shape={shape} form={form}"
                    pq.check(L.pqps_filter_scan(ctx.h, carr, len(shape), n, 0, C.byref(pred), out.ids, out.cap, out.count, None), what)
                    got = out.ids_value()
                    assert len(got) == len(want) and np.array_equal(got, want), what
                    pq.check(L.pqps_filter_count(ctx.h, carr, len(shape), n, C.byref(pred), out.count, None), what)
                    assert out.count_value() == len(want), what
                    pq.check(L.pqps_filter_flags(ctx.h, carr, len(shape), n, C.byref(pred), out.flags, out.count, None), what)
                    assert out.count_value() == len(want), what
                    flags = np.zeros(max(n, 1), dtype=np.uint8)
                    ctx.download(flags.ctypes.data, out.flags, n)
                    assert np.array_equal(np.nonzero(flags[:n])[0], want), what
                dev.free()
            out.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_pack_kernel_matches_numpy_packbits(n):
    ctx = pq.Context(0)
    dev = Dev(ctx)
    try:
        rng = np.random.default_rng(n)
        a = rng.integers(0, 2, n).astype(np.uint8)
        a[rng.integers(0, n, max(n // 100, 1))] = 7                # any non-zero byte is TRUE
        nb = plane_bytes(n)
        p = dev.plane(a, n)
        got = np.zeros(nb, dtype=np.uint8)
        ctx.download(got.ctypes.data, p, nb)
        want = np.zeros(nb, dtype=np.uint8)
        packed = np.packbits(a != 0, bitorder="little")
        want[:packed.size] = packed
        assert np.array_equal(got, want)
        if n > 16:                                                  # a partial repack (what INSERT does): bytes [1, plane_bytes) only
            a2 = a.copy()
            a2[8:] ^= 1
            src = dev.column(a2, nb * 8)
            pq.check(pq.lib().pqps_pack_bits(ctx.h, src, n, p, 1, nb, None), "partial pack")
            ctx.download(got.ctypes.data, p, nb)
            packed2 = np.packbits(a2 != 0, bitorder="little")
            want[1:packed2.size] = packed2[1:]
            assert np.array_equal(got, want)
    finally:
        dev.free()
        ctx.close()


def test_entry_points_without_plane_support_refuse_one():
    ctx = pq.Context(0)
    L = pq.lib()
    dev = Dev(ctx)
    n = 5000
    try:
        plane = dev.plane(np.ones(n, dtype=np.uint8), n)
        col = pq.Column(plane, pq.WIDTH_BITS, 0)
        carr = pq.column_array([(plane, pq.WIDTH_BITS)])
        pred = pq.Predicate()
        pred.n_leaves, pred.n_columns, pred.truth = 1, 1, 2
        pred.leaf[0].lo = 1
        pred.on_true[0], pred.on_false[0] = pq.ACCEPT, pq.REJECT
        out = Out(ctx, n)
        cand = dev.column(np.arange(n, dtype=np.uint32), n)
        range_dev = dev.column(np.array([0, n], dtype=np.uint64), 2)
        keys = dev.column(np.zeros(n, dtype=np.uint8), n)
        byte_col = pq.Column(keys, 1, 0)
        assert L.pqps_filter_gather(ctx.h, carr, 1, cand, range_dev, n, 0, C.byref(pred), out.ids, out.cap, out.count, None) == EINVAL
        assert L.pqps_index_select(ctx.h, carr, 1, C.byref(byte_col), cand, keys, 0, n, 1, 1, 0, C.byref(pred), range_dev,
                                   out.ids, out.cap, out.count, None) == EINVAL
        assert L.pqps_index_build(ctx.h, C.byref(col), n, 0, cand, keys, None) == EINVAL
        assert L.pqps_compact_rows(ctx.h, carr, 1, n, keys, C.byref(C.c_uint64()), None) == EINVAL
        assert L.pqps_project_column(ctx.h, C.byref(col), cand, out.count, n, 0, keys, None) == EINVAL
        assert L.pqps_gather_keys(ctx.h, C.byref(col), 0, cand, out.count, n, 0, keys, None) == EINVAL
        pq.check(L.pqps_filter_count(ctx.h, carr, 1, n, C.byref(pred), out.count, None), "count")     # ... while the scans take it
        assert out.count_value() == n
        out.free()
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("n", SIZES[:5])
def test_shapes_with_a_plane_small_tables(n):
    check_shapes([n])


def test_shapes_with_a_plane_one_million_rows():
    check_shapes([SIZES[-1]], shapes=[(2, B), (4, B), (4, 1, B), (8, 4, B), (1, B), (4, 2, 1, B)])


def test_shapes_with_a_plane_streaming_loads():
    """The `nt` instantiations (the default from 256 MB of columns on), forced at test sizes in a process of their own."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_bit_plane as t; t.check_shapes([1, 1025, 70001]); print('OK')"
            % str(q.ROOT / "tests"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


# ---- engine level ---------------------------------------------------------------------------------------------------
ENGINE_CHAINS = {
    "S1": [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")],
    "Q_B": [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">", "2")],
    "cid": [("command_id", "<", "40000"), "AND", ("sudo_used", "!=", "TRUE")],
    "u8": [("shell_type", "=", "bash"), "AND", ("sudo_used", "=", "TRUE")],
    "host_u8": [("host_name", "=", "labpc-03"), "AND", ("sudo_used", "=", "FALSE")],
    "three": [("risk_level", ">=", "2"), "AND", ("user_id", "<", "1500"), "AND", ("sudo_used", "<=", "FALSE")],
    "three_u8": [("user_name", "<", "student1500"), "AND", ("shell_type", "!=", "zsh"), "AND", ("sudo_used", ">=", "TRUE")],
    "S7": [("sudo_used", "=", "TRUE"), "OR", [("risk_level", "=", "5"), "AND", ("shell_type", "=", "bash")]],
    "or2": [("sudo_used", "=", "FALSE"), "OR", ("risk_level", "!=", "3")],
    "five": [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">", "1"), "AND", ("user_id", ">", "1100"), "AND",
             ("shell_type", "=", "bash"), "AND", ("user_name", "<", "student1900")],
    "wide": [("risk_level", "=", "1"), "OR", ("risk_level", "=", "2"), "OR", ("risk_level", "=", "4"), "OR",
             ("exit_code", "=", "1"), "OR", ("exit_code", "=", "2"), "OR", ("risk_level", "=", "9"), "OR", ("sudo_used", "=", "TRUE")],
    "lone": [("sudo_used", "=", "TRUE")],
}


def engine_check(eng, host, names=None):
    for name in names or ENGINE_CHAINS:
        chain = ENGINE_CHAINS[name]
        want = host.oracle_scan(chain).tolist()
        assert eng.select_ids(chain) == want, name
        assert eng.count(chain) == len(want), name


@pytest.mark.parametrize("n", SIZES)
def test_engine_answers_with_the_plane(n):
    eng = pq.HipEngine.synthetic(n, seed=0x5EED)
    try:
        engine_check(eng, q.HostSynth(n, seed=0x5EED, full=True))
    finally:
        eng.close()


def _with_rows(host, added):
    """The HostSynth model with rows appended (values of the inserted records; dictionary codes of their strings)."""
    m = q.HostSynth.__new__(q.HostSynth)
    m.__dict__.update(host.__dict__)
    k = len(added)
    cols = np.array(added, dtype=np.int64).T
    extra = {"command_id": cols[0], "exit_code": cols[1], "sudo_used": cols[2], "user_id": cols[3], "risk_level": cols[4],
             "shell_type": [pq.SYNTH_SHELLS.index(b"bash")] * k, "user_name": [pq.SYNTH_USERS_DICT.index(b"student1030")] * k,
             "host_name": [pq.SYNTH_HOSTS.index(b"labpc-03")] * k, "base_command": [pq.SYNTH_BASES.index(b"cmd005")] * k}
    m.arr = {}
    for name, a in host.arr.items():
        tail = np.asarray(extra[name], dtype=a.dtype) if name in extra else np.zeros(k, dtype=a.dtype)
        m.arr[name] = np.ascontiguousarray(np.concatenate([a, tail]))
    m.n = host.n + k
    return m


def test_engine_after_inserts_and_a_delete():
    """INSERTs that cross a plane byte and a 1024-row step, then a DELETE that closes the rows up: the plane follows."""
    n = 1019
    host = q.HostSynth(n, seed=0x5EED, full=True)
    eng = pq.HipEngine.synthetic(n, seed=0x5EED)
    L = pq.lib()
    try:
        r = pq.Record()
        r.raw_command, r.base_command, r.timestamp, r.working_directory = b"cmd", b"cmd005", b"2025-01-01T00:00:00.000Z", b"/home/u"
        r.shell_type, r.user_name, r.host_name = b"bash", b"student1030", b"labpc-03"
        added = []
        for i in range(14):                                        # rows 1019 .. 1032: past plane byte 127 and step 0
            sudo = i % 3 != 1
            r.command_id, r.exit_code, r.sudo_used, r.user_id, r.risk_level = 900000 + i, i % 2, sudo, 1030, 1 + i % 5
            assert L.executeQueryInsertHIP(eng.e, b"commands", C.byref(r))
            added.append((900000 + i, i % 2, int(sudo), 1030, 1 + i % 5))
            if i in (0, 4, 5, 13):
                engine_check(eng, _with_rows(host, added), ["S1", "Q_B", "S7", "five", "wide", "u8"])
        model = _with_rows(host, added)
        wl = pq.WhereList([("risk_level", "=", "2")])
        rs = L.executeQueryDeleteHIP(eng.e, b"commands", wl.ptr)
        assert rs.contents.success
        L.freeResultSet(rs)
        keep = model.arr["risk_level"] != 2
        for k in model.arr:
            model.arr[k] = np.ascontiguousarray(model.arr[k][keep])
        model.n = int(keep.sum())
        assert eng.e.contents.num_records == model.n
        engine_check(eng, model)
    finally:
        eng.close()


DEVICES_CODE = textwrap.dedent("""
    import sys
    sys.path.insert(0, ROOT_TESTS)
    import qpelib as q
    import test_gpu_bit_plane as t
    pq = q.pq
    for n in (4097, 1000013):
        eng = pq.HipEngine.synthetic(n, seed=0x5EED)
        assert len(eng.shards()) == 3, eng.shards()
        t.engine_check(eng, q.HostSynth(n, seed=0x5EED, full=True))
        eng.close()
    print("OK")
""")


def test_engine_over_device_shards():
    two = pq.lib().pqps_device_count() >= 2
    env = dict(os.environ, PQPS_DEVICES="0,1,0" if two else "0,0,0")
    p = subprocess.run([sys.executable, "-c", DEVICES_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=900, env=env, cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


RANKS_CODE = textwrap.dedent("""
    import os, sys, threading, traceback
    import numpy as np
    sys.path.insert(0, ROOT_TESTS)
    import qpelib as q
    import test_gpu_bit_plane as t
    pq = q.pq
    LOOPBACK = os.path.join(ROOT_TESTS, "loopback", "libloopback_rccl.so")
    world, n = 2, 1000013
    names = ["S1", "Q_B", "S7", "or2", "three"]
    gate = threading.Barrier(world)
    ident = [None]
    out = [None] * world

    def rank_main(rank):
        try:
            eng = pq.HipEngine.synthetic_rank(n, world, rank, seed=0x5EED)
            if rank == 0:
                ident[0] = pq.HipEngine.rccl_id(LOOPBACK)
            gate.wait()
            eng.join_ranks(LOOPBACK, ident[0])
            ctx = pq.Context(0)
            res = {}
            for name in names:
                tc = eng.select_async(t.ENGINE_CHAINS[name], count_only=True)
                tk = eng.select_async(t.ENGINE_CHAINS[name])
                kc, _ = eng.await_ticket(tc)
                k, r = eng.await_ticket(tk)
                ids = np.zeros(max(k, 1), dtype=np.uint32)
                if k > 0:
                    ctx.download(ids.ctypes.data, r.ids_dev, 4 * k)
                res[name] = [int(kc), ids[:k].tolist()]
                eng.release_ticket(tc)
                eng.release_ticket(tk)
            out[rank] = res
            gate.wait()
            eng.leave_ranks()
            ctx.close()
            eng.close()
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            os._exit(3)

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads: th.start()
    for th in threads: th.join()
    host = q.HostSynth(n, seed=0x5EED, full=True)
    for name in names:
        want = host.oracle_scan(t.ENGINE_CHAINS[name]).tolist()
        for rank in range(world):
            kc, ids = out[rank][name]
            assert kc == len(want) and ids == want, (name, rank, kc, len(want))
    print("OK")
""")


def test_engine_over_ranks_on_the_loopback_exchange():
    p = subprocess.run([sys.executable, "-c", RANKS_CODE.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
