"""u16 dictionary codes read from a 12-bit packed copy (PQPS_WIDTH_P12: row r = the 12 bits at bit offset 12 r).

The engine keeps a packed copy of every u16 dictionary column of at most 4096 values beside the column and hands it to
the scans that read that column alone or with the plane of sudo_used; every answer must stay what the u16 column gives.
Shim level: the pack kernel against tests/pack12_model.py; the shapes (P) and (P,B) as IDs, COUNT(*) and flags against
numpy on the u16 codes, over the windows a code leaf can carry, AND / OR / tree / one-leaf forms, row counts around the
8-row field group, the 1024-row step and the 64 K-row group, plain and streaming loads; every other position and entry
point refuses a packed column.  Engine level: which kernel a query takes, the copy after every kind of writer, without
the copy (a dictionary of 4097 values, PQPS_PACK12=0), over three shards and over two ranks.  All comparisons exact."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import column_model as cm
import kernel_model
import pack12_model as pm
import qpelib as q
import test_gpu_bit_plane as bp
import test_gpu_insert_batch as ib

pq = q.pq
pytestmark = pytest.mark.gpu

P, B = "P", "B"
EINVAL = -1
SCAN_SIZES = [1, 1023, 1024, 1025, 4097, 65537, 70001]
# (lo, span, negate) of a leaf on the packed column, as the u16 column's 32-bit window test takes them
WINDOWS = {
    "= 0": (0, 0, 0), "= 4095": (4095, 0, 0), "> 4095": (4096, 0xFFFF - 4096, 0), "!= 7": (7, 0, 1), "not <= 2000": (0, 2000, 1),
    "full range": (0, 0xFFFF, 0), "= 1030": (1030, 0, 0), "<= 1638": (0, 1638, 0), "in 100..2200": (100, 2100, 0),
}
BOOL_WINDOWS = [(0, 0), (1, 0), (0, 1), (2, 0)]                    # FALSE, TRUE, every row, no row


def padded(n):
    return max((n + pq.TILE_ROWS - 1) // pq.TILE_ROWS, 1) * pq.TILE_ROWS


def codes_of(rng, n):
    a = rng.integers(0, 4096, n).astype(np.uint16)
    a[rng.integers(0, n, max(n // 50, 1))] = 0
    a[rng.integers(0, n, max(n // 50, 1))] = 4095
    a[rng.integers(0, n, max(n // 300, 1))] = 1030
    return a


def packed_copy(dev, codes, n):
    """The copy of `codes` made by the product's pack kernel (garbage in the buffer first: the kernel clears the padding)."""
    rows = padded(n)
    src = dev.column(codes, rows)
    p = dev.ctx.malloc(rows // 2 * 3)
    dev.ctx.memset(p, 0xA5, rows // 2 * 3)
    dev.ctx.pack12(src, n, p, 0, rows)
    dev.ptrs.append(p)
    return p


def predicate(leaves, form, n_cols):
    """leaves: [(column, lo, span, negate)], sorted by column."""
    pred = pq.Predicate()
    k = len(leaves)
    pred.n_leaves, pred.n_columns = k, n_cols
    for i, (c, lo, span, neg) in enumerate(leaves):
        pred.leaf[i].column, pred.leaf[i].negate, pred.leaf[i].lo, pred.leaf[i].span = c, neg, lo, span
        pred.on_true[i], pred.on_false[i], pred.order[i] = pq.ACCEPT, pq.REJECT, i
    rows = 1 << k
    if form in ("and", "one"):
        pred.truth = 1 << (rows - 1)
    elif form == "or":
        pred.truth = ((1 << rows) - 1) & ~1
    else:                                                         # a tree: (leaf 0 AND last leaf) OR (NOT leaf 0 AND leaf 1) ...
        pred.truth = sum(1 << e for e in range(rows) if ((e & 1) and (e >> (k - 1)) & 1) or (not (e & 1) and (e >> 1) & 1))
    return pred


def cases(shape, rng):
    """[(what, leaves, form)] for one shape: every window as a lone leaf and inside each form."""
    out = []
    names = list(WINDOWS)
    for i, name in enumerate(names):
        w = WINDOWS[name]
        if shape == (P,):
            out.append((name, [(0,) + w], "one"))
            other = WINDOWS[names[(i + 3) % len(names)]]
            out.append((name + " and", [(0,) + w, (0,) + other], "and"))
            out.append((name + " or", [(0,) + w, (0,) + other], "or"))
            out.append((name + " tree", [(0,) + w, (0,) + other, (0,) + WINDOWS["<= 1638"]], "tree"))
        else:
            b = BOOL_WINDOWS[int(rng.integers(0, len(BOOL_WINDOWS)))]
            out.append((name + " one", [(0,) + w], "one"))         # (a leaf on the packed column alone, the plane unread)
            out.append((name + " and", [(0,) + w, (1, b[0], b[1], 0)], "and"))
            out.append((name + " and not", [(0,) + w, (1, 1, 0, 1)], "and"))
            out.append((name + " or", [(0,) + w, (1, 1, 0, 0)], "or"))
            out.append((name + " tree", [(0,) + w, (0,) + WINDOWS["in 100..2200"], (1, 0, 0, 0)], "tree"))
    return out


def check_scans(sizes, seed=12, only=None):
    ctx = pq.Context(0)
    L = pq.lib()
    rng = np.random.default_rng(seed)
    try:
        for n in sizes:
            out = bp.Out(ctx, n)
            dev = bp.Dev(ctx)
            codes = codes_of(rng, n)
            sudo = (rng.random(n) < 0.4).astype(np.uint8)
            packed, plane = packed_copy(dev, codes, n), dev.plane(sudo, n)
            for shape in ((P,), (P, B)):
                cols = [(packed, pq.WIDTH_P12)] + ([(plane, pq.WIDTH_BITS)] if len(shape) == 2 else [])
                arrays = [codes, sudo][:len(shape)]
                carr = pq.column_array(cols)
                for what, leaves, form in cases(shape, rng):
                    if only and not any(o in what for o in only):
                        continue
                    pred = predicate(leaves, form, len(shape))
                    want = np.nonzero(kernel_model.evaluate(pred, arrays))[0].astype(np.uint32)
                    tag = f"n={n} shape={shape} {what}"
                    pq.check(L.pqps_filter_scan(ctx.h, carr, len(shape), n, 0, C.byref(pred), out.ids, out.cap, out.count, None), tag)
                    assert "W0=P12" in L.pqps_last_kernel().decode(), tag
                    got = out.ids_value()
                    assert len(got) == len(want) and np.array_equal(got, want), tag
                    pq.check(L.pqps_filter_count(ctx.h, carr, len(shape), n, C.byref(pred), out.count, None), tag)
                    assert "W0=P12" in L.pqps_last_kernel().decode(), tag
                    assert out.count_value() == len(want), tag
                    pq.check(L.pqps_filter_flags(ctx.h, carr, len(shape), n, C.byref(pred), out.flags, out.count, None), tag)
                    assert "W0=P12" in L.pqps_last_kernel().decode(), tag
                    assert out.count_value() == len(want), tag
                    flags = np.zeros(max(n, 1), dtype=np.uint8)
                    ctx.download(flags.ctypes.data, out.flags, n)
                    assert np.array_equal(np.nonzero(flags[:n])[0], want), tag
            dev.free()
            out.free()
    finally:
        ctx.close()


# ---- the packer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 1023, 1024, 1025, 65537])
def test_pack_kernel_matches_the_model(n):
    ctx = pq.Context(0)
    dev = bp.Dev(ctx)
    try:
        rng = np.random.default_rng(n)
        codes = codes_of(rng, n)
        rows = padded(n)
        p = packed_copy(dev, codes, n)
        got = np.zeros(rows // 2 * 3, dtype=np.uint8)
        ctx.download(got.ctypes.data, p, got.size)
        want = pm.pack(codes, rows)
        assert np.array_equal(got, want)
        assert not pm.unpack(got, rows)[n:].any()                  # zero up to the 1024-row multiple (and the tile's end)
        assert np.array_equal(pm.unpack(got, n), codes)
        if n > 16:                                                  # a suffix repack from a row that is no multiple of 8
            first = min(n - 1, 13 if n < 2000 else 1029)
            codes2 = codes ^ np.uint16(0x5A5)
            src = dev.column(codes2, rows)
            ctx.pack12(src, n, p, first, rows)
            ctx.download(got.ctypes.data, p, got.size)
            mixed = codes2.copy()
            mixed[:first // 8 * 8] = codes[:first // 8 * 8]         # the rows before the 8-row group of `first` are untouched
            assert np.array_equal(got, pm.pack(mixed, rows))
    finally:
        dev.free()
        ctx.close()


def test_pack_refuses_unaligned_buffers_and_short_padding():
    ctx = pq.Context(0)
    dev = bp.Dev(ctx)
    L = pq.lib()
    try:
        src = dev.column(np.zeros(64, dtype=np.uint16), 4096)
        p = ctx.malloc(4096 // 2 * 3 + 64)
        dev.ptrs.append(p)
        assert L.pqps_pack12(ctx.h, src, 64, p + 4, 0, 4096, None) == EINVAL
        assert L.pqps_pack12(ctx.h, src + 2, 64, p, 0, 4096, None) == EINVAL
        assert L.pqps_pack12(ctx.h, src, 64, p, 0, 60, None) == EINVAL
        assert L.pqps_pack12(ctx.h, src, 64, p, 0, 4100, None) == EINVAL
        assert L.pqps_pack12(ctx.h, src, 64, p, 4096, 4096, None) == 0          # nothing to do
    finally:
        dev.free()
        ctx.close()


# ---- the scans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_shapes_with_a_packed_column(n):
    check_scans([n])


def test_shapes_with_a_packed_column_one_million_rows():
    """A sparse and a dense predicate per shape: slots and tiny words, the list area and (full range) bit masks."""
    check_scans([10**6 + 13], only=["= 1030", "<= 1638", "full range"])


def test_shapes_with_a_packed_column_streaming_loads():
    """The `nt` instantiations (the default from 256 MB of columns on), forced at test sizes in a process of their own."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_packed12 as t; t.check_scans([1, 1025, 70001]); print('OK')"
            % str(q.ROOT / "tests"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_every_other_position_and_entry_point_refuses_a_packed_column():
    ctx = pq.Context(0)
    L = pq.lib()
    dev = bp.Dev(ctx)
    n = 5000
    try:
        rng = np.random.default_rng(5)
        codes = codes_of(rng, n)
        sudo = (rng.random(n) < 0.4).astype(np.uint8)
        packed, plane = packed_copy(dev, codes, n), dev.plane(sudo, n)
        u16 = dev.column(codes, padded(n))
        u32 = dev.column(codes.astype(np.uint32), padded(n))
        out = bp.Out(ctx, n)
        one = predicate([(0, 1030, 0, 0)], "one", 1)
        want = np.nonzero(codes == 1030)[0].astype(np.uint32)

        def valid(what):
            carr = pq.column_array([(packed, pq.WIDTH_P12)])
            pq.check(L.pqps_filter_scan(ctx.h, carr, 1, n, 0, C.byref(one), out.ids, out.cap, out.count, None), what)
            assert np.array_equal(out.ids_value(), want), what

        def scans(cols, pred):
            carr = pq.column_array(cols)
            k = len(cols)
            return [L.pqps_filter_scan(ctx.h, carr, k, n, 0, C.byref(pred), out.ids, out.cap, out.count, None),
                    L.pqps_filter_count(ctx.h, carr, k, n, C.byref(pred), out.count, None),
                    L.pqps_filter_flags(ctx.h, carr, k, n, C.byref(pred), out.flags, out.count, None)]

        valid("before")
        two = predicate([(0, 0, 9, 0), (1, 1030, 0, 0)], "and", 2)
        three = predicate([(0, 0, 9, 0), (1, 0, 9, 0), (2, 1030, 0, 0)], "and", 3)
        refused = {
            "P second": scans([(u32, 4), (packed, pq.WIDTH_P12)], two),
            "P third": scans([(u32, 4), (u16, 2), (packed, pq.WIDTH_P12)], three),
            "P with a byte column behind it": scans([(packed, pq.WIDTH_P12), (u16, 2)], two),
            "P, B and a third column": scans([(packed, pq.WIDTH_P12), (plane, pq.WIDTH_BITS), (plane, pq.WIDTH_BITS)], three),
            "two packed columns": scans([(packed, pq.WIDTH_P12), (packed, pq.WIDTH_P12)], two),
            "eight leaves": scans([(packed, pq.WIDTH_P12)], bp.make_pred(rng, 1, set(), "wide")),
            "unaligned base": scans([(packed + 4, pq.WIDTH_P12)], one),
        }
        for what, codes_back in refused.items():
            assert codes_back == [EINVAL] * 3, what
            valid("after " + what)
        # gathers, the fused and the grouped scans
        carr = pq.column_array([(packed, pq.WIDTH_P12)])
        col = pq.Column(packed, pq.WIDTH_P12, 0)
        byte_col = pq.Column(dev.column(sudo, padded(n)), 1, 0)
        cand = dev.column(np.arange(n, dtype=np.uint32), n)
        range_dev = dev.column(np.array([0, n], dtype=np.uint64), 2)
        keys = dev.column(np.zeros(n, dtype=np.uint8), n)
        bins = dev.column(np.zeros(4096, dtype=np.uint32), 4096)
        assert L.pqps_filter_gather(ctx.h, carr, 1, cand, range_dev, n, 0, C.byref(one), out.ids, out.cap, out.count, None) == EINVAL
        valid("after the gather")
        assert L.pqps_index_select(ctx.h, carr, 1, C.byref(byte_col), cand, keys, 0, n, 1, 1, 0, C.byref(one), range_dev,
                                   out.ids, out.cap, out.count, None) == EINVAL
        assert L.pqps_filter_group(ctx.h, carr, 1, n, C.byref(one), C.byref(byte_col), 0, 2, bins, None) == EINVAL      # a fused call: P in the WHERE
        valid("after the grouped scan")
        u16_arr = pq.column_array([(u16, 2)])
        assert L.pqps_filter_group(ctx.h, u16_arr, 1, n, C.byref(one), C.byref(col), 0, 4096, bins, None) == EINVAL     # ... and as the group column
        assert L.pqps_index_build(ctx.h, C.byref(col), n, 0, cand, keys, None) == EINVAL
        assert L.pqps_compact_rows(ctx.h, carr, 1, n, keys, C.byref(C.c_uint64()), None) == EINVAL
        assert L.pqps_project_column(ctx.h, C.byref(col), cand, out.count, n, 0, keys, None) == EINVAL
        valid("at the end")
        # no WHERE: no leaf, no column, `cols` NULL -- the entry points that look for a packed first column must not look here
        every = pq.Predicate()
        every.n_leaves, every.n_columns, every.truth = 0, 0, 1
        for k in (n, 1025, 1):
            pq.check(L.pqps_filter_flags(ctx.h, None, 0, k, C.byref(every), out.flags, out.count, None), "flags without a WHERE")
            assert out.count_value() == k
            flags = np.zeros(k, dtype=np.uint8)
            ctx.download(flags.ctypes.data, out.flags, k)
            assert flags.all()
            pq.check(L.pqps_filter_count(ctx.h, None, 0, k, C.byref(every), out.count, None), "count without a WHERE")
            assert out.count_value() == k
            pq.check(L.pqps_filter_scan(ctx.h, None, 0, k, 0, C.byref(every), out.ids, out.cap, out.count, None), "scan without a WHERE")
            assert np.array_equal(out.ids_value(), np.arange(k, dtype=np.uint32))
        valid("after the scans without a WHERE")
        out.free()
    finally:
        dev.free()
        ctx.close()


# ---- engine level ---------------------------------------------------------------------------------------------------
X = "student1030"
PACKED_CHAINS = {
    "S1": [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", X)],
    "eq": [("user_name", "=", X)],
    "ne": [("user_name", "!=", X)],
    "ge_and_sudo": [("user_name", ">=", "student2900"), "AND", ("sudo_used", "=", "TRUE")],
    "or2": [("user_name", "=", X), "OR", ("user_name", "=", "student2999")],
}
UNPACKED_CHAINS = {
    "Q_A": [("risk_level", ">", "3")],
    "Q_B": [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">", "2")],
    "third column": [("user_name", "<", "student1500"), "AND", ("shell_type", "!=", "zsh"), "AND", ("sudo_used", ">=", "TRUE")],
    "u16 and i32": [("user_name", "=", X), "AND", ("risk_level", ">", "2")],
}


def last_kernel():
    return pq.lib().pqps_last_kernel().decode()


def synthetic_check(eng, host, packed=True):
    """Every chain's IDs and COUNT against the oracle; the packed chains name the P12 kernels (or, `packed` False, none does)."""
    for name, chain in {**PACKED_CHAINS, **UNPACKED_CHAINS}.items():
        want = host.oracle_scan(chain).tolist()
        assert eng.select_ids(chain) == want, name
        ids_kernel = last_kernel()
        assert eng.count(chain) == len(want), name
        for kernel in (ids_kernel, last_kernel()):
            assert ("W0=P12" in kernel) == (packed and name in PACKED_CHAINS), (name, kernel)


def test_engine_which_kernel():
    n = 200003
    host = q.HostSynth(n, seed=0x5EED, full=True)
    eng = pq.HipEngine.synthetic(n, seed=0x5EED)
    try:
        synthetic_check(eng, host)
    finally:
        eng.close()
    eng = pq.HipEngine.synthetic(n, seed=0x5EED, indexes=[("sudo_used", pq.FIELD_BOOL)])
    try:
        eng.probe_bool_indexes()
        chain = PACKED_CHAINS["S1"]                                # index mode: a probe of sudo_used, its rows gathered from the u16 column
        assert sorted(eng.select_ids(chain)) == host.oracle_scan(chain).tolist()
        assert "GATHER=true" in last_kernel() and "P12" not in last_kernel(), last_kernel()
        want = host.oracle_scan(chain).tolist()                     # ... while COUNT(*) is the scan-mode count
        assert eng.count(chain) == len(want) and "W0=P12" in last_kernel(), last_kernel()
    finally:
        eng.close()


USERS300 = [b"user%04d" % (3 * i) for i in range(300)]              # u16 codes: more than 256 names


def model_u16(users=USERS300, seed=2025):
    m = ib.base_model()
    rng = np.random.default_rng(seed)
    m["user_name"] = (rng.integers(0, len(users), ib.N).astype(np.uint16), list(users))
    return m


def writer_chains(a, b):
    return [[("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", a)], [("user_name", "=", a)], [("user_name", "!=", a)],
            [("user_name", ">=", b), "AND", ("sudo_used", "=", "TRUE")], [("user_name", "=", a), "OR", ("user_name", "=", b)],
            [("user_name", "<", b)]]


def model_check(eng, model, chains, packed=True, what=None):
    for chain in chains:
        want = model.select_ids(chain, ())
        assert eng.select_ids(chain) == want, (what, chain)
        kernel = last_kernel()
        assert eng.count(chain) == len(want), (what, chain)
        for k in (kernel, last_kernel()):
            assert ("W0=P12" in k) == packed and ("W0=2" in k) != packed, (what, chain, k)


def one_row(command_id, user_name, sudo=False):
    return {"command_id": command_id, "raw_command": ib.RAW, "base_command": b"ls", "shell_type": b"zsh", "exit_code": 2, "timestamp": ib.STAMP,
            "sudo_used": sudo, "working_directory": ib.DIR, "user_id": 1003, "user_name": user_name, "host_name": b"host-003", "risk_level": 4}


def insert_one(eng, model, row):
    assert model.insert_one(row) is True
    r = pq.Record()
    for column, value in row.items():
        setattr(r, column, value)
    assert pq.lib().executeQueryInsertHIP(eng.e, b"commands", C.byref(r))


def test_engine_writers_keep_the_copy():
    m = model_u16()
    eng = ib.engine_of(m, ())
    model = cm.ColumnModel(m, len(eng.shards()))
    chains = writer_chains("user0300", "user0600")
    try:
        model_check(eng, model, chains, what="fresh")
        insert_one(eng, model, one_row(9_000_001, b"user0300"))
        model_check(eng, model, chains, what="INSERT of an existing name")
        insert_one(eng, model, one_row(9_000_002, b"aaa-first", sudo=True))                # every code moves up by one
        model_check(eng, model, chains + writer_chains("aaa-first", "user0003"), what="INSERT of a name that sorts first")
        b = ib.make_batch(40, 3)
        names = [b"user0300", b"user0301x", b"zzz-last", b"a-second", b"user0600"]
        b["user_name"] = cm.coded([names[i % len(names)] for i in range(40)], dtype=np.uint16)
        assert eng.insert_columns(40, b) == model.insert_batch(b)
        model_check(eng, model, chains + writer_chains("user0301x", "zzz-last"), what="batch INSERT")
        where = [("user_name", "=", "user0600")]
        assert eng.update({"user_name": "user0300"}, where) == model.update({"user_name": "user0300"}, where) > 0
        model_check(eng, model, chains, what="UPDATE SET user_name")
        where = [("risk_level", "<=", "3")]
        assert eng.update({"user_name": "mmm-new"}, where) == model.update({"user_name": "mmm-new"}, where) > 1000     # a new string: codes bumped
        model_check(eng, model, chains + writer_chains("mmm-new", "user0600"), what="UPDATE SET user_name to a new string")
        where = [("exit_code", "=", "1")]
        want = model.delete(where)
        rs = pq.lib().executeQueryDeleteHIP(eng.e, b"commands", pq.WhereList(where).ptr)
        assert rs.contents.success and rs.contents.numRecords == want > 1000
        pq.lib().freeResultSet(rs)
        model_check(eng, model, chains + writer_chains("mmm-new", "zzz-last"), what="DELETE")
    finally:
        eng.close()


def test_engine_drops_the_copy_when_the_dictionary_outgrows_it():
    users = [b"u%05d" % (2 * i) for i in range(4096)]
    m = model_u16(users)
    eng = ib.engine_of(m, ())
    model = cm.ColumnModel(m, len(eng.shards()))
    chains = writer_chains("u00300", "u06000")
    try:
        model_check(eng, model, chains, what="4096 values: code 4095 is in use")
        insert_one(eng, model, one_row(9_000_001, b"u00301"))                               # value 4097
        assert len(model.m["user_name"][1]) == 4097
        model_check(eng, model, chains + writer_chains("u00301", "u08190"), packed=False, what="4097 values")
        insert_one(eng, model, one_row(9_000_002, b"u00300"))
        model_check(eng, model, chains, packed=False, what="4097 values, another INSERT")
    finally:
        eng.close()


SWITCHED_OFF_CODE = textwrap.dedent("""
    import sys
    sys.path.insert(0, ROOT_TESTS)
    import qpelib as q
    import test_gpu_packed12 as t
    n = 70001
    eng = q.pq.HipEngine.synthetic(n, seed=0x5EED)
    t.synthetic_check(eng, q.HostSynth(n, seed=0x5EED, full=True), packed=False)
    eng.close()
    print("OK")
""")


def run_child(code, **env):
    p = subprocess.run([sys.executable, "-c", code.replace("ROOT_TESTS", repr(str(q.ROOT / "tests")))],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, **env), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_engine_with_the_copy_switched_off():
    run_child(SWITCHED_OFF_CODE, PQPS_PACK12="0")


DEVICES_CODE = textwrap.dedent("""
    import sys
    sys.path.insert(0, ROOT_TESTS)
    import qpelib as q
    import test_gpu_packed12 as t
    for n in (4097, 200003):
        eng = q.pq.HipEngine.synthetic(n, seed=0x5EED)
        assert len(eng.shards()) == 3, eng.shards()
        t.synthetic_check(eng, q.HostSynth(n, seed=0x5EED, full=True))
        eng.close()
    print("OK")
""")


def test_engine_over_three_device_shards():
    two = pq.lib().pqps_device_count() >= 2
    run_child(DEVICES_CODE, PQPS_DEVICES="0,1,0" if two else "0,0,0")


def test_engine_over_two_ranks_on_the_loopback_exchange():
    """The exchange's scans read the copy too: the answers of both ranks against the oracle (bp.RANKS_CODE with these chains)."""
    code = bp.RANKS_CODE.replace("import test_gpu_bit_plane as t", "import test_gpu_packed12 as p\nclass t: ENGINE_CHAINS = p.PACKED_CHAINS")
    code = code.replace('names = ["S1", "Q_B", "S7", "or2", "three"]', "names = list(p.PACKED_CHAINS)").replace("n = 2, 1000013", "n = 2, 200003")
    assert "list(p.PACKED_CHAINS)" in code and "class t:" in code and "n = 2, 200003" in code
    run_child(code)
