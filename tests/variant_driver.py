#!/usr/bin/env python3
"""Runs ONE parity sweep of the HIP filter in this process and exits non-zero on the first difference.

The shim reads its tuning switches (PQPS_NT_LOADS, PQPS_EXPAND_LAG, PQPS_SUM_LAG, PQPS_EXPAND_SPIN_LIMIT, ...)
once per process, so tests/test_gpu_variants.py starts this script once per setting.  Test infrastructure:
the oracle (and, for hand-built predicates, the numpy model of the kernel arithmetic) is the checker.

    python tests/variant_driver.py sizes  [n ...]     seeded synthetic tables, the suite's queries, vs the oracle
    python tests/variant_driver.py shapes [n]         every (W0, W1, W2) kernel shape, chain and tree form, vs numpy
    python tests/variant_driver.py windows [n ...]    leaf windows at the edges of each column's range, every shape and
                                                      entry point, vs a numpy restatement of the 32 / 64-bit window test
"""
import ctypes as C
import itertools
import sys

import numpy as np

import qpelib as q
import kernel_model

pq = q.pq

QUERIES = {
    "S1": [("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")],
    "Q_A": [("risk_level", ">", "3")],
    "Q_B": [("sudo_used", "=", "TRUE"), "AND", ("risk_level", ">", "2")],
    "Q_C": [("exit_code", "!=", "0"), "AND", ("user_id", ">=", "1500"), "OR", ("risk_level", "=", "5")],
    "S7": [("sudo_used", "=", "TRUE"), "OR", [("risk_level", "=", "5"), "AND", ("shell_type", "=", "bash")]],
    "dense": [("sudo_used", "=", "FALSE")],
    "u8": [("sudo_used", "=", "TRUE")],                        # one 1-byte column, ~7 %: four steps per wave scan in the expander
    "u8_dict": [("shell_type", "=", "zsh")],
    "mid": [("risk_level", ">", "1")],                          # ~43 %: steps of ~440 matches (staged 64-row path)
    "mid_u8": [("shell_type", "!=", "bash")],
    "all": [],
    "none": [("risk_level", ">", "9")],
    "seven_leaves": [("risk_level", "=", "1"), "OR", ("risk_level", "=", "2"), "AND", ("exit_code", "=", "0"), "OR",
                     [("host_name", "<", "labpc-05"), "AND", ("shell_type", "!=", "zsh"), "AND", ("user_id", "<", "1900")],
                     "OR", ("sudo_used", "=", "1")],
}


class Out:
    def __init__(self, ctx, cap):
        self.ctx, self.cap = ctx, cap
        self.ids, self.count = ctx.malloc(max(cap, 1) * 4), ctx.malloc(64)

    def result(self):
        self.ctx.sync()                      # raises if a launch reported an incomplete result
        k = C.c_uint64()
        self.ctx.download(C.byref(k), self.count, 8)
        a = np.zeros(max(k.value, 1), dtype=np.uint32)
        if k.value:
            self.ctx.download(a.ctypes.data, self.ids, 4 * min(k.value, self.cap))
        return k.value, a[:min(k.value, self.cap)]

    def free(self):
        self.ctx.free(self.ids)
        self.ctx.free(self.count)


def sweep_sizes(ctx, sizes):
    L = pq.lib()
    for n in sizes:
        dev = pq.SyntheticTable(ctx, n, seed=0xC0FFEE)
        host = q.HostSynth(n, seed=0xC0FFEE)
        out = Out(ctx, n + 8)
        for name, chain in QUERIES.items():
            pred, cols, nc, _ = dev.bind(chain)
            for rep in range(2):             # twice: the second run finds the words the first one left behind
                pq.check(L.pqps_filter_scan(ctx.h, cols, nc, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), name)
                k, got = out.result()
                want = host.oracle_scan(chain)
                if k != len(want) or not np.array_equal(got, want):
                    sys.exit(f"DIFF ids: n={n} query={name} rep={rep}: {k} vs {len(want)} matches")
            pq.check(L.pqps_filter_count(ctx.h, cols, nc, n, C.byref(pred), out.count, None), name)
            k, _ = out.result()
            if k != len(want):
                sys.exit(f"DIFF count: n={n} query={name}: {k} vs {len(want)}")
        out.free()
        dev.free()
        print(f"sizes: n={n} ok", flush=True)


SHAPES = [s for s in itertools.product((8, 4, 2, 1, 0), repeat=3)
          if s[0] != 0 and s[0] >= s[1] >= s[2] and not (s[1] == 0 and s[2] != 0)]
DT = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}


def sweep_shapes(ctx, n):
    """Columns of random small values (so that equality windows hit), one to two leaves per column."""
    L = pq.lib()
    rng = np.random.default_rng(1234)
    pad = (n + 4095) // 4096 * 4096
    out = Out(ctx, n + 8)
    assert len(SHAPES) == 34
    for shape in SHAPES:
        widths = [w for w in shape if w]
        arrays, ptrs = [], []
        for w in widths:
            a = rng.integers(0, 7, n).astype(DT[w])
            a[rng.integers(0, n, n // 50)] = np.iinfo(DT[w]).max       # a few extreme values
            p = ctx.malloc(pad * w)
            ctx.memset(p, 0, pad * w)
            ctx.upload(p, a.ctypes.data, a.nbytes)
            arrays.append(a)
            ptrs.append(p)
        cols = pq.column_array(list(zip(ptrs, widths)))
        for form in ("and", "or", "tree", "one"):
            pred = pq.Predicate()
            leaves = []
            for c in range(len(widths)):
                for _ in range(1 if form == "one" or len(widths) == 3 else 2):
                    lo, span = int(rng.integers(0, 5)), int(rng.integers(0, 3))
                    leaves.append((c, int(rng.integers(0, 2)), lo, span))
                if form == "one":
                    break
            k = len(leaves)
            pred.n_leaves, pred.n_columns = k, len(widths)
            for i, (c, neg, lo, span) in enumerate(leaves):
                pred.leaf[i].column, pred.leaf[i].negate, pred.leaf[i].lo, pred.leaf[i].span = c, neg, lo, span
                pred.on_true[i], pred.on_false[i], pred.order[i] = pq.ACCEPT, pq.REJECT, i
            rows = 1 << k
            if form in ("and", "one"):
                pred.truth = 1 << (rows - 1)                         # all leaves true
            elif form == "or":
                pred.truth = ((1 << rows) - 1) & ~1                  # any leaf true
            else:
                pred.truth = int(rng.integers(1, 1 << min(rows, 62))) | (1 << (rows - 1))
            want = np.nonzero(kernel_model.evaluate(pred, arrays))[0].astype(np.uint32)
            pq.check(L.pqps_filter_scan(ctx.h, cols, len(widths), n, 0, C.byref(pred), out.ids, out.cap, out.count, None), "scan")
            kk, got = out.result()
            if kk != len(want) or not np.array_equal(got, want):
                sys.exit(f"DIFF ids: shape={shape} form={form}: {kk} vs {len(want)} matches")
            pq.check(L.pqps_filter_count(ctx.h, cols, len(widths), n, C.byref(pred), out.count, None), "count")
            kk, _ = out.result()
            if kk != len(want):
                sys.exit(f"DIFF count: shape={shape} form={form}: {kk} vs {len(want)}")
        for p in ptrs:
            ctx.free(p)
    out.free()
    print(f"shapes: {len(SHAPES)} shapes x 4 forms ok at n={n}", flush=True)


def sweep_wrap(ctx, n):
    """Scan, index gather and query-stream queries in turn, many times over: with PQPS_EPOCH_START=65530 every scratch
    (the context's and both lanes') takes its epoch through 65535 and starts over at 1 (the tagged hand-off words are
    zeroed, csrc/pqps_hip.hip:run_filter) while words of the epochs before are still lying around."""
    L = pq.lib()
    dev = pq.SyntheticTable(ctx, n, seed=0xC0FFEE)
    host = q.HostSynth(n, seed=0xC0FFEE)
    out = Out(ctx, n + 8)
    names = ["S1", "Q_A", "dense", "Q_C", "none", "u8"]
    want = {k: host.oracle_scan(QUERIES[k]) for k in names}
    bound = {k: dev.bind(QUERIES[k]) for k in names}
    # an index on risk_level for the gather launches
    perm, keys, rng = ctx.malloc(4 * n), ctx.malloc(4 * n), ctx.malloc(64)
    col = pq.column_array([(dev.ptr["risk_level"], 4)])
    pq.check(L.pqps_index_build(ctx.h, col, n, 1, perm, keys, None), "index build")
    order = q.host_index_order(host.arr["risk_level"])
    full = {k: np.zeros(n, dtype=bool) for k in names}
    for k in names:
        full[k][want[k]] = True
    qs = C.c_void_p()
    pq.check(L.pqps_qstream_create(ctx.h, 3, C.byref(qs)), "qstream")
    ring = [Out(ctx, n + 8) for _ in range(3)]
    issued = []
    for it in range(40):
        k = names[it % len(names)]
        pred, cols, nc, _ = bound[k]
        # plain scan on the context
        pq.check(L.pqps_filter_scan(ctx.h, cols, nc, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), k)
        kk, got = out.result()
        if kk != len(want[k]) or not np.array_equal(got, want[k]):
            sys.exit(f"DIFF scan: it={it} query={k}")
        # index gather: rows with risk_level >= 4 in leaf order, re-filtered by the query
        ctx.memset(out.count, 0, 8)
        pq.check(L.pqps_index_probe(ctx.h, keys, 4, 1, n, 4, 0x7FFFFFFF, rng, None), "probe")
        pq.check(L.pqps_filter_gather(ctx.h, cols, nc, perm, rng, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), "gather")
        kk, got = out.result()
        cand = order[host.arr["risk_level"][order] >= 4]
        exp = cand[full[k][cand]].astype(np.uint32)
        if kk != len(exp) or not np.array_equal(got, exp):
            sys.exit(f"DIFF gather: it={it} query={k}: {kk} vs {len(exp)}")
        # the query stream: two lanes, each with a scratch (and an epoch) of its own
        slot = ring[it % 3]
        if len(issued) == 3:
            k0, s0 = issued.pop(0)
            pq.check(L.pqps_qstream_wait(qs, ring.index(s0)), "wait")
            c = C.c_uint64()
            ctx.download(C.byref(c), s0.count, 8)
            a = np.zeros(max(c.value, 1), dtype=np.uint32)
            if c.value:
                ctx.download(a.ctypes.data, s0.ids, 4 * c.value)
            if c.value != len(want[k0]) or not np.array_equal(a[:c.value], want[k0]):
                sys.exit(f"DIFF qstream: it={it} query={k0}")
        pq.check(L.pqps_qstream_scan_slot(qs, it % 3, cols, nc, n, 0, C.byref(pred), slot.ids, slot.cap, slot.count, None), "qstream scan")
        issued.append((k, slot))
    pq.check(L.pqps_qstream_sync(qs), "qstream sync")
    pq.check(L.pqps_qstream_destroy(qs), "qstream destroy")
    print(f"wrap: 40 rounds of scan + gather + query stream ok at n={n}", flush=True)



# ---- leaf windows at the edges of a column's range -------------------------------------------------------------------
# pqps_leaf: hit = ((x - lo) <= span) ^ negate in 32-bit arithmetic for widths 1, 2, 4 and bit planes, in 64 bits for
# width 8.  The catalogue holds the windows engine/hip/hipPredicate.c emits at the edges (window_dict with lb / ub at 0,
# M - 1 and M for a dictionary of M = 2^(8w) values, window_i32 around INT_MIN / -1 / 0 / INT_MAX, which wrap,
# window_unsigned near the top) and raw windows that mean something else in the column's own width.
BIT = "B"                                                  # a bit-plane column in a shape
PLANE_SHAPES = [(8, BIT), (4, BIT), (2, BIT), (1, BIT), (8, 4, BIT), (8, 2, BIT), (8, 1, BIT), (4, 4, BIT), (4, 2, BIT),
                (4, 1, BIT), (2, 2, BIT), (2, 1, BIT), (1, 1, BIT)]
GENERIC_SHAPES = [(BIT, 4), (4, 2, 1, BIT), (BIT,), (8, 4, 2, 1)]    # a plane first, four columns, a lone plane
U64 = (1 << 64) - 1
TOP32 = 0xFFFFFFFF
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def dict_windows(lb, ub):
    """window_dict for a literal with lb values below it and ub = lb + (present): (lo, span, negate) per operator."""
    out = [(ub, TOP32 - ub, 0), (lb, TOP32 - lb, 0)]                    # >, >=
    if lb > 0:
        out.append((0, lb - 1, 0))                                      # <
    if ub > 0:
        out.append((0, ub - 1, 0))                                      # <=
    if ub > lb:
        out += [(lb, 0, 0), (lb, 0, 1)]                                 # =, !=
    return out


def i32_windows(v):
    uv, umin, umax = v & TOP32, 0x80000000, 0x7FFFFFFF
    out = [(uv, 0, 0), (uv, 0, 1), (uv, (umax - uv) & TOP32, 0), (umin, (uv - umin) & TOP32, 0)]     # =, !=, >=, <=
    if v != I32_MAX:
        out.append(((uv + 1) & TOP32, (umax - (uv + 1)) & TOP32, 0))                                  # >
    if v != I32_MIN:
        out.append((umin, ((uv - 1) - umin) & TOP32, 0))                                              # <
    return out


def unsigned_windows(v, top):
    out = [(v, 0, 0), (v, 0, 1), (0, min(v, top), 0)]                   # =, !=, <=
    if v < top:
        out.append((v + 1, top - (v + 1), 0))                           # >
    if v > 0:
        out.append((0, v - 1, 0))                                       # <
    if v <= top:
        out.append((v, top - v, 0))                                     # >=
    return out


def leaf_catalogue(w):
    """(lo, span) pairs at the edges of a column of width w (a bit plane: w = BIT, values 0 / 1)."""
    M = 2 if w == BIT else 1 << (8 * w)
    top = 1 if w == BIT else M - 1
    cat = set()
    for lb in (0, M - 1, M):
        for ub in {lb, lb + 1} if lb < M else {lb}:
            cat.update(dict_windows(lb, ub))
    if w == BIT:
        cat.update(dict_windows(255, 256) + dict_windows(256, 256))    # a bool leaf with a 1-byte dictionary's lo
    for v in (I32_MIN, -1, 0, I32_MAX):
        cat.update(i32_windows(v))
    for v in {0, 1, top - 1, top, U64 - 1, U64}:
        cat.update(unsigned_windows(v, U64 if w == 8 else top))
    for lo in (M, M + 1, TOP32):
        for span in (M - 1, M, TOP32):
            cat.add((lo, span, 0))
    return sorted({(lo & U64, span & U64) for lo, span, _ in cat})


def edge_column(rng, w, n):
    """Random values of the column's whole range mixed with its edges (a bit plane: random 0 / 1)."""
    if w == BIT:
        return (rng.random(n) < 0.4).astype(np.uint8)
    dt, M = DT[w], 1 << (8 * w)
    a = rng.integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
    edges = [0, 1, 2, M - 2, M - 1]
    if w == 4:
        edges += [0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001]
    if w == 8:
        edges += [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, U64]
    pick = rng.random(n) < 0.5
    a[pick] = np.array(edges, dtype=dt)[rng.integers(0, len(edges), int(pick.sum()))]
    a[:len(edges)] = edges                                 # every edge at least once, and at the table's both ends
    a[n - len(edges):] = edges
    return a


def window_hits(x, w, lo, span, negate):
    """The reference: the window test restated in u32 (widths 1, 2, 4, planes) or u64 (width 8) arithmetic."""
    if w == 8:
        hit = (x.astype(np.uint64) - np.uint64(lo)) <= np.uint64(span)
    else:
        hit = (x.astype(np.int64) - (lo & TOP32)) % (1 << 32) <= (span & TOP32)
    return hit != bool(negate)


def reference(pred, arrays, widths):
    hits = [window_hits(arrays[pred.leaf[k].column], widths[pred.leaf[k].column], pred.leaf[k].lo, pred.leaf[k].span,
                        pred.leaf[k].negate) for k in range(pred.n_leaves)]
    if pred.n_leaves <= pq.TT_LEAVES:
        idx = sum(h.astype(np.int64) << k for k, h in enumerate(hits))
        return ((np.uint64(pred.truth) >> idx.astype(np.uint64)) & np.uint64(1)) == 1
    state = np.zeros(len(arrays[0]), dtype=np.int64)
    for s in range(pred.n_leaves):                          # the jump program, step by step
        state = np.where(state == s, np.where(hits[pred.order[s]], pred.on_true[s], pred.on_false[s]), state)
    return state == pq.ACCEPT


def edge_predicate(rng, widths, form):
    cats = [leaf_catalogue(w) for w in widths]
    per = {"one": [1], "wide": [8] + [1] * (len(widths) - 1)}.get(form, [2 if len(widths) <= 2 else 1] * len(widths))
    if form == "one":
        widths = widths[:1]
    leaves = []
    for c in range(len(widths)):
        for _ in range(per[c]):
            lo, span = cats[c][int(rng.integers(0, len(cats[c])))]
            leaves.append((c, int(rng.integers(0, 2)), lo, span))
    pred = pq.Predicate()
    k = len(leaves)
    pred.n_leaves, pred.n_columns = k, len(widths)
    for i, (c, neg, lo, span) in enumerate(leaves):
        pred.leaf[i].column, pred.leaf[i].negate, pred.leaf[i].lo, pred.leaf[i].span = c, neg, lo, span
        pred.order[i] = i
    if k > pq.TT_LEAVES:                                    # AND / OR mixed: each step goes on, or decides
        for s in range(k):
            last = s + 1 == k
            pred.on_true[s] = pq.ACCEPT if last or rng.random() < 0.3 else s + 1
            pred.on_false[s] = pq.REJECT if last or pred.on_true[s] != pq.ACCEPT or rng.random() < 0.5 else s + 1
        return pred
    for i in range(k):
        pred.on_true[i], pred.on_false[i] = pq.ACCEPT, pq.REJECT
    rows = 1 << k
    if form in ("and", "one"):
        pred.truth = 1 << (rows - 1)
    elif form == "or":
        pred.truth = ((1 << rows) - 1) & ~1
    else:
        pred.truth = int(rng.integers(1, 1 << min(rows, 62))) | (1 << (rows - 1))
    return pred


def sweep_windows(ctx, sizes):
    """Every byte shape, every plane shape and the generic layouts; one leaf, AND, OR, a truth-table tree and a jump program
    of more than six leaves; scan, COUNT(*), flags, the query stream and (byte columns) the gather filter over a permuted
    candidate range -- each against the numpy restatement, which must agree with kernel_model.evaluate as well."""
    L = pq.lib()
    rng = np.random.default_rng(0xED6E)
    qs = C.c_void_p()
    pq.check(L.pqps_qstream_create(ctx.h, 2, C.byref(qs)), "qstream")
    cases = 0
    for n in sizes:
        pad = (n + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS
        out = Out(ctx, n + 8)
        flags, cand, rng_dev = ctx.malloc(pad + 64), ctx.malloc(4 * pad), ctx.malloc(64)
        perm = rng.permutation(n).astype(np.uint32)
        ctx.upload(cand, perm.ctypes.data, perm.nbytes)
        r0, r1 = n // 7, n - n // 5
        ctx.upload(rng_dev, np.array([r0, r1], dtype=np.uint64).ctypes.data, 16)
        for shape in SHAPES + PLANE_SHAPES + GENERIC_SHAPES:
            widths = list(w for w in shape if w)
            arrays, ptrs = [], []
            for w in widths:
                a = edge_column(rng, w, n)
                if w == BIT:
                    a_dev = np.zeros(pad // 8, dtype=np.uint8)
                    packed = np.packbits(a, bitorder="little")
                    a_dev[:packed.size] = packed
                else:
                    a_dev = np.zeros(pad, dtype=a.dtype)
                    a_dev[:n] = a
                p = ctx.malloc(a_dev.nbytes)
                ctx.upload(p, a_dev.ctypes.data, a_dev.nbytes)
                arrays.append(a)
                ptrs.append(p)
            cols = pq.column_array([(p, pq.WIDTH_BITS if w == BIT else w) for p, w in zip(ptrs, widths)])
            planes = BIT in widths
            for form in ("one", "and", "or", "tree", "wide"):
                pred = edge_predicate(rng, widths, form)
                nc = pred.n_columns
                mask = reference(pred, arrays, widths)
                assert np.array_equal(mask, kernel_model.evaluate(pred, arrays[:nc])), (shape, form)
                want = np.nonzero(mask)[0].astype(np.uint32)
                what = f"n={n} shape={shape} form={form} leaves={[(l.column, l.negate, hex(l.lo), hex(l.span)) for l in pred.leaf[:pred.n_leaves]]}"
                pq.check(L.pqps_filter_scan(ctx.h, cols, nc, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), what)
                k, got = out.result()
                if k != len(want) or not np.array_equal(got, want):
                    sys.exit(f"DIFF scan ids: {what}: {k} vs {len(want)} matches ({pq.lib().pqps_last_kernel().decode()})")
                pq.check(L.pqps_filter_count(ctx.h, cols, nc, n, C.byref(pred), out.count, None), what)
                k, _ = out.result()
                if k != len(want):
                    sys.exit(f"DIFF count: {what}: {k} vs {len(want)} ({pq.lib().pqps_last_kernel().decode()})")
                pq.check(L.pqps_filter_flags(ctx.h, cols, nc, n, C.byref(pred), flags, out.count, None), what)
                k, _ = out.result()
                f = np.zeros(n, dtype=np.uint8)
                ctx.download(f.ctypes.data, flags, n)
                if k != len(want) or not np.array_equal(f != 0, mask):
                    sys.exit(f"DIFF flags: {what}: {k} vs {len(want)} ({pq.lib().pqps_last_kernel().decode()})")
                slot = cases % 2
                pq.check(L.pqps_qstream_scan_slot(qs, slot, cols, nc, n, 0, C.byref(pred), out.ids, out.cap, out.count, None), what)
                pq.check(L.pqps_qstream_wait(qs, slot), "qstream wait")
                k, got = out.result()
                if k != len(want) or not np.array_equal(got, want):
                    sys.exit(f"DIFF qstream ids: {what}: {k} vs {len(want)} matches")
                if not planes:                               # the gather filter takes byte columns only
                    ctx.memset(out.count, 0, 8)
                    pq.check(L.pqps_filter_gather(ctx.h, cols, nc, cand, rng_dev, n, 0, C.byref(pred), out.ids, out.cap,
                                                  out.count, None), what)
                    k, got = out.result()
                    exp = perm[r0:r1][mask[perm[r0:r1]]]
                    if k != len(exp) or not np.array_equal(got, exp):
                        sys.exit(f"DIFF gather: {what}: {k} vs {len(exp)} matches")
                cases += 1
            for p in ptrs:
                ctx.free(p)
        for p in (flags, cand, rng_dev):
            ctx.free(p)
        out.free()
        print(f"windows: n={n} ok", flush=True)
    pq.check(L.pqps_qstream_sync(qs), "qstream sync")
    pq.check(L.pqps_qstream_destroy(qs), "qstream destroy")
    print(f"windows: {cases} predicates x every entry point ok", flush=True)


def main():
    mode = sys.argv[1]
    ctx = pq.Context(0)
    if mode == "sizes":
        sweep_sizes(ctx, [int(x) for x in sys.argv[2:]] or [1, 4097, 65_537, 300_001, (1 << 21) + 17])
    elif mode == "shapes":
        sweep_shapes(ctx, int(sys.argv[2]) if len(sys.argv) > 2 else 70_001)
    elif mode == "windows":
        sweep_windows(ctx, [int(x) for x in sys.argv[2:]] or [70_001, (1 << 21) + 17])
    elif mode == "wrap":
        sweep_wrap(ctx, int(sys.argv[2]) if len(sys.argv) > 2 else 300_001)
    else:
        sys.exit("usage: variant_driver.py sizes|shapes|windows|wrap ...")
    ctx.close()
    print("OK")


if __name__ == "__main__":
    main()
