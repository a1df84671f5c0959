#!/usr/bin/env python3
"""Runs ONE family of the fused filter-and-aggregate entry points AT THE SHIM in this process and exits non-zero on the
first difference.

The engine reaches pqps_filter_group / _aggregate / _topk / _distinct and their list forms with exact bin ranges, zeroed
padding, bit-plane bool columns and tables far below the streaming threshold; the contract of include/pqps_hip.h is
wider.  This driver calls the shim through pq.lib() with inputs the engine cannot produce and compares the raw device
words with numpy / Python-int references computed from the uploaded arrays -- equality, no tolerances.  The shim reads
PQPS_NT_LOADS once per process, so tests/test_gpu_fused_variants.py starts this script once per family and setting;
after every fused call pqps_last_kernel() must name the expected path AND the load flavour of that setting.

    python tests/fused_driver.py group|aggregate|topk|distinct [n ...]   one family on the GPU (default sizes + one size
                                                                         at which a wave takes a second step)
    python tests/fused_driver.py --self-check                            the references alone (no GPU): against a row-by-
                                                                         row Python loop at n = 1025, and that every
                                                                         declared boundary, K and extreme occurs

Inputs of every case: a u32 column p and a bit plane b carry four predicates -- no WHERE (the engine's chain=None form),
SPARSE p == 1 (rows 0, 1023, 1024, n - 1 and ~30 random ones: whole steps without a match, steps with exactly one), DENSE
b == 1 AND p <= 3 (about half the rows) and NOTHING p == 1 AND b == 1 (no row).  Columns are allocated at ceil(n / 4096) *
4096 rows and the padding past n MATCHES every predicate, with group / value / key entries that would change the answer
(an in-range bin no real row uses, INT32_MIN, UINT64_MAX, the smallest and the largest key): a wrong trim of the partial
last step shows.
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

import qpelib as q

pq = q.pq

BIT = "B"
DT = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}
U64 = (1 << 64) - 1
TOP32 = 0xFFFFFFFF
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
STEP = 1024
DEFAULT_SIZES = [1, 1023, 1024, 1025, 4097, 70_001]
SLOW_N = 1025                                   # the size at which --self-check replays every case row by row
PRED_NAMES = ("all", "sparse", "dense", "nothing")
HIGH_BASE = 3_000_000_000                       # id_base / row_base at the top of the u32 range
SBASE = (-45) & TOP32                           # bin base of the signed column: uint32(min) + 5 with min = -50

# domains (bins, values, groups) of the cases; each has a HOLE, an in-range bin no real row uses, for the padding
GROUP_BINS = (1, 2, 16, 17, 2000, 16384, 16385, 65536)
AGG_BINS = (1, 16, 2304, 2305, 40000)
# (n_values, n_groups): both sides of 64 bits and of 16 384 words.  The last two are there for the instance they reach: without
# a group column only a domain of more than 16 384 words (524 288 values) leaves the LDS form, and
# dist_scan_kernel<DIST_GLOBAL, GROUPED=false> is one of the twelve dist_scan instances
DIST_SHAPES = ((2, 1), (16, 4), (64, 1), (65, 1), (2000, 16), (32768, 16), (32769, 16), (524288, 1), (524289, 1))
TOPK_NARROW = (1, 63, 64, 65, 127, 128, 129, 1024)
TOPK_WIDE = (1, 64, 65, 512)
LIST_CAPS = ("below", "equal", "above")
PQ_TOPK_MAX = 1024                              # PQPS_TOPK_MAX: no case asks for more keys


def hole_for(d):
    return d // 3 + 1 if d >= 6 else None


DOMAINS = sorted(set(GROUP_BINS) | set(AGG_BINS) | {v for v, _ in DIST_SHAPES})
HOLES = sorted({hole_for(d) for d in DOMAINS if hole_for(d) is not None})
EDGES = sorted({e for d in DOMAINS for e in (d - 1, d, d + 1)} | {0, 1, 2, 255, 256, 65535, 65536})
assert not set(HOLES) & set(EDGES) and 3 not in HOLES
I32_EXTREMES = (I32_MIN, I32_MAX, -1, 0, 1)
U64_EXTREMES = (0, (1 << 63) - 1, 1 << 63, U64)
SEVEN = {1: (0, 1, 2, 127, 128, 254, 255), 2: (0, 1, 2, 32767, 32768, 65534, 65535),
         4: (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF), "i4": (I32_MIN, -1000, -1, 0, 1, 1000, I32_MAX),
         8: (0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, U64), BIT: (0, 1)}


def fail(msg):
    print("DIFF " + msg, file=sys.stderr, flush=True)
    sys.exit(3)


def pad_rows(n):
    return (n + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS


def width_top(w):
    return 1 if w == BIT else (1 << (8 * w)) - 1


# ---- the GPU side: buffers, calls, the kernel-name check -------------------------------------------------------------
class Gpu:
    def __init__(self):
        self.ctx = pq.Context(0)
        self.L = pq.lib()
        self.cus = self.ctx.info()[1]
        nt = os.environ.get("PQPS_NT_LOADS")
        self.nt = "NT=true" if nt is not None and int(nt) != 0 else "NT=false"
        self.kernels = set()
        self.out = self.ctx.malloc(4 * 40000 * 8 + 64)           # the largest result: 4 x 40 000 u64
        self.out_bytes = 4 * 40000 * 8
        self.words = self.ctx.malloc(256)                        # count / total words
        self.extra = self.ctx.malloc(16 * 8 + 64)                # distinct[]
        self.scratch, self.scratch_bytes = None, 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        if a.nbytes:
            self.ctx.upload(p, a.ctypes.data, a.nbytes)
            self.ctx.sync()
        return p

    def get(self, ptr, dtype, count):
        self.ctx.sync()                                          # raises if a launch failed
        a = np.zeros(max(count, 1), dtype=dtype)
        if count:
            self.ctx.download(a.ctypes.data, ptr, count * a.itemsize)
        return a[:count]

    def topk_scratch(self, need):
        if need > self.scratch_bytes:
            if self.scratch:
                self.ctx.sync()
                self.ctx.free(self.scratch)
            self.scratch, self.scratch_bytes = self.ctx.malloc(need + 4096), need + 4096
        return self.scratch

    def fused(self, want_kernel, what):
        """After a fused call: the instance the shim says it launched is the case's path with this process's load flavour."""
        got = self.L.pqps_last_kernel().decode()
        want = want_kernel.replace("NT=?", self.nt)
        if got != want:
            fail(f"kernel: {what}: ran {got}, expected {want}")
        self.kernels.add(got)

    def close(self):
        self.ctx.sync()
        self.ctx.close()


class Col:
    """One column: `full` the padded host values (a bit plane: 0 / 1 bytes), `real` = its rows [0, n)."""

    def __init__(self, gpu, full, width, n):
        self.width, self.full, self.real = width, full, full[:n]
        self.u = self.real.astype(np.uint64) if width == 8 else self.real.astype(np.int64).astype(np.uint32)
        self.c = None
        if gpu:
            host = np.packbits(full.astype(np.uint8), bitorder="little") if width == BIT else full
            self.ptr = gpu.put(host)
            self.c = pq.Column(self.ptr, pq.WIDTH_BITS if width == BIT else width, 0)

    def ref(self):
        return C.byref(self.c)


def make_pred(leaves, n_columns, truth):
    pred = pq.Predicate()
    pred.n_leaves, pred.n_columns, pred.truth = len(leaves), n_columns, truth
    for i, (c, neg, lo, span) in enumerate(leaves):
        pred.leaf[i].column, pred.leaf[i].negate, pred.leaf[i].lo, pred.leaf[i].span = c, neg, lo, span
        pred.on_true[i], pred.on_false[i], pred.order[i] = pq.ACCEPT, pq.REJECT, i
    return pred


# name -> (leaves (column, negate, lo, span), columns bound, truth table): column 0 = p (u32), column 1 = b (bit plane).
# "all" is what hipCompileWhere makes of no WHERE clause: no leaf, no column, truth bit 0 set.
PREDS = {"all": ([], 0, 1), "sparse": ([(0, 0, 1, 0)], 1, 0b10), "dense": ([(0, 0, 0, 3), (1, 0, 1, 0)], 2, 1 << 3),
         "nothing": ([(0, 0, 1, 0), (1, 0, 1, 0)], 2, 1 << 3)}


def pred_masks(p, b):
    """The four predicates in plain numpy."""
    return {"all": np.ones(len(p), bool), "sparse": p == 1, "dense": (b == 1) & (p <= 3), "nothing": (p == 1) & (b == 1)}


def pred_row(name, p, b):
    """... and for one row, for the slow loops."""
    return {"all": True, "sparse": p == 1, "dense": b == 1 and p <= 3, "nothing": p == 1 and b == 1}[name]


class Inputs:
    """The predicate columns of one table size, its masks, and the family columns made on demand."""

    def __init__(self, n, gpu):
        self.n, self.pad, self.gpu = n, pad_rows(n), gpu
        rng = self.rng("pred")
        p = rng.choice(np.array([0, 2, 3, 4, 5], dtype=np.uint32), self.pad)
        b = (rng.random(self.pad) < 0.9).astype(np.uint8)
        fixed = [r for r in (0, 1023, 1024, n - 1) if 0 <= r < n]
        sparse = list(dict.fromkeys(fixed + rng.integers(0, n, min(30, n)).tolist()))
        p[sparse], b[sparse] = 1, 0
        p[n:], b[n:] = 1, 1                                      # the padding matches sparse, dense and nothing
        self.p, self.b = p, b
        self.mask = pred_masks(p[:n], b[:n])
        self.sel = {k: np.flatnonzero(m) for k, m in self.mask.items()}
        self.sparse_rows, self.dense_rows = np.array(sparse), self.sel["dense"]
        self.cache, self.lists, self.memo = {}, {}, {}
        if gpu:
            self.pc, self.bc = Col(gpu, p, 4, n), Col(gpu, b, BIT, n)
            self.cols = pq.column_array([(self.pc.ptr, 4), (self.bc.ptr, pq.WIDTH_BITS)])
            self.preds = {k: make_pred(*v) for k, v in PREDS.items()}

    def rng(self, key):
        return np.random.default_rng([0xF05ED, self.n, zlib.crc32(repr(key).encode())])

    def bound(self, pname):
        """(column array, n_cols, predicate) of a fused call."""
        return self.cols, PREDS[pname][1], C.byref(self.preds[pname])

    def plant(self, a, values):
        """`values` at rows that match: the sparse rows and the first dense ones, as many as there are."""
        for rows in (self.sparse_rows, self.dense_rows):
            k = min(len(rows), len(values))
            a[rows[:k]] = values[:k]

    def column(self, key):
        if key not in self.cache:
            full, width = BUILDERS[key[0]](self, *key[1:])
            self.cache[key] = Col(self.gpu, full, width, self.n)
        return self.cache[key]

    def id_list(self, pname, id_base):
        """The matching rows as an ID list: every seventh entry listed twice, shuffled.  -> (rows, device ids, device count)."""
        if (pname, id_base) not in self.lists:
            rows = self.sel[pname]
            rows = self.rng(("list", pname)).permutation(np.concatenate([rows, rows[::7]]))
            ids = (rows + id_base).astype(np.uint32)
            dev = (self.gpu.put(ids), self.gpu.put(np.array([len(ids)], dtype=np.uint64))) if self.gpu else (None, None)
            self.lists[(pname, id_base)] = (rows, ids) + dev
        return self.lists[(pname, id_base)]

    def free(self):
        if self.gpu:
            self.gpu.ctx.sync()
            for c in list(self.cache.values()) + [self.pc, self.bc]:
                self.gpu.ctx.free(c.ptr)
            for _, _, a, b in self.lists.values():
                self.gpu.ctx.free(a)
                self.gpu.ctx.free(b)


# ---- columns ------------------------------------------------------------------------------------------------------------
def pad_pattern(top):
    """Padding of a domain column: bin 0 and every hole the width can hold, in turn."""
    return np.array([0] + [h for h in HOLES if h <= top], dtype=np.uint64)


def domain_values(inp, key, top):
    """Unsigned values over [0, top]: half of them small (0 .. 17), the domain edges, the rest anywhere; no hole."""
    rng, m = inp.rng(key), inp.pad
    edges = np.array([e for e in EDGES if e <= top] + [top], dtype=np.uint64)
    sel = rng.random(m)
    a = np.where(sel < 0.5, rng.integers(0, 18, m).astype(np.uint64),
                 np.where(sel < 0.8, edges[rng.integers(0, len(edges), m)], rng.integers(0, top, m, dtype=np.uint64, endpoint=True)))
    inp.plant(a, edges)
    a[np.isin(a, HOLES)] = 3
    pat = pad_pattern(top)
    a[inp.n:] = pat[np.arange(inp.pad - inp.n) % len(pat)]
    return a


def build_dom(inp, w):
    """Group / value column of width w (bit plane: random bits, padding 0 = in range)."""
    if w == BIT:
        a = (inp.rng(("dom", w)).random(inp.pad) < 0.5).astype(np.uint8)
        a[inp.n:] = 0
        return a, BIT
    return domain_values(inp, ("dom", w), width_top(w)).astype(DT[w]), w


def build_dom_signed(inp):
    """A signed 4-byte column whose minimum is -50: domain values minus 45, so bins against SBASE = uint32(-50) + 5 are
    the domain values; -50 .. -46 fall below the base (and wrap), the top of the domain at or above base + n_bins."""
    a = domain_values(inp, ("dom_s4",), (1 << 31) - 1000).astype(np.int64) - 45
    below = np.array([-50, -46, -48, -47, -49], dtype=np.int64)
    for rows in (inp.sparse_rows[4:], inp.dense_rows[len(EDGES) + 1:]):      # not where the domain's edges were planted
        k = min(len(rows), len(below))
        a[rows[:k]] = below[:k]
    if inp.n:
        a[inp.sparse_rows[0]] = -50                              # the minimum, whatever n
    return a.astype(np.int32), 4


def build_grp18(inp, w):
    """Group column of the COUNT(DISTINCT) cases: 0 .. 17 (rows past every n_groups used), padding 0."""
    rng = inp.rng(("grp18", w))
    a = (rng.random(inp.pad) < 0.5).astype(np.uint8) if w == BIT else rng.integers(0, 18, inp.pad).astype(DT[w])
    a[inp.n:] = 0
    return a, w


def build_val_i32(inp):
    rng = inp.rng("val_i32")
    a = np.where(rng.random(inp.pad) < 0.5, rng.integers(-100, 100, inp.pad), rng.integers(I32_MIN, I32_MAX, inp.pad, endpoint=True))
    inp.plant(a, np.array(I32_EXTREMES, dtype=np.int64))
    a[inp.n:] = I32_MIN
    return a.astype(np.int32), 4


def build_val_u64(inp):
    rng = inp.rng("val_u64")
    a = np.where(rng.random(inp.pad) < 0.3, rng.integers(0, 100, inp.pad).astype(np.uint64),
                 rng.integers(0, U64, inp.pad, dtype=np.uint64, endpoint=True))
    inp.plant(a, np.array(U64_EXTREMES, dtype=np.uint64))
    a[inp.n:] = U64
    return a.astype(np.uint64), 8


def build_key(inp, kind, dist):
    """ORDER BY key: "ties" = seven distinct values (two for a bit plane); "inc" = increasing with the row (strictly where
    the width has the values).  Padding: the smallest and the largest value in turn -- the best key of either direction."""
    rows = np.arange(inp.pad, dtype=np.int64)
    w = 4 if kind == "i4" else kind
    if dist == "ties":
        seven = np.array(SEVEN[kind], dtype=np.int64 if kind == "i4" else np.uint64)
        a = seven[inp.rng(("key", kind)).integers(0, len(seven), inp.pad)]
    elif kind == "i4":
        a = rows - inp.n // 2
    elif kind == 8:
        a = (rows * 3 + 5).astype(np.uint64) << np.uint64(33)
    elif kind == 4:
        a = rows * 2 + 1
    else:
        a = rows * (width_top(w) + 1) // inp.pad
    lo, hi = (I32_MIN, I32_MAX) if kind == "i4" else (0, width_top(w))
    a = a.astype(np.int64 if kind == "i4" else np.uint64)
    a[inp.n::2], a[inp.n + 1::2] = lo, hi
    return a.astype(np.int32 if kind == "i4" else np.uint8 if w == BIT else DT[w]), w


BUILDERS = {"dom": build_dom, "dom_s4": build_dom_signed, "grp18": build_grp18, "val_i32": build_val_i32, "val_u64": build_val_u64,
            "key": build_key}


def list_rows(inp, cfg, pname):
    """The rows a list form reads: ids[0 .. min(count, capacity)) - id_base."""
    rows = inp.id_list(pname, cfg["id_base"])[0]
    return rows[:list_capacity(cfg, len(rows))]


def list_capacity(cfg, count):
    return {"below": count // 2, "equal": count, "above": count + 5}[cfg.get("cap", "equal")]


def case_rows(inp, cfg, pname):
    return list_rows(inp, cfg, pname) if cfg["form"] == "list" else inp.sel[pname]


def bins_of(col, base, rows):
    """(value - base) in 32-bit arithmetic."""
    return (col.u[rows].astype(np.int64) - base) % (1 << 32)


# ---- grouped COUNT(*) -------------------------------------------------------------------------------------------------
def group_path(nb):
    return "GROUP_SMALL" if nb <= 16 else "GROUP_LDS" if nb <= 16384 else "GROUP_GLOBAL"


def group_configs(big):
    if big:
        return [dict(form="scan", col=("dom", 1), base=0, nb=16, preds=("dense",))]
    out = []
    for w in (1, 2, 4, BIT):
        out += [dict(form="scan", col=("dom", w), base=0, nb=nb) for nb in GROUP_BINS if w != BIT or nb <= 2]
    out += [dict(form="scan", col=("dom_s4",), base=SBASE, nb=nb) for nb in GROUP_BINS]
    for i, w in enumerate((1, 2, 4)):
        for nb in (1, 17, 16384, 16385):
            for j, cap in enumerate(LIST_CAPS):
                out.append(dict(form="list", col=("dom", w), base=0, nb=nb, cap=cap, id_base=HIGH_BASE if (i + j) % 2 else 0,
                                preds=("sparse", "dense", "nothing")))
    out.append(dict(form="list", col=("dom_s4",), base=SBASE, nb=2000, cap="above", id_base=HIGH_BASE, preds=("sparse", "dense")))
    return out


def group_reference(inp, cfg, pname):
    d = bins_of(inp.column(cfg["col"]), cfg["base"], case_rows(inp, cfg, pname))
    return {"bins": np.bincount(d[d < cfg["nb"]], minlength=cfg["nb"]).astype(np.uint32)}


def group_slow(inp, cfg, pname):
    col, bins = inp.column(cfg["col"]).real.tolist(), [0] * cfg["nb"]
    rows = list_rows(inp, cfg, pname).tolist() if cfg["form"] == "list" else \
        [r for r in range(inp.n) if pred_row(pname, int(inp.p[r]), int(inp.b[r]))]
    for r in rows:
        d = (col[r] - cfg["base"]) & TOP32
        if d < cfg["nb"]:
            bins[d] += 1
    return {"bins": np.array(bins, dtype=np.uint32)}


def group_execute(gpu, inp, cfg, pname, what):
    L, ctx, nb = gpu.L, gpu.ctx, cfg["nb"]
    col = inp.column(cfg["col"])
    ctx.memset(gpu.out, 0xA5, 4 * nb)                            # the call zeroes its bins
    if cfg["form"] == "scan":
        cols, nc, pred = inp.bound(pname)
        pq.check(L.pqps_filter_group(ctx.h, cols, nc, inp.n, pred, col.ref(), cfg["base"], nb, gpu.out, None), what)
        gpu.fused(f"group_scan_kernel<{group_path(nb)}, NT=?>", what)
    else:
        rows, _, ids, count = inp.id_list(pname, cfg["id_base"])
        pq.check(L.pqps_group_list(ctx.h, col.ref(), inp.n, ids, count, list_capacity(cfg, len(rows)), cfg["id_base"], cfg["base"],
                                   nb, gpu.out, None), what)
    return {"bins": gpu.get(gpu.out, np.uint32, nb)}


# ---- COUNT / SUM / MIN / MAX ------------------------------------------------------------------------------------------
def agg_path(cfg):
    return "AGG_ONE" if cfg["col"] is None else "AGG_LDS" if cfg["nb"] <= 2304 else "AGG_GLOBAL"


def agg_configs(big):
    if big:
        return [dict(form="scan", val="val_i32", col=None, base=0, nb=1, preds=("dense",))]
    out = []
    for val in ("val_i32", "val_u64"):
        out.append(dict(form="scan", val=val, col=None, base=0, nb=1))
        for w in (1, 2, 4, BIT):
            out += [dict(form="scan", val=val, col=("dom", w), base=0, nb=nb) for nb in AGG_BINS if w != BIT or nb <= 16]
        out += [dict(form="scan", val=val, col=("dom_s4",), base=SBASE, nb=nb) for nb in (16, 2304, 2305)]
        lists = [(None, 1)] + [(("dom", w), nb) for w in (1, 2, 4) for nb in (16, 2304, 2305)] + [(("dom_s4",), 2000)]
        for i, (col, nb) in enumerate(lists):
            out.append(dict(form="list", val=val, col=col, base=SBASE if col == ("dom_s4",) else 0, nb=nb, cap=LIST_CAPS[i % 3],
                            id_base=HIGH_BASE if i % 2 else 0, preds=("sparse", "dense", "nothing")))
    return out


def agg_wide_image(col, rows):
    """(the u64 a sum adds, its order-preserving image) per the header: i32 sign-extended and ^ 2^63, u64 as is."""
    if col.width == 8:
        v = col.real[rows].astype(np.uint64)
        return v, v
    v = col.real[rows].astype(np.int64).astype(np.uint64)
    return v, v ^ np.uint64(1 << 63)


def agg_reference(inp, cfg, pname):
    rows, nb = case_rows(inp, cfg, pname), cfg["nb"]
    wide, img = agg_wide_image(inp.column((cfg["val"],)), rows)
    out = np.zeros(4 * nb, dtype=np.uint64)
    out[2 * nb:3 * nb] = U64
    if cfg["col"] is None:
        if len(rows):
            out[0], out[1], out[2], out[3] = len(rows), wide.sum(dtype=np.uint64), img.min(), img.max()
        return {"out": out}
    d = bins_of(inp.column(cfg["col"]), cfg["base"], rows)
    ok = d < nb
    d, wide, img = d[ok], wide[ok], img[ok]
    out[:nb] = np.bincount(d, minlength=nb)
    np.add.at(out[nb:2 * nb], d, wide)                           # u64: wraps mod 2^64
    np.minimum.at(out[2 * nb:3 * nb], d, img)
    np.maximum.at(out[3 * nb:], d, img)
    return {"out": out}


def agg_slow(inp, cfg, pname):
    nb = cfg["nb"]
    val = inp.column((cfg["val"],))
    vals = val.real.tolist()
    grp = inp.column(cfg["col"]).real.tolist() if cfg["col"] else None
    rows = list_rows(inp, cfg, pname).tolist() if cfg["form"] == "list" else \
        [r for r in range(inp.n) if pred_row(pname, int(inp.p[r]), int(inp.b[r]))]
    cnt, tot, mn, mx = [0] * nb, [0] * nb, [U64] * nb, [0] * nb
    for r in rows:
        d = (grp[r] - cfg["base"]) & TOP32 if grp else 0
        if d >= nb:
            continue
        wide = vals[r] & U64                                      # two's complement of the sign-extended value
        img = wide if val.width == 8 else wide ^ (1 << 63)
        cnt[d] += 1
        tot[d] = (tot[d] + wide) & U64
        mn[d], mx[d] = min(mn[d], img), max(mx[d], img)
    return {"out": np.array(cnt + tot + mn + mx, dtype=np.uint64)}


def agg_execute(gpu, inp, cfg, pname, what):
    L, ctx, nb = gpu.L, gpu.ctx, cfg["nb"]
    val = inp.column((cfg["val"],))
    grp = inp.column(cfg["col"]).ref() if cfg["col"] else None
    ctx.memset(gpu.out, 0xA5, 32 * nb)                           # the call initialises its output
    if cfg["form"] == "scan":
        cols, nc, pred = inp.bound(pname)
        pq.check(L.pqps_filter_aggregate(ctx.h, cols, nc, inp.n, pred, val.ref(), grp, cfg["base"], nb, gpu.out, None), what)
        gpu.fused(f"agg_scan_kernel<{agg_path(cfg)}, {'u64' if val.width == 8 else 'i32'}, NT=?>", what)
    else:
        rows, _, ids, count = inp.id_list(pname, cfg["id_base"])
        pq.check(L.pqps_aggregate_list(ctx.h, val.ref(), grp, inp.n, ids, count, list_capacity(cfg, len(rows)), cfg["id_base"],
                                       cfg["base"], nb, gpu.out, None), what)
    return {"out": gpu.get(gpu.out, np.uint64, 4 * nb)}


# ---- ORDER BY .. LIMIT K ----------------------------------------------------------------------------------------------
TOPK_KINDS = (1, 2, 4, "i4", BIT, 8, None)                       # key column: width, signed i32, bit plane, u64, NULL


def topk_configs(big):
    if big:                                                      # the best keys sit in the steps a wave takes second
        return [dict(form="scan", kind=4, dist="inc", desc=1, k=64, base=0, preds=("dense",))]
    out = []
    for kind in TOPK_KINDS:
        ks = TOPK_WIDE if kind == 8 else TOPK_NARROW
        orders = [("ties", 0), ("ties", 1)] if kind is None else [("ties", 0), ("ties", 1), ("inc", 1)]
        for dist, desc in orders:
            out += [dict(form="scan", kind=kind, dist=dist, desc=desc, k=k, base=0) for k in ks]
            out += [dict(form="scan", kind=kind, dist=dist, desc=desc, k=k, base=HIGH_BASE) for k in (64, 65)]
            if kind != BIT:                                      # the list form takes no bit plane
                out += [dict(form="list", kind=kind, dist=dist, desc=desc, k=k, base=HIGH_BASE if i % 2 else 0,
                             preds=("sparse", "dense", "nothing")) for i, k in enumerate((ks[0], 64, 65, ks[-1]))]
    return out


def topk_empty_configs():
    """n == 0 for both entry points: no candidate at all, every word of `out` all ones."""
    out = []
    for kind in (4, 8, None):
        for k in (1, 65):
            out += [dict(form="scan", kind=kind, dist="ties", desc=0, k=k, base=0, empty=True),
                    dict(form="list", kind=kind, dist="ties", desc=1, k=k, base=0, empty=True)]
    return out


def topk_key_values(inp, cfg, rows):
    """(order-preserving image ^ x, wide) of the rows' keys as the header states them."""
    kind, desc = cfg["kind"], cfg["desc"]
    if kind == 8:
        return inp.column(("key", 8, cfg["dist"])).real[rows].astype(np.uint64) ^ np.uint64(U64 if desc else 0), True
    if kind is None:
        img = np.zeros(len(rows), dtype=np.uint64)
    else:
        img = inp.column(("key", kind, cfg["dist"])).u[rows].astype(np.uint64) ^ np.uint64(0x80000000 if kind == "i4" else 0)
    return img ^ np.uint64(TOP32 if desc else 0), False


def topk_reference(inp, cfg, pname):
    k = cfg["k"]
    rows = np.zeros(0, dtype=np.int64) if cfg.get("empty") else \
        inp.id_list(pname, cfg["base"])[0] if cfg["form"] == "list" else inp.sel[pname]
    memo = (cfg["form"], cfg["kind"], cfg["dist"], cfg["desc"], cfg["base"], bool(cfg.get("empty")), pname)
    if memo not in inp.memo:                                     # the sorted composite keys: the same for every K
        img, wide = topk_key_values(inp, cfg, rows)
        table_rows = (rows + cfg["base"]).astype(np.uint64)
        if wide:
            order = np.lexsort((table_rows, img))[:PQ_TOPK_MAX]
            inp.memo[memo] = np.stack([img[order], table_rows[order]], axis=1).reshape(-1)
        else:
            inp.memo[memo] = np.sort((img << np.uint64(32)) | table_rows)[:PQ_TOPK_MAX]
    words = 2 if cfg["kind"] == 8 else 1
    out = np.full(words * k, U64, dtype=np.uint64)
    m = min(k, len(rows))
    out[:words * m] = inp.memo[memo][:words * m]
    want = {"out": out}
    if cfg["form"] == "scan":
        want["count"] = np.array([len(rows)], dtype=np.uint64)
    return want


def topk_slow(inp, cfg, pname):
    kind, k, x = cfg["kind"], cfg["k"], cfg["desc"]
    rows = [] if cfg.get("empty") else inp.id_list(pname, cfg["base"])[0].tolist() if cfg["form"] == "list" else \
        [r for r in range(inp.n) if pred_row(pname, int(inp.p[r]), int(inp.b[r]))]
    vals = inp.column(("key", kind, cfg["dist"])).real.tolist() if kind is not None else None
    keys = []
    for r in rows:
        v = vals[r] if vals else 0
        if kind == 8:
            keys.append((v ^ (U64 if x else 0), r + cfg["base"]))
        else:
            img = (v & TOP32) ^ (0x80000000 if kind == "i4" else 0)
            keys.append((((img ^ (TOP32 if x else 0)) << 32) | (r + cfg["base"]),))
    keys = sorted(keys)[:k]
    flat = [w for key in keys for w in key]
    flat += [U64] * ((2 if kind == 8 else 1) * k - len(flat))
    want = {"out": np.array(flat, dtype=np.uint64)}
    if cfg["form"] == "scan":
        want["count"] = np.array([len(rows)], dtype=np.uint64)
    return want


def topk_execute(gpu, inp, cfg, pname, what):
    L, ctx, kind, k = gpu.L, gpu.ctx, cfg["kind"], cfg["k"]
    wide = 1 if kind == 8 else 0
    key = inp.column(("key", kind, cfg["dist"])).ref() if kind is not None else None
    words = k * (2 if wide else 1)
    ctx.memset(gpu.out, 0, 8 * words)                            # every word is the call's to write
    ctx.memset(gpu.words, 0xA5, 8)
    got = {}
    if cfg["form"] == "scan":
        n = 0 if cfg.get("empty") else inp.n
        need = L.pqps_topk_scratch_bytes(ctx.h, n, k, wide, 1)
        cols, nc, pred = inp.bound(pname)
        pq.check(L.pqps_filter_topk(ctx.h, cols, nc, n, pred, key, 1 if kind == "i4" else 0, cfg["desc"], cfg["base"], k,
                                    gpu.topk_scratch(need), need, gpu.out, gpu.words, None), what)
        if n:
            gpu.fused(f"topk_scan_kernel<{'wide' if wide else 'narrow'}, NT=?>", what)
        got["count"] = gpu.get(gpu.words, np.uint64, 1)
    else:
        rows, _, ids, _ = inp.id_list(pname, cfg["base"])
        n = 0 if cfg.get("empty") else len(rows)
        need = L.pqps_topk_scratch_bytes(ctx.h, n, k, wide, 0)
        pq.check(L.pqps_topk_list(ctx.h, key, 1 if kind == "i4" else 0, cfg["desc"], ids, n, cfg["base"], k, gpu.topk_scratch(need),
                                  need, gpu.out, None), what)
    got["out"] = gpu.get(gpu.out, np.uint64, words)
    return got


# ---- COUNT(DISTINCT) ----------------------------------------------------------------------------------------------------
def dist_path(nv, ng):
    return "DIST_REG" if nv * ng <= 64 else "DIST_LDS" if ng * ((nv + 31) // 32) <= 16384 else "DIST_GLOBAL"


def dist_configs(big):
    if big:
        return [dict(form="scan", val=("dom", 1), grp=None, vb=0, gb=0, nv=64, ng=1, preds=("dense",))]
    out = []
    for nv, ng in DIST_SHAPES:
        vws = [w for w in (1, 2, 4, BIT) if (w != BIT or nv <= 16) and (w != 1 or nv <= 2000) and (nv < 500000 or w == 4)]
        gws = ([None] if ng == 1 else []) + ([w for w in (1, 2, 4, BIT) if w != BIT or ng <= 4] if nv < 500000 else [])
        out += [dict(form="scan", val=("dom", vw), grp=("grp18", gw) if gw else None, vb=0, gb=0, nv=nv, ng=ng) for vw in vws for gw in gws]
    # both bases non-zero, rows out of range on both sides of both: values below SBASE wrap, groups 0 / 1 wrap, 6 .. 17 are past
    out += [dict(form="scan", val=("dom_s4",), grp=("grp18", 4), vb=SBASE, gb=2, nv=nv, ng=4) for nv in (16, 2000)]
    i = 0
    for nv, ng in DIST_SHAPES[:7]:
        for vw in (1, 2, 4):
            if vw == 1 and nv > 2000:
                continue
            gw = (None, 1, 2, 4)[i % 4] if ng == 1 else (1, 2, 4)[i % 3]
            out.append(dict(form="list", val=("dom", vw), grp=("grp18", gw) if gw else None, vb=0, gb=0, nv=nv, ng=ng,
                            cap=LIST_CAPS[i % 3], id_base=HIGH_BASE if i % 2 else 0, preds=("sparse", "dense", "nothing")))
            i += 1
    out.append(dict(form="list", val=("dom_s4",), grp=("grp18", 4), vb=SBASE, gb=2, nv=2000, ng=4, cap="above", id_base=HIGH_BASE,
                    preds=("sparse", "dense")))
    return out


def dist_reference(inp, cfg, pname):
    rows, nv, ng = case_rows(inp, cfg, pname), cfg["nv"], cfg["ng"]
    vb = bins_of(inp.column(cfg["val"]), cfg["vb"], rows)
    gb = bins_of(inp.column(cfg["grp"]), cfg["gb"], rows) if cfg["grp"] else np.zeros(len(rows), dtype=np.int64)
    ok = (vb < nv) & (gb < ng)
    row_bits = (nv + 31) // 32 * 32
    bits = np.zeros(ng * row_bits, dtype=bool)
    bits[gb[ok] * row_bits + vb[ok]] = True
    want = {"bitmap": np.packbits(bits, bitorder="little").view(np.uint32), "distinct": bits.reshape(ng, row_bits).sum(axis=1).astype(np.uint64)}
    if cfg["form"] == "scan":
        want["total"] = np.array([len(rows)], dtype=np.uint64)   # every matching row, in range or not
    return want


def dist_slow(inp, cfg, pname):
    nv, ng = cfg["nv"], cfg["ng"]
    vals = inp.column(cfg["val"]).real.tolist()
    grps = inp.column(cfg["grp"]).real.tolist() if cfg["grp"] else None
    rows = list_rows(inp, cfg, pname).tolist() if cfg["form"] == "list" else \
        [r for r in range(inp.n) if pred_row(pname, int(inp.p[r]), int(inp.b[r]))]
    nw = (nv + 31) // 32
    words, seen = [0] * (ng * nw), [set() for _ in range(ng)]
    for r in rows:
        vb = (vals[r] - cfg["vb"]) & TOP32
        gb = (grps[r] - cfg["gb"]) & TOP32 if grps else 0
        if vb < nv and gb < ng:
            words[gb * nw + (vb >> 5)] |= 1 << (vb & 31)
            seen[gb].add(vb)
    want = {"bitmap": np.array(words, dtype=np.uint32), "distinct": np.array([len(s) for s in seen], dtype=np.uint64)}
    if cfg["form"] == "scan":
        want["total"] = np.array([len(rows)], dtype=np.uint64)
    return want


def dist_execute(gpu, inp, cfg, pname, what):
    L, ctx, nv, ng = gpu.L, gpu.ctx, cfg["nv"], cfg["ng"]
    val = inp.column(cfg["val"])
    grp = inp.column(cfg["grp"]).ref() if cfg["grp"] else None
    words = int(L.pqps_distinct_bitmap_words(nv, ng))
    assert 4 * words <= gpu.out_bytes
    ctx.memset(gpu.out, 0xA5, 4 * words)                         # the call initialises its outputs
    ctx.memset(gpu.words, 0xA5, 8)
    ctx.memset(gpu.extra, 0xA5, 8 * ng)
    got = {}
    grouped = "true" if cfg["grp"] else "false"
    if cfg["form"] == "scan":
        cols, nc, pred = inp.bound(pname)
        pq.check(L.pqps_filter_distinct(ctx.h, cols, nc, inp.n, pred, val.ref(), cfg["vb"], nv, grp, cfg["gb"], ng, gpu.out, gpu.words,
                                        gpu.extra, None), what)
        gpu.fused(f"dist_scan_kernel<{dist_path(nv, ng)}, GROUPED={grouped}, NT=?>", what)
        got["total"] = gpu.get(gpu.words, np.uint64, 1)
    else:
        rows, _, ids, count = inp.id_list(pname, cfg["id_base"])
        cap = list_capacity(cfg, len(rows))
        pq.check(L.pqps_distinct_list(ctx.h, val.ref(), cfg["vb"], nv, grp, cfg["gb"], ng, inp.n, ids, count, cap, cfg["id_base"],
                                      gpu.out, gpu.extra, None), what)
        if cap:
            name = L.pqps_last_kernel().decode()
            if name != f"dist_list_kernel<{dist_path(nv, ng)}, GROUPED={grouped}>":
                fail(f"kernel: {what}: ran {name}")
    got["bitmap"] = gpu.get(gpu.out, np.uint32, words)
    got["distinct"] = gpu.get(gpu.extra, np.uint64, ng)
    return got


FAMILIES = {
    "group": dict(configs=group_configs, reference=group_reference, slow=group_slow, execute=group_execute),
    "aggregate": dict(configs=agg_configs, reference=agg_reference, slow=agg_slow, execute=agg_execute),
    "topk": dict(configs=topk_configs, reference=topk_reference, slow=topk_slow, execute=topk_execute),
    "distinct": dict(configs=dist_configs, reference=dist_reference, slow=dist_slow, execute=dist_execute),
}
# the fused scan instances of each family, without the load flavour: 3, 6, 2 and 6
INSTANCES = {
    "group": {f"group_scan_kernel<{p}>" for p in ("GROUP_SMALL", "GROUP_LDS", "GROUP_GLOBAL")},
    "aggregate": {f"agg_scan_kernel<{p}, {v}>" for p in ("AGG_ONE", "AGG_LDS", "AGG_GLOBAL") for v in ("i32", "u64")},
    "topk": {"topk_scan_kernel<narrow>", "topk_scan_kernel<wide>"},
    "distinct": {f"dist_scan_kernel<{p}, GROUPED={g}>" for p in ("DIST_REG", "DIST_LDS", "DIST_GLOBAL") for g in ("false", "true")},
}


def compare(what, got, want):
    for field, w in want.items():
        g = got[field]
        if g.shape != w.shape or not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0]) if g.shape == w.shape else -1
            fail(f"{what}: {field}[{at}] = {g[at] if at >= 0 else g.shape} != {w[at] if at >= 0 else w.shape} "
                 f"({int((g != w).sum()) if at >= 0 else '?'} of {w.size} words differ)")


def describe(family, n, cfg, pname):
    return f"{family} n={n} pred={pname} " + " ".join(f"{k}={v}" for k, v in cfg.items() if k != "preds")


def run_case(family, gpu, inp, n, cfg, pname, slow):
    """One case: the shim (with a GPU) or, where `slow`, the row-by-row loop against the numpy reference."""
    fam, what = FAMILIES[family], describe(family, n, cfg, pname)
    want = fam["reference"](inp, cfg, pname)
    if gpu:
        compare(what, fam["execute"](gpu, inp, cfg, pname, what), want)
    elif slow:
        compare("self-check " + what, want, fam["slow"](inp, cfg, pname))


def sweep(family, gpu, sizes, big):
    """Every case of the family at every size.  With a GPU: the shim against the numpy reference.  Without: the numpy
    reference against the row-by-row loop at SLOW_N, elsewhere computed and discarded (that it runs at every size)."""
    fam, cases = FAMILIES[family], 0
    for n in sizes + ([big] if big else []):
        inp = Inputs(n, gpu)
        for cfg in fam["configs"](n == big):
            for pname in cfg.get("preds", PRED_NAMES):
                run_case(family, gpu, inp, n, cfg, pname, n == SLOW_N)
                cases += 1
        inp.free()
        print(f"{family}: n={n} ok", flush=True)
    if family == "topk":                                         # last: no input at all (a one-row table lends valid pointers)
        inp = Inputs(1, gpu)
        for cfg in topk_empty_configs():
            run_case(family, gpu, inp, 0, cfg, "all", True)
            cases += 1
        inp.free()
        print(f"{family}: n=0 ok", flush=True)
    return cases


def planned_cases(family, sizes=len(DEFAULT_SIZES), big=True):
    """The cases a sweep of the family over `sizes` table sizes (and the large one) runs, counted from the case lists alone."""
    def count(configs):
        return sum(len(cfg.get("preds", PRED_NAMES)) for cfg in configs)
    configs = FAMILIES[family]["configs"]
    return sizes * count(configs(False)) + (count(configs(True)) if big else 0) + (len(topk_empty_configs()) if family == "topk" else 0)


# ---- --self-check: what the generated inputs must contain ---------------------------------------------------------------
def check_inputs():
    for n in DEFAULT_SIZES:
        inp = Inputs(n, None)
        full = pred_masks(inp.p, inp.b)
        assert not inp.mask["nothing"].any() and inp.mask["all"].all()
        assert all(full[k][n:].all() for k in PRED_NAMES), "the padding must match every predicate"
        for r in (0, 1023, 1024, n - 1):
            assert not 0 <= r < n or inp.mask["sparse"][r]
        assert inp.mask["sparse"].sum() <= 34 and (n < 1023 or 0.35 < inp.mask["dense"].mean() < 0.65)
        if n >= 4097:                                            # whole steps without a match, and steps with exactly one
            per_step = np.bincount(inp.sel["sparse"] // STEP, minlength=(n + STEP - 1) // STEP)
            assert (per_step == 1).any() and (n < 70_001 or (per_step == 0).any())
        step_end = min((n + STEP - 1) // STEP * STEP, inp.pad)
        for w in (1, 2, 4):
            col = inp.column(("dom", w))
            assert not np.isin(col.real, HOLES).any()
            for d in DOMAINS:
                h = hole_for(d)
                if n >= SLOW_N and h is not None and h <= width_top(w):      # the hole of every domain is in the partial step's padding
                    assert h in col.full[n:step_end], (n, w, d)
                if n >= 1023 and d - 1 <= width_top(w):                      # the last bin of every domain holds a matching row
                    assert (col.real[inp.sel["dense"]] == d - 1).any() and (col.real[inp.sel["all"]] == min(d, width_top(w))).any(), (n, w, d)
        s4 = inp.column(("dom_s4",))
        assert s4.real.min() == -50 and (n < 1023 or all((s4.real[inp.sel[k]] < -45).any() for k in ("sparse", "dense")))
        assert n < 1023 or (s4.real[inp.sel["dense"]].astype(np.int64) + 45 >= 65536).any()
        assert n == inp.pad or (inp.column(("val_i32",)).full[n:] == I32_MIN).all() and (inp.column(("val_u64",)).full[n:] == U64).all()
        if n >= 1023:
            for key, extremes in ((("val_i32",), I32_EXTREMES), (("val_u64",), U64_EXTREMES)):
                vals = inp.column(key).real
                for k in ("sparse", "dense"):
                    assert all((vals[inp.sel[k]] == vals.dtype.type(e)).any() for e in extremes), (n, key, k)
            assert sum(int(v) for v in inp.column(("val_u64",)).real[inp.sel["dense"]]) >= 1 << 64, "the u64 sum must wrap"
            inc = inp.column(("key", 4, "inc")).real.astype(np.int64)
            assert (np.diff(inc) > 0).all() and (np.diff(inp.column(("key", 8, "inc")).real.astype(object)) > 0).all()
            for kind in TOPK_KINDS[:-1]:
                assert len(set(inp.column(("key", kind, "ties")).real.tolist())) == len(SEVEN[kind]), (n, kind)
            assert len(inp.sel["sparse"]) < 63 < 1024 < len(inp.sel["dense"]) or n < 4097       # M < K and M > K both occur


def check_plans():
    seen = {}
    for family, fam in FAMILIES.items():
        configs = fam["configs"](False)
        scans = [c for c in configs if c["form"] == "scan"]
        assert scans and [c for c in configs if c["form"] == "list"] and fam["configs"](True), family
        seen[family] = configs
    g, a, t, d = (seen[f] for f in ("group", "aggregate", "topk", "distinct"))
    names = {
        "group": {f"group_scan_kernel<{group_path(c['nb'])}>" for c in g if c["form"] == "scan"},
        "aggregate": {f"agg_scan_kernel<{agg_path(c)}, {'u64' if c['val'] == 'val_u64' else 'i32'}>" for c in a if c["form"] == "scan"},
        "topk": {f"topk_scan_kernel<{'wide' if c['kind'] == 8 else 'narrow'}>" for c in t if c["form"] == "scan"},
        "distinct": {f"dist_scan_kernel<{dist_path(c['nv'], c['ng'])}, GROUPED={'true' if c['grp'] else 'false'}>" for c in d if c["form"] == "scan"},
    }
    assert names == INSTANCES, names
    assert sorted(len(v) for v in INSTANCES.values()) == [2, 3, 6, 6]
    for w in (1, 2, 4):                                          # both sides of every switch, for every byte width
        assert {c["nb"] for c in g if c["form"] == "scan" and c["col"] == ("dom", w)} == set(GROUP_BINS)
        assert {c["nb"] for c in a if c["form"] == "scan" and c["col"] == ("dom", w)} == set(AGG_BINS)
    assert {c["nb"] for c in g if c["col"] == ("dom", BIT)} == {1, 2} and {c["nb"] for c in g if c["base"]} >= set(GROUP_BINS)
    assert [group_path(nb) for nb in (16, 17, 16384, 16385)] == ["GROUP_SMALL", "GROUP_LDS", "GROUP_LDS", "GROUP_GLOBAL"]
    assert [agg_path(dict(col=1, nb=nb)) for nb in (2304, 2305)] == ["AGG_LDS", "AGG_GLOBAL"] and 2304 * 28 == 64512
    assert {c["col"] for c in a if c["form"] == "scan"} >= {None, ("dom", BIT), ("dom_s4",)}
    for kind in TOPK_KINDS:
        for form in ("scan", "list"):
            ks = {c["k"] for c in t if c["kind"] == kind and c["form"] == form}
            if form == "scan":
                assert ks == set(TOPK_WIDE if kind == 8 else TOPK_NARROW), (kind, ks)
            else:
                assert (not ks) if kind == BIT else ks >= {1, 64, 65}, (kind, ks)
            assert kind == BIT and form == "list" or {c["base"] for c in t if c["kind"] == kind and c["form"] == form} == {0, HIGH_BASE}
        assert {(c["dist"], c["desc"]) for c in t if c["kind"] == kind} == {("ties", 0), ("ties", 1)} | ({("inc", 1)} if kind is not None else set())
    empty = topk_empty_configs()
    assert {c["form"] for c in empty} == {"scan", "list"} and {c["kind"] for c in empty} == {4, 8, None}
    assert {(c["nv"], c["ng"]) for c in d if c["form"] == "scan" and not c["vb"]} == set(DIST_SHAPES)
    assert [dist_path(*s) for s in DIST_SHAPES] == ["DIST_REG"] * 3 + ["DIST_LDS"] * 3 + ["DIST_GLOBAL", "DIST_LDS", "DIST_GLOBAL"]
    assert {c["val"][1] for c in d if c["val"][0] == "dom"} == {1, 2, 4, BIT} and {c["grp"][1] for c in d if c["grp"]} == {1, 2, 4, BIT}
    assert any(c["vb"] and c["gb"] for c in d if c["form"] == "scan") and any(c["vb"] and c["gb"] for c in d if c["form"] == "list")
    for configs in (g, a, d):
        lists = [c for c in configs if c["form"] == "list"]
        assert {c["cap"] for c in lists} == set(LIST_CAPS) and {c["id_base"] for c in lists} == {0, HIGH_BASE}


def self_check(sizes=DEFAULT_SIZES):
    """The case lists and the generated inputs of every default size, then the references at `sizes`."""
    check_plans()
    check_inputs()
    for family in FAMILIES:
        cases = sweep(family, None, list(sizes), None)
        assert cases == planned_cases(family, len(sizes), big=False) > 0, (family, cases)
        print(f"{family}: {cases} cases", flush=True)


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in list(FAMILIES) + ["--self-check"]:
        sys.exit("usage: fused_driver.py group|aggregate|topk|distinct [n ...]  |  fused_driver.py --self-check")
    if sys.argv[1] == "--self-check":
        self_check()
        print("OK")
        return
    family = sys.argv[1]
    gpu = Gpu()
    sizes = [int(x) for x in sys.argv[2:]]
    # the smallest table at which a wave of the persistent grid (8 workgroups of 4 waves per CU) takes a second step
    big = None if sizes else STEP * (4 * 8 * gpu.cus + 1) + 3
    cases = sweep(family, gpu, sizes or DEFAULT_SIZES, big)
    gpu.close()
    assert cases == planned_cases(family, len(sizes or DEFAULT_SIZES), big is not None), (cases, "no case may be skipped")
    print(f"{family}: {gpu.nt} cases={cases} kernels={len(gpu.kernels)}")
    for name in sorted(gpu.kernels):
        print("  " + name)
    print("OK")


if __name__ == "__main__":
    main()
