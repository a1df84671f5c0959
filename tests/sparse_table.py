"""Sparse tables: a background of zero bytes plus a few patches of constructed rows.

A table of hundreds of millions of rows is cheap when it is nearly empty: allocate, zero, upload a few KB at the places that matter
and scan.  The expected answer is exact, because the model has to evaluate the placed rows only.

  * The BACKGROUND is every column's bytes zero: code 0 and sudo_used FALSE in every shape used here.
  * A PATCH is a window of whole 1024-row steps at a step-aligned row: u16 codes and booleans built on the host by the constructors
    of test_gpu_packed12_eq.py (which place the code by step, chunk, lane and field of the patch -- a patch starts at an even step, so
    a wave's first and second step stay what the constructor meant).  A window a constructor built as a table of its own (73 729
    rows) is a patch as it is: its partial last step ends in background rows.
  * The patches become the bytes of each column KIND -- "u16", "u8", "plane" (bit r & 7 of byte r >> 3, the layout
    test_gpu_bit_plane.py models with numpy.packbits) and "p12" (pack12_model: 8 rows in 12 bytes, linear) -- and only those byte
    ranges are written over the zero buffers.
  * The buffers keep the contracts of include/pqps_hip.h: whole 4096-row tiles, so every step a scan loads is readable; a step-aligned
    patch begins on a multiple of 128 bytes in every kind; the rows of the last step at and past n are zero in every kind, the
    packed fields among them.
  * The TAIL patch -- the last three steps of the table, its partial last step included, a matching row at n - 1 -- moves: set_n()
    zeroes the old tail's byte ranges and places a new one, so one allocation serves every n, taken in ascending order.  A fixed
    patch is placed as soon as it lies whole below the tail.

SparseTable plans (no device: tests/test_sparse_table.py lays its operations over numpy buffers); DeviceTable carries the
operations out through the shim's malloc / memset / upload."""
import numpy as np

import kernel_model
import pack12_model as pm
import test_gpu_packed12_eq as eq

STEP, TILE, GROUP, QUAD, SUPER = 1024, 8192, 65536, 4 * 65536, 64 * 65536
BUFFER_TILE = 4096                                                  # PQPS_TILE_ROWS: column buffers are whole tiles of this many rows
CODE = eq.CODE
TAIL_STEPS = 3
DENSE_FIRST, DENSE_ROWS = 7 * GROUP, 2 * GROUP                      # two whole groups, either side of the second quad-of-groups boundary
KINDS = ("u16", "u8", "plane", "p12")
EIGHTHS = {"u16": 16, "u8": 8, "plane": 1, "p12": 12}              # bytes per row, in eighths
MAKERS = {"positions": eq.table_positions, "straddle": eq.table_straddle, "decoys": eq.table_decoys, "every step": eq.table_every_step}


def tail_first(n):
    """first row of the table's last three steps (full or partial)"""
    return max((n + STEP - 1) // STEP - TAIL_STEPS, 0) * STEP


def buffer_bytes(kind, n):
    return max((n + BUFFER_TILE - 1) // BUFFER_TILE, 1) * BUFFER_TILE * EIGHTHS[kind] // 8


class Patch:
    """rows [first, first + rows) of the table; codes / sudo cover whole steps, zero (= background) past `rows`"""

    def __init__(self, name, first, codes, sudo):
        assert first % STEP == 0 and len(codes) == len(sudo) > 0
        self.name, self.first, self.rows = name, first, len(codes)
        whole = (len(codes) + STEP - 1) // STEP * STEP
        self.codes, self.sudo = np.zeros(whole, dtype=np.uint16), np.zeros(whole, dtype=np.uint8)
        self.codes[:self.rows], self.sudo[:self.rows] = codes, sudo
        assert int(self.codes.max()) < 4096 and int(self.sudo.max()) <= 1

    @property
    def end(self):
        return self.first + len(self.codes)

    def byte_range(self, kind):
        return self.first * EIGHTHS[kind] // 8, len(self.codes) * EIGHTHS[kind] // 8

    def bytes_of(self, kind):
        """(byte offset in the column's buffer, the patch's bytes there)"""
        if kind == "u16":
            b = self.codes.view(np.uint8)
        elif kind == "u8":
            b = self.sudo
        elif kind == "plane":
            b = np.packbits(self.sudo != 0, bitorder="little")
        else:
            b = pm.pack(self.codes, rows=len(self.codes))
        off, size = self.byte_range(kind)
        assert b.dtype == np.uint8 and b.size == size and off % 128 == 0
        return off, np.ascontiguousarray(b)


def dense_patch(code):
    return Patch("dense", DENSE_FIRST, np.full(DENSE_ROWS, code, dtype=np.uint16), np.zeros(DENSE_ROWS, dtype=np.uint8))


def made(name, first, rows, maker, code):
    assert first % (2 * STEP) == 0                                  # an even step: the constructor's first steps are the waves' first steps
    codes, sudo = MAKERS[maker](rows, code, seed=first // STEP % 1000 + len(maker))
    return Patch(name, first, codes, sudo)


def tail_patch(n, code):
    first = tail_first(n)
    codes, sudo = eq.table_positions(n - first, code, seed=n % 1000)
    codes[-1], sudo[-1] = code, 0                                   # row n - 1 matches the equality AND FALSE
    return Patch("tail", first, codes, sudo)


def fixed_specs(sizes):
    """[(name, first row, rows, maker)] in row order: the table's start, the first group / quad-of-groups / supergroup boundary, the
    dense patch and the last supergroup boundary below each size's tail -- each boundary with two steps on either side."""
    specs = {0: ("start", 0, 2 * TILE, "positions"),                # the table's first two tiles (of two-step waves)
             GROUP: ("group edge", GROUP - 2 * STEP, 73729, "every step"),      # a constructor's own table size: over two group boundaries
             QUAD: ("quad edge", QUAD - 2 * STEP, 4 * STEP, "decoys"),
             DENSE_FIRST: ("dense", DENSE_FIRST, DENSE_ROWS, None)}
    around = [SUPER]
    for n in sizes:
        around.append((tail_first(n) - 2 * STEP) // SUPER * SUPER)  # the last supergroup boundary with room for its patch below the tail
    makers = ["straddle", "positions", "every step", "decoys"]
    for row in sorted(set(around)):
        if row >= SUPER:
            specs[row] = ("supergroup edge", row - 2 * STEP, 4 * STEP, makers[row // SUPER % 4])
    return [specs[k] for k in sorted(specs)]


class SparseTable:
    """The plan of one sparse table: which patches lie in it at the current n, and the byte operations that get the column buffers of
    `kinds` from one n to the next.  `sizes`: every n the table will take (ascending); `edges`: further rows that get a fixed
    patch around them (the rows at which a launch decision switches)."""

    def __init__(self, kinds, sizes, edges=(), code=CODE):
        assert all(k in KINDS for k in kinds) and list(sizes) == sorted(sizes)
        self.kinds, self.code, self.n, self.n_max = tuple(kinds), code, 0, max(sizes)
        specs = {s[1]: s for s in fixed_specs(sizes)}
        for i, row in enumerate(sorted(edges)):
            assert row % (2 * STEP) == 0
            specs.setdefault(row - 2 * STEP, ("switch edge", row - 2 * STEP, 4 * STEP, ["decoys", "every step", "positions", "straddle"][i % 4]))
        self.specs = [specs[k] for k in sorted(specs)]
        for a, b in zip(self.specs, self.specs[1:]):
            assert a[1] + (a[2] + STEP - 1) // STEP * STEP <= b[1], (a, b)      # no two patches overlap
        self.fixed, self.tail = [], None

    def buffer_bytes(self, kind):
        return buffer_bytes(kind, self.n_max)

    def set_n(self, n):
        """-> [("zero", kind, offset, size) | ("write", kind, offset, bytes)], to be carried out in this order"""
        assert self.n <= n <= self.n_max and n >= 1
        ops = []
        if self.tail is not None:
            ops += [("zero", k) + self.tail.byte_range(k) for k in self.kinds]
        new = []
        for name, first, rows, maker in self.specs[len(self.fixed):]:
            if first + (rows + STEP - 1) // STEP * STEP > tail_first(n):
                break
            new.append(dense_patch(self.code) if maker is None else made(name, first, rows, maker, self.code))
        self.fixed += new
        self.tail = tail_patch(n, self.code)
        self.n = n
        for p in new + [self.tail]:
            ops += [("write", k) + p.bytes_of(k) for k in self.kinds]
        return ops

    def patches(self):
        """in row order"""
        return self.fixed + [self.tail]

    # ---- the expected answers: kernel_model on the placed rows, and on one background row ----
    def _columns(self, p, n_cols):
        return [p.codes[:p.rows], p.sudo[:p.rows]][:n_cols]

    def background_matches(self, pred):
        return bool(kernel_model.evaluate(pred, [np.zeros(1, dtype=np.uint16), np.zeros(1, dtype=np.uint8)][:pred.n_columns])[0])

    def expected_ids(self, pred):
        assert not self.background_matches(pred), "an ID list needs a background that does not match"
        ids = [p.first + np.nonzero(kernel_model.evaluate(pred, self._columns(p, pred.n_columns)))[0] for p in self.patches()]
        return np.concatenate(ids).astype(np.uint32)

    def expected_count(self, pred):
        hits = sum(int(kernel_model.evaluate(pred, self._columns(p, pred.n_columns)).sum()) for p in self.patches())
        if not self.background_matches(pred):
            return hits
        return self.n - sum(p.rows for p in self.patches()) + hits

    def full_arrays(self):
        """codes, sudo of all n rows (small n only: the CPU test's reference)"""
        codes, sudo = np.zeros(self.n, dtype=np.uint16), np.zeros(self.n, dtype=np.uint8)
        for p in self.patches():
            codes[p.first:p.first + p.rows], sudo[p.first:p.first + p.rows] = p.codes[:p.rows], p.sudo[:p.rows]
        return codes, sudo


def classes(ids, n, edges=()):
    """{patch class: how many of `ids` lie there}, by row range -- the table's start, two steps either side of the first group
    boundary and of every supergroup boundary, the dense patch, the tail, and for every row of `edges` that the table reaches the
    tail's length either side of it (a table that ends at such a row has its tail there)."""
    ids = np.asarray(ids, dtype=np.int64)
    out = {"start": ids < 2 * TILE,
           "group edge": np.abs(ids + 0.5 - GROUP) < 2 * STEP,
           "supergroup edge": (ids >= SUPER - 2 * STEP) & ((ids + 2 * STEP) % SUPER < 4 * STEP),
           "dense": (ids >= DENSE_FIRST) & (ids < DENSE_FIRST + DENSE_ROWS),
           "tail": ids >= tail_first(n)}
    for e in edges:
        if e <= n:
            out[f"switch edge {e}"] = np.abs(ids + 0.5 - e) < TAIL_STEPS * STEP
    return {k: int(v.sum()) for k, v in out.items()}


class DeviceTable:
    """A SparseTable in device memory: zero-filled buffers for the largest n, one allocation per column."""

    def __init__(self, ctx, kinds, sizes, edges=(), code=CODE):
        self.ctx, self.plan, self.ptrs = ctx, SparseTable(kinds, sizes, edges, code), []
        try:
            for k in kinds:
                nbytes = self.plan.buffer_bytes(k)
                self.ptrs.append(ctx.malloc(nbytes))
                assert self.ptrs[-1] % 16 == 0                      # (pqps_column.data: 16-byte aligned)
                ctx.memset(self.ptrs[-1], 0, nbytes)
        except BaseException:
            self.free()
            raise

    def set_n(self, n):
        for op, kind, off, what in self.plan.set_n(n):
            p = self.ptrs[self.plan.kinds.index(kind)] + off
            if op == "zero":
                self.ctx.memset(p, 0, what)
            else:
                self.ctx.upload(p, what.ctypes.data, what.nbytes)
        self.ctx.sync()

    def bytes_allocated(self):
        return sum(self.plan.buffer_bytes(k) for k in self.plan.kinds)

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []
