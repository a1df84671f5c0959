"""Leaf windows at the edges of a column's range, on every filter path.

A WHERE leaf reaches the device as the window test of pqps_leaf, ((x - lo) <= span) ^ negate, in 32-bit arithmetic for
1-, 2- and 4-byte columns and bit planes and in 64 bits for 8-byte columns.  The host compiler depends on that: `col > x`
past the last value of a full 256-entry dictionary is lo = 256 on a 1-byte column, which selects no row in 32 bits and
every row in 8.  Here:

  * the window sweep of variant_driver.py (every shape, every entry point, edge data and edge windows), under plain and
    streaming loads, each in a process of its own (the shim reads PQPS_NT_LOADS once);
  * pqps_index_select, which copies a probe's rows instead of evaluating them only when the leaf selects exactly the
    probed keys -- in the leaf's arithmetic, not modulo the key width;
  * pqps_bump_codes (INSERT renumbering of dictionary codes) and pqps_ids_checksum (what bench.py's checks rest on)
    against numpy.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import qpelib as q
from variant_driver import window_hits

pq = q.pq
pytestmark = pytest.mark.gpu
DRIVER = str(q.ROOT / "tests" / "variant_driver.py")
U64 = (1 << 64) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.mark.parametrize("nt", ["0", "1"])
def test_window_edges_every_shape_and_entry_point(nt):
    p = subprocess.run([sys.executable, DRIVER, "windows", "70001", str((1 << 21) + 17)], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, PQPS_NT_LOADS=nt), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


# ---- pqps_index_select: copy only what the leaf really accepts -------------------------------------------------------
def one_leaf(lo, span, negate=0, accept_hit=True):
    """A one-leaf predicate on slot 0; accept_hit=False accepts the rows the window test rejects."""
    pred = pq.Predicate()
    pred.n_leaves, pred.n_columns = 1, 1
    pred.leaf[0].column, pred.leaf[0].negate, pred.leaf[0].lo, pred.leaf[0].span = 0, negate, lo & U64, span & U64
    pred.on_true[0], pred.on_false[0], pred.order[0] = pq.ACCEPT, pq.REJECT, 0
    pred.truth = 2 if accept_hit else 1
    return pred


def key_column(rng, kind, n):
    """(numpy keys, width, key_kind) with the edges of the key's range present."""
    if kind == "u8":
        a = rng.integers(0, 256, n, dtype=np.uint8)
        a[:6] = [0, 1, 5, 254, 255, 3]
        return a, 1, 0
    if kind == "i32":
        a = rng.integers(-6, 7, n).astype(np.int32)
        a[rng.random(n) < 0.1] = I32_MIN
        a[rng.random(n) < 0.1] = I32_MAX
        a[:4] = [I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX]
        return a, 4, 1
    a = rng.integers(0, 12, n).astype(np.uint64)
    edges = np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, U64], dtype=np.uint64)
    pick = rng.random(n) < 0.3
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    a[:len(edges)] = edges
    return a, 8, 0


def expected_index_select(keys, w, key_kind, key_lo, key_hi, pred):
    """The probe's rows in index order (key asc, row desc; the probe reads the key window in the key's width), then the
    leaf in the arithmetic of pqps_leaf."""
    mask = U64 if w == 8 else (1 << (8 * w)) - 1
    lo, hi = np.array([key_lo & mask, key_hi & mask], dtype={1: np.uint8, 4: np.uint32, 8: np.uint64}[w])
    if key_kind == 1:
        lo, hi = np.array([lo, hi]).view(np.int32)
    order = q.host_index_order(keys)
    sk = keys[order]
    b, e = np.searchsorted(sk, lo, "left"), np.searchsorted(sk, hi, "right")
    cand = order[b:max(b, e)]
    x = keys.view(np.uint32) if key_kind == 1 else keys
    lf = pred.leaf[0]
    hit = window_hits(x[cand], w, lf.lo, lf.span, lf.negate)
    keep = hit if pred.truth == 2 else ~hit
    return cand[keep].astype(np.uint32)


# (key column, key_lo, key_hi, leaf, copied?): the copy is right only when the leaf selects exactly the probed keys
INDEX_CASES = [
    # a 1-byte key: leaves that equal the key window modulo 2^8 but not in 32 bits select other keys (here: none)
    ("u8", 0, 0, one_leaf(0, 0), True),
    ("u8", 3, 255, one_leaf(3, 252), True),
    ("u8", 0, 255, one_leaf(0, 255), True),
    ("u8", 0, 0, one_leaf(0, 0, negate=1, accept_hit=False), True),
    ("u8", 0, 0, one_leaf(1 << 32, 0), True),                  # lo mod 2^32 is the key window: the same test
    ("u8", 0, 0, one_leaf(256, 0), False),                     # `code = 256`: no row of a 1-byte column
    ("u8", 5, 5, one_leaf(5 + 256, 0), False),
    ("u8", 1, 255, one_leaf(257, 254), False),
    ("u8", 0, 255, one_leaf(256, 0xFFFFFFFF - 256), False),    # `code >= 256` of a full dictionary (hipPredicate.c: window_dict)
    ("u8", 3, 255, one_leaf(3, 252 + 256), False),             # a wider window: every probed row passes all the same
    ("u8", 0, 0, one_leaf(0, 0, negate=1), False),             # the negated window
    ("u8", 256, 256, one_leaf(256, 0), False),                 # a key window beyond the key width (the probe reads [0, 0])
    # an i32 key: windows wrap in two's complement; lo / span are taken mod 2^32 by the leaf test as well
    ("i32", 4, I32_MAX, one_leaf(4, I32_MAX - 4), True),       # risk_level > 3
    ("i32", I32_MIN & 0xFFFFFFFF, 2, one_leaf(0x80000000, (2 - I32_MIN) & 0xFFFFFFFF), True),     # < 3
    ("i32", I32_MIN & U64, 2, one_leaf(0x80000000, (2 - I32_MIN) & 0xFFFFFFFF), True),            # ... key_lo sign-extended
    ("i32", -1 & 0xFFFFFFFF, -1 & 0xFFFFFFFF, one_leaf(0xFFFFFFFF, 0), True),
    ("i32", I32_MAX, I32_MAX, one_leaf(I32_MAX + (1 << 32), 1 << 32), True),                     # the same test mod 2^32
    ("i32", 4, I32_MAX, one_leaf(4, 0xFFFFFFFF - 4), False),   # a window that wraps past INT_MAX into the negative keys
    ("i32", 0, 0, one_leaf(1 << 31, 0), False),
    ("i32", 1 << 32, 1 << 32, one_leaf(0, 0), False),          # a key window beyond 32 bits
    # a u64 key: 64-bit windows; a leaf that agrees only in the low 32 bits selects other keys
    ("u64", 1 << 32, U64, one_leaf(1 << 32, U64 - (1 << 32)), True),
    ("u64", 0, U64, one_leaf(0, U64), True),
    ("u64", 1 << 63, 1 << 63, one_leaf(1 << 63, 0), True),
    ("u64", 1 << 32, 1 << 32, one_leaf(0, 0), False),
    ("u64", 5, U64, one_leaf(5, 0xFFFFFFFF - 5), False),
]


@pytest.mark.parametrize("kind", ["u8", "i32", "u64"])
def test_index_select_copies_only_what_the_leaf_accepts(kind):
    ctx = pq.Context(0)
    L = pq.lib()
    rng = np.random.default_rng(31)
    n = 70_001
    pad = (n + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS
    keys, w, key_kind = key_column(rng, kind, n)
    col, perm, sorted_keys = ctx.malloc(pad * w), ctx.malloc(4 * pad), ctx.malloc(pad * w)
    ids, scratch = ctx.malloc(4 * (n + 8)), ctx.malloc(64)
    try:
        ctx.memset(col, 0, pad * w)
        ctx.upload(col, keys.ctypes.data, keys.nbytes)
        carr = pq.column_array([(col, w)])
        key_col = pq.Column(col, w, 0)
        pq.check(L.pqps_index_build(ctx.h, carr, n, key_kind, perm, sorted_keys, None), "index build")
        copied = 0
        for case_kind, key_lo, key_hi, pred, copy in INDEX_CASES:
            if case_kind != kind:
                continue
            what = (kind, hex(key_lo), hex(key_hi), hex(pred.leaf[0].lo), hex(pred.leaf[0].span), pred.leaf[0].negate, pred.truth)
            want = expected_index_select(keys, w, key_kind, key_lo, key_hi, pred)
            ctx.memset(scratch, 0, 8)
            pq.check(L.pqps_index_select(ctx.h, carr, 1, C.byref(key_col), perm, sorted_keys, key_kind, n, key_lo, key_hi, 0,
                                         C.byref(pred), scratch + 16, ids, n + 8, scratch, None), str(what))
            path = L.pqps_last_kernel().decode()
            ctx.sync()
            k = C.c_uint64()
            ctx.download(C.byref(k), scratch, 8)
            got = np.zeros(max(k.value, 1), dtype=np.uint32)
            if k.value:
                ctx.download(got.ctypes.data, ids, 4 * min(k.value, n + 8))
            assert k.value == len(want) and np.array_equal(got[:k.value], want), (what, k.value, len(want), path)
            if os.environ.get("PQPS_INDEX_COPY", "1") != "0":
                assert path.startswith("append_range_kernel") == copy, (what, path)
            copied += copy
        assert copied >= 2
    finally:
        for p in (col, perm, sorted_keys, ids, scratch):
            ctx.free(p)
        ctx.close()


# ---- pqps_bump_codes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_bump_codes_matches_numpy(width):
    """codes[i] += 1 where codes[i] >= threshold, for i < n_rows only: thresholds 0, a middle value, the largest code and
    one above it; row counts that are not a multiple of 256 (and a guard past the last row)."""
    ctx = pq.Context(0)
    L = pq.lib()
    rng = np.random.default_rng(width)
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[width]
    top = {1: 254, 2: 65534, 4: 0xFFFFFFFE}[width]           # codes of a dictionary that can take one more value
    guard = 4096
    try:
        for n in (1, 255, 257, 70_001, 1_000_003):
            a = rng.integers(0, top + 1, n, dtype=np.uint64).astype(dt)
            a[:min(n, 3)] = [0, top, top // 2][:min(n, 3)]
            p = ctx.malloc((n + guard) * width)
            try:
                full = np.full(n + guard, np.iinfo(dt).max - 1, dtype=dt)
                full[:n] = a
                for t in (0, int(top // 2), int(a.max()), int(a.max()) + 1):
                    ctx.upload(p, full.ctypes.data, full.nbytes)
                    pq.check(L.pqps_bump_codes(ctx.h, p, width, n, t, None), "bump")
                    ctx.sync()
                    got = np.zeros_like(full)
                    ctx.download(got.ctypes.data, p, got.nbytes)
                    want = full.copy()
                    want[:n] = (a.astype(np.uint64) + (a.astype(np.uint64) >= t)).astype(dt)
                    assert np.array_equal(got, want), (width, n, t)
            finally:
                ctx.free(p)
        assert L.pqps_bump_codes(ctx.h, None, width, 0, 0, None) == 0          # nothing to do
    finally:
        ctx.close()


# ---- pqps_ids_checksum -------------------------------------------------------------------------------------------------
def checksum_reference(ids):
    """bench.numpy_checksum restated: (sum ids[i], sum ids[i] * (2 i + 1)) mod 2^64."""
    v = ids.astype(np.uint64)
    with np.errstate(over="ignore"):
        s0 = int(v.sum(dtype=np.uint64))
        s1 = int((v * (np.arange(len(v), dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))
    return s0, s1


def test_ids_checksum_matches_numpy():
    """IDs near 2^32 - 1, so that the order-dependent sum wraps past 2^64 (the plain sum of fewer than 2^32 u32 IDs cannot);
    small counts also against exact Python integers."""
    ctx = pq.Context(0)
    rng = np.random.default_rng(5)
    big = (1 << 22) + 5
    ids_dev = ctx.malloc(4 * big)
    try:
        for count in (0, 1, 63, 64, 65, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, big):
            ids = (0xFFFFFFFF - rng.integers(0, 1 << 20, count)).astype(np.uint32)
            if count:
                ids[0] = 0xFFFFFFFF
                ctx.upload(ids_dev, ids.ctypes.data, ids.nbytes)
            got = ctx.ids_checksum(ids_dev, count)
            want = checksum_reference(ids)
            assert got == want, count
            if count <= 65:
                exact = (sum(int(x) for x in ids) % (1 << 64), sum(int(x) * (2 * i + 1) for i, x in enumerate(ids)) % (1 << 64))
                assert got == exact, count
            if count == big:                                      # the second sum did wrap
                assert float(ids.astype(np.float64) @ (2.0 * np.arange(count) + 1.0)) > 2.0 ** 64
        # the order matters to the second sum only
        ids = np.arange(1000, dtype=np.uint32)
        ctx.upload(ids_dev, ids.ctypes.data, ids.nbytes)
        a = ctx.ids_checksum(ids_dev, 1000)
        ids = ids[::-1].copy()
        ctx.upload(ids_dev, ids.ctypes.data, ids.nbytes)
        b = ctx.ids_checksum(ids_dev, 1000)
        assert a[0] == b[0] and a[1] != b[1] and a == checksum_reference(np.arange(1000, dtype=np.uint32))
    finally:
        ctx.free(ids_dev)
        ctx.close()
