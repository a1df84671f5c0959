"""pqps_sort_list, pqps_distinct_sort, pqps_distinct_count and pqps_column_bounds called at the shim, against the contract of
include/pqps_hip.h, with inputs the engine never sends; every comparison is equality on the downloaded device words.

The engine hands the two sort forms ascending, duplicate-free scan lists, keys and exact bins it made itself, and never reads
`out_keys`; the popcount and the bounds call it reaches with its own bitmaps and columns only.  Here:

  * lists of 0 .. 300 001 entries drawn from a 70 001-row table, shuffled, every seventh entry listed twice, never ascending, with
    id_base 0 and 3 000 000 000: the tile edges of dist_unique_kernel (63 .. 65), one and two sort tiles (4095 .. 4097), a
    digit-major histogram that takes a second scan block (65 536 / 65 537 = 16 / 17 tiles), and, on its own, a list of
    8 x CUs x 4096 + 4097 entries, the shortest at which a workgroup of the sort takes a second tile
  * pqps_sort_list: keys of 1, 2, 4 bytes, signed i32, u64 and NULL, both directions; every key equal (no pass runs), seven
    values with ties and extremes, keys that differ in one byte only (each byte of the image: the number of passes, and with it
    the buffer the result ends in, changes with the byte), INT32_MIN / INT32_MAX, full-range random keys; out_ids and out_keys
    against numpy.lexsort((rows, image ^ x)), out_keys NULL too, n = 0 writes nothing
  * pqps_distinct_sort: value columns of 1, 2, 4 bytes, i32 against its minimum and against minimum + 5 (values below the base
    wrap and still count), u64 with the extremes and many duplicates; no group column, 1-, 2- and 4-byte group columns with
    rows outside the bins below and above, ONE group with rows outside, 65 536 groups, every row outside; distinct[] against
    sets, out_keys (group-major, rows outside the bins last), out_keys NULL, n = 0 zeroes distinct[], pqps_last_kernel()
  * pqps_distinct_count: bitmaps of 1 .. 257 words per row, 65 536 rows, exactly the 2^30-bit cap, all zero, all ones; the refusals
  * pqps_column_bounds: 0 .. 300 001 rows, the extremes alone and at row 0, row n - 1 and in the last partial wave; the refusal
  * every output buffer holds 0xA5 bytes before the call and the words behind the documented output must still hold them

Found by it: pqps_distinct_sort over an 8-byte value column with a group column and n_groups == 1 skipped the stable group pass,
so rows outside the single bin stayed interleaved with the rows inside it and a value listed (in, out, in) counted twice.  On the
library before the fix exactly the wide one-group cases in which a value is listed that way fail: 12 of the 289 cases, all in
test_distinct_sort_at_the_shim[u8] (the three hand-made rows count 2 for 1; 65 entries 24 for 17; 65 537 entries 20 098 for 8 652).

The CPU tests (no `gpu` mark) check the two sort references against row-by-row Python loops at 1025 entries, and that the case
lists hold every edge named above.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import fused_driver as fd
import qpelib as q

pq = q.pq
U64, TOP32, HIGH_BASE = fd.U64, fd.TOP32, fd.HIGH_BASE
I32_MIN, I32_MAX = fd.I32_MIN, fd.I32_MAX
N_ROWS = 70_001                                 # the table of every list but the long one
MS = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 65_536, 65_537, 300_001)
ID_BASES = (0, HIGH_BASE)
GUARD = 16                                      # words checked behind every documented output
SLOW_M = 1025                                   # the list length at which the CPU tests replay the references row by row
SORT_TILE = 4096                                # pairs per workgroup of the radix sort
PQPS_OK, PQPS_EINVAL = 0, -1


def rng(*key):
    return np.random.default_rng([0x50F7, zlib.crc32(repr(key).encode())])


@functools.lru_cache(maxsize=None)
def make_list(m, n_rows=N_ROWS):
    """m rows of the table: shuffled, every seventh entry listed twice, never ascending (m >= 2)."""
    r = rng("list", m, n_rows)
    if m == 2:
        return np.sort(r.permutation(n_rows)[:2])[::-1].astype(np.int64)
    b = (7 * m + 7) // 8                                         # b + ceil(b / 7) >= m
    base = r.permutation(n_rows)[:b] if b <= n_rows else r.integers(0, n_rows, b)
    rows = r.permutation(np.concatenate([base, base[::7]]))[:m].astype(np.int64)
    rows.setflags(write=False)
    return rows


def ascending(rows):
    return bool((np.diff(rows) >= 0).all())


def differs(what, got, want):
    """fused_driver.compare, returning the case instead of ending the process (the difference goes to stderr)."""
    try:
        fd.compare(what, got, want)
    except SystemExit:
        return True
    return False


# ---- pqps_sort_list: the case list --------------------------------------------------------------------------------------
KINDS = (1, 2, 4, "i4", 8, None)                                 # key column: bytes, signed i32, u64, NULL


def kind_width(kind):
    return 4 if kind == "i4" else kind


def patterns_of(kind):
    """(a) equal, (b) seven, (c) one differing byte per byte of the image (+ INT32_MIN / INT32_MAX for i32), (d) random."""
    if kind is None:
        return ("equal",)                                        # a NULL column: every value 0
    return ("equal", "seven") + tuple(("byte", b) for b in range(kind_width(kind))) + (("minmax",) if kind == "i4" else ()) + ("random",)


@functools.lru_cache(maxsize=None)
def key_raw(kind, pattern, n_rows=N_ROWS):
    """The key column as unsigned bit patterns (u64)."""
    if kind is None:
        return np.zeros(n_rows, dtype=np.uint64)
    w, r = kind_width(kind), rng("key", kind, pattern, n_rows)
    mask = (1 << (8 * w)) - 1
    seven = np.array([v & mask for v in fd.SEVEN[kind]], dtype=np.uint64)
    if pattern == "equal":
        a = np.full(n_rows, seven[3], dtype=np.uint64)
    elif pattern == "seven":
        a = seven[r.integers(0, len(seven), n_rows)]
    elif pattern == "minmax":
        a = np.array([I32_MIN & mask, I32_MAX], dtype=np.uint64)[r.integers(0, 2, n_rows)]
    elif pattern == "random":
        a = r.integers(0, mask, n_rows, dtype=np.uint64, endpoint=True)
    else:
        shift = 8 * pattern[1]
        base = 0x5A5A5A5A5A5A5A5A & mask & ~(0xFF << shift)
        a = np.uint64(base) | (r.integers(0, 256, n_rows, dtype=np.uint64) << np.uint64(shift))
    a.setflags(write=False)
    return a


def typed(raw, kind):
    """The bit patterns as the column's own array."""
    w = kind_width(kind)
    a = raw.astype(fd.DT[w])
    return a.view(np.int32) if kind == "i4" else a


def sort_image(kind, desc, raw):
    """image ^ x per the header: v ^ 2^31 for i32, v otherwise; x all ones over 32 (narrow) or 64 (wide) bits for DESC."""
    if kind == 8:
        return raw ^ np.uint64(U64 if desc else 0)
    return raw ^ np.uint64(0x80000000 if kind == "i4" else 0) ^ np.uint64(TOP32 if desc else 0)


def sort_reference(raw, kind, desc, rows):
    """(rows in the answer's order, their sort keys): ties by ascending row, a row listed twice appears twice."""
    key = sort_image(kind, desc, raw[rows])
    order = np.lexsort((rows, key))
    return rows[order], key[order]


def sort_slow(raw, kind, desc, rows):
    vals, x = raw.tolist(), (U64 if kind == 8 else TOP32) if desc else 0
    flip = 0x80000000 if kind == "i4" else 0
    pairs = sorted(((vals[r] ^ flip ^ x, r) for r in rows.tolist()), key=lambda p: (p[0], p[1]))
    return np.array([p[1] for p in pairs], dtype=np.int64), np.array([p[0] for p in pairs], dtype=np.uint64)


def sort_cases():
    """Every kind x direction meets every M; every pattern meets 4097 and 65 537 in both directions.  `keys`: out_keys given."""
    out, i = [], 0
    for kind in KINDS:
        pats = patterns_of(kind)
        for desc in (0, 1):
            for m in MS:
                out.append(dict(kind=kind, desc=desc, pattern=pats[i % len(pats)], m=m, id_base=ID_BASES[(i + i // len(MS)) % 2], keys=i % 3 != 2))
                i += 1
    for kind in KINDS:
        for pattern in patterns_of(kind):
            for desc in (0, 1):
                for m in (4097, 65_537):
                    out.append(dict(kind=kind, desc=desc, pattern=pattern, m=m, id_base=ID_BASES[(i // 2) % 2], keys=i % 3 != 2))
                    i += 1
    return tuple(out)


SORT_CASES = sort_cases()


def long_list_length(cus):
    """The shortest list at which a workgroup of the sort (8 per CU) takes a second tile, plus a partial tile."""
    return 8 * cus * SORT_TILE + SORT_TILE + 1


# ---- pqps_distinct_sort: the case list ------------------------------------------------------------------------------------
VALUE_SPECS = ("u1", "u2", "u4", "i4min", "i4min5", "u8")
HEAVY_U64 = fd.U64_EXTREMES                                      # 60 % of the u64 rows hold one of these
G18 = tuple((("g18", w), gb, ng) for w in (1, 2, 4) for gb, ng in ((0, 18), (2, 13), (0, 1)))
# (group column, g_base, n_groups): none; 0 .. 17 over all bins, with rows below and above, with ONE bin and rows above it; 65 536
# groups; every row outside (0 .. 17 minus 18 wraps past every bin)
GROUP_SPECS = ((None, 0, 1),) + G18 + ((("g16", 2), 0, 65_536), (("g18", 2), 18, 4))
DEFECT_MS = (3, 65, 4097, 65_537)                                # wide values, a group column, one group, rows outside


@functools.lru_cache(maxsize=None)
def value_column(spec, n_rows=N_ROWS):
    """-> (the column, v_base)."""
    r = rng("value", spec[:2] if spec.startswith("i4") else spec)
    sel = r.random(n_rows)
    if spec == "u1":
        return r.integers(0, 256, n_rows).astype(np.uint8), 0
    if spec == "u2":
        return np.where(sel < 0.5, r.integers(0, 50, n_rows), r.integers(0, 65_536, n_rows)).astype(np.uint16), 0
    if spec == "u4":
        a = np.where(sel < 0.5, r.integers(0, 100, n_rows), r.integers(0, TOP32, n_rows, endpoint=True))
        a[r.integers(0, n_rows, 700)] = np.array(fd.SEVEN[4] * 100)
        return a.astype(np.uint32), 0
    if spec in ("i4min", "i4min5"):                              # the same column: five values below the second base
        a = np.where(sel < 0.5, r.integers(-50, 50, n_rows), r.integers(I32_MIN, I32_MAX, n_rows, endpoint=True))
        a[r.integers(0, n_rows, 500)] = np.array(fd.I32_EXTREMES * 100)
        a[r.integers(0, n_rows, 700)] = np.array([I32_MIN + d for d in range(7)] * 100)
        a = a.astype(np.int32)
        return a, ((int(a.min()) & TOP32) + (5 if spec == "i4min5" else 0)) & TOP32
    # 10 % small numbers, 30 % anywhere in u64, 60 % one of the four extremes
    a = np.where(sel < 0.1, r.integers(0, 100, n_rows).astype(np.uint64), r.integers(0, U64, n_rows, dtype=np.uint64, endpoint=True))
    heavy = np.array(HEAVY_U64, dtype=np.uint64)[r.integers(0, len(HEAVY_U64), n_rows)]
    return np.where(sel < 0.4, a, heavy).astype(np.uint64), 0


@functools.lru_cache(maxsize=None)
def group_column(gkey, n_rows=N_ROWS):
    name, w = gkey
    r = rng("group", gkey)
    if name == "g16":
        return r.integers(0, 65_536, n_rows).astype(np.uint16)
    return np.where(r.random(n_rows) < 0.5, 0, r.integers(1, 18, n_rows)).astype(fd.DT[w])      # half the rows in bin 0


def dist_bins(value, group, rows):
    """(group bins, value bins, inside the bins) of the listed rows: (value - base) in 32-bit arithmetic, u64 values as they are."""
    col, v_base = value_column(value)
    gkey, g_base, n_groups = group
    v = col[rows]
    vb = v.astype(np.uint64) if col.dtype == np.uint64 else ((v.astype(np.int64) - v_base) % (1 << 32)).astype(np.uint64)
    gb = (group_column(gkey)[rows].astype(np.int64) - g_base) % (1 << 32) if gkey else np.zeros(len(rows), dtype=np.int64)
    return gb.astype(np.uint64), vb, gb < n_groups


def dist_reference(value, group, rows):
    """distinct[g] = the different value bins among the listed rows of group bin g; the in-range rows' keys sorted by (group,
    value) -- as `keys` (group << 32 | value) for narrow values, as (`vals`, `grps`) for u64 values."""
    n_groups = group[2]
    gb, vb, ok = dist_bins(value, group, rows)
    gb, vb = gb[ok], vb[ok]
    want = {"k_in": int(ok.sum())}
    if value == "u8":
        order = np.lexsort((vb, gb))
        vals, grps = vb[order], gb[order]
        first = np.ones(len(vals), dtype=bool)
        first[1:] = (vals[1:] != vals[:-1]) | (grps[1:] != grps[:-1])
        want.update(vals=vals, grps=grps.astype(np.uint32), distinct=np.bincount(grps[first].astype(np.int64), minlength=n_groups).astype(np.uint64))
    else:
        keys = np.sort((gb << np.uint64(32)) | vb)
        want.update(keys=keys, distinct=np.bincount((np.unique(keys) >> np.uint64(32)).astype(np.int64), minlength=n_groups).astype(np.uint64))
    return want


def dist_slow(value, group, rows):
    col, v_base = value_column(value)
    gkey, g_base, n_groups = group
    vals, grps = col.tolist(), group_column(gkey).tolist() if gkey else None
    seen, pairs = {}, []
    for r in rows.tolist():
        vb = vals[r] if value == "u8" else (vals[r] - v_base) & TOP32
        gb = (grps[r] - g_base) & TOP32 if grps else 0
        if gb < n_groups:
            seen.setdefault(gb, set()).add(vb)
            pairs.append((gb, vb))
    pairs.sort()
    return {"k_in": len(pairs), "distinct": np.array([len(seen.get(g, ())) for g in range(n_groups)], dtype=np.uint64), "pairs": pairs}


def value_order_count(value, group, rows):
    """What a walk over the keys in VALUE order alone counts (u64 values): the predecessor test `value or group differs` sees a
    value listed (in, out, in) twice.  The wide one-group cases must all tell this from the answer."""
    gb, vb, ok = dist_bins(value, group, rows)
    order = np.argsort(vb, kind="stable")
    gb, vb, ok = np.minimum(gb, np.uint64(group[2]))[order], vb[order], ok[order]
    first = np.ones(len(vb), dtype=bool)
    first[1:] = (vb[1:] != vb[:-1]) | (gb[1:] != gb[:-1])
    return int((first & ok).sum())


@functools.lru_cache(maxsize=None)
def hand_rows():
    """Three rows by hand: the same u64 value inside the single bin, outside it, inside it."""
    vals, grps = value_column("u8")[0], group_column(("g18", 2))
    same = vals == np.uint64(HEAVY_U64[-1])
    inside, outside = np.flatnonzero(same & (grps == 0)), np.flatnonzero(same & (grps != 0))
    return np.array([inside[1], outside[0], inside[0]], dtype=np.int64)


def dist_cases():
    """Every value column meets every M (the group forms in turn) and every group form at 65, 4097 and 65 537; the hand-made case."""
    out, i = [], 0
    for vi, value in enumerate(VALUE_SPECS):
        for mi, m in enumerate(MS):
            out.append(dict(value=value, group=GROUP_SPECS[(5 * vi + mi) % len(GROUP_SPECS)], m=m, id_base=ID_BASES[(i + vi) % 2], keys=i % 3 != 2))
            i += 1
    for value in VALUE_SPECS:
        for group in GROUP_SPECS:
            for m in (65, 4097, 65_537):
                out.append(dict(value=value, group=group, m=m, id_base=ID_BASES[(i // 3) % 2], keys=i % 4 != 3))
                i += 1
    out.append(dict(value="u8", group=(("g18", 2), 0, 1), m=3, id_base=HIGH_BASE, keys=True, hand=True))
    return tuple(out)


DIST_CASES = dist_cases()


def case_rows(case):
    return hand_rows() if case.get("hand") else make_list(case["m"])


def is_defect_case(case):
    """u64 values, a group column, ONE group: rows outside the bin (the column holds 0 .. 17)."""
    return case["value"] == "u8" and case["group"][0] is not None and case["group"][1:] == (0, 1)


# ---- pqps_distinct_count / pqps_column_bounds: the case lists ---------------------------------------------------------------
COUNT_SHAPES = ((1, 1), (31, 1), (32, 3), (33, 3), (8192, 1), (8193, 5), (8193, 65_536), (1 << 25, 32))
COUNT_CASES = tuple(("random", s) for s in COUNT_SHAPES) + (("zeros", (8193, 5)), ("ones", (8193, 5)))
COUNT_BAD = ((0, 1), (1, 0), ((1 << 25) + 1, 32))
CAP_BITS = 1 << 30


def bitmap_words(n_values):
    return (n_values + 31) // 32


def make_bitmap(fill, n_values, n_groups):
    """[n_groups][W] u32 words, density about 0.5 (or 0, or 1), the bits past n_values in a row's last word clear."""
    nw = bitmap_words(n_values)
    if fill == "random":
        a = rng("bitmap", n_values, n_groups).integers(0, TOP32, (n_groups, nw), dtype=np.uint32, endpoint=True)
    else:
        a = np.full((n_groups, nw), TOP32 if fill == "ones" else 0, dtype=np.uint32)
    if n_values % 32:
        a[:, -1] &= np.uint32((1 << (n_values % 32)) - 1)
    return a


def popcount_rows(a):
    return np.bitwise_count(a).sum(axis=1, dtype=np.uint64)


BOUNDS_SIZES = (0, 1, 63, 64, 65, 1025, 70_001, 300_001)
BOUNDS_CONTENTS = ("random", "all_max", "all_min", "min@0", "min@last", "min@wave", "max@0", "max@last", "max@wave", "negative", "zero")
BOUNDS_CASES = ((0, "empty"),) + tuple((n, c) for n in BOUNDS_SIZES if n for c in BOUNDS_CONTENTS)


def bounds_column(n, content):
    """-> (the i32 column, (min, max) as the content says them)."""
    r = rng("bounds", n, content)
    if content == "empty":
        return np.zeros(0, dtype=np.int32), (I32_MAX, I32_MIN)
    if content == "random":
        a = r.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
        return a, (int(a.min()), int(a.max()))
    if content in ("all_max", "all_min", "zero"):
        v = {"all_max": I32_MAX, "all_min": I32_MIN, "zero": 0}[content]
        return np.full(n, v, dtype=np.int32), (v, v)
    if content == "negative":
        a = r.integers(I32_MIN, -1, n, endpoint=True).astype(np.int32)
        return a, (int(a.min()), int(a.max()))
    a = r.integers(-1000, 1000, n, endpoint=True).astype(np.int32)
    which, where = content.split("@")
    at = {"0": 0, "last": n - 1, "wave": (n - 1) // 64 * 64}[where]          # the first row of the last (partial) wave
    a[at] = I32_MIN if which == "min" else I32_MAX
    return a, (int(a.min()), int(a.max()))


# ---- the GPU side -----------------------------------------------------------------------------------------------------------
class Dev:
    """fused_driver's upload / download over this module's context, and what the cases share on the device."""
    put, get = fd.Gpu.put, fd.Gpu.get

    def __init__(self, ctx):
        self.ctx, self.L, self.held = ctx, pq.lib(), {}

    def hold(self, key, make):
        if key not in self.held:
            self.held[key] = self.put(make())
        return self.held[key]

    def column(self, key, make, width):
        return pq.Column(self.hold(key, make), width, 0)

    def ids(self, rows, key, id_base):
        return self.hold(("ids", key, id_base), lambda: (rows + id_base).astype(np.uint32))

    def drop(self):
        self.ctx.sync()
        for p in self.held.values():
            self.ctx.free(p)
        self.held = {}

    def filled(self, nbytes):
        """A buffer of 0xA5 bytes."""
        p = self.ctx.malloc(nbytes)
        self.ctx.memset(p, 0xA5, nbytes)
        return p


A5_32, A5_64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    c = pq.Context(0)
    yield c
    c.close()


@pytest.fixture()
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.drop()


def run_sort_case(dev, case, rows, raw, out_ids, out_keys, what):
    """One pqps_sort_list call; -> True if a word differs."""
    kind, m = case["kind"], len(rows)
    col = None if kind is None else dev.column(("key", kind, case["pattern"], len(raw)), lambda: typed(raw, kind), kind_width(kind))
    ids = dev.ids(rows, ("list", m, len(raw)), case["id_base"])
    dev.ctx.memset(out_ids, 0xA5, 4 * (m + GUARD))
    dev.ctx.memset(out_keys, 0xA5, 8 * (m + GUARD))
    pq.check(dev.L.pqps_sort_list(dev.ctx.h, C.byref(col) if col else None, 1 if kind == "i4" else 0, case["desc"], ids, m, case["id_base"],
                                  out_ids, out_keys if case["keys"] else None, None), what)
    want_rows, want_keys = sort_reference(raw, kind, case["desc"], rows)
    want = {"out_ids": np.concatenate([(want_rows + case["id_base"]).astype(np.uint32), np.full(GUARD, A5_32, dtype=np.uint32)]),
            "out_keys": np.concatenate([want_keys if case["keys"] else np.full(m, A5_64, dtype=np.uint64), np.full(GUARD, A5_64, dtype=np.uint64)])}
    return differs(what, {"out_ids": dev.get(out_ids, np.uint32, m + GUARD), "out_keys": dev.get(out_keys, np.uint64, m + GUARD)}, want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=str)
def test_sort_list_at_the_shim(dev, kind):
    cases = [c for c in SORT_CASES if c["kind"] == kind]
    out_ids, out_keys = dev.filled(4 * (max(MS) + GUARD)), dev.filled(8 * (max(MS) + GUARD))
    ran, bad = 0, []
    for case in cases:
        what = "sort_list " + " ".join(f"{k}={v}" for k, v in case.items())
        if run_sort_case(dev, case, make_list(case["m"]), key_raw(kind, case["pattern"]), out_ids, out_keys, what):
            bad.append(what)
        ran += 1
    dev.ctx.free(out_ids)
    dev.ctx.free(out_keys)
    assert ran == len(cases) > 0, "no case may be skipped"
    assert not bad, (len(bad), bad)


@pytest.mark.gpu
def test_sort_list_second_tile_of_a_workgroup(dev):
    """A list of more than 8 x CUs sort tiles: workgroups of the histogram and scatter kernels take a second tile."""
    m = long_list_length(dev.ctx.info()[1])
    case = dict(kind=4, desc=0, pattern="random", m=m, id_base=0, keys=True)
    out_ids, out_keys = dev.filled(4 * (m + GUARD)), dev.filled(8 * (m + GUARD))
    bad = run_sort_case(dev, case, make_list(m, m), key_raw(4, "random", m), out_ids, out_keys, f"sort_list long m={m}")
    dev.ctx.free(out_ids)
    dev.ctx.free(out_keys)
    assert not bad


def run_dist_case(dev, case, distinct, out_keys, what):
    """One pqps_distinct_sort call; -> the fields that differ."""
    value, group, rows = case["value"], case["group"], case_rows(case)
    gkey, g_base, n_groups = group
    m, wide = len(rows), value == "u8"
    col, v_base = value_column(value)
    vcol = dev.column(("value", value[:2] if value.startswith("i4") else value), lambda: col, col.dtype.itemsize)
    gcol = dev.column(("group", gkey), lambda: group_column(gkey), gkey[1]) if gkey else None
    ids = dev.ids(rows, ("hand",) if case.get("hand") else ("list", m), case["id_base"])
    key_words = (3 if wide else 2) * m                           # u32 words of out_keys: n u64 (+ n u32 groups)
    dev.ctx.memset(distinct, 0xA5, 8 * (n_groups + GUARD))
    dev.ctx.memset(out_keys, 0xA5, 4 * (key_words + GUARD))
    pq.check(dev.L.pqps_distinct_sort(dev.ctx.h, C.byref(vcol), v_base, C.byref(gcol) if gcol else None, g_base, n_groups, ids, m,
                                      case["id_base"], distinct, out_keys if case["keys"] else None, None), what)
    name = dev.L.pqps_last_kernel().decode()
    assert name == f"dist_unique_kernel<{'wide' if wide else 'narrow'}> (sort)", (what, name)
    want = dist_reference(value, group, rows)
    k_in = want["k_in"]
    words = dev.get(out_keys, np.uint32, key_words + GUARD)
    got = {"distinct": dev.get(distinct, np.uint64, n_groups + GUARD), "guard": words[key_words:]}
    exp = {"distinct": np.concatenate([want["distinct"], np.full(GUARD, A5_64, dtype=np.uint64)]), "guard": np.full(GUARD, A5_32, dtype=np.uint32)}
    if not case["keys"]:
        got["untouched"], exp["untouched"] = words[:key_words], np.full(key_words, A5_32, dtype=np.uint32)
    elif wide:
        vals, grps = words[:2 * m].view(np.uint64), words[2 * m:3 * m]
        got.update(vals=vals[:k_in], grps=grps[:k_in], outside=grps[k_in:] >= n_groups)
        exp.update(vals=want["vals"], grps=want["grps"], outside=np.ones(m - k_in, dtype=bool))
    else:
        keys = words[:2 * m].view(np.uint64)
        got.update(keys=keys[:k_in], outside=(keys[k_in:] >> np.uint64(32)) >= n_groups)
        exp.update(keys=want["keys"], outside=np.ones(m - k_in, dtype=bool))
    return [f for f in exp if differs(what, {f: got[f]}, {f: exp[f]})]


@pytest.mark.gpu
@pytest.mark.parametrize("value", VALUE_SPECS)
def test_distinct_sort_at_the_shim(dev, value):
    cases = [c for c in DIST_CASES if c["value"] == value]
    distinct, out_keys = dev.filled(8 * (65_536 + GUARD)), dev.filled(4 * (3 * max(MS) + GUARD))
    ran, bad = 0, []
    for case in cases:
        what = "distinct_sort " + " ".join(f"{k}={v}" for k, v in case.items())
        fields = run_dist_case(dev, case, distinct, out_keys, what)
        if fields:
            bad.append((what, fields))
        ran += 1
    dev.ctx.free(distinct)
    dev.ctx.free(out_keys)
    assert ran == len(cases) > 0, "no case may be skipped"
    assert not bad, (len(bad), bad)


@pytest.mark.gpu
def test_distinct_count_at_the_shim(dev):
    L, ctx = dev.L, dev.ctx
    ran, bad = 0, []
    for fill, (n_values, n_groups) in COUNT_CASES:
        what = f"distinct_count {fill} {n_values} x {n_groups}"
        a = make_bitmap(fill, n_values, n_groups)
        bitmap, distinct = dev.put(a), dev.filled(8 * (n_groups + GUARD))
        pq.check(L.pqps_distinct_count(ctx.h, bitmap, n_values, n_groups, distinct, None), what)
        want = np.concatenate([popcount_rows(a), np.full(GUARD, A5_64, dtype=np.uint64)])
        if differs(what, {"distinct": dev.get(distinct, np.uint64, n_groups + GUARD)}, {"distinct": want}):
            bad.append(what)
        ctx.free(bitmap)
        ctx.free(distinct)
        ran += 1
    bitmap, distinct = dev.put(make_bitmap("ones", 64, 2)), dev.filled(8 * (32 + GUARD))
    for n_values, n_groups in COUNT_BAD:
        if L.pqps_distinct_count(ctx.h, bitmap, n_values, n_groups, distinct, None) != PQPS_EINVAL:
            bad.append(f"distinct_count {n_values} x {n_groups}: no PQPS_EINVAL")
        ran += 1
    if not (dev.get(distinct, np.uint64, 32 + GUARD) == A5_64).all():
        bad.append("a refused call wrote")
    ctx.free(bitmap)
    ctx.free(distinct)
    assert ran == len(COUNT_CASES) + len(COUNT_BAD), "no case may be skipped"
    assert not bad, bad


@pytest.mark.gpu
def test_column_bounds_at_the_shim(dev):
    L, ctx = dev.L, dev.ctx
    out = dev.filled(4 * (2 + GUARD))
    ran, bad = 0, []
    for n, content in BOUNDS_CASES:
        what = f"column_bounds n={n} {content}"
        a, (lo, hi) = bounds_column(n, content)
        ptr = dev.put(a)
        col = pq.Column(ptr, 4, 0)
        ctx.memset(out, 0xA5, 4 * (2 + GUARD))
        pq.check(L.pqps_column_bounds(ctx.h, C.byref(col), n, out, None), what)
        want = np.concatenate([np.array([lo, hi], dtype=np.int32), np.full(GUARD, A5_32, dtype=np.uint32).view(np.int32)])
        if differs(what, {"bounds": dev.get(out, np.int32, 2 + GUARD)}, {"bounds": want}):
            bad.append(what)
        ctx.free(ptr)
        ran += 1
    ptr = dev.put(np.arange(64, dtype=np.uint16))
    ctx.memset(out, 0xA5, 4 * (2 + GUARD))
    if L.pqps_column_bounds(ctx.h, C.byref(pq.Column(ptr, 2, 0)), 64, out, None) != PQPS_EINVAL:
        bad.append("a 2-byte column: no PQPS_EINVAL")
    if not (dev.get(out, np.uint32, 2 + GUARD) == A5_32).all():
        bad.append("a refused call wrote")
    ctx.free(ptr)
    ctx.free(out)
    assert ran == len(BOUNDS_CASES), "no case may be skipped"
    assert not bad, bad


# ---- CPU: the references and the case lists ---------------------------------------------------------------------------------
def test_sort_references_against_a_loop():
    """The numpy references of the two sort forms == a row-by-row Python loop, 1025 entries, every column kind."""
    rows = make_list(SLOW_M)
    for kind in KINDS:
        for pattern in patterns_of(kind):
            for desc in (0, 1):
                raw = key_raw(kind, pattern)
                got, want = sort_reference(raw, kind, desc, rows), sort_slow(raw, kind, desc, rows)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kind, pattern, desc)
    for value in VALUE_SPECS:
        for group in GROUP_SPECS:
            got, want = dist_reference(value, group, rows), dist_slow(value, group, rows)
            assert got["k_in"] == want["k_in"] and np.array_equal(got["distinct"], want["distinct"]), (value, group)
            if value == "u8":
                pairs = list(zip(got["grps"].tolist(), got["vals"].tolist()))
            else:
                pairs = [(k >> 32, k & TOP32) for k in got["keys"].tolist()]
            assert pairs == want["pairs"], (value, group)
    a = make_bitmap("random", 8193, 5)
    assert popcount_rows(a).tolist() == [sum(bin(w).count("1") for w in row) for row in a.tolist()]


def test_lists_are_shuffled_with_repeats():
    for m in MS:
        rows = make_list(m)
        assert len(rows) == m and (m == 0 or 0 <= rows.min() and rows.max() < N_ROWS)
        assert m < 2 or not ascending(rows), m
        assert m < 63 or m - len(np.unique(rows)) >= m // 10, m  # every seventh entry twice (a few pairs lost to the cut)
    hand = hand_rows()
    assert len(set(hand.tolist())) == 3 and not ascending(hand)
    gb, vb, ok = dist_bins("u8", (("g18", 2), 0, 1), hand)
    assert ok.tolist() == [True, False, True] and len(set(vb.tolist())) == 1


def test_case_lists_cover_the_declared_edges():
    # pqps_sort_list: every kind x direction meets every M; every pattern meets 4097 and 65 537 in both directions; each byte of
    # the image as the only differing byte; both id_bases; out_keys given and NULL
    for kind in KINDS:
        mine = [c for c in SORT_CASES if c["kind"] == kind]
        for desc in (0, 1):
            assert {c["m"] for c in mine if c["desc"] == desc} == set(MS), (kind, desc)
            for pattern in patterns_of(kind):
                assert {c["m"] for c in mine if c["desc"] == desc and c["pattern"] == pattern} >= {4097, 65_537}, (kind, desc, pattern)
        assert {c["id_base"] for c in mine} == set(ID_BASES) and {c["keys"] for c in mine} == {True, False}
        if kind is not None:
            assert {p[1] for p in patterns_of(kind) if p[0] == "byte"} == set(range(kind_width(kind)))
            for p in patterns_of(kind):
                if p[0] == "byte":                               # ... and it is the only one
                    img = sort_image(kind, 0, key_raw(kind, p))
                    assert int(img.min() ^ img.max()) == 0xFF << (8 * p[1]) and len(np.unique(img)) == 256, (kind, p)
    assert {patterns_of(k)[0] for k in KINDS} == {"equal"} and all(len(np.unique(key_raw(k, "equal"))) == 1 for k in KINDS)
    assert set(typed(key_raw("i4", "minmax"), "i4").tolist()) == {I32_MIN, I32_MAX}
    assert all(set(typed(key_raw(k, "seven"), k).tolist()) == set(fd.SEVEN[k]) for k in KINDS if k is not None)
    assert sum(len([c for c in SORT_CASES if c["kind"] == k]) for k in KINDS) == len(SORT_CASES)
    assert {c["m"] for c in SORT_CASES if c["id_base"] == 0} == {c["m"] for c in SORT_CASES if c["id_base"] == HIGH_BASE} == set(MS)
    assert {63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 16 * SORT_TILE, 16 * SORT_TILE + 1} <= set(MS)
    assert 256 * 16 == 4096 < 256 * 17                           # the histogram of 17 tiles takes a second scan block
    assert long_list_length(256) == 8_392_705 and (long_list_length(256) + SORT_TILE - 1) // SORT_TILE > 8 * 256
    # pqps_distinct_sort: every value column meets every M and every group form; both sides of one group with rows outside
    assert sum(len([c for c in DIST_CASES if c["value"] == v]) for v in VALUE_SPECS) == len(DIST_CASES)
    for value in VALUE_SPECS:
        mine = [c for c in DIST_CASES if c["value"] == value]
        assert {c["m"] for c in mine} >= set(MS) and {c["group"] for c in mine} == set(GROUP_SPECS), value
        assert {c["id_base"] for c in mine} == set(ID_BASES) and {c["keys"] for c in mine} == {True, False}
    assert {c["group"] for c in DIST_CASES if c["m"] == 0} >= {(None, 0, 1), (("g16", 2), 0, 65_536)}      # n = 0 zeroes 1 and 65 536 words
    assert {g[0][1] for g in GROUP_SPECS if g[0] and g[1:] == (0, 1)} == {g[0][1] for g in GROUP_SPECS if g[1:] == (2, 13)} == {1, 2, 4}
    rows = make_list(65_537)
    for group in GROUP_SPECS[1:]:
        gb, _, ok = dist_bins("u1", group, rows)
        below = (gb >= 1 << 31).any()                            # a group under the base wraps to the top of u32
        above = ((gb >= group[2]) & (gb < 1 << 31)).any()
        want = {(0, 18): (False, False), (2, 13): (True, True), (0, 1): (False, True), (0, 65_536): (False, False), (18, 4): (True, False)}
        assert (below, above) == want[group[1:]], group
        assert ok.any() != (group[1:] == (18, 4)) and ok.all() == (group[1:] in ((0, 18), (0, 65_536)))
    col, base = value_column("i4min")
    assert base == I32_MIN & TOP32 and value_column("i4min5")[1] == base + 5 and (col[rows] < I32_MIN + 5).any()
    u8 = value_column("u8")[0]
    assert all((u8 == np.uint64(e)).mean() > 0.05 for e in fd.U64_EXTREMES) and len(np.unique(u8)) > N_ROWS // 4
    # the wide one-group cases: at every declared M, and each of them tells the value-order walk from the answer
    defect = [c for c in DIST_CASES if is_defect_case(c)]
    assert {c["m"] for c in defect} >= set(DEFECT_MS) and {c["group"][0][1] for c in defect} == {1, 2, 4}
    for c in defect:
        if c["m"] in DEFECT_MS:
            want = int(dist_reference(c["value"], c["group"], case_rows(c))["distinct"][0])
            assert value_order_count(c["value"], c["group"], case_rows(c)) > want > 0, c
    hand = [c for c in DIST_CASES if c.get("hand")]
    assert len(hand) == 1 and value_order_count("u8", hand[0]["group"], hand_rows()) == 2
    assert dist_reference("u8", hand[0]["group"], hand_rows())["distinct"].tolist() == [1]
    # pqps_distinct_count: both sides of 256 words (a second segment) and of the cap
    shapes = [s for _, s in COUNT_CASES]
    assert {bitmap_words(v) for v, _ in shapes} >= {1, 2, 256, 257} and {f for f, _ in COUNT_CASES} == {"random", "zeros", "ones"}
    assert max(bitmap_words(v) * 32 * g for v, g in shapes) == CAP_BITS and (8193, 65_536) in shapes
    assert any(v and g and bitmap_words(v) * 32 * g > CAP_BITS for v, g in COUNT_BAD) and {(0, 1), (1, 0)} <= set(COUNT_BAD)
    a = make_bitmap("ones", 33, 3)
    assert popcount_rows(a).tolist() == [33] * 3 and 0.45 < popcount_rows(make_bitmap("random", 8192, 1))[0] / 8192 < 0.55
    # pqps_column_bounds: every size with every content; the extremes where the contents say
    assert {n for n, _ in BOUNDS_CASES} == set(BOUNDS_SIZES) and all({c for k, c in BOUNDS_CASES if k == n} == set(BOUNDS_CONTENTS) for n in BOUNDS_SIZES if n)
    for n, content in BOUNDS_CASES:
        a, (lo, hi) = bounds_column(n, content)
        assert len(a) == n and (n == 0 or (lo, hi) == (min(a.tolist()), max(a.tolist())))
        if "@" in content:
            at = {"0": 0, "last": n - 1, "wave": (n - 1) // 64 * 64}[content.split("@")[1]]
            v = I32_MIN if content.startswith("min") else I32_MAX
            assert a[at] == v and (a == v).sum() == 1 and v in (lo, hi), (n, content)
            assert content.endswith("@0") or n - at <= 64, (n, content)
    assert bounds_column(0, "empty")[1] == (I32_MAX, I32_MIN) and bounds_column(65, "negative")[1][1] < 0 and bounds_column(65, "zero")[1] == (0, 0)
