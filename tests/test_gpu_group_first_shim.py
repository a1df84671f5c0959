"""pqps_filter_group_first / pqps_group_first_list AT THE SHIM: arrays planted with numpy, the raw device words compared
exactly with tests/group_first_model.py.  The predicate columns, their four WHEREs (all / sparse / dense / nothing), the
matching padding past n and the ID lists (shuffled, every seventh entry twice) are tests/fused_driver.py's; key and group
columns are made here, with padding that would change every answer (the smallest and the largest key, in-range bins).
Sizes: a partial last step, one workgroup, several workgroups.  Bins: no group column, both sides of the LDS / GLOBAL switch."""
import itertools

import numpy as np
import pytest

import fused_driver as fd
import group_first_model as m

pq = m.q.pq
SIZES = (1, 1023, 1024, 1025, 4097, 65537)
BINS = (1, 2, 16, 8192, 8193, 65536)                          # 1: no group column; 8192 | 8193: LDS | GLOBAL
KINDS = (1, 2, 4, fd.BIT, "i4", None, 8)                      # key column: width, bit plane, signed i32, NULL, u64
I32_POOL = np.array([fd.I32_MIN, fd.I32_MIN + 1, -1, 0, 1, fd.I32_MAX - 1, fd.I32_MAX], np.int64)
U64_POOL = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, fd.U64 - 1, fd.U64], np.uint64)
PATHS = {1: "FIRST_ONE", 2: "FIRST_LDS", 16: "FIRST_LDS", 8192: "FIRST_LDS", 8193: "FIRST_GLOBAL", 65536: "FIRST_GLOBAL"}


def key_column(inp, kind, flavour="random"):
    """-> (Col or None, keys as the model orders them, KIND_* of the word).  The padding alternates the extremes."""
    n, pad = inp.n, inp.pad
    rng = inp.rng(("key", kind, flavour))
    if kind is None:
        return None, np.zeros(n, np.int64), m.KIND_DICT
    if kind == "i4":
        full = rng.choice(I32_POOL, pad) if flavour == "random" else np.full(pad, -7, np.int64)
        full[n:] = np.where(np.arange(pad - n) % 2 == 0, fd.I32_MIN, fd.I32_MAX)
        col = fd.Col(inp.gpu, full.astype(np.int32), 4, n)
        return col, full[:n], m.KIND_I32
    if kind == 8:
        full = rng.choice(U64_POOL, pad) if flavour == "random" else np.full(pad, 1 << 63, np.uint64)
        full[n:] = np.where(np.arange(pad - n) % 2 == 0, np.uint64(0), np.uint64(fd.U64))
        return fd.Col(inp.gpu, full, 8, n), full[:n], m.KIND_U64
    top = fd.width_top(kind)
    pool = np.array(sorted({0, 1, top // 2, top - 1, top}), np.uint64)
    full = rng.choice(pool, pad) if flavour == "random" else np.full(pad, min(3, top), np.uint64)
    full[n:] = np.where(np.arange(pad - n) % 2 == 0, np.uint64(0), np.uint64(top))
    dtype = np.uint8 if kind == fd.BIT else fd.DT[kind]
    return fd.Col(inp.gpu, full.astype(dtype), kind, n), full[:n].astype(np.int64), m.KIND_BOOL if kind == fd.BIT else m.KIND_DICT


def group_column(inp, n_bins, width, flavour="random"):
    """-> (Col or None, bins of the real rows (int64; >= n_bins: left out), bin_base).  Values reach past the bins where
    the width has room; the padding sits in bins 0 and n_bins - 1."""
    n, pad = inp.n, inp.pad
    if n_bins == 1 and width is None:
        return None, None, 0
    rng = inp.rng(("group", n_bins, width, flavour))
    top = fd.width_top(width)
    base = 3 if top >= n_bins + 3 else 0
    room = min(top - base + 1, n_bins + n_bins // 4 + 2)          # values base .. base + room - 1 fit the width
    bins = rng.integers(0, room, pad) if flavour == "random" else np.full(pad, min(n_bins - 1, 5), np.int64)
    bins[n:] = np.where(np.arange(pad - n) % 2 == 0, 0, n_bins - 1)
    if flavour == "random" and base and n > 8:
        bins[rng.integers(0, n, 4)] = -2                         # below the base: bin 2^32 - 2, left out
    values = (bins + base) & fd.TOP32
    dtype = np.uint8 if width == fd.BIT else fd.DT[width]
    col = fd.Col(inp.gpu, values.astype(dtype), width, n)
    real = bins[:n].astype(np.int64)
    real[real < 0] += 1 << 32
    return col, real, base


def group_width(n_bins, turn, plane_ok):
    if n_bins == 1:
        return None
    if n_bins == 2:
        return (fd.BIT if plane_ok else 1, 1, 2)[turn % 3]
    if n_bins == 16:
        return (1, 2, 4)[turn % 3]
    return 4 if n_bins == 65536 or turn % 2 else 2


class Harness:
    def __init__(self, n):
        self.gpu = fd.Gpu()
        self.inp = fd.Inputs(n, self.gpu)
        self.best = self.gpu.ctx.malloc(65536 * 8)

    def close(self):
        self.gpu.ctx.sync()
        self.gpu.ctx.free(self.best)
        self.inp.free()
        self.gpu.close()

    def expected(self, kkind, desc, rows, keys, bins, n_bins, base):
        keys = keys[rows]
        bins = None if bins is None else bins[rows]
        if kkind == m.KIND_U64:
            return m.expected_wide(n_bins, desc, rows, keys, bins, base)
        return m.expected_words(n_bins, kkind, desc, rows, keys, bins, base), None

    def compare(self, what, kkind, want, want_best, n_bins):
        gpu = self.gpu
        got = gpu.get(gpu.out, np.uint64, n_bins)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (what, "out", bad[:5].tolist(), [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[bad[:5]]])
        if kkind == m.KIND_U64:
            best = gpu.get(self.best, np.uint64, n_bins)
            live = want != m.EMPTY                                    # best means something only where out has a row
            assert np.array_equal(best[live], want_best[live]), (what, "best")

    def fused(self, pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, row_base, path=None):
        gpu, inp = self.gpu, self.inp
        what = (inp.n, pname, kkind, None if kcol is None else kcol.width, None if gcol is None else gcol.width, n_bins, desc, row_base)
        cols, n_cols, pred = inp.bound(pname)
        pq.filter_group_first(gpu.ctx, cols, n_cols, inp.n, pred, None if kcol is None else kcol.c, kkind == m.KIND_I32, desc, row_base,
                              None if gcol is None else gcol.c, base, n_bins, gpu.out, self.best if kkind == m.KIND_U64 else None,
                              gpu.words)
        mode = "FIRST_WIDE_B" if kkind == m.KIND_U64 else "FIRST_NARROW"
        gpu.fused(f"first_scan_kernel<{path or PATHS[n_bins]}, {mode}, NT=?>", what)
        rows = inp.sel[pname]
        want, want_best = self.expected(kkind, desc, rows, keys, bins, n_bins, row_base)
        self.compare(what, kkind, want, want_best, n_bins)
        assert int(gpu.get(gpu.words, np.uint64, 1)[0]) == len(rows), (what, "count")
        if pname == "nothing":
            assert (want == m.EMPTY).all()

    def listed(self, pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, id_base, cap="equal", n_rows=None):
        gpu, inp = self.gpu, self.inp
        rows, _, ids_dev, count_dev = inp.id_list(pname, id_base)
        capacity = {"below": len(rows) * 2 // 3, "equal": len(rows), "above": len(rows) + 100}[cap]
        what = ("list", inp.n, pname, kkind, n_bins, desc, id_base, cap, n_rows)
        pq.group_first_list(gpu.ctx, None if kcol is None else kcol.c, kkind == m.KIND_I32, desc, None if gcol is None else gcol.c, base,
                            n_bins, inp.n if n_rows is None else n_rows, ids_dev, count_dev, capacity, id_base, gpu.out,
                            self.best if kkind == m.KIND_U64 else None)
        used = rows[:min(capacity, len(rows))] if n_rows is None else rows[:0]
        want, want_best = self.expected(kkind, desc, used, keys, bins, n_bins, id_base)
        self.compare(what, kkind, want, want_best, n_bins)


@pytest.fixture(scope="module", params=SIZES)
def harness(request):
    h = Harness(request.param)
    yield h
    h.close()


@pytest.mark.gpu
def test_every_bin_count_key_and_direction(harness):
    """Fused scan and list form over bins x key kinds x directions; the WHERE and the bases take turns."""
    h, inp = harness, harness.inp
    for turn, (n_bins, kind, desc) in enumerate(itertools.product(BINS, KINDS, (False, True))):
        pname = ("all", "sparse", "dense")[turn % 3]
        base_row = (0, fd.HIGH_BASE)[(turn // 3) % 2]
        kcol, keys, kkind = key_cache(inp, kind)
        gcol, bins, base = group_cache(inp, n_bins, group_width(n_bins, turn, True))
        h.fused(pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, base_row)
        if kind != fd.BIT:                                       # the list form gathers bytes: no bit planes
            gcol, bins, base = group_cache(inp, n_bins, group_width(n_bins, turn, False))
            h.listed(pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, base_row, cap=fd.LIST_CAPS[turn % 3])


def key_cache(inp, kind, flavour="random"):
    key = ("gf_key", kind, flavour)
    if key not in inp.memo:
        inp.memo[key] = key_column(inp, kind, flavour)
        if inp.memo[key][0] is not None:
            inp.cache[key] = inp.memo[key][0]                    # freed with the inputs
    return inp.memo[key]


def group_cache(inp, n_bins, width, flavour="random"):
    key = ("gf_group", n_bins, width, flavour)
    if key not in inp.memo:
        inp.memo[key] = group_column(inp, n_bins, width, flavour)
        if inp.memo[key][0] is not None:
            inp.cache[key] = inp.memo[key][0]
    return inp.memo[key]


@pytest.mark.gpu
def test_no_match_and_empty_list(harness):
    """A WHERE that matches nothing: every word all ones, count 0.  n_rows = 0 in the list form launches nothing."""
    h, inp = harness, harness.inp
    for n_bins, kind in itertools.product(BINS, (4, 8)):
        kcol, keys, kkind = key_cache(inp, kind)
        gcol, bins, base = group_cache(inp, n_bins, group_width(n_bins, 0, False))
        for desc in (False, True):
            h.fused("nothing", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0)
            h.listed("nothing", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0)
            h.listed("all", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, n_rows=0)


@pytest.mark.gpu
def test_every_key_equal_lowest_row_wins(harness):
    """Ties go to the lowest row number in both directions, for every key form."""
    h, inp = harness, harness.inp
    for n_bins, kind, desc in itertools.product((1, 16, 8193), KINDS, (False, True)):
        kcol, keys, kkind = key_cache(inp, kind, "equal")
        gcol, bins, base = group_cache(inp, n_bins, group_width(n_bins, 1, False))
        h.fused("dense", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 7)
        rows = inp.sel["dense"]
        if kkind != m.KIND_U64 and n_bins == 1 and len(rows):
            word = int(h.gpu.get(h.gpu.out, np.uint64, 1)[0])
            assert pq.first_key_decode(kkind, desc, word)[1] == int(rows[0]) + 7
        if kind != fd.BIT:
            h.listed("dense", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 7)


@pytest.mark.gpu
def test_every_row_in_one_bin_of_many(harness):
    """Maximum contention: one LDS word, one global word."""
    h, inp = harness, harness.inp
    for n_bins, kind, desc in itertools.product((8192, 65536), (2, "i4", 8), (False, True)):
        kcol, keys, kkind = key_cache(inp, kind)
        gcol, bins, base = group_cache(inp, n_bins, 4, "one")
        h.fused("all", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0)
        h.listed("all", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, cap="above")


@pytest.mark.gpu
def test_refused_arguments(harness):
    h, inp = harness, harness.inp
    gpu = h.gpu
    cols, n_cols, pred = inp.bound("all")
    kcol, _, _ = key_cache(inp, 4)
    wide, _, _ = key_cache(inp, 8)
    gcol, _, _ = group_cache(inp, 16, 1)
    L = pq.lib()

    def fused(key, group, n_bins, best, row_base=0):
        return L.pqps_filter_group_first(gpu.ctx.h, cols, n_cols, inp.n, pred, key.ref() if key else None, 0, 0, row_base,
                                         group.ref() if group else None, 0, n_bins, gpu.out, best, gpu.words, None)

    assert fused(kcol, None, 2, None) != 0                       # no group column: one bin
    assert fused(kcol, gcol, 0, None) != 0
    assert fused(kcol, gcol, 65537, None) != 0
    assert fused(wide, gcol, 16, None) != 0                      # an 8-byte key needs `best`
    assert fused(kcol, gcol, 16, None, row_base=0xFFFFFFFF - inp.n) != 0
    assert fused(kcol, gcol, 16, None) == 0
    gpu.ctx.sync()
