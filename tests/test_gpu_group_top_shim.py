"""pqps_filter_group_wide, pqps_group_wide_list, pqps_bins_compact and pqps_group_sort called at the shim and compared word for
word with numpy over the uploaded arrays (the buffers, predicates and padding rule of tests/fused_driver.py: columns are
allocated at a multiple of 4096 rows and the padding past n MATCHES the predicate and carries an in-range bin, so a wrong trim
of the last step shows).

  * n_rows 1, 1023, 1024, 1025 and 200 000; n_bins 1, 65 536, 65 537, T - 1, T, T + 1, 3 T + 5 for the compaction tile T
  * group columns 1, 2 and 4 bytes wide, each with a non-zero base: rows below bin_base and at or past bin_base + n_bins are
    left out (the 4-byte column is signed, its base wraps in 32-bit arithmetic)
  * occupancy: all bins, none, only bin 0, only the last bin, every other bin
  * skew: one bin with 90 % of 200 000 rows and the rest over 100 000 other bins (the slot that stays hot), with the front on
    and off; more busy bins than the front has slots (every slot claimed, the rest overflow to the global atomics); bins that
    share a slot
  * values: negative i32, INT_MIN, INT_MAX, u64 at and above 2^63, a u64 sum that wraps modulo 2^64
  * the list form: ids outside the table are skipped, *count_dev below and above the capacity, an id_base at the top of u32
  * pqps_group_sort with n_bins = 2^32 and both extreme bins; its runs equal pqps_bins_compact's whenever both apply
"""
import ctypes as C

import numpy as np
import pytest

import fused_driver as fd
import qpelib as q

pq = q.pq
T = pq.COMPACT_TILE
M64 = (1 << 64) - 1
SIGN = np.uint64(1 << 63)
SIZES = (1, 1023, 1024, 1025, 200_000)
BINS = (1, 65536, 65537, T - 1, T, T + 1, 3 * T + 5)
VALS = (None, "i32", "u64")
BASES = {1: 100, 2: 1000, 4: (-45) & 0xFFFFFFFF}             # the 4-byte column holds signed values from -50 up
EINVAL = -1


@pytest.fixture(scope="module")
def gpu():
    g = fd.Gpu()
    yield g
    g.close()


def rng_for(*key):
    return np.random.default_rng([0x70B5, *[int(k) & 0xFFFFFFFF for k in key]])


def value_column(kind, n, pad, seed):
    """Padded values: the extremes among random ones; the padding holds what would change every aggregate."""
    rng = rng_for(seed, n, 1 if kind == "i32" else 2)
    if kind == "i32":
        v = rng.integers(-(1 << 31), 1 << 31, pad, dtype=np.int64).astype(np.int32)
        ext = np.array(fd.I32_EXTREMES + (-1000, -7), dtype=np.int32)
        pick = rng.random(pad) < 0.3
        v[pick] = ext[rng.integers(0, len(ext), int(pick.sum()))]
        v[n:] = -(1 << 31)
        return v
    v = rng.integers(0, 1 << 64, pad, dtype=np.uint64)
    ext = np.array(fd.U64_EXTREMES + ((1 << 63) + 12345,), dtype=np.uint64)
    pick = rng.random(pad) < 0.5
    v[pick] = ext[rng.integers(0, len(ext), int(pick.sum()))]
    v[n:] = M64
    return v


class Table:
    """One table size: the predicate column p (p == 1 matches), both value columns, group columns on demand."""

    def __init__(self, gpu, n, mask=None, seed=0):
        self.gpu, self.n, self.pad = gpu, n, fd.pad_rows(n)
        self.mask = (rng_for(seed, n, 3).random(n) < 0.6) if mask is None else np.asarray(mask, dtype=bool)
        p = np.ones(self.pad, dtype=np.uint32)
        p[:n] = self.mask
        self.rows = np.flatnonzero(self.mask)
        self.p = fd.Col(gpu, p, 4, n)
        self.cols = pq.column_array([(self.p.ptr, 4)])
        self.pred = fd.make_pred(*fd.PREDS["sparse"])            # p == 1
        self.pred_all = fd.make_pred(*fd.PREDS["all"])
        self.values = {k: fd.Col(gpu, value_column(k, n, self.pad, seed), 8 if k == "u64" else 4, n) for k in ("i32", "u64")}
        self.made = []

    def group(self, real, width, pad_value):
        dt = np.int32 if width == 4 else fd.DT[width]
        full = np.full(self.pad, pad_value, dtype=np.int64)
        full[:self.n] = real
        col = fd.Col(self.gpu, full.astype(dt), width, self.n)
        self.made.append(col)
        return col

    def free(self):
        self.gpu.ctx.sync()
        for c in [self.p, *self.values.values(), *self.made]:
            self.gpu.ctx.free(c.ptr)


def dense_reference(g, base, n_bins, v, rows):
    """The dense output over `rows` (repeats count): n_bins u32 counts, or the [4][n_bins] u64 fields."""
    rows = np.asarray(rows, dtype=np.int64)
    b = (g.u[rows] - np.uint32(base)).astype(np.uint64)          # g.u: the column as u32, so the subtraction wraps
    ok = b < n_bins
    b = b[ok].astype(np.int64)
    if v is None:
        return np.bincount(b, minlength=n_bins).astype(np.uint32)
    wide, img = fd.agg_wide_image(v, rows)
    out = np.zeros(4 * n_bins, dtype=np.uint64)
    out[2 * n_bins:3 * n_bins] = M64
    out[:n_bins] = np.bincount(b, minlength=n_bins)
    np.add.at(out[n_bins:2 * n_bins], b, wide[ok])
    np.minimum.at(out[2 * n_bins:3 * n_bins], b, img[ok])
    np.maximum.at(out[3 * n_bins:], b, img[ok])
    return out


def runs_reference(dense, n_bins, valued):
    """The run format from dense bins: keys, counts [, sums, min images, max images], concatenated."""
    nz = np.flatnonzero(dense[:n_bins])
    fields = [nz.astype(np.uint64)] + [dense[f * n_bins:(f + 1) * n_bins][nz].astype(np.uint64) for f in range(4 if valued else 1)]
    return np.concatenate(fields)


def same(what, got, want):
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.flatnonzero(got != want) if got.shape == want.shape else []
        at = int(bad[0]) if len(bad) else -1
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {at}: got {got[at] if at >= 0 else got.shape}, want {want[at] if at >= 0 else want.shape}")


def fetch_runs(gpu, runs_dev, n_runs, valued):
    words = n_runs.value * (5 if valued else 2)
    assert bool(runs_dev.value) == bool(words)
    got = gpu.get(runs_dev, np.uint64, words)
    if runs_dev.value:
        gpu.ctx.free(runs_dev)
    return got


def check_case(gpu, t, g, width, base, n_bins, val, what, pred="sparse", lists=True):
    """All four calls on one shape: the fused scan, its compaction, the list form over a list with repeats and strangers, and
    the sort form over the same list, whose runs equal the compaction's."""
    L, ctx = gpu.L, gpu.ctx
    v = t.values[val] if val else None
    vref = v.ref() if v else None
    words, dt = (n_bins, np.uint32) if val is None else (4 * n_bins, np.uint64)
    nbytes = words * np.dtype(dt).itemsize
    out = ctx.malloc(nbytes + 64)
    rows = t.rows if pred == "sparse" else np.arange(t.n)
    # fused scan
    ctx.memset(out, 0xA5, nbytes)                                # the call initialises its output
    pq.check(L.pqps_filter_group_wide(ctx.h, t.cols, 1 if pred == "sparse" else 0, t.n, C.byref(t.pred if pred == "sparse" else t.pred_all),
                                      vref, g.ref(), base, n_bins, out, None), what)
    name = L.pqps_last_kernel().decode()
    assert "_WIDE" in name and ("i32" in name or "u64" in name) == (val is not None), name
    want = dense_reference(g, base, n_bins, v, rows)
    same(what + " scan", gpu.get(out, dt, words), want)
    # compaction
    runs_dev, n_runs = C.c_void_p(), C.c_uint64(12345)
    pq.check(L.pqps_bins_compact(ctx.h, out, n_bins, int(val is not None), C.byref(runs_dev), C.byref(n_runs), None), what)
    want_runs = runs_reference(want, n_bins, val is not None)
    assert n_runs.value * (5 if val else 2) == len(want_runs), (what, n_runs.value)
    same(what + " compact", fetch_runs(gpu, runs_dev, n_runs, val is not None), want_runs)
    if lists:
        # the list: the matching rows, every seventh twice, shuffled, then two ids outside the table and one more real row
        base_id = fd.HIGH_BASE
        listed = rng_for(t.n, n_bins, 7).permutation(np.concatenate([rows, rows[::7]]))
        listed = np.concatenate([listed, [t.n, t.n + 3], listed[:1]]).astype(np.int64)
        ids = gpu.put(((listed + base_id) & 0xFFFFFFFF).astype(np.uint32))
        count = gpu.put(np.array([len(listed)], dtype=np.uint64))
        for cap in (len(listed) // 2, len(listed) + 5):         # *count_dev above and below the capacity
            ctx.memset(out, 0xA5, nbytes)
            pq.check(L.pqps_group_wide_list(ctx.h, vref, g.ref(), t.n, ids, count, cap, base_id & 0xFFFFFFFF, base, n_bins, out, None), what)
            part = listed[:cap]
            want = dense_reference(g, base, n_bins, v, part[part < t.n])
            same(f"{what} list cap={cap}", gpu.get(out, dt, words), want)
        # (out now holds the bins of the whole list) the sort form over the same list: the same runs as the compaction
        pq.check(L.pqps_bins_compact(ctx.h, out, n_bins, int(val is not None), C.byref(runs_dev), C.byref(n_runs), None), what)
        compact = fetch_runs(gpu, runs_dev, n_runs, val is not None)
        same(what + " list compact", compact, runs_reference(want, n_bins, val is not None))
        pq.check(L.pqps_group_sort(ctx.h, g.ref(), base, n_bins, vref, t.n, ids, len(listed), base_id & 0xFFFFFFFF,
                                   C.byref(runs_dev), C.byref(n_runs), None), what)
        same(what + " sort == compact", fetch_runs(gpu, runs_dev, n_runs, val is not None), compact)
        ctx.free(ids)
        ctx.free(count)
    ctx.sync()
    ctx.free(out)


def spread(n, width, base, n_bins, seed):
    """Values around [base, base + n_bins): most inside, some just below the base and some at or past the end (as far as the
    width reaches)."""
    rng = rng_for(seed, n, width, n_bins)
    lo = -50 if width == 4 else 0
    signed_base = base - (1 << 32) if width == 4 and base >= 1 << 31 else base
    top = (1 << 31) - 1 if width == 4 else (1 << (8 * width)) - 1
    a = signed_base + rng.integers(-60, n_bins + 60, n)
    edge = np.array([signed_base - 1, signed_base, signed_base + n_bins - 1, signed_base + n_bins])
    a[: min(n, 4)] = edge[: min(n, 4)]
    return np.clip(a, lo, top)


@pytest.mark.gpu
@pytest.mark.parametrize("val", VALS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_bins_and_widths(gpu, n, val):
    t = Table(gpu, n)
    for k, n_bins in enumerate(BINS):
        width = (1, 2, 4)[(k + SIZES.index(n)) % 3]
        base = BASES[width]
        g = t.group(spread(n, width, base, n_bins, k), width, base if width != 4 else -45)
        check_case(gpu, t, g, width, base, n_bins, val, f"n={n} n_bins={n_bins} width={width} val={val}")
    t.free()


OCCUPANCY = ("all", "none", "none_in_range", "bin0", "last", "every_other")


@pytest.mark.gpu
@pytest.mark.parametrize("val", (None, "i32"))
@pytest.mark.parametrize("occupancy", OCCUPANCY)
def test_occupancy(gpu, occupancy, val):
    n = 140_000
    t = Table(gpu, n, mask=np.zeros(n, bool) if occupancy == "none" else np.ones(n, bool))
    for n_bins in (65537, 3 * T + 5):
        k = np.arange(n) % n_bins
        real = {"all": k, "none": k, "none_in_range": n_bins + (k % 1000), "bin0": np.zeros(n, np.int64),
                "last": np.full(n, n_bins - 1), "every_other": (k // 2) * 2}[occupancy]
        g = t.group(real, 4, 0)
        check_case(gpu, t, g, 4, 0, n_bins, val, f"occupancy={occupancy} n_bins={n_bins} val={val}", pred="all" if occupancy != "none" else "sparse")
    t.free()


def skew_column(kind, n):
    """-> (per-row bins, n_bins)."""
    rng = rng_for(n, len(kind))
    if kind == "hot":                                            # one bin owns 90 % of the rows, 100 000 others share the rest
        b = rng.integers(0, 100_000, n)
        b[b >= 77] += 1
        b[rng.random(n) < 0.9] = 77
        return b, 100_001
    if kind == "busy":                                           # three times as many busy bins as the count front has slots
        return rng.integers(0, 3 * pq.WIDE_COUNT_SLOTS, n), 70_000
    # bins that share a slot of the count front and of the value front: 5, 5 + slots, 5 + 2 * slots, ...
    strides = np.array([0, pq.WIDE_VALUE_SLOTS, pq.WIDE_COUNT_SLOTS, 2 * pq.WIDE_COUNT_SLOTS, 5 * pq.WIDE_COUNT_SLOTS])
    return 5 + strides[rng.integers(0, len(strides), n)], 70_000


@pytest.mark.gpu
@pytest.mark.parametrize("val", VALS)
@pytest.mark.parametrize("kind", ("hot", "busy", "shared"))
def test_skew_and_the_front(gpu, kind, val):
    n = 200_000
    b, n_bins = skew_column(kind, n)
    t = Table(gpu, n, mask=np.ones(n, bool))
    g = t.group(b, 4, 0)
    if val == "u64":                                             # the hot bin's exact sum passes 2^64: the device sum wraps
        rows = np.flatnonzero(b == b[0])
        assert sum(int(x) for x in t.values["u64"].real[rows]) > M64
    try:
        for front in (-1, 0):
            gpu.ctx.set_option("wide_front", front)
            check_case(gpu, t, g, 4, 0, n_bins, val, f"skew={kind} val={val} front={front}", pred="all", lists=front < 0 or kind == "hot")
    finally:
        gpu.ctx.set_option("wide_front", -1)
    t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("val", VALS)
def test_group_sort_over_the_whole_u32_domain(gpu, val):
    """n_bins = 2^32: every u32 value is a bin, 0 and 0xFFFFFFFF included; and one bin fewer leaves the last value out."""
    n = 5000
    t = Table(gpu, n, mask=np.ones(n, bool))
    rng = rng_for(n, 32)
    real = rng.integers(0, 1 << 32, n)
    real[:6] = (0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFE, 1)
    real[6:3000] = real[rng.integers(0, 6, 2994)]                 # long runs of the extremes
    g = fd.Col(gpu, np.concatenate([real, np.zeros(t.pad - n, np.int64)]).astype(np.uint32), 4, n)
    t.made.append(g)
    v = t.values[val] if val else None
    listed = np.concatenate([rng.permutation(n), [n + 1], np.arange(0, n, 3)]).astype(np.int64)
    ids = gpu.put(listed.astype(np.uint32))
    rows = listed[listed < n]
    for base, n_bins in ((0, 1 << 32), (0, (1 << 32) - 1), (1, 1 << 32), (0xFFFFFFFE, 3)):
        runs_dev, n_runs = C.c_void_p(), C.c_uint64()
        pq.check(gpu.L.pqps_group_sort(gpu.ctx.h, g.ref(), base, n_bins, v.ref() if v else None, n, ids, len(listed), 0,
                                       C.byref(runs_dev), C.byref(n_runs), None), "sort")
        bins = (g.u[rows] - np.uint32(base)).astype(np.uint64)
        ok = bins < n_bins
        keys, inv, counts = np.unique(bins[ok], return_inverse=True, return_counts=True)
        fields = [keys, counts.astype(np.uint64)]
        if v:
            wide, img = fd.agg_wide_image(v, rows)
            s, lo, hi = np.zeros(len(keys), np.uint64), np.full(len(keys), M64, np.uint64), np.zeros(len(keys), np.uint64)
            inv = np.asarray(inv).reshape(-1)
            np.add.at(s, inv, wide[ok])
            np.minimum.at(lo, inv, img[ok])
            np.maximum.at(hi, inv, img[ok])
            fields += [s, lo, hi]
        if n_bins == 1 << 32 and base == 0:
            assert keys[0] == 0 and keys[-1] == 0xFFFFFFFF
        same(f"sort base={base} n_bins={n_bins} val={val}", fetch_runs(gpu, runs_dev, n_runs, v is not None), np.concatenate(fields))
    gpu.ctx.free(ids)
    t.free()


@pytest.mark.gpu
def test_bad_arguments_and_the_old_limit(gpu):
    L, ctx = gpu.L, gpu.ctx
    n = 1025
    t = Table(gpu, n)
    g = t.group(np.arange(n), 4, 0)
    out = ctx.malloc(1 << 20)
    ids, count = gpu.put(np.arange(n, dtype=np.uint32)), gpu.put(np.array([n], dtype=np.uint64))
    runs_dev, n_runs = C.c_void_p(), C.c_uint64()
    pred = C.byref(t.pred)
    assert L.pqps_filter_group_wide(ctx.h, t.cols, 1, n, pred, None, g.ref(), 0, 0, out, None) == EINVAL
    assert L.pqps_group_wide_list(ctx.h, None, g.ref(), n, ids, count, n, 0, 0, 0, out, None) == EINVAL
    assert L.pqps_bins_compact(ctx.h, out, 0, 0, C.byref(runs_dev), C.byref(n_runs), None) == EINVAL
    for bad in (0, (1 << 32) + 1):
        assert L.pqps_group_sort(ctx.h, g.ref(), 0, bad, None, n, ids, n, 0, C.byref(runs_dev), C.byref(n_runs), None) == EINVAL
    plane = pq.Column(g.ptr, pq.WIDTH_BITS, 0)                   # no bit plane as the group column of the wide calls
    assert L.pqps_filter_group_wide(ctx.h, t.cols, 1, n, pred, None, C.byref(plane), 0, 2, out, None) == EINVAL
    # the calls that were there keep their refusal above 65 536 bins
    assert L.pqps_filter_group(ctx.h, t.cols, 1, n, pred, g.ref(), 0, 65537, out, None) == EINVAL
    assert L.pqps_group_list(ctx.h, g.ref(), n, ids, count, n, 0, 0, 65537, out, None) == EINVAL
    assert L.pqps_filter_aggregate(ctx.h, t.cols, 1, n, pred, t.values["i32"].ref(), g.ref(), 0, 65537, out, None) == EINVAL
    assert L.pqps_ctx_set_option(ctx.h, b"wide_front", 0) == 0 and L.pqps_ctx_set_option(ctx.h, b"wide_front", -1) == 0
    for p in (out, ids, count):
        ctx.free(p)
    t.free()


def test_shapes_straddle_the_tile_the_cap_and_the_front():
    """CPU: the case lists hold both sides of every switch."""
    assert {65536, 65537, T - 1, T, T + 1} <= set(BINS) and 3 * T + 5 in BINS and 1 in BINS
    assert {1, 1023, 1024, 1025} <= set(SIZES) and max(SIZES) == 200_000
    for kind in ("hot", "busy", "shared"):
        b, n_bins = skew_column(kind, 200_000)
        assert b.min() >= 0 and b.max() < n_bins and n_bins > 65536
        used = np.unique(b)
        if kind == "hot":
            assert np.count_nonzero(b == 77) > 0.89 * len(b) and len(used) > 15_000
        if kind == "busy":
            assert len(used) > 2 * pq.WIDE_COUNT_SLOTS
        if kind == "shared":
            assert len(set((used % pq.WIDE_VALUE_SLOTS).tolist())) == 1 and len(used) == 5
