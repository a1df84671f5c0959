"""pqps_filter_group_head / pqps_group_head_list / pqps_runs_head_flags / pqps_group_head_sort AT THE SHIM: the inputs of
tests/fused_driver.py, the key and group columns of tests/test_gpu_group_first_shim.py (padding past n that would change
every answer), the raw [round][bin] device words compared exactly with tests/group_head_model.py.  The number of rounds, the
WHERE and the row base rotate across bins x key forms x directions, so every test takes seconds.
Bins: no group column; 4096 | 4097: the floor leaves LDS; 8192 | 8193: the min table leaves LDS."""
import itertools

import numpy as np
import pytest

import fused_driver as fd
import group_first_model as m
import group_head_model as hm
import test_gpu_group_first_shim as gf

pq = m.q.pq
SIZES = (1, 1023, 1024, 1025, 4097, 65537)
BINS = (1, 2, 16, 4096, 4097, 8192, 8193, 65536)
ROUNDS = (1, 2, 3, 5, 16)
MAX_ROUNDS = 16
assert MAX_ROUNDS == pq.HEAD_ROUNDS_MAX


def head_path(n_bins, wide):
    if n_bins == 1:
        return "HEAD_ONE"
    return "HEAD_LDS2" if n_bins <= 4096 and not wide else "HEAD_LDS" if n_bins <= 8192 else "HEAD_GLOBAL"


def group_width(n_bins, turn, plane_ok):
    return gf.group_width(n_bins, turn, plane_ok) if n_bins <= 16 else 4 if n_bins == 65536 or turn % 2 else 2


class Harness(gf.Harness):
    def __init__(self, n):
        super().__init__(n)
        ctx = self.gpu.ctx
        self.out, self.bests = ctx.malloc(MAX_ROUNDS * 65536 * 8), ctx.malloc(MAX_ROUNDS * 65536 * 8)
        self.short_bins = 0                                           # bins met with 0 < rows < rounds

    def close(self):
        self.gpu.ctx.sync()
        self.gpu.ctx.free(self.out)
        self.gpu.ctx.free(self.bests)
        super().close()

    def want(self, kkind, desc, rows, keys, bins, n_bins, rounds, base):
        keys = keys[rows]
        bins = None if bins is None else bins[rows]
        if kkind == m.KIND_U64:
            return hm.expected_round_wide(n_bins, rounds, desc, rows, keys, bins, base)
        return hm.expected_round_words(n_bins, rounds, kkind, desc, rows, keys, bins, base), None

    def check(self, what, kkind, want, want_best, n_bins, rounds):
        gpu = self.gpu
        got = gpu.get(self.out, np.uint64, rounds * n_bins).reshape(rounds, n_bins)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, "out", bad[:5].tolist(), [hex(int(got[r, b])) for r, b in bad[:5]], [hex(int(want[r, b])) for r, b in bad[:5]])
        if kkind == m.KIND_U64:
            best = gpu.get(self.bests, np.uint64, rounds * n_bins).reshape(rounds, n_bins)
            live = want != m.EMPTY                                    # best means something only where out has a row
            assert np.array_equal(best[live], want_best[live]), (what, "best")
        have = (want != m.EMPTY).sum(axis=0)
        self.short_bins += int(((have > 0) & (have < rounds)).sum())
        return got

    def fused(self, pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, row_base, rounds):
        gpu, inp = self.gpu, self.inp
        wide = kkind == m.KIND_U64
        what = (inp.n, pname, kkind, None if kcol is None else kcol.width, None if gcol is None else gcol.width, n_bins, desc, row_base, rounds)
        cols, n_cols, pred = inp.bound(pname)
        gpu.ctx.memset(self.out, 0xA5, rounds * n_bins * 8)          # the call initialises its outputs
        pq.filter_group_head(gpu.ctx, cols, n_cols, inp.n, pred, None if kcol is None else kcol.c, kkind == m.KIND_I32, desc, row_base,
                             None if gcol is None else gcol.c, base, n_bins, rounds, self.out, self.bests if wide else None, gpu.words)
        mode = "FIRST_WIDE_B" if wide else "FIRST_NARROW"
        gpu.fused(f"head_scan_kernel<{head_path(n_bins, wide)}, {mode}, NT=?>" if rounds > 1 else
                  f"first_scan_kernel<{gf.PATHS[8192 if 16 < n_bins <= 8192 else n_bins]}, {mode}, NT=?>", what)
        rows = inp.sel[pname]
        want, want_best = self.want(kkind, desc, rows, keys, bins, n_bins, rounds, row_base)
        got = self.check(what, kkind, want, want_best, n_bins, rounds)
        assert int(gpu.get(gpu.words, np.uint64, 1)[0]) == len(rows), (what, "count")
        return got

    def listed(self, pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, id_base, rounds, cap="equal"):
        gpu, inp = self.gpu, self.inp
        wide = kkind == m.KIND_U64
        rows, _, ids_dev, count_dev = inp.id_list(pname, id_base)
        capacity = {"below": len(rows) * 2 // 3, "equal": len(rows), "above": len(rows) + 100}[cap]
        what = ("list", inp.n, pname, kkind, n_bins, desc, id_base, cap, rounds)
        gpu.ctx.memset(self.out, 0xA5, rounds * n_bins * 8)
        pq.group_head_list(gpu.ctx, None if kcol is None else kcol.c, kkind == m.KIND_I32, desc, None if gcol is None else gcol.c, base,
                           n_bins, inp.n, ids_dev, count_dev, capacity, id_base, rounds, self.out, self.bests if wide else None)
        used = rows[:min(capacity, len(rows))]                       # an id listed twice is one candidate: the model removes it
        want, want_best = self.want(kkind, desc, used, keys, bins, n_bins, rounds, id_base)
        self.check(what, kkind, want, want_best, n_bins, rounds)


@pytest.fixture(scope="module", params=SIZES)
def harness(request):
    h = Harness(request.param)
    yield h
    h.close()


@pytest.mark.gpu
def test_every_bin_count_key_and_direction(harness):
    """Fused scan and list form over bins x key kinds x directions; the rounds, the WHERE and the bases take turns."""
    h, inp = harness, harness.inp
    for turn, (n_bins, kind, desc) in enumerate(itertools.product(BINS, gf.KINDS, (False, True))):
        pname = ("all", "sparse", "dense")[turn % 3]
        base_row = (0, fd.HIGH_BASE)[(turn // 3) % 2]
        rounds = ROUNDS[(turn // 2 + turn // 14) % len(ROUNDS)]
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, turn, True))
        h.fused(pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, base_row, rounds)
        if kind != fd.BIT:                                           # the list form gathers bytes: no bit planes
            gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, turn, False))
            h.listed(pname, kcol, keys, kkind, gcol, bins, base, n_bins, desc, base_row, rounds, cap=fd.LIST_CAPS[turn % 3])
    if inp.n >= 1023:                                                # bins with exactly r rows, 0 < r < n_rounds: later rounds all ones
        assert h.short_bins > 0


@pytest.mark.gpu
def test_every_round_count_on_every_path(harness):
    """n_rounds 1, 2, 3, 5 and 16 on each floor placement, narrow and wide."""
    h, inp = harness, harness.inp
    for n_bins, kind, rounds in itertools.product((1, 16, 4097, 8193), ("i4", 8), ROUNDS):
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, 1, False))
        h.fused("dense", kcol, keys, kkind, gcol, bins, base, n_bins, rounds % 2 == 0, 0, rounds)
        h.listed("dense", kcol, keys, kkind, gcol, bins, base, n_bins, rounds % 2 == 1, fd.HIGH_BASE, rounds)


@pytest.mark.gpu
def test_one_round_is_the_first_row_call(harness):
    h, inp = harness, harness.inp
    gpu = h.gpu
    for n_bins, kind, desc in itertools.product((1, 4096, 65536), (2, 8), (False, True)):
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, 0, False))
        got = h.fused("dense", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 11, 1)
        pq.filter_group_first(gpu.ctx, *inp.bound("dense")[:2], inp.n, inp.bound("dense")[2], None if kcol is None else kcol.c, False, desc,
                              11, None if gcol is None else gcol.c, base, n_bins, gpu.out, h.best if kkind == m.KIND_U64 else None, gpu.words)
        assert np.array_equal(got[0], gpu.get(gpu.out, np.uint64, n_bins))


@pytest.mark.gpu
def test_no_match_and_more_rounds_than_matches(harness):
    """A WHERE that matches nothing: every word of every round all ones, count 0.  The sparse WHERE over many bins: more
    rounds than any bin has rows."""
    h, inp = harness, harness.inp
    for n_bins, kind in itertools.product((1, 16, 4097, 8193), (4, 8)):
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, 0, False))
        for desc in (False, True):
            got = h.fused("nothing", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, 5)
            assert (got == m.EMPTY).all()
            h.listed("nothing", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, 5)
            got = h.fused("sparse", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, 16)
            if n_bins > 16 or inp.n == 1:
                assert (got[-1] == m.EMPTY).all()                    # no bin holds 16 of the ~34 sparse rows


@pytest.mark.gpu
def test_every_key_equal_rounds_advance_by_row(harness):
    """Every key equal: round r of a bin is its (r + 1)-th lowest row, in both directions, for every key form."""
    h, inp = harness, harness.inp
    for turn, (n_bins, kind, desc) in enumerate(itertools.product((1, 16, 8193), gf.KINDS, (False, True))):
        kcol, keys, kkind = gf.key_cache(inp, kind, "equal")
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, 1, False))
        rounds = ROUNDS[1 + turn % 4]
        got = h.fused("dense", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 7, rounds)
        rows = inp.sel["dense"]
        if n_bins == 1 and len(rows) >= rounds:
            low = got[:, 0] & np.uint64(0xFFFFFFFF)
            assert low.tolist() == (rows[:rounds] + 7).tolist()
        if kind != fd.BIT:
            h.listed("dense", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 7, rounds)


@pytest.mark.gpu
def test_every_row_in_one_bin_of_many(harness):
    """Maximum contention on one word, on each floor placement."""
    h, inp = harness, harness.inp
    for n_bins, kind, desc in itertools.product((4096, 8192, 65536), (2, "i4", 8), (False, True)):
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, 4, "one")
        h.fused("all", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, 5)
        h.listed("all", kcol, keys, kkind, gcol, bins, base, n_bins, desc, 0, 3, cap="above")


@pytest.mark.gpu
def test_refused_arguments(harness):
    h, inp = harness, harness.inp
    gpu = h.gpu
    cols, n_cols, pred = inp.bound("all")
    kcol, _, _ = gf.key_cache(inp, 4)
    wide, _, _ = gf.key_cache(inp, 8)
    gcol, _, _ = gf.group_cache(inp, 16, 1)
    L = pq.lib()

    def fused(key, group, n_bins, best, rounds):
        return L.pqps_filter_group_head(gpu.ctx.h, cols, n_cols, inp.n, pred, key.ref() if key else None, 0, 0, 0,
                                        group.ref() if group else None, 0, n_bins, rounds, h.out, best, gpu.words, None)

    assert fused(kcol, gcol, 16, None, 0) != 0
    assert fused(kcol, gcol, 16, None, MAX_ROUNDS + 1) != 0
    assert fused(kcol, None, 2, None, 2) != 0                        # no group column: one bin
    assert fused(kcol, gcol, 65537, None, 2) != 0
    assert fused(wide, gcol, 16, None, 2) != 0                       # an 8-byte key needs `best`
    rows, _, ids_dev, count_dev = inp.id_list("all", 0)
    assert L.pqps_group_head_list(gpu.ctx.h, kcol.ref(), 0, 0, gcol.ref(), 0, 16, inp.n, ids_dev, count_dev, len(rows), 0, MAX_ROUNDS + 1,
                                  h.out, None, None) != 0
    assert L.pqps_runs_head_flags(gpu.ctx.h, h.out, 5, 0, h.bests, None) != 0        # limit 0
    assert fused(kcol, gcol, 16, None, 2) == 0
    gpu.ctx.sync()


# ---- the sort form ----------------------------------------------------------------------------------------------------
def run_keys(n, limit, rng):
    """n sorted u64 keys in runs of length 1, limit - 1, limit, limit + 1 and random lengths; the first run's key is 0, the
    last run's all ones."""
    lengths = []
    while sum(lengths) < n:
        lengths += [1, max(limit - 1, 1), limit, limit + 1, int(rng.integers(1, 50))]
    keys = np.repeat(np.arange(len(lengths), dtype=np.uint64) * np.uint64(3) + np.uint64(9), lengths)[:n]
    if n:
        first, last = keys[0], keys[-1]
        keys[keys == last] = fd.U64
        keys[keys == first] = 0
    return keys


@pytest.mark.gpu
def test_runs_head_flags():
    gpu = fd.Gpu()
    ctx = gpu.ctx
    rng = np.random.default_rng(0x4EAD)
    keep = ctx.malloc(65537 + 64)
    for n, limit in itertools.product((0, 1, 1023, 1024, 1025, 65537), (1, 2, 3, 17, 70000)):
        for one_run in (False, True):
            keys = np.full(n, 7, np.uint64) if one_run else run_keys(n, min(limit, 40), rng)
            dev = gpu.put(keys)
            ctx.memset(keep, 0xA5, n + 64)
            pq.runs_head_flags(ctx, dev, n, limit, keep)
            got = gpu.get(keep, np.uint8, n + 64)
            assert np.array_equal(got[:n], hm.runs_head_flags(keys, limit)), (n, limit, one_run)
            assert (got[n:] == 0xA5).all(), (n, limit, "written past n")
            ctx.free(dev)
    ctx.free(keep)
    gpu.close()


@pytest.mark.gpu
def test_sort_form_over_a_list(harness):
    """pqps_group_head_sort: the list (every seventh id twice) sorted, repeats out, the first `limit` of every group kept."""
    h, inp = harness, harness.inp
    gpu = h.gpu
    for turn, (n_bins, kind, desc) in enumerate(itertools.product((1, 16, 8193), (1, "i4", None, 8), (False, True))):
        limit = (1, 3, 17, 100000)[turn % 4]
        id_base = (0, fd.HIGH_BASE)[turn % 2]
        kcol, keys, kkind = gf.key_cache(inp, kind)
        gcol, bins, base = gf.group_cache(inp, n_bins, group_width(n_bins, turn, False))
        rows, _, ids_dev, _ = inp.id_list("dense", id_base)
        n = len(rows)
        out_ids, out_keys = gpu.ctx.malloc(max(n, 1) * 4), gpu.ctx.malloc(max(n, 1) * 16)
        kept = pq.group_head_sort(gpu.ctx, None if kcol is None else kcol.c, kkind == m.KIND_I32, desc, None if gcol is None else gcol.c,
                                  False, ids_dev, n, id_base, limit, True, out_ids, out_keys)
        got_rows = gpu.get(out_ids, np.uint32, kept).astype(np.int64) - id_base
        got_groups = gpu.get(out_keys, np.uint64, kept)
        got_images = gpu.get(out_keys, np.uint64, n + kept)[n:]
        gpu.ctx.free(out_ids)
        gpu.ctx.free(out_keys)
        values = None if gcol is None else gcol.u[rows].astype(np.int64)      # the group IMAGE is the column's value: no bins
        _, offsets, want_rows, want_keys = hm.head_rows(rows, keys[rows], values, desc, limit)
        what = (inp.n, n_bins, kind, desc, limit)
        assert kept == len(want_rows) and np.array_equal(got_rows, want_rows), what
        assert np.array_equal(got_groups, np.zeros(kept, np.uint64) if gcol is None else gcol.u[want_rows].astype(np.uint64)), what
        if kkind == m.KIND_U64:
            image = want_keys.astype(np.uint64) ^ np.uint64(fd.U64 if desc else 0)
        elif kcol is None:
            image = np.zeros(kept, np.uint64)
        else:
            image = np.array([m.pack_word(kkind, desc, int(k), 0) >> 32 for k in want_keys], np.uint64)
        assert np.array_equal(got_images, image), what
