"""Index mode and the result-list tail called at the shim, against the contract of include/pqps_hip.h as tests/result_list_model.py
restates it in numpy, with inputs the engine never sends; every comparison is equality on the downloaded device words.

  * pqps_index_build: the five key types, 0 .. 70 001 rows around the sort's tile edges, keys that need 0 .. width passes (the result
    copied back after an even number, in place after an odd one), the extremes, both signs, heavy duplicates; perm and sorted_keys
  * pqps_index_probe: every key type over arange(n) and arange(n) // 3 (i32 also around zero), n on both sides of 64, 64^2 and 64^3,
    windows between every pair of the keys at the chunk edges of the 64-ary search, outside the keys, the type's extremes zero- and
    sign-extended, lo > hi; both words of `range`
  * the append through pqps_index_probe + pqps_filter_gather and through pqps_index_select's copy: ranges of 0 .. 9, 1023 .. 1025 rows
    and the whole table from odd and even positions of perm, *out_count preset to 0, 1, 3, 1000, id_base 0 and 4 000 000 000, the
    capacity below / at the count, inside / at the end of / beyond the rows; three probes into one buffer
  * pqps_gather_keys / pqps_project_column: shuffled lists with repeats, 0 .. 257 entries and one past the capped grid, three id_bases
    (one past which row + id_base wraps), *count_dev below, at and far above the capacity
  * pqps_merge_slots / pqps_merge_index_slots: worlds of 1 .. 1024, a slot longer than the grid, empty / full / overflowing slots,
    markers behind every count, merged_capacity 0 / total - 1 / total / total + 7, key slots strided by slot_stride - 4, keys that
    differ in 0, 1, 2 or 8 bytes, signed images made by pqps_gather_keys, IDs above 2^31, leaf order and shuffled slots
  * every output buffer has 64 bytes of slack, holds 0xA5 before the call, and the words behind the documented output must still
    hold it

The sort's second tile per workgroup is left to test_gpu_sort_shim.py, tables of millions of rows to test_gpu_index_scale.py.

The library passed as it was.  What the tests are there to catch, each planted once in a scratch build: `p0 <= r0` in probe_kernel
and an unclamped range[1] (test_index_probe_at_the_shim), a build without the copy-back after an even pass count
(test_index_build_at_the_shim), gather_keys_kernel without the sign bias (test_list_gathers_at_the_shim[keys-i32] and the signed key
set of test_merge_index_slots_at_the_shim), key slots read slot_stride apart and a merge without its ~id pass
(test_merge_index_slots_at_the_shim), append_range_kernel without its scalar tail (test_append_at_the_shim[*-copy]), displacements
summed from the reported counts (test_merge_slots_at_the_shim).  Input buffers carry 64 bytes of zeros behind them and the key slots
a whole slot_stride per rank, so that such a defect reads inside what the test allocated.
"""
import ctypes as C

import numpy as np
import pytest

import qpelib as q
import result_list_model as m

pq = q.pq
SLACK = 64                                      # bytes behind every buffer
GUARD = 16                                      # u32 words (8 u64) checked behind every documented output


class Dev:
    def __init__(self, ctx):
        self.ctx, self.L, self.mine = ctx, pq.lib(), []

    def alloc(self, nbytes, fill):
        p = self.ctx.malloc(nbytes + SLACK)
        self.ctx.memset(p, fill, nbytes + SLACK)
        self.mine.append(p)
        return p

    def put(self, a, pad_bytes=0):
        """An input: the array, zeros behind it (pad_bytes + the slack)."""
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes + pad_bytes, 0)
        if a.nbytes:
            self.ctx.upload(p, a.ctypes.data, a.nbytes)
        return p

    def out(self, nbytes):
        """An output: 0xA5 bytes."""
        return self.alloc(nbytes, 0xA5)

    def refill(self, p, nbytes):
        self.ctx.memset(p, 0xA5, nbytes + SLACK)

    def set_u64(self, p, value):
        w = C.c_uint64(value)
        self.ctx.upload(p, C.byref(w), 8)

    def get(self, p, dtype, count):
        self.ctx.sync()                                          # raises if a launch failed
        a = np.zeros(max(count, 1), dtype=dtype)
        if count:
            self.ctx.download(a.ctypes.data, p, count * a.itemsize)
        return a[:count]

    def free(self, p):
        self.ctx.sync()
        self.mine.remove(p)
        self.ctx.free(p)

    def drop(self):
        self.ctx.sync()
        for p in self.mine:
            self.ctx.free(p)
        self.mine = []


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


def diff(what, got, want):
    """None, or where the first word differs."""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} != {want.shape}"
    at = int(np.flatnonzero(got != want)[0])
    return f"{what}: [{at}] = {got[at]} != {want[at]} ({int((got != want).sum())} of {want.size} words differ)"


def done(ran, cases, bad):
    assert ran == len(cases) > 0, "no case may be skipped"
    assert not bad, (len(bad), bad[:8])


def fill_of(dtype, count):
    return np.full(count, m.A5_64 & ((1 << (8 * np.dtype(dtype).itemsize)) - 1), dtype=dtype)


# ---- pqps_index_build ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("t", m.TYPES)
def test_index_build_at_the_shim(dev, t):
    w, kind, udt, nmax = m.width_of(t), m.kind_of(t), m.UNSIGNED[m.width_of(t)], max(m.BUILD_NS)
    tail = SLACK // w                                            # keys checked behind sorted_keys[n - 1]
    perm, skeys = dev.out(4 * nmax), dev.out(w * nmax)
    cases, ran, bad = m.build_cases(t), 0, []
    for content, n in cases:
        what = f"index_build {t} {content} n={n}"
        keys = m.build_keys(t, content, n)
        col = dev.put(keys)
        dev.refill(perm, 4 * nmax)
        dev.refill(skeys, w * nmax)
        rc = dev.L.pqps_index_build(dev.ctx.h, C.byref(pq.Column(col, w, 0)), n, kind, perm, skeys, None)
        order = m.index_order(keys)
        problems = [f"{what}: returned {rc}" if rc != m.PQPS_OK else None,
                    diff(what + " perm", dev.get(perm, np.uint32, n + GUARD), np.concatenate([order.astype(np.uint32), fill_of(np.uint32, GUARD)])),
                    diff(what + " sorted_keys", dev.get(skeys, udt, n + tail), np.concatenate([keys[order].view(udt), fill_of(udt, tail)]))]
        bad += [p for p in problems if p]
        dev.free(col)
        ran += 1
    done(ran, cases, bad)


# ---- pqps_index_probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("t", m.TYPES)
def test_index_probe_at_the_shim(dev, t):
    w, kind = m.width_of(t), m.kind_of(t)
    cases, ran, bad = m.probe_cases(t), 0, []
    for index_kind, n in cases:
        skeys, windows = m.probe_index(t, index_kind, n), m.probe_windows(t, index_kind, n)
        keys_dev = dev.put(skeys)                                # (zeros behind the last key)
        ranges = dev.out(32 * len(windows))                      # per window: range[0], range[1], two words that stay
        for i, (lo, hi) in enumerate(windows):
            pq.check(dev.L.pqps_index_probe(dev.ctx.h, keys_dev, w, kind, n, lo, hi, ranges + 32 * i, None), f"probe {t} {index_kind} n={n}")
        got = dev.get(ranges, np.uint64, 4 * len(windows) + GUARD // 2).astype(object)
        for i, (lo, hi) in enumerate(windows):
            want = list(m.probe(skeys, m.as_key(lo, t), m.as_key(hi, t))) + [m.A5_64, m.A5_64]
            if got[4 * i:4 * i + 4].tolist() != want:
                bad.append(f"probe {t} {index_kind} n={n} lo={lo:#x} hi={hi:#x}: {got[4 * i:4 * i + 4].tolist()} != {want}")
        if not (got[4 * len(windows):] == m.A5_64).all():
            bad.append(f"probe {t} {index_kind} n={n}: the words behind the ranges changed")
        dev.free(keys_dev)
        dev.free(ranges)
        ran += 1
    done(ran, cases, bad)


# ---- the append: pqps_index_probe + pqps_filter_gather, pqps_index_select ---------------------------------------------------------
def one_leaf(lo, span):
    """One leaf on column 0, accepted when its window holds."""
    pred = pq.Predicate()
    pred.n_leaves, pred.n_columns, pred.truth = 1, 1, 2
    pred.leaf[0].column, pred.leaf[0].negate, pred.leaf[0].lo, pred.leaf[0].span = 0, 0, lo, span
    pred.on_true[0], pred.on_false[0], pred.order[0] = pq.ACCEPT, pq.REJECT, 0
    return pred


class Appender:
    """One index on the device and one buffer [count | - | range[0] | range[1] | 4 spare u64][out_ids ...]."""
    HEAD = 16                                                    # u32 words in front of out_ids

    def __init__(self, dev, name, path):
        self.dev, self.path = dev, path
        self.t, keys, flag, self.perm, self.skeys = m.select_table(name)
        self.n, self.w, self.kind = len(keys), m.width_of(self.t), m.kind_of(self.t)
        pad = (-self.n) % pq.TILE_ROWS                           # column buffers are padded to a multiple of PQPS_TILE_ROWS rows
        self.key_col = pq.Column(dev.put(keys, pad * self.w), self.w, 0)
        self.flag_col = pq.Column(dev.put(flag, pad), 1, 0)
        self.perm_dev, self.skeys_dev = dev.put(self.perm), dev.put(self.skeys)
        self.passes = flag.astype(bool) if path == "gather_flag" else None
        self.words = self.HEAD + 1000 + 3 * self.n + 8 + GUARD
        self.buf = dev.out(4 * self.words)
        self.dirty = 0

    def rows(self, window):
        _, _, b, e = window
        return e - b if self.passes is None else int(self.passes[self.perm[b:e]].sum())

    def run(self, windows, preset, id_base, cap, what):
        """The probes one after another into the same list -> what differs."""
        dev, L, h = self.dev, self.dev.L, self.dev.ctx.h
        need = self.HEAD + max(cap, preset + sum(self.rows(x) for x in windows)) + GUARD
        dev.ctx.memset(self.buf, 0xA5, 4 * max(need, self.dirty))
        self.dirty = need
        dev.set_u64(self.buf, preset)
        count_p, range_p, out_p = self.buf, self.buf + 16, self.buf + 4 * self.HEAD
        want = np.full(need, m.A5_32, dtype=np.uint32)
        count = preset
        for lo, hi, b, e in windows:
            if self.path == "copy":
                span = (int(m.as_key(hi, self.t)) - int(m.as_key(lo, self.t))) & (m.U64 if self.w == 8 else m.TOP32)
                pred = one_leaf(lo & m.mask_of(self.t), span)
                pq.check(L.pqps_index_select(h, C.byref(self.key_col), 1, C.byref(self.key_col), self.perm_dev, self.skeys_dev, self.kind, self.n,
                                             lo, hi, id_base, C.byref(pred), range_p, out_p, cap, count_p, None), what)
                name = L.pqps_last_kernel().decode()
                assert name.startswith("append_range_kernel"), (what, name)      # the copy, not the filter
            else:
                pq.check(L.pqps_index_probe(h, self.skeys_dev, self.w, self.kind, self.n, lo, hi, range_p, None), what)
                if self.path == "gather":                        # the probed comparison itself, evaluated
                    span = (int(m.as_key(hi, self.t)) - int(m.as_key(lo, self.t))) & m.TOP32
                    col, pred = self.key_col, one_leaf(lo & m.mask_of(self.t), span)
                else:
                    col, pred = self.flag_col, one_leaf(1, 0)
                pq.check(L.pqps_filter_gather(h, C.byref(col), 1, self.perm_dev, range_p, self.n, id_base, C.byref(pred), out_p, cap, count_p, None), what)
            count = m.select_append(want[self.HEAD:], count, self.perm, b, e, self.passes, id_base, cap)
        head = want[:self.HEAD].view(np.uint64)
        head[0], head[2], head[3] = count, windows[-1][2], windows[-1][3]
        return diff(what, dev.get(self.buf, np.uint32, need), want)


@pytest.mark.gpu
@pytest.mark.parametrize("path", m.SELECT_PATHS)
@pytest.mark.parametrize("name", m.SELECT_TABLES)
def test_append_at_the_shim(dev, name, path):
    ap = Appender(dev, name, path)
    windows, ran, bad, skipped = m.select_windows(name), 0, [], 0
    cases = m.select_cases(name)
    for wi, preset, id_base, place in cases:
        cap = m.place_capacity(place, preset, ap.rows(windows[wi]))
        ran += 1
        if cap is None:                                          # no such place: nothing below a count of 0, nothing inside one row
            skipped += 1
            continue
        what = f"append {name} {path} window={windows[wi]} preset={preset} id_base={id_base} capacity={cap} ({place})"
        problem = ap.run([windows[wi]], preset, id_base, cap, what)
        if problem:
            bad.append(problem)
    assert skipped < len(cases) // 4
    sequences = m.select_sequences(name)
    for wis, preset, id_base, place in sequences:
        three = [windows[i] for i in wis]
        cap = m.sequence_capacity(place, preset, [ap.rows(x) for x in three])
        problem = ap.run(three, preset, id_base, cap, f"append {name} {path} three probes {three} preset={preset} id_base={id_base} capacity={cap} ({place})")
        if problem:
            bad.append(problem)
        ran += 1
    done(ran, cases + sequences, bad)


# ---- pqps_gather_keys / pqps_project_column -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("t", m.TYPES)
@pytest.mark.parametrize("call", ("project", "keys"))
def test_list_gathers_at_the_shim(dev, call, t):
    w, kind, udt = m.width_of(t), m.kind_of(t), m.UNSIGNED[m.width_of(t)]
    column = m.list_column(t)
    col = pq.Column(dev.put(column), w, 0)
    long_m = m.long_list(16 if call == "project" else 8, dev.ctx.info()[1])
    out_dt = udt if call == "project" else np.uint64
    out_w = np.dtype(out_dt).itemsize
    tail = SLACK // out_w
    out, count_dev = dev.out(out_w * long_m), dev.out(8)
    cases, ran, bad, dirty, lists = m.list_cases(long_m), 0, [], long_m, {}
    for mm, id_base, how in cases:
        what = f"{call} {t} m={mm} id_base={id_base} count={how}"
        if (mm, id_base) not in lists:
            lists[mm, id_base] = dev.put(m.list_ids(mm, id_base))
        count = m.list_count(how, mm)
        dev.ctx.memset(out, 0xA5, out_w * max(dirty, mm) + SLACK)
        dirty = mm
        dev.set_u64(count_dev, count)
        if call == "project":
            rc = dev.L.pqps_project_column(dev.ctx.h, C.byref(col), lists[mm, id_base], count_dev, mm, id_base, out, None)
        else:
            rc = dev.L.pqps_gather_keys(dev.ctx.h, C.byref(col), kind, lists[mm, id_base], count_dev, mm, id_base, out, None)
        pq.check(rc, what)
        values = m.project(column, m.list_ids(mm, id_base), id_base, count, mm)
        want = values.view(udt) if call == "project" else m.key_image(values, kind == 1)
        want = np.concatenate([want, fill_of(out_dt, mm - len(want) + tail)])
        problems = [diff(what, dev.get(out, out_dt, mm + tail), want), diff(what + " count", dev.get(count_dev, np.uint64, 1 + GUARD // 2),
                                                                         np.concatenate([np.array([count], dtype=np.uint64), fill_of(np.uint64, GUARD // 2)]))]
        bad += [p for p in problems if p]
        ran += 1
    done(ran, cases, bad)


# ---- pqps_merge_slots -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", m.MERGE_LAYOUTS, ids=lambda x: f"{x[0]}x{x[1]}")
def test_merge_slots_at_the_shim(dev, layout):
    world, stride = layout
    room = world * (stride - m.HEADER_WORDS) + 7
    merged, totals = dev.out(4 * room), dev.out(16)
    cases, ran, bad, held = [c for c in m.merge_cases() if c[:2] == layout], 0, [], {}
    for _, _, counts, place, given in cases:
        what = f"merge_slots {world} x {stride} counts={counts[:6]} capacity={place} totals={'given' if given else 'NULL'}"
        slots = m.plain_slots(world, stride, counts)
        if counts not in held:
            held[counts] = dev.put(slots)
        total = sum(min(c, stride - m.HEADER_WORDS) for c in counts)
        cap = m.capacity_of(place, total)
        dev.refill(merged, 4 * room)
        dev.refill(totals, 16)
        pq.check(dev.L.pqps_merge_slots(dev.ctx.h, held[counts], world, stride, merged, cap, totals if given else None, None), what)
        ids, want_totals = m.merge_slots(slots, world, stride, cap)
        assert len(ids) == min(total, cap)
        problems = [diff(what + " merged", dev.get(merged, np.uint32, room + GUARD), np.concatenate([ids, fill_of(np.uint32, room + GUARD - len(ids))])),
                    diff(what + " totals", dev.get(totals, np.uint64, 2 + GUARD // 2),
                         np.concatenate([want_totals if given else fill_of(np.uint64, 2), fill_of(np.uint64, GUARD // 2)]))]
        bad += [p for p in problems if p]
        ran += 1
    done(ran, cases, bad)


# ---- pqps_merge_index_slots ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", m.INDEX_LAYOUTS, ids=lambda x: f"{x[0]}x{x[1]}")
def test_merge_index_slots_at_the_shim(dev, layout):
    world, stride = layout
    seg = stride - m.HEADER_WORDS
    room = world * seg + 7
    merged, totals = dev.out(4 * room), dev.out(16)
    signed_col = pq.Column(dev.put(m.key_column("signed5", world * seg)[1]), 4, 0)
    cases, ran, bad = [c for c in m.index_merge_cases() if c[:2] == layout], 0, []
    for _, _, counts, key_set, id_mode, place in cases:
        what = f"merge_index_slots {world} x {stride} counts={counts[:6]} keys={key_set} ids={id_mode} capacity={place}"
        slots, key_slots, id_base, _ = m.index_slots(world, stride, counts, key_set, id_mode)
        slots_dev = dev.put(slots)
        # the key slots lie seg apart; the buffer holds world x stride u64 so that a reader that took the wrong stride stays inside it
        if key_set == "signed5":                                 # the images as pqps_gather_keys makes them, count read from the slot's head
            keys_dev = dev.put(np.full(world * stride, m.MARK_KEY, dtype=np.uint64))
            for r in range(world):
                pq.check(dev.L.pqps_gather_keys(dev.ctx.h, C.byref(signed_col), 1, slots_dev + 4 * (r * stride + m.HEADER_WORDS), slots_dev + 4 * r * stride,
                                                seg, id_base, keys_dev + 8 * r * seg, None), what)
            problem = diff(what + " gathered keys", dev.get(keys_dev, np.uint64, world * seg), key_slots)
            if problem:
                bad.append(problem)
        else:
            keys_dev = dev.put(np.concatenate([key_slots, np.full(world * m.HEADER_WORDS, m.MARK_KEY, dtype=np.uint64)]))
        total = sum(min(c, seg) for c in counts)
        cap = m.capacity_of(place, total)
        dev.refill(merged, 4 * room)
        dev.refill(totals, 16)
        rc = dev.L.pqps_merge_index_slots(dev.ctx.h, slots_dev, keys_dev, world, stride, merged, cap, totals, None)
        want_rc, ids, want_totals = m.merge_index_slots(slots, key_slots, world, stride, cap)
        ids = np.zeros(0, dtype=np.uint32) if ids is None else ids          # an overflow leaves `merged` as it was
        problems = [f"{what}: returned {rc}, not {want_rc}" if rc != want_rc else None,
                    diff(what + " merged", dev.get(merged, np.uint32, room + GUARD), np.concatenate([ids, fill_of(np.uint32, room + GUARD - len(ids))])),
                    diff(what + " totals", dev.get(totals, np.uint64, 2 + GUARD // 2), np.concatenate([want_totals, fill_of(np.uint64, GUARD // 2)]))]
        bad += [p for p in problems if p]
        if ran == 0:                                             # totals is not optional here
            dev.refill(merged, 4 * room)
            rc = dev.L.pqps_merge_index_slots(dev.ctx.h, slots_dev, keys_dev, world, stride, merged, room, None, None)
            if rc != m.PQPS_EINVAL or not (dev.get(merged, np.uint32, room + GUARD) == m.A5_32).all():
                bad.append(f"{what}: totals == NULL returned {rc} or wrote")
        dev.free(slots_dev)
        dev.free(keys_dev)
        ran += 1
    done(ran, cases, bad)
