"""result_list_model.py without a GPU: every numpy reference against its row-by-row twin on hand-made and seeded inputs, and
every case list of tests/test_gpu_result_list_shim.py for the edges it is there for."""
import numpy as np

import result_list_model as m


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the references against loops -----------------------------------------------------------------------------------------
def test_index_order_and_probe_against_loops():
    hand = {"u8": [3, 3, 0, 255, 3, 0], "u16": [65535, 0, 65535, 1], "u32": [5, 5, 5], "i32": [0, -1, m.I32_MIN, m.I32_MAX, -1, 0],
            "u64": [m.U64, 0, 1 << 63, (1 << 63) - 1, m.U64]}
    for t in m.TYPES:
        columns = [np.array(hand[t], dtype=m.dtype_of(t)), np.zeros(0, dtype=m.dtype_of(t))]
        columns += [m.build_keys(t, content, n) for content in m.build_contents(t) for n in (1, 2, 257)]
        for keys in columns:
            order = m.index_order(keys)
            assert same(order, m.index_order_slow(keys)), (t, keys[:8])
            skeys = keys[order]
            assert (np.diff(skeys.astype(object)) >= 0).all()
            values = sorted({int(v) for v in skeys.tolist()} | {m.type_min(t), m.type_max(t), 0, 1})
            values += [v + d for v in values for d in (-1, 1) if m.type_min(t) <= v + d <= m.type_max(t)]
            r = m.rng("probe", t, len(keys))
            for lo, hi in [(values[i], values[j]) for i, j in r.integers(0, len(values), (40, 2))]:
                b, e = m.probe(skeys, lo, hi)
                assert (b, e) == m.probe_slow(skeys, lo, hi), (t, lo, hi)
                assert e >= b and ((skeys.astype(object) >= lo) & (skeys.astype(object) <= hi)).sum() == e - b
    # an i32 key means the same zero- and sign-extended; a raw pattern is read in the key's width
    assert m.as_key(m.raw_zero(-1, "i32"), "i32") == m.as_key(m.raw_sign(-1, "i32"), "i32") == -1 and m.raw_zero(-1, "i32") != m.raw_sign(-1, "i32")
    assert m.as_key(0x1FF, "u8") == 255 and m.as_key(m.U64, "u64") == m.U64 and m.as_key(0x80000000, "i32") == m.I32_MIN


def test_select_append_against_a_loop():
    for name in m.SELECT_TABLES:
        t, keys, flag, perm, skeys = m.select_table(name)
        r = m.rng("append", name)
        windows = m.select_windows(name)
        for k in range(40):
            lo, hi, b, e = windows[int(r.integers(0, len(windows)))]
            if e - b > 2000:
                continue
            passes = (None, flag.astype(bool))[k % 2]
            preset, base = m.SELECT_PRESETS[k % 4], m.SELECT_BASES[(k // 4) % 2]
            cap = int(r.integers(0, preset + (e - b) + 9))
            a, c = np.full(preset + e - b + 16, m.A5_32, dtype=np.uint32), np.full(preset + e - b + 16, m.A5_32, dtype=np.uint32)
            assert m.select_append(a, preset, perm, b, e, passes, base, cap) == m.select_append_slow(c, preset, perm, b, e, passes, base, cap)
            assert same(a, c) and (a[cap:] == m.A5_32).all() and (a[:preset] == m.A5_32).all()
    out = np.full(8, m.A5_32, dtype=np.uint32)                   # by hand: rows 5, 2, 9 at count 1, room for two
    assert m.select_append(out, 1, np.array([7, 5, 2, 9, 1], dtype=np.uint32), 1, 4, None, m.HIGH_BASE, 3) == 4
    assert out.tolist() == [m.A5_32, m.HIGH_BASE + 5, m.HIGH_BASE + 2] + [m.A5_32] * 5


def test_key_image_and_project_against_loops():
    for t in m.TYPES:
        col = m.list_column(t)
        signed = m.kind_of(t) == 1
        img = m.key_image(col, signed)
        assert same(img, m.key_image_slow(col, signed))
        order = np.argsort(col, kind="stable")
        assert (np.diff(img[order].astype(object)) >= 0).all(), t   # order preserving
        for mm in (0, 1, 255, 257):
            for base in m.LIST_BASES:
                ids = m.list_ids(mm, base)
                for how in m.LIST_COUNTS:
                    count = m.list_count(how, mm)
                    got = m.project(col, ids, base, count, mm)
                    assert same(got, m.project_slow(col, ids, base, count, mm)) and len(got) == min(count, mm)
                    assert same(got, col[m.list_rows(mm)[:len(got)]])
    assert m.key_image(np.array([m.I32_MIN, -1, 0, 1, m.I32_MAX], dtype=np.int32), True).tolist() == [0, 0x7FFFFFFF, 0x80000000, 0x80000001, m.TOP32]
    assert m.key_image(np.array([m.U64], dtype=np.uint64), False).tolist() == [m.U64]


def small_merge_cases():
    return [c for c in m.merge_cases() if c[0] * c[1] <= 40_000]


def test_merges_against_loops():
    seen = 0
    for world, stride, counts, place, _ in small_merge_cases()[::3]:
        slots = m.plain_slots(world, stride, counts)
        total = sum(min(c, stride - 4) for c in counts)
        cap = m.capacity_of(place, total)
        got, want = m.merge_slots(slots, world, stride, cap), m.merge_slots_slow(slots, world, stride, cap)
        assert same(got[0], want[0]) and same(got[1], want[1]) and len(got[0]) == min(total, cap), (world, stride, counts[:4], place)
        assert int(got[1][0]) == total and int(got[1][1]) == sum(counts) and m.MARK_ID not in got[0]
        seen += 1
    assert seen > 40
    seen = 0
    for world, stride, counts, key_set, id_mode, place in [c for c in m.index_merge_cases() if c[0] * c[1] <= 40_000][::17]:
        slots, key_slots, base, _ = m.index_slots(world, stride, counts, key_set, id_mode)
        total = sum(min(c, stride - 4) for c in counts)
        cap = m.capacity_of(place, total)
        got, want = m.merge_index_slots(slots, key_slots, world, stride, cap), m.merge_index_slots_slow(slots, key_slots, world, stride, cap)
        assert got[0] == want[0] == (m.PQPS_EOVERFLOW if total > cap else m.PQPS_OK) and same(got[2], want[2])
        assert (got[1] is None and want[1] is None) or (same(got[1], want[1]) and m.MARK_ID not in got[1] and len(got[1]) == total)
        seen += 1
    assert seen > 40
    # by hand: two slots of two, keys strided by stride - 4 = 2; equal keys give IDs descending
    slots = np.array([2, 0, 9, 9, 10, 11, 5, 0, 9, 9, 20, 21], dtype=np.uint32)
    keys = np.array([7, 3, 3, 7], dtype=np.uint64)
    rc, merged, totals = m.merge_index_slots(slots, keys, 2, 6, 4)
    assert rc == m.PQPS_OK and merged.tolist() == [20, 11, 21, 10] and totals.tolist() == [4, 7]
    assert m.merge_slots(slots, 2, 6, 3)[0].tolist() == [10, 11, 20] and m.merge_index_slots(slots, keys, 2, 6, 3)[:2] == (m.PQPS_EOVERFLOW, None)


# ---- the case lists -----------------------------------------------------------------------------------------------------------
def test_build_cases_cover_the_declared_edges():
    assert set(m.BUILD_NS) == {0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, 70_001}
    for t in m.TYPES:
        w, cases = m.width_of(t), m.build_cases(t)
        assert {n for _, n in cases} == set(m.BUILD_NS) and all({n for c, n in cases if c == content} == set(m.BUILD_NS) for content in m.build_contents(t))
        for n in m.BUILD_NS[3:]:
            passes = {content: m.sort_passes(m.build_keys(t, content, n), t) for content in m.build_contents(t)}
            assert passes["equal"] == 0 and passes["top"] == w and passes["random"] == w, (t, n, passes)
            assert all(passes[("bytes", k)] == k + 1 for k in range(w)), (t, n, passes)       # copy-back after 0, 2, ... passes, in place after 1, 3, ...
            assert {p % 2 for p in passes.values()} == {0, 1}
            img = m.key_image(m.build_keys(t, "top", n), m.kind_of(t) == 1)
            assert int(img.min() ^ img.max()) >> (8 * (w - 1)) and (int(img.min() ^ img.max()) & ((1 << (8 * (w - 1))) - 1)) == 0
            rnd = m.build_keys(t, "random", n)
            assert int(rnd.min()) == m.type_min(t) and int(rnd.max()) == m.type_max(t)
            dups = m.build_keys(t, "dups", n)
            assert len(np.unique(dups)) <= 5 and {m.type_min(t), m.type_max(t)} <= set(dups.tolist())
        assert all(len(m.build_keys(t, content, n)) == n and m.build_keys(t, content, n).dtype == m.dtype_of(t) for content, n in cases)
    assert {m.I32_MIN, -1, 0, m.I32_MAX} <= set(m.build_keys("i32", "signs", 255).tolist())
    signs = m.build_keys("i32", "signs", 70_001)
    assert (signs < 0).mean() > 0.3 and (signs > 0).mean() > 0.3 and (signs == -1).sum() > 1000


def test_probe_cases_cover_the_declared_edges():
    assert set(m.PROBE_NS) == {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 262_143, 262_144, 262_145} and {64, 64 ** 2, 64 ** 3} <= set(m.PROBE_NS)
    for t in m.TYPES:
        assert set(m.probe_cases(t)) == {(k, n) for k in m.probe_kinds(t) for n in m.PROBE_NS} and {"arange", "thirds"} <= set(m.probe_kinds(t))
        for kind, n in m.probe_cases(t):
            keys, windows = m.probe_index(t, kind, n), m.probe_windows(t, kind, n)
            assert len(keys) == n and keys.dtype == m.dtype_of(t) and (n < 2 or (np.diff(keys.astype(object)) >= 0).all())
            c = (n + 63) // 64
            named = [p for p in (0, 1, 62, 63, 64, 65, c - 1, c, c + 1, n - 2, n - 1) if 0 <= p < n]
            assert m.probe_positions(n) == sorted(set(named))
            at = {m.raw_zero(keys[p], t) for p in named}
            assert {(a, b) for a in at for b in at} <= set(windows), (t, kind, n)
            typed = [(int(m.as_key(lo, t)), int(m.as_key(hi, t))) for lo, hi in windows]
            assert any(lo > hi for lo, hi in typed) and (m.type_min(t), m.type_max(t)) in typed and (m.type_max(t), m.type_min(t)) in typed
            if n:
                assert any(hi < int(keys[0]) for lo, hi in typed) == (int(keys[0]) > m.type_min(t)), (t, kind, n)
                assert any(lo > int(keys[-1]) for lo, hi in typed) == (int(keys[-1]) < m.type_max(t)), (t, kind, n)
        if m.width_of(t) >= 4:                                   # every position a boundary / runs of three
            assert len(np.unique(m.probe_index(t, "arange", 4097))) == 4097 and len(np.unique(m.probe_index(t, "thirds", 4097))) == 1366
    assert len(np.unique(m.probe_index("u8", "arange", 4097))) == 256 and int(m.probe_index("u16", "arange", 262_145).max()) == 65_535
    centred = m.probe_index("i32", "centred", 65)
    assert int(centred[0]) == -32 and int(centred[-1]) == 32
    wins = m.probe_windows("i32", "arange", 65)                  # the extremes zero- and sign-extended
    assert {(0x80000000, 0x7FFFFFFF), (0xFFFFFFFF80000000, 0x7FFFFFFF)} <= set(wins)


def test_select_cases_cover_the_declared_edges():
    assert m.SELECT_PRESETS == (0, 1, 3, 1000) and m.SELECT_BASES == (0, 4_000_000_000)
    for name, n in (("i32", 70_001), ("u8", 1025)):
        t, keys, flag, perm, skeys = m.select_table(name)
        assert t == name and len(keys) == n and same(skeys, keys[perm]) and 0.4 < flag.mean() < 0.6
        windows = m.select_windows(name)
        starts = {}
        for lo, hi, b, e in windows:
            starts.setdefault(e - b, set()).add(b % 2)
        assert set(starts) == set(m.SELECT_LENGTHS) | {n}, name
        assert all(starts[ln] == {0, 1} for ln in m.SELECT_LENGTHS if ln != n), (name, starts)
        assert {b % 4 for _, _, b, e in windows if e - b >= 8} >= ({0, 2, 3} if name == "i32" else {0, 1, 2})       # the 16-byte path from any offset
        cases = m.select_cases(name)
        assert {(w, p, pl) for w, p, _, pl in cases} == {(w, p, pl) for w in range(len(windows)) for p in m.SELECT_PRESETS for pl in m.SELECT_PLACES}
        for place in m.SELECT_PLACES:
            assert {(p, base) for _, p, base, pl in cases if pl == place} == {(p, base) for p in m.SELECT_PRESETS for base in m.SELECT_BASES}
        seqs = m.select_sequences(name)
        assert {(pl, base) for _, _, base, pl in seqs} == {(pl, base) for pl in m.SELECT_PLACES for base in m.SELECT_BASES}
        assert {p for _, p, _, _ in seqs} == set(m.SELECT_PRESETS) and all(len(ws) == 3 for ws, _, _, _ in seqs)
    assert (m.select_table("i32")[1] < 0).mean() > 0.4 and {m.I32_MIN, m.I32_MAX} <= set(m.select_table("i32")[1].tolist())
    assert [m.place_capacity(pl, 3, 10) for pl in m.SELECT_PLACES] == [2, 3, 8, 13, 20] and m.place_capacity("below", 0, 5) is None
    assert [m.sequence_capacity(pl, 1, (4, 6, 8)) for pl in m.SELECT_PLACES] == [3, 5, 8, 11, 26]


def test_list_cases_cover_the_declared_edges():
    cases = m.list_cases(m.long_list(16, 256))
    assert m.long_list(16, 256) == 1_048_577 and m.long_list(8, 256) == 524_289
    assert {c[0] for c in cases} == {0, 1, 255, 256, 257, 1_048_577} and m.LIST_BASES[:2] == (0, 4_000_000_000)
    assert all({(b, h) for mm, b, h in cases if mm == k} == {(b, h) for b in m.LIST_BASES for h in m.LIST_COUNTS} for k in m.LIST_MS)
    assert {h for mm, b, h in cases if mm > 257} == set(m.LIST_COUNTS)
    for t in m.TYPES:
        col = m.list_column(t)
        assert len(col) == 5000 and {m.type_min(t), m.type_max(t)} <= set(col.tolist())
    assert {m.I32_MIN, -1, 0, m.I32_MAX} <= set(m.list_column("i32").tolist()) and (m.list_column("i32") < 0).mean() > 0.4
    for mm in (255, 256, 257, 524_289):
        rows = m.list_rows(mm)
        assert (np.diff(rows) < 0).any() and len(np.unique(rows)) < mm and {999, 1000} <= set(rows.tolist())
        ids = m.list_ids(mm, m.WRAP_BASE)
        assert (ids < 5000).any() and (ids >= m.WRAP_BASE).any()   # the sum wraps for some rows and not for others
    assert [m.list_count(h, 256) for h in m.LIST_COUNTS] == [255, 256, 1 << 40]


def test_merge_cases_cover_the_declared_edges():
    assert m.MERGE_LAYOUTS == ((1, 6), (2, 6), (3, 258), (8, 4100), (1024, 10), (2, 262_404)) and m.INDEX_LAYOUTS[4] == (1024, 8)
    assert [l for i, l in enumerate(m.INDEX_LAYOUTS) if i != 4] == [l for i, l in enumerate(m.MERGE_LAYOUTS) if i != 4]
    assert 262_404 - 4 > 1024 * 256                              # a slot longer than the capped grid
    cases = m.merge_cases()
    for world, stride in m.MERGE_LAYOUTS:
        seg = stride - 4
        mine = [c for c in cases if c[:2] == (world, stride)]
        assert {v for c in mine for v in c[2]} >= {0, 1, seg - 1, seg, seg + 1, 1 << 40}, (world, stride)
        assert {(c[3], c[4]) for c in mine} == {(p, g) for p in m.CAPACITY_PLACES for g in (True, False)}
        counts = {p: m.pattern_counts(p, world, stride) for p in m.COUNT_PATTERNS}
        assert not any(counts["empty"]) and counts["full"] == (seg,) * world and counts["first_empty"][0] == 0 and counts["last_empty"][-1] == 0
        assert counts["middle_empty"][world // 2] == 0 and sum(c > seg for c in counts["over_one"]) == 1 and counts["over_huge"][0] == 1 << 40
        if world > 2:
            assert counts["middle_empty"][0] and counts["middle_empty"][-1] and counts["first_empty"][1] and counts["last_empty"][0]
        slots = m.plain_slots(world, stride, counts["over_one"])
        assert (slots.reshape(world, stride)[:, 2:4] == m.MARK_ID).all() and slots[(world // 2) * stride + 4 + seg - 1] != m.MARK_ID
        assert (slots.reshape(world, stride)[0, 4 + seg - 1:] == m.MARK_ID).all() or world == 1
    assert [m.capacity_of(p, 10) for p in m.CAPACITY_PLACES] == [0, 9, 10, 17]
    # the index merge: every layout meets every pattern, key set and id mode; the named totals; overflow and spare capacity
    icases = m.index_merge_cases()
    for world, stride in m.INDEX_LAYOUTS:
        mine = [c for c in icases if c[:2] == (world, stride)]
        assert {c[2] for c in mine} >= {m.pattern_counts(p, world, stride) for p in m.COUNT_PATTERNS}
        assert {c[3] for c in mine} == set(m.KEY_SETS) and {c[4] for c in mine} == set(m.ID_MODES) and {c[5] for c in mine} >= {"exact", "short", "spare"}
        assert any(max(c[2]) > stride - 4 for c in mine)         # a slot that reports more than it holds
    totals = {sum(min(v, c[1] - 4) for v in c[2]) for c in icases}
    assert totals >= set(m.INDEX_TOTALS)
    for total in m.INDEX_TOTALS:
        assert {c[3] for c in icases if sum(min(v, c[1] - 4) for v in c[2]) == total} == set(m.KEY_SETS), total
    # the key sets: how many bytes differ, and so how many passes an LSD sort of the compacted keys needs
    diff = {k: int(m.key_column(k, 4096)[0].min() ^ m.key_column(k, 4096)[0].max()) for k in m.KEY_SETS}
    assert diff["equal"] == 0 and diff["byte0"] == 0xFF and diff["bytes01"] == 0xFFFF and diff["byte7"] == 0xFF << 56 and diff["random"] == m.U64
    img, col = m.key_column("signed5", 4096)
    assert set(col.tolist()) == {m.I32_MIN, -1, 0, 1, m.I32_MAX} and same(img, m.key_image(col, True))
    assert {0, m.U64} <= set(m.key_column("random", 4096)[0].tolist())
    # inside a slot: leaf order or not; a higher rank's rows are higher; the same key on every rank gives the IDs descending
    world, stride = 8, 4100
    counts = m.pattern_counts("below_full", world, stride)
    for mode in m.ID_MODES:
        slots, key_slots, base, _ = m.index_slots(world, stride, counts, "byte0", mode)
        ids = slots.reshape(world, stride)[:, 4:4 + counts[0]].astype(np.int64)
        keys = key_slots.reshape(world, stride - 4)[:, :counts[0]]
        assert (ids.min() >= 1 << 31) == mode.endswith("high") and (ids[1:].min(axis=1) > ids[:-1].max(axis=1)).all()
        leaf = all(np.array_equal(np.lexsort((-ids[k], keys[k])), np.arange(counts[0])) for k in range(world))
        assert leaf == mode.startswith("leaf")
        assert (slots.reshape(world, stride)[:, -1] == m.MARK_ID).all() and (key_slots.reshape(world, stride - 4)[:, -1] == m.MARK_KEY).all()
    slots, key_slots, _, _ = m.index_slots(world, stride, counts, "equal", "leaf_high")
    rc, merged, _ = m.merge_index_slots(slots, key_slots, world, stride, sum(counts))
    assert rc == m.PQPS_OK and (np.diff(merged.astype(np.int64)) < 0).all() and merged[0] >= m.HIGH_BASE + 7 * 4096
    # keys strided by stride - 4: read at `stride` apart instead, a rank's keys would be another rank's
    slots, key_slots, _, _ = m.index_slots(world, stride, counts, "byte0", "leaf")
    wrong = np.concatenate([key_slots, np.zeros(4 * world, dtype=np.uint64)])
    assert not np.array_equal(wrong.reshape(world, stride)[1, :counts[1]], key_slots.reshape(world, stride - 4)[1, :counts[1]])
