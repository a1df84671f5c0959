"""pqps_filter_topk_multi / pqps_topk_list_multi / pqps_sort_list_multi AT THE SHIM: small tables planted with numpy, the rows of
the answers compared with np.lexsort over the RAW column values (each key negated where it is descending, the row last) --
the expectation never packs a key.  The predicate columns, their WHEREs (all / sparse / dense / nothing), the matching padding
past n and the ID lists (shuffled, every seventh entry twice) are tests/fused_driver.py's; the field columns are made here,
their padding holding the extremes that would lead every answer.  Every case goes through all three calls, which must agree.
The shim reads PQPS_NT_LOADS once per process, so test_both_load_flavours runs this file again in a child process under either
flavour and checks that all sixteen instances of the scan kernel were launched between them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_driver as fd

pq = fd.pq
SIZES = (1, 63, 64, 1023, 1024, 1025, 4097)                   # step and padding edges
KS_NARROW = (1, 2, 63, 64, 65, 511, 512, 513, 1024)
KS_WIDE = (1, 2, 63, 64, 65, 511, 512)
EMPTY = (1 << 64) - 1

# a field: (column kind, bits); kinds: 1 / 2 / 4 bytes unsigned, fd.BIT the bit plane, "i4" a signed i32 over [lo, lo + 2^bits)
B = fd.BIT
LAYOUTS = [
    [(B, 1)],                                                  # T = 1
    [(1, 8), (2, 16), (4, 7)],                                 # T = 31
    [(2, 16), (4, 8), (1, 8)],                                 # T = 32
    [(4, 32), (B, 1)],                                         # T = 33
    [("i4", 31), (4, 32)],                                     # T = 63
    [("i4", 32), ("i4", 32)],                                  # T = 64: two full-range i32 columns
    [(B, 1), (1, 3), (2, 10), (4, 17)],                        # every kind in every position: four rotations
    [(1, 3), (2, 10), (4, 17), (B, 1)],
    [(2, 10), (4, 17), (B, 1), (1, 3)],
    [(4, 17), (B, 1), (1, 3), (2, 10)],
    [("i4", 7), (1, 0), (2, 9)],                               # a field of no bits in the middle
    [(2, 16), (4, 24), (1, 8)],                                # T = 48: three fields in a wide key
    [(4, 20), (2, 12), (1, 5), (B, 1)],                        # T = 38: four fields in a wide key
]
KERNELS = set()                                               # the scan instances this process launched


def desc_patterns(nf):
    """No DESC, DESC in each position alone, DESC everywhere."""
    pats = [tuple(False for _ in range(nf))] + [tuple(j == i for j in range(nf)) for i in range(nf)] + [tuple(True for _ in range(nf))]
    return list(dict.fromkeys(pats))


def field_lo(kind, bits):
    if kind != "i4":
        return 0
    return fd.I32_MIN if bits == 32 else -50


class Field:
    """One field column: raw[r] = the value as the column's type orders it (int64), base / bits as the shim takes them."""

    def __init__(self, inp, tag, kind, bits, flavour):
        n, pad = inp.n, inp.pad
        rng = inp.rng(("omf", tag, kind, bits, flavour))
        lo = field_lo(kind, bits)
        dom = 1 << bits
        if flavour == "equal":
            full = np.full(pad, lo + min(dom - 1, 3), np.int64)
        elif flavour == "ties":                                # a handful of values: long runs of equal keys
            pool = np.array(sorted({0, min(1, dom - 1), dom // 2, max(dom - 2, 0), dom - 1}), np.int64) + lo
            full = rng.choice(pool, pad)
        else:
            full = rng.integers(0, dom, pad, dtype=np.int64) + lo
            edge = rng.integers(0, max(n, 1), 4)
            full[edge] = np.array([lo, lo + dom - 1, lo, lo + dom - 1])
        full[n:] = np.where(np.arange(pad - n) % 2 == 0, lo, lo + dom - 1)   # the padding would lead in either direction
        self.kind, self.bits, self.base = kind, bits, lo & 0xFFFFFFFF
        self.raw = full[:n].copy()
        if kind == "i4":
            self.col = fd.Col(inp.gpu, full.astype(np.int32), 4, n)
        else:
            self.col = fd.Col(inp.gpu, full.astype(np.uint8 if kind == B else fd.DT[kind]), kind, n)
        inp.cache[("omf", tag, kind, bits, flavour)] = self.col      # freed with the inputs
        self.lcol = self.col                                         # what the list forms gather: bytes, never a plane
        if kind == B:
            self.lcol = inp.cache[("omf-bytes", tag, flavour)] = fd.Col(inp.gpu, full.astype(np.uint8), 1, n)


def shim_fields(fields, desc, listed=False, lift=0):
    out, shift = [], lift
    for f, d in reversed(list(zip(fields, desc))):
        out.append(((f.lcol if listed else f.col).c, f.base, f.bits, shift, d))
        shift += f.bits
    out.reverse()
    return out


def expected_order(rows, raws, desc):
    """rows (int64, duplicates allowed) ordered by the raw keys, each in its direction, ties by row."""
    cols = [rows]
    for raw, d in reversed(list(zip(raws, desc))):
        cols.append(-raw[rows] if d else raw[rows])
    return rows[np.lexsort(cols)]


class Harness:
    def __init__(self, n):
        self.gpu = fd.Gpu()
        self.inp = fd.Inputs(n, self.gpu)
        self.ids_out = self.gpu.ctx.malloc(4 * (2 * n + 64))
        self.fields = {}

    def close(self):
        KERNELS.update(self.gpu.kernels)
        self.gpu.ctx.sync()
        self.gpu.ctx.free(self.ids_out)
        self.inp.free()
        self.gpu.close()

    def layout(self, li, flavours):
        key = (li, tuple(flavours))
        if key not in self.fields:
            self.fields[key] = [Field(self.inp, (li, j), kind, bits, fl) for j, ((kind, bits), fl) in enumerate(zip(LAYOUTS[li], flavours))]
        return self.fields[key]

    def topk_rows(self, wide, k, m, what):
        """The rows of out[0 .. k): the first min(k, m) real, the rest all ones."""
        words = self.gpu.get(self.gpu.out, np.uint64, k * (2 if wide else 1))
        real = min(k, m)
        if wide:
            pairs = words.reshape(k, 2)
            assert (pairs[real:] == EMPTY).all(), (what, "empty slots")
            return pairs[:real, 1].astype(np.int64)
        assert (words[real:] == EMPTY).all(), (what, "empty slots")
        return (words[:real] & np.uint64(0xFFFFFFFF)).astype(np.int64)

    def run(self, pname, fields, desc, k, base, raws=None, lift=0):
        """One case through the three calls; raws: the keys the expectation orders by (default: the fields' own); lift: every
        field `lift` bits higher in the packed word (the order is the same, the key form may not be)."""
        gpu, inp, ctx = self.gpu, self.inp, self.gpu.ctx
        raws = raws or [f.raw for f in fields]
        sf = shim_fields(fields, desc, lift=lift)
        total = sum(f.bits for f in fields) + lift
        wide = total > 32
        nf = max(1, sum(1 for f in fields if f.bits))
        what = (inp.n, pname, [(f.kind, f.bits) for f in fields], desc, k, base)
        # the fused scan
        sel = inp.sel[pname].astype(np.int64)
        want = expected_order(sel, raws, desc) + base
        cols, n_cols, pred = inp.bound(pname)
        need = gpu.L.pqps_topk_scratch_bytes(ctx.h, inp.n, k, int(wide), 1)
        ctx.memset(gpu.out, 0, 16 * k)
        ctx.memset(gpu.words, 0xA5, 8)
        pq.check(pq.filter_topk_multi(ctx, cols, n_cols, inp.n, pred, sf, base, k, gpu.topk_scratch(need), need, gpu.out, gpu.words), what)
        gpu.fused(f"topk_pack_scan_kernel<{'pack64' if wide else 'pack32'}, NF={nf}, NT=?>", what)
        assert int(gpu.get(gpu.words, np.uint64, 1)[0]) == len(sel), (what, "count")
        got = self.topk_rows(wide, k, len(sel), what)
        assert np.array_equal(got, want[:k]), (what, "fused", got[:8], want[:8])
        # the same rows as a list, every seventh entry twice (a bit plane's rows from its byte twin)
        sf = shim_fields(fields, desc, listed=True, lift=lift)
        rows, _, ids_dev, _ = inp.id_list(pname, base)
        rows = rows.astype(np.int64)
        want_l = expected_order(rows, raws, desc) + base
        need = gpu.L.pqps_topk_scratch_bytes(ctx.h, len(rows), k, int(wide), 0)
        ctx.memset(gpu.out, 0, 16 * k)
        pq.check(pq.topk_list_multi(ctx, sf, ids_dev, len(rows), base, k, gpu.topk_scratch(need), need, gpu.out), what)
        got_l = self.topk_rows(wide, k, len(rows), what)
        assert np.array_equal(got_l, want_l[:k]), (what, "list", got_l[:8], want_l[:8])
        ctx.memset(self.ids_out, 0xEE, 4 * max(len(rows), 1))
        pq.check(pq.sort_list_multi(ctx, sf, ids_dev, len(rows), base, self.ids_out, gpu.out), what)
        got_s = gpu.get(self.ids_out, np.uint32, len(rows)).astype(np.int64)
        assert np.array_equal(got_s, want_l), (what, "sort", got_s[:8], want_l[:8])
        keys = gpu.get(gpu.out, np.uint64, len(rows))
        assert (np.diff(keys.astype(object)) >= 0).all() if len(rows) > 1 else True, (what, "sort keys ascending")
        # all three give one answer: without the duplicates the list is the selection
        uniq = got_s[np.concatenate([[True], got_s[1:] != got_s[:-1]])] if len(got_s) else got_s
        assert np.array_equal(uniq[:k], got[:k]), (what, "fused vs sort")


@pytest.fixture(scope="module", params=SIZES)
def harness(request):
    h = Harness(request.param)
    yield h
    h.close()


def layout_with(h, li, flavour_of):
    return h.layout(li, [flavour_of(j, len(LAYOUTS[li])) for j in range(len(LAYOUTS[li]))])


@pytest.mark.gpu
def test_layouts_directions_and_k(harness):
    """Every layout x DESC pattern; K, the WHERE and the row base take turns.  The last field is spread over its domain, the
    others hold a handful of values, so that every earlier key has long ties for the later ones to break."""
    h = harness
    turn = 0
    for li in range(len(LAYOUTS)):
        fields = layout_with(h, li, lambda j, nf: "random" if j == nf - 1 else "ties")
        wide = sum(f.bits for f in fields) > 32
        ks = KS_WIDE if wide else KS_NARROW
        for desc in desc_patterns(len(fields)):
            for _ in range(2):
                pname = ("all", "sparse", "dense")[turn % 3]
                base = (0, fd.HIGH_BASE)[(turn // 3) % 2]
                h.run(pname, fields, desc, ks[turn % len(ks)], base)
                turn += 1


@pytest.mark.gpu
def test_every_k_on_both_forms(harness):
    """Every K of the list on a PACK32 and a PACK64 layout, dense WHERE (K above the matches at the small sizes)."""
    h = harness
    for li, ks in ((2, KS_NARROW), (4, KS_WIDE)):
        fields = layout_with(h, li, lambda j, nf: "random" if j == nf - 1 else "ties")
        for i, k in enumerate(ks):
            desc = desc_patterns(len(fields))[i % (len(fields) + 2)]
            h.run("dense", fields, desc, k, 0)
            h.run("sparse", fields, desc, k, 5)


@pytest.mark.gpu
def test_one_field_in_the_high_word(harness):
    """One field placed above bit 32: the wide key with a single field (no key list of the engine's gives it, the shim allows it)."""
    h = harness
    fields = [Field(h.inp, "high", 2, 16, "random")]
    for desc, k in (((False,), 20), ((True,), 512)):
        h.run("dense", fields, desc, k, 0, lift=20)


@pytest.mark.gpu
def test_sort_list_chain(harness):
    """pqps_sort_list_chain: whole one-column keys (a signed i32, a u64, a u16), one stable sort per key; the rows against
    np.lexsort, the returned images ascending as (image 0, image 1, image 2, row)."""
    h, inp, gpu = harness, harness.inp, harness.gpu
    ctx = gpu.ctx
    a, c = Field(inp, "ch_a", "i4", 32, "ties"), Field(inp, "ch_c", 2, 16, "ties")
    pool = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)
    wide = inp.rng("ch_b").choice(pool, inp.pad)
    wcol = inp.cache[("omf", "ch_b")] = fd.Col(gpu, wide, 8, inp.n)
    wraw = np.unique(wide[:inp.n], return_inverse=True)[1].astype(np.int64)      # ranks: the unsigned order
    rows, _, ids_dev, _ = inp.id_list("dense", 5)
    rows = rows.astype(np.int64)
    m = len(rows)
    images = ctx.malloc(8 * 3 * max(m, 1))
    try:
        for desc in ((False, False, False), (True, False, True), (False, True, False), (True, True, True)):
            keys = [(a.col.c, 1, desc[0]), (wcol.c, 0, desc[1]), (c.col.c, 0, desc[2])]
            pq.check(pq.sort_list_chain(ctx, keys, ids_dev, m, 5, h.ids_out, images), ("chain", inp.n, desc))
            got = gpu.get(h.ids_out, np.uint32, m).astype(np.int64)
            assert np.array_equal(got, expected_order(rows, [a.raw, wraw, c.raw], desc) + 5), (inp.n, desc)
            img = gpu.get(images, np.uint64, 3 * m).reshape(3, m)
            tuples = list(zip(img[0].tolist(), img[1].tolist(), img[2].tolist(), got.tolist()))
            assert tuples == sorted(tuples), (inp.n, desc, "images")
        one = [(a.col.c, 1, 0)]
        plane = Field(inp, "ch_p", B, 1, "random")
        assert pq.sort_list_chain(ctx, [], ids_dev, m, 5, h.ids_out) == -1           # PQPS_EINVAL: 1 .. 4 keys
        assert pq.sort_list_chain(ctx, one * 5, ids_dev, m, 5, h.ids_out) == -1
        assert pq.sort_list_chain(ctx, [(plane.col.c, 0, 0)], ids_dev, m, 5, h.ids_out) == -1    # gathered by row: no bit plane
        assert pq.sort_list_chain(ctx, one, ids_dev, 0, 5, h.ids_out) == 0             # an empty list: nothing to do
    finally:
        ctx.sync()
        ctx.free(images)


@pytest.mark.gpu
def test_no_match(harness):
    h = harness
    for li in (1, 5):
        fields = layout_with(h, li, lambda j, nf: "ties")
        h.run("nothing", fields, (False,) * len(fields), 20, 0)
        h.run("nothing", fields, (True,) * len(fields), 512, 7)


@pytest.mark.gpu
def test_ties(harness):
    """All keys equal: the answer is the row order in both directions.  Ties in the first key only: the later keys decide."""
    h = harness
    for li in (1, 4, 5, 9):
        nf = len(LAYOUTS[li])
        fields = layout_with(h, li, lambda j, n: "equal")
        for desc in ((False,) * nf, (True,) * nf):
            h.run("dense", fields, desc, 64, 3)                          # (expected_order of equal keys is the row order)
        fields = layout_with(h, li, lambda j, n: "equal" if j == 0 else "random")
        for desc in desc_patterns(nf)[:3]:
            h.run("all", fields, desc, 65, 0)


@pytest.mark.gpu
def test_out_of_domain_values_are_clamped(harness):
    """A column whose values pass the field's domain on both sides: each is ordered as the field's last value, and no other
    field moves -- the expectation clamps the raw bins and never packs."""
    h = harness
    inp = h.inp
    lo_field = Field(inp, "clamp_a", 2, 10, "random")                    # u16 values 0 .. 1023, declared as 6 bits from base 100
    hi_field = Field(inp, "clamp_b", "i4", 7, "random")                  # i32 -50 .. 77, declared as 5 bits from base -40
    last = Field(inp, "clamp_c", 1, 8, "random")
    lo_field.base, lo_field.bits = 100, 6
    hi_field.base, hi_field.bits = (-40) & 0xFFFFFFFF, 5
    fields = [lo_field, hi_field, last]
    clamped = [np.minimum((lo_field.raw - 100) & 0xFFFFFFFF, 63), np.minimum((hi_field.raw + 40) & 0xFFFFFFFF, 31), last.raw]
    for desc in desc_patterns(3):
        h.run("all", fields, desc, 64, 0, raws=clamped)
        h.run("dense", fields, desc, 512, 0, raws=clamped)


@pytest.mark.gpu
def test_refused_arguments(harness):
    h, inp, gpu = harness, harness.inp, harness.gpu
    ctx = gpu.ctx
    cols, n_cols, pred = inp.bound("all")
    f4 = Field(inp, "ref4", 4, 32, "random")
    f1 = Field(inp, "ref1", 1, 8, "random")
    fb = Field(inp, "refb", B, 1, "random")
    rows, _, ids_dev, _ = inp.id_list("all", 0)
    need = gpu.L.pqps_topk_scratch_bytes(ctx.h, max(inp.n, len(rows)), 512, 1, 1) * 2 + (1 << 20)
    scratch = gpu.topk_scratch(need)

    def calls(sf, k=8):
        return (pq.filter_topk_multi(ctx, cols, n_cols, inp.n, pred, sf, 0, k, scratch, need, gpu.out, gpu.words),
                pq.topk_list_multi(ctx, sf, ids_dev, len(rows), 0, k, scratch, need, gpu.out),
                pq.sort_list_multi(ctx, sf, ids_dev, len(rows), 0, h.ids_out, None))

    c4, c1, cb = f4.col.c, f1.col.c, fb.col.c
    EINVAL = gpu.L.pqps_filter_topk_multi(None, None, 0, 0, None, None, 0, 0, 0, None, 0, None, None, None)
    assert EINVAL != 0
    assert calls([]) == (EINVAL,) * 3                                    # n_fields outside 1 .. 4
    assert calls([(c1, 0, 8, 8 * j, 0) for j in range(5)]) == (EINVAL,) * 3
    assert calls([(c4, 0, 32, 33, 0), (c4, 0, 32, 1, 0), (c1, 0, 1, 0, 0)]) == (EINVAL,) * 3     # 65 bits
    assert calls([(c4, 0, 33, 0, 0)]) == (EINVAL,) * 3                   # a field of more than 32 bits
    assert calls([(c4, 0, 16, 8, 0), (c1, 0, 9, 0, 0)]) == (EINVAL,) * 3 # overlapping fields
    assert calls([(c4, 0, 32, 40, 0)]) == (EINVAL,) * 3                  # past bit 64
    narrow, wide = [(c4, 0, 24, 8, 0), (c1, 0, 8, 0, 0)], [(c4, 0, 32, 8, 0), (c1, 0, 8, 0, 0)]
    assert calls(narrow, 1025)[:2] == (EINVAL,) * 2 and calls(narrow, 0)[:2] == (EINVAL,) * 2
    assert calls(wide, 513)[:2] == (EINVAL,) * 2
    plane = [(c1, 0, 8, 1, 0), (cb, 0, 1, 0, 0)]
    got = calls(plane)
    assert got[0] == 0 and got[1:] == (EINVAL,) * 2                      # a bit plane: the scan only
    assert calls(narrow, 1024) == (0, 0, 0) and calls(wide, 512) == (0, 0, 0)
    ctx.sync()


@pytest.mark.gpu
def test_every_match_beats_tau():
    """The worst case of the selection: over 8192 rows the first key falls as the rows rise, so under ASC every match in scan
    order beats the threshold so far and every compaction throws away what it kept."""
    h = Harness(8192)
    try:
        inp = h.inp
        first = Field(inp, "mono", 4, 13, "random")
        mono = (8191 - np.arange(inp.pad, dtype=np.int64)).clip(0)
        first.raw = mono[:inp.n].copy()
        first.col = first.lcol = fd.Col(inp.gpu, mono.astype(np.uint32), 4, inp.n)
        inp.cache[("omf", "mono2")] = first.col
        second = Field(inp, "mono_b", 2, 16, "random")
        for k in (64, 1024):
            h.run("all", [first, second], (False, False), k, 0)
            h.run("all", [second, first], (True, False), k, 0)
        wide = Field(inp, "mono_c", 4, 32, "random")
        for k in (65, 512):
            h.run("all", [first, wide], (False, True), k, 0)
    finally:
        h.close()


def test_zz_report_kernels():
    """Last in the file: the scan instances this process launched, for test_both_load_flavours' child runs (-s shows them)."""
    print()                                                      # (-q -s: the progress dots share the line)
    for name in sorted(KERNELS):
        print("KERNEL " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", ["0", "1"])
def test_both_load_flavours(nt):
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", __file__, "-k", "not both_load_flavours"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PQPS_NT_LOADS=nt), cwd=str(fd.q.ROOT))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "skipped" not in p.stdout
    flavour = "NT=true" if nt == "1" else "NT=false"
    kernels = {ln.split("KERNEL ", 1)[1].strip() for ln in p.stdout.splitlines() if "KERNEL " in ln}
    want = {f"topk_pack_scan_kernel<{form}, NF={nf}, {flavour}>" for form in ("pack32", "pack64") for nf in (1, 2, 3, 4)}
    assert kernels == want, (sorted(kernels), sorted(want))
