#!/usr/bin/env python3
"""Runs pqps_filter_digit_hist and pqps_digit_hist_list -- one pass of the radix select behind exact percentiles -- AT THE
SHIM in this process and exits non-zero on the first difference.

The engine reaches the two calls with planned key bits, exact bin ranges, zeroed padding and prefixes that hipQuantilePick
made; the contract of include/pqps_hip.h is wider.  This driver calls the shim through pq.lib() with inputs the engine cannot
produce and compares the raw device counts with a numpy reference computed from the uploaded arrays -- equality, no
tolerances.  The shim reads PQPS_NT_LOADS once per process, so tests/test_gpu_digit_hist_shim.py starts this script once per
setting; after every call pqps_last_kernel() must name the expected table home (LDS up to 16 384 counts, global memory
above), the key width, and for the fused form the load flavour of that setting.

    python tests/digit_hist_driver.py run [n ...]     on the GPU (default sizes + one size at which a wave of the LDS-full
                                                      grid takes a second step)
    python tests/digit_hist_driver.py --self-check    the references alone (no GPU): numpy against a row-by-row Python loop at
                                                      n = 1025, and that every declared shape occurs in the case list

Predicates, padding and ID lists are those of tests/fused_driver.py (its Inputs): no WHERE, SPARSE (whole steps without a
match), DENSE, NOTHING; columns padded to a multiple of 4096 rows, and the padding MATCHES every predicate with a key that is
in range and a group that is in range (the HOLE: a bin no real row uses, whose prefix slot is the padding key's) -- a wrong
trim of the partial last step changes a count.  Lists hold every seventh id twice (counted twice) and are cut by capacity.
"""
import ctypes as C
import sys

import numpy as np

import fused_driver as fd

pq = fd.pq
BIT, U64, TOP32 = fd.BIT, fd.U64, fd.TOP32
I32_MIN, I32_MAX = fd.I32_MIN, fd.I32_MAX
NONE = U64                                      # the prefix word of an unused slot
LDS_WORDS = 16384                               # kCountLdsBins: the tables' home switches above it
OUT_WORDS = 2000 * 2 * 256                      # the largest case
SKEW_KEY, SKEW_GROUP = 0x12345678, 3


def hole_for(groups):
    return groups // 3 + 1 if groups >= 6 else None


# ---- key columns: name -> (width, key_base as the shim takes it, key_bits, builder of the padded values) ---------------
def key_u8(rng, m):
    return rng.integers(0, 256, m).astype(np.uint8)


def key_u16(rng, m):
    a = rng.integers(0, 65536, m).astype(np.uint16)
    edges = np.array([0, 1, 31, 32, 2047, 2048, 65534, 65535], np.uint16)
    pick = rng.random(m) < 0.3
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return a


def key_u32(rng, m):
    a = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    edges = np.array(fd.SEVEN[4] + ((1 << 21) - 1, 1 << 21, (1 << 20) - 1, 1 << 20), np.uint32)
    pick = rng.random(m) < 0.5
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    small = rng.random(m) < 0.3
    a[small] = rng.integers(0, 1 << 20, int(small.sum())).astype(np.uint32)
    return a


def key_i32(rng, m):
    a = rng.integers(I32_MIN, I32_MAX, m, endpoint=True).astype(np.int32)
    edges = np.array(fd.SEVEN["i4"], np.int32)
    pick = rng.random(m) < 0.4
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return a


def key_i32w(rng, m):
    """[-50, 4045] is the 12-bit window above the base -50; the extremes and 4046 are outside it."""
    a = rng.integers(-50, 4046, m).astype(np.int32)
    edges = np.array([-50, -49, 4045, 4046, -51, I32_MIN, I32_MAX, 0], np.int32)
    pick = rng.random(m) < 0.3
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return a


def key_bit(rng, m):
    return (rng.random(m) < 0.4).astype(np.uint8)


def key_u64(rng, m):
    a = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m).astype(np.uint64)
    edges = np.array(fd.SEVEN[8] + ((1 << 32) + 1, (1 << 53) - 1, 1 << 53, (1 << 63) + (1 << 32)), np.uint64)
    pick = rng.random(m) < 0.5
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return a


def key_u64b(rng, m):
    """Base 5, 40 bits: values below 5 wrap to the top of the u64 range, values from 5 + 2^40 on have a bit above the key."""
    a = rng.integers(5, 5 + (1 << 40), m, dtype=np.uint64)
    edges = np.array([0, 4, 5, 6, 4 + (1 << 40), 5 + (1 << 40), 1 << 63, U64, (1 << 32) + 5], np.uint64)
    pick = rng.random(m) < 0.3
    a[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return a


def key_skew(rng, m):
    return np.full(m, SKEW_KEY, np.uint32)


KEYS = {"u8": (1, 0, 8, key_u8), "u16": (2, 0, 16, key_u16), "u32": (4, 0, 32, key_u32), "u32n": (4, 0, 20, key_u32),
        "i32": (4, I32_MIN & TOP32, 32, key_i32), "i32w": (4, (-50) & TOP32, 12, key_i32w), "bit": (BIT, 0, 1, key_bit),
        "u64": (8, 0, 64, key_u64), "u64b": (8, 5, 40, key_u64b), "skew": (4, 0, 32, key_skew)}


def is_wide(cfg):
    return KEYS[cfg["key"]][0] == 8


def key_column(inp, cfg):
    name = cfg["key"]
    if ("key", name) not in inp.cache:
        width, base, _, build = KEYS[name]
        a = build(inp.rng(("digit key", name)), inp.pad)
        unsigned = np.uint8 if width == BIT else fd.DT[width]
        a[inp.n:] = np.array([(base + 1) & (U64 if width == 8 else TOP32)], dtype=unsigned).view(a.dtype)[0]   # padding: image 1
        inp.cache[("key", name)] = fd.Col(inp.gpu, a, width, inp.n)
    return inp.cache[("key", name)]


def group_column(inp, cfg):
    """Values 0 .. groups + 1 (the last two are past every window) without the hole; the padding is the hole (or bin 0)."""
    if cfg["grp"] is None:
        return None
    width, groups = cfg["grp"], cfg["groups"]
    key = ("digit group", width, groups, cfg["key"] == "skew")
    if key not in inp.cache:
        rng, hole = inp.rng(key), hole_for(groups)
        top = 1 if width == BIT else groups + 1
        a = rng.integers(0, top + 1, inp.pad)
        if cfg["key"] == "skew":
            a[:] = SKEW_GROUP
        if hole is not None:
            a[a == hole] = 0
        a[inp.n:] = hole if hole is not None else 0
        inp.cache[key] = fd.Col(inp.gpu, a.astype(np.uint8 if width in (1, BIT) else fd.DT[width]), width, inp.n)
    return inp.cache[key]


def window(cfg):
    """(bin_base, n_bins): the whole range, or one that cuts two groups off at either end."""
    if cfg["grp"] is None:
        return 0, 1
    return (2, cfg["groups"] - 4) if cfg.get("window") else (0, cfg["groups"])


# ---- the definition, twice ------------------------------------------------------------------------------------------------
def images_of(col, cfg, rows):
    _, base, _, _ = KEYS[cfg["key"]]
    if col.width == 8:
        return col.u[rows] - np.full(len(rows), base, np.uint64)        # wraps mod 2^64
    return ((col.u[rows].astype(np.int64) - base) % (1 << 32)).astype(np.uint64)


def bins_of_rows(inp, cfg, rows):
    grp = group_column(inp, cfg)
    bin_base, n_bins = window(cfg)
    if grp is None:
        return np.zeros(len(rows), np.int64), n_bins
    return (grp.u[rows].astype(np.int64) - bin_base) % (1 << 32), n_bins


def prefixes_of(inp, cfg):
    """[n_bins][Q] u64, or None on the first pass: per group up to Q (Q - 1 where `unused`) of the upper parts its real rows
    hold, spread over what there is, ascending; the hole's first slot is the padding key's upper part; the rest all ones."""
    q = cfg["slots"]
    if not cfg["prefix"]:
        return None
    key = ("digit prefix",) + tuple(sorted((k, str(v)) for k, v in cfg.items() if k not in ("form", "cap", "id_base", "preds")))
    if key in inp.memo:
        return inp.memo[key]
    _, _, bits, _ = KEYS[cfg["key"]]
    rows = np.arange(inp.n)
    img = images_of(key_column(inp, cfg), cfg, rows)
    t0, n_bins = bins_of_rows(inp, cfg, rows)
    ok = (t0 < n_bins) & ((img >> np.uint64(bits) == 0) if bits < 64 else True)
    upper = img >> np.uint64(cfg["shift"] + cfg["d"])
    out = np.full((n_bins, q), NONE, np.uint64)
    order = np.lexsort((upper[ok], t0[ok]))
    gs, us = t0[ok][order], upper[ok][order]
    first = np.r_[True, (gs[1:] != gs[:-1]) | (us[1:] != us[:-1])] if len(gs) else np.zeros(0, bool)
    gs, us = gs[first], us[first]
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if len(gs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(gs)]
    take = q - 1 if cfg.get("unused") and q > 1 else q
    for a, b in zip(starts, ends):
        have = us[a:b]
        pick = have if len(have) <= take else have[np.unique(np.linspace(0, len(have) - 1, take).astype(np.int64))]
        out[int(gs[a]), :len(pick)] = pick
    hole = hole_for(cfg["groups"]) if cfg["grp"] is not None else None
    if hole is not None and 0 <= hole - window(cfg)[0] < n_bins:
        out[hole - window(cfg)[0], 0] = np.uint64(1) >> np.uint64(cfg["shift"] + cfg["d"])
    inp.memo[key] = out
    return out


def words_of(cfg):
    return (window(cfg)[1] * cfg["slots"]) << cfg["d"]


def digit_reference(inp, cfg, pname):
    rows = fd.case_rows(inp, cfg, pname)
    _, _, bits, _ = KEYS[cfg["key"]]
    shift, d, q = cfg["shift"], cfg["d"], cfg["slots"]
    img = images_of(key_column(inp, cfg), cfg, rows)
    t0, n_bins = bins_of_rows(inp, cfg, rows)
    ok = t0 < n_bins
    if bits < 64:
        ok &= (img >> np.uint64(bits)) == 0
    t = np.where(ok, t0, 0)
    prefix = prefixes_of(inp, cfg)
    if prefix is not None:
        upper, flat, found = img >> np.uint64(shift + d), prefix.reshape(-1), np.full(len(rows), -1, np.int64)
        for j in range(q):
            hit = ok & (flat[t * q + j] == upper)
            found[hit] = (t * q + j)[hit]
        ok &= found >= 0
        t = np.where(ok, found, 0)
    digit = ((img >> np.uint64(shift)) & np.uint64((1 << d) - 1)).astype(np.int64)
    return {"tables": np.bincount(((t << d) | digit)[ok], minlength=words_of(cfg)).astype(np.uint32)}


def digit_slow(inp, cfg, pname):
    """Row by row, in Python ints, from the words of the header."""
    width, base, bits, _ = KEYS[cfg["key"]]
    shift, d, q = cfg["shift"], cfg["d"], cfg["slots"]
    key, grp = key_column(inp, cfg).real.tolist(), group_column(inp, cfg)
    groups = grp.real.tolist() if grp is not None else None
    bin_base, n_bins = window(cfg)
    prefix = prefixes_of(inp, cfg)
    prefix = None if prefix is None else [int(x) for x in prefix.reshape(-1)]
    rows = fd.list_rows(inp, cfg, pname).tolist() if cfg["form"] == "list" else \
        [r for r in range(inp.n) if fd.pred_row(pname, int(inp.p[r]), int(inp.b[r]))]
    out = [0] * words_of(cfg)
    for r in rows:
        image = (key[r] - base) & (U64 if width == 8 else TOP32)
        b = (groups[r] - bin_base) & TOP32 if groups is not None else 0
        if image >> bits or b >= n_bins:
            continue
        t = b
        if prefix is not None:
            slots = [j for j in range(q) if prefix[b * q + j] == image >> (shift + d)]
            if not slots:
                continue
            assert len(slots) == 1, "the slots of one group hold distinct prefixes"
            t = b * q + slots[0]
        out[(t << d) | ((image >> shift) & ((1 << d) - 1))] += 1
    return {"tables": np.array(out, dtype=np.uint32)}


# ---- the cases --------------------------------------------------------------------------------------------------------------
def cfg(key, shift, d, grp=None, groups=1, slots=1, prefix=False, **more):
    return dict(form="scan", key=key, shift=shift, d=d, grp=grp, groups=groups, slots=slots, prefix=prefix or slots > 1, **more)


def scan_configs(big):
    if big:                                                     # the LDS-full table: 2 workgroups per CU, a second step per wave
        return [cfg("u16", 5, 11, grp=1, groups=8, preds=("dense",))]
    return [
        cfg("u8", 0, 8), cfg("u8", 7, 1), cfg("bit", 0, 1), cfg("bit", 0, 1, grp=BIT, groups=2),
        cfg("u16", 5, 11, grp=1, groups=8), cfg("u16", 5, 11, grp=1, groups=9),                 # 8 / 9 tables of 11 bits
        cfg("u16", 0, 5, grp=1, groups=8, slots=2, unused=True),
        cfg("u32", 24, 8, grp=2, groups=64), cfg("u32", 24, 8, grp=2, groups=65),               # 64 / 65 tables of 8 bits
        cfg("u32", 21, 11), cfg("u32", 11, 8, slots=16), cfg("u32", 0, 11, slots=2), cfg("u32n", 9, 11, grp=4, groups=12, window=True),
        cfg("i32", 21, 11), cfg("i32", 0, 8, grp=1, groups=8, window=True, slots=2), cfg("i32w", 1, 11, grp=BIT, groups=2),
        cfg("i32w", 0, 1, slots=16, unused=True),
        cfg("u64", 53, 11), cfg("u64", 21, 11, slots=16), cfg("u64", 0, 8, grp=1, groups=12, window=True, slots=2),
        cfg("u64", 11, 1, prefix=True), cfg("u64b", 29, 11), cfg("u64b", 0, 8, grp=2, groups=70, slots=2),
        cfg("u16", 0, 8, grp=2, groups=2000, slots=2, window=True),                             # 2000 groups x 2 slots (1996 in the window)
        cfg("skew", 21, 11, grp=1, groups=8), cfg("skew", 0, 8, grp=1, groups=65, slots=1, prefix=True),
    ]


def list_configs():
    out = []
    for i, c in enumerate(c for c in scan_configs(False) if KEYS[c["key"]][0] != BIT and c["grp"] != BIT):
        out.append(dict(c, form="list", cap=fd.LIST_CAPS[i % 3], id_base=fd.HIGH_BASE if i % 2 else 0, preds=("sparse", "dense", "nothing")))
    return out


def configs(big):
    return scan_configs(big) + ([] if big else list_configs())


def kernel_name(cfg):
    home = "DIGIT_LDS" if words_of(cfg) <= LDS_WORDS else "DIGIT_GLOBAL"
    width = "u64" if is_wide(cfg) else "u32"
    return f"digit_scan_kernel<{home}, {width}, NT=?>" if cfg["form"] == "scan" else f"digit_list_kernel<{home}, {width}>"


def execute(gpu, inp, cfg, pname, what):
    L, ctx = gpu.L, gpu.ctx
    _, base, bits, _ = KEYS[cfg["key"]]
    key, grp = key_column(inp, cfg), group_column(inp, cfg)
    bin_base, n_bins = window(cfg)
    prefix, words = prefixes_of(inp, cfg), words_of(cfg)
    pdev = gpu.put(prefix.reshape(-1)) if prefix is not None else None
    ctx.memset(gpu.digit_out, 0xA5, 4 * words)                  # the call zeroes its tables
    if cfg["form"] == "scan":
        cols, nc, pred = inp.bound(pname)
        pq.check(L.pqps_filter_digit_hist(ctx.h, cols, nc, inp.n, pred, key.ref(), int(is_wide(cfg)), base, bits, grp.ref() if grp else None,
                                          bin_base, n_bins, cfg["slots"], pdev, cfg["shift"], cfg["d"], gpu.digit_out, None), what)
        gpu.fused(kernel_name(cfg), what)
    else:
        rows, _, ids, count = inp.id_list(pname, cfg["id_base"])
        cap = fd.list_capacity(cfg, len(rows))
        pq.check(L.pqps_digit_hist_list(ctx.h, key.ref(), int(is_wide(cfg)), base, bits, grp.ref() if grp else None, bin_base, n_bins,
                                        cfg["slots"], pdev, cfg["shift"], cfg["d"], inp.n, ids, count, cap, cfg["id_base"],
                                        gpu.digit_out, None), what)
        got = L.pqps_last_kernel().decode()
        if cap and got != kernel_name(cfg):
            fd.fail(f"kernel: {what}: ran {got}, expected {kernel_name(cfg)}")
    out = {"tables": gpu.get(gpu.digit_out, np.uint32, words)}
    if pdev:
        ctx.free(pdev)
    return out


def run_case(gpu, inp, n, cfg, pname, slow):
    what = f"digit n={n} pred={pname} " + " ".join(f"{k}={v}" for k, v in cfg.items() if k != "preds")
    want = digit_reference(inp, cfg, pname)
    if gpu:
        fd.compare(what, execute(gpu, inp, cfg, pname, what), want)
    elif slow:
        fd.compare(what + " (row by row)", digit_slow(inp, cfg, pname), want)


def sweep(gpu, sizes, big):
    cases = 0
    for n in sizes + ([big] if big else []):
        inp = fd.Inputs(n, gpu)
        for c in configs(n == big):
            for pname in c.get("preds", fd.PRED_NAMES):
                run_case(gpu, inp, n, c, pname, n == fd.SLOW_N)
                cases += 1
        inp.free()
        print(f"digit: n={n} ok", flush=True)
    return cases


def planned_cases(sizes=len(fd.DEFAULT_SIZES), big=True):
    count = lambda cs: sum(len(c.get("preds", fd.PRED_NAMES)) for c in cs)
    return sizes * count(configs(False)) + (count(configs(True)) if big else 0)


SCAN_KERNELS = 4                                # {LDS, GLOBAL} x {u32, u64} per load flavour


def check_plans():
    scans, lists = scan_configs(False), list_configs()
    names = {kernel_name(c) for c in scans}
    assert len(names) == SCAN_KERNELS and {kernel_name(c) for c in lists} == {n.replace("scan", "list").replace(", NT=?", "") for n in names}
    tables = {(window(c)[1] * c["slots"], c["d"]) for c in scans}
    assert tables >= {(1, 11), (8, 11), (9, 11), (64, 8), (65, 8), (1996 * 2, 8)}
    assert [kernel_name(cfg("u32", 24, 8, grp=2, groups=g)) for g in (64, 65)] == ["digit_scan_kernel<DIGIT_LDS, u32, NT=?>", "digit_scan_kernel<DIGIT_GLOBAL, u32, NT=?>"]
    assert [words_of(cfg("u16", 5, 11, grp=1, groups=g)) for g in (8, 9)] == [16384, 18432]
    assert {c["d"] for c in scans} >= {1, 8, 11} and {c["shift"] for c in scans} >= {0, 11, 21, 53}
    assert {c["slots"] for c in scans} == {1, 2, 16} and any(c.get("unused") for c in scans) and any(c.get("window") for c in scans)
    assert {c["key"] for c in scans} == set(KEYS) and {c["grp"] for c in scans} == {None, 1, 2, 4, BIT}
    assert all(c["shift"] + c["d"] <= KEYS[c["key"]][2] and words_of(c) <= OUT_WORDS for c in scans)
    assert {c["cap"] for c in lists} == set(fd.LIST_CAPS) and {c["id_base"] for c in lists} == {0, fd.HIGH_BASE}
    assert any(is_wide(c) for c in lists) and any(c["slots"] == 16 for c in lists) and any(c["key"] == "skew" for c in lists)


def check_inputs():
    for n in fd.DEFAULT_SIZES:
        inp = fd.Inputs(n, None)
        for c in scan_configs(False):
            width, base, bits, _ = KEYS[c["key"]]
            key, grp = key_column(inp, c), group_column(inp, c)
            img = images_of(key, c, np.arange(n))
            if n >= 1023 and bits < (64 if width == 8 else 32) and c["key"] not in ("bit", "u8", "u16"):
                assert (img >> np.uint64(bits) != 0).any(), (n, c["key"], "an image at or above 2^key_bits must occur")
            if n < inp.pad:                                      # the padding would count: image 1, the hole (or bin 0)
                pad_img = images_of(fd.Col(None, key.full[n:], key.width, inp.pad - n), c, np.arange(inp.pad - n))
                assert (pad_img == 1).all()
                if grp is not None:
                    hole = hole_for(c["groups"])
                    assert (grp.full[n:] == (hole if hole is not None else 0)).all() and (hole is None or hole not in grp.real)
            prefix = prefixes_of(inp, c)
            if prefix is not None:
                for row in prefix:
                    used = row[row != NONE]
                    assert len(set(used.tolist())) == len(used), "distinct prefixes per group"
                if c.get("unused") and c["slots"] > 1:
                    assert (prefix[:, -1] == NONE).all()
        u64 = key_column(inp, cfg("u64", 53, 11)).real
        if n >= 1023:
            assert all((u64 == np.uint64(v)).any() for v in ((1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63))
            i32 = key_column(inp, cfg("i32", 21, 11)).real
            assert (i32 == I32_MIN).any() and (i32 == I32_MAX).any()
            skew = digit_reference(inp, cfg("skew", 21, 11, grp=1, groups=8), "dense")["tables"]
            assert np.count_nonzero(skew) == 1 and skew.max() == len(inp.sel["dense"])       # all 64 lanes on one counter


def self_check(sizes=fd.DEFAULT_SIZES):
    check_plans()
    check_inputs()
    cases = sweep(None, list(sizes), None)
    assert cases == planned_cases(len(sizes), big=False) > 0, cases
    print(f"digit: {cases} cases", flush=True)


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in ("run", "--self-check"):
        sys.exit("usage: digit_hist_driver.py run [n ...]  |  digit_hist_driver.py --self-check")
    if sys.argv[1] == "--self-check":
        self_check()
        print("OK")
        return
    gpu = fd.Gpu()
    gpu.digit_out = gpu.ctx.malloc(4 * OUT_WORDS + 64)
    sizes = [int(x) for x in sys.argv[2:]]
    # the smallest table at which a wave of the LDS-full grid (2 workgroups of 4 waves per CU) takes a second step
    big = None if sizes else fd.STEP * (4 * 2 * gpu.cus + 1) + 3
    cases = sweep(gpu, sizes or fd.DEFAULT_SIZES, big)
    gpu.close()
    assert cases == planned_cases(len(sizes or fd.DEFAULT_SIZES), big is not None), (cases, "no case may be skipped")
    print(f"digit: {gpu.nt} cases={cases} kernels={len(gpu.kernels)}")
    for name in sorted(gpu.kernels):
        print("  " + name)
    print("OK")


if __name__ == "__main__":
    main()
