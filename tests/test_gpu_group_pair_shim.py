"""pqps_filter_group_pair, pqps_group_pair_list and pqps_group_pair_sort called at the shim on inputs the engine never sends,
the way tests/test_gpu_fused_variants.py calls the other four families: under both load flavours -- each in its own process,
because the shim reads PQPS_NT_LOADS once (this file is its own driver: `python test_gpu_group_pair_shim.py run`) -- with
the tables, predicates and padding of tests/fused_driver.py (rows in the readable padding match every predicate and carry
in-range bins), and compared word for word with numpy over the uploaded arrays.

  * n in {1, 1025, 300 001}; no WHERE, a sparse, a dense and an empty selection
  * group columns 1, 2 and 4 bytes wide in both positions, the bit plane as A and as B, a signed column with a non-zero base
    (values below the base wrap out of range), n_b that is no power of two, rows whose bin_a or bin_b is out of range
  * both sides of the LDS limits (16 384 bins without a value, 2 304 with one) and the dense cap; after every fused call
    pqps_last_kernel() names the expected instance and this process's load flavour
  * n_a x n_b of 0 or over 65 536 returns PQPS_EINVAL from the dense calls; the sort call takes 65 536 x 65 536
  * the list call with *count_dev above and below its capacity, an id_base at the top of u32, a listed row past n_rows
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_driver as fd
import qpelib as q

pq = q.pq
BIT = fd.BIT
U64 = fd.U64
SIZES = (1, 1025, 300_001)
VALS = (None, "val_i32", "val_u64")
VAL_NAME = {None: "PAIR_COUNT", "val_i32": "PAIR_I32", "val_u64": "PAIR_U64"}
# (A column, a_base, n_a, B column, b_base, n_b)
SCAN_SHAPES = (
    (("dom", 1), 0, 256, ("grp18", 2), 0, 16),          # 4 096
    (("dom", 2), 0, 1024, ("grp18", 4), 0, 16),         # 16 384: the last LDS histogram
    (("dom", 2), 0, 1025, ("grp18", 1), 0, 16),         # 16 400: global bins
    (("dom", 4), 0, 4096, ("grp18", 1), 0, 16),         # 65 536: the dense cap
    (("dom", 4), 0, 144, ("grp18", 2), 0, 16),          # 2 304: the last LDS table
    (("dom", 1), 0, 145, ("grp18", 4), 0, 16),          # 2 320
    (("dom", 2), 0, 700, ("grp18", 1), 2, 13),          # n_b no power of two, B below its base wraps out
    (("dom_s4",), fd.SBASE, 2000, ("grp18", 2), 0, 18), # a signed A with a base
    (("dom", BIT), 0, 2, ("dom", 2), 0, 1000),          # the bit plane as A
    (("dom", 1), 0, 200, ("grp18", BIT), 0, 2),         # ... as B
    (("grp18", BIT), 0, 1, ("dom", BIT), 0, 2),         # ... as both, bin_a = 1 out of range
    (("grp18", 4), 0, 18, ("dom", 4), 0, 3000),         # 4 bytes as B
)
LIST_SHAPES = tuple(s for s in SCAN_SHAPES if BIT not in (s[0][-1], s[3][-1]))
SORT_SHAPES = LIST_SHAPES[:3] + ((("dom", 4), 0, 65536, ("dom", 2), 0, 65536), (("dom_s4",), fd.SBASE, 65536, ("dom", 4), 0, 65536),
                                 (("dom", 2), 0, 40000, ("grp18", 1), 2, 13))
BAD_SHAPES = ((0, 5), (5, 0), (65536, 2), (65537, 1), (1, 65537), (257, 256))


def planned_cases():
    return len(SIZES) * len(VALS) * len(fd.PRED_NAMES) * (len(SCAN_SHAPES) + len(LIST_SHAPES) + len(SORT_SHAPES)) + len(BAD_SHAPES) * 2 + 1


def path_of(D, val):
    return "PAIR_LDS" if D <= (16384 if val is None else 2304) else "PAIR_GLOBAL"


def pair_bins(inp, shape, rows):
    """(bin_a, bin_b, in range) of the rows."""
    ca, a0, na, cb, b0, nb = shape
    ba, bb = fd.bins_of(inp.column(ca), a0, rows), fd.bins_of(inp.column(cb), b0, rows)
    return ba, bb, (ba < na) & (bb < nb)


def dense_reference(inp, shape, val, rows):
    na, nb = shape[2], shape[5]
    D = na * nb
    ba, bb, ok = pair_bins(inp, shape, rows)
    d = (ba * nb + bb)[ok]
    if val is None:
        return np.bincount(d, minlength=D).astype(np.uint32)
    wide, img = fd.agg_wide_image(inp.column((val,)), rows)
    out = np.zeros(4 * D, dtype=np.uint64)
    out[2 * D:3 * D] = U64
    out[:D] = np.bincount(d, minlength=D)
    np.add.at(out[D:2 * D], d, wide[ok])
    np.minimum.at(out[2 * D:3 * D], d, img[ok])
    np.maximum.at(out[3 * D:], d, img[ok])
    return out


def sort_reference(inp, shape, val, rows):
    """The compact runs: keys, counts [, sums, min images, max images], concatenated."""
    ba, bb, ok = pair_bins(inp, shape, rows)
    keys = ((ba.astype(np.uint64) << np.uint64(32)) | bb.astype(np.uint64))[ok]
    uniq, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    fields = [uniq, counts.astype(np.uint64)]
    if val is not None:
        wide, img = fd.agg_wide_image(inp.column((val,)), rows)
        s, lo, hi = np.zeros(len(uniq), np.uint64), np.full(len(uniq), U64, np.uint64), np.zeros(len(uniq), np.uint64)
        np.add.at(s, inv, wide[ok])
        np.minimum.at(lo, inv, img[ok])
        np.maximum.at(hi, inv, img[ok])
        fields += [s, lo, hi]
    return np.concatenate(fields) if len(uniq) else np.zeros(0, np.uint64)


def run():
    gpu = fd.Gpu()
    L, ctx = gpu.L, gpu.ctx
    out = ctx.malloc(4 * 65536 * 8 + 64)
    cases = 0
    for n in SIZES:
        inp = fd.Inputs(n, gpu)
        lists = {}
        for k, pname in enumerate(fd.PRED_NAMES):
            # the matching rows, every seventh twice, shuffled, then a row past n_rows (skipped) and one more real row
            rows = inp.sel[pname]
            rows = inp.rng(("pairlist", pname)).permutation(np.concatenate([rows, rows[::7]]))
            listed = np.concatenate([rows, [n + 3], rows[:1]]).astype(np.int64)
            base = fd.HIGH_BASE if k % 2 else 0
            lists[pname] = (listed, base, gpu.put((listed + base).astype(np.uint32)), gpu.put(np.array([len(listed)], dtype=np.uint64)))
        for val in VALS:
            vref = inp.column((val,)).ref() if val else None
            for shape in SCAN_SHAPES:
                ca, a0, na, cb, b0, nb = shape
                D = na * nb
                words, dt = (D, np.uint32) if val is None else (4 * D, np.uint64)
                for pname in fd.PRED_NAMES:
                    what = f"pair scan n={n} val={val} pred={pname} shape={shape}"
                    ctx.memset(out, 0xA5, words * np.dtype(dt).itemsize)               # the call initialises its output
                    cols, nc, pred = inp.bound(pname)
                    pq.check(L.pqps_filter_group_pair(ctx.h, cols, nc, n, pred, inp.column(ca).ref(), a0, na, inp.column(cb).ref(), b0, nb,
                                                      vref, out, None), what)
                    gpu.fused(f"pair_scan_kernel<{path_of(D, val)}, {VAL_NAME[val]}, NT=?>", what)
                    fd.compare(what, {"out": gpu.get(out, dt, words)}, {"out": dense_reference(inp, shape, val, inp.sel[pname])})
                    cases += 1
            for i, shape in enumerate(LIST_SHAPES):
                ca, a0, na, cb, b0, nb = shape
                D = na * nb
                words, dt = (D, np.uint32) if val is None else (4 * D, np.uint64)
                for j, pname in enumerate(fd.PRED_NAMES):
                    listed, base, ids, count = lists[pname]
                    cap = (len(listed) // 2, len(listed), len(listed) + 5)[(i + j) % 3]       # *count_dev above / at / below the capacity
                    what = f"pair list n={n} val={val} pred={pname} cap={cap}/{len(listed)} shape={shape}"
                    ctx.memset(out, 0xA5, words * np.dtype(dt).itemsize)
                    pq.check(L.pqps_group_pair_list(ctx.h, inp.column(ca).ref(), a0, na, inp.column(cb).ref(), b0, nb, vref, n, ids, count,
                                                    cap, base, out, None), what)
                    rows = listed[:cap]
                    fd.compare(what, {"out": gpu.get(out, dt, words)}, {"out": dense_reference(inp, shape, val, rows[rows < n])})
                    cases += 1
            for shape in SORT_SHAPES:
                ca, a0, na, cb, b0, nb = shape
                for pname in fd.PRED_NAMES:
                    listed, base, ids, _ = lists[pname]
                    what = f"pair sort n={n} val={val} pred={pname} shape={shape}"
                    runs_dev, n_runs = C.c_void_p(), C.c_uint64(12345)
                    pq.check(L.pqps_group_pair_sort(ctx.h, inp.column(ca).ref(), a0, na, inp.column(cb).ref(), b0, nb, vref, n, ids, len(listed),
                                                    base, C.byref(runs_dev), C.byref(n_runs), None), what)
                    want = sort_reference(inp, shape, val, listed[listed < n])
                    fields = 2 if val is None else 5
                    if n_runs.value * fields != len(want) or bool(runs_dev.value) != bool(len(want)):
                        fd.fail(f"{what}: {n_runs.value} runs, expected {len(want) // fields}")
                    fd.compare(what, {"runs": gpu.get(runs_dev, np.uint64, len(want))}, {"runs": want})
                    if runs_dev.value:
                        ctx.free(runs_dev)
                    cases += 1
        if n == SIZES[-1]:
            a, b = inp.column(("dom", 2)).ref(), inp.column(("grp18", 1)).ref()
            cols, nc, pred = inp.bound("dense")
            listed, base, ids, count = lists["dense"]
            for na, nb in BAD_SHAPES:
                for rc in (L.pqps_filter_group_pair(ctx.h, cols, nc, n, pred, a, 0, na, b, 0, nb, None, out, None),
                           L.pqps_group_pair_list(ctx.h, a, 0, na, b, 0, nb, None, n, ids, count, len(listed), base, out, None)):
                    if rc != -1:                                 # PQPS_EINVAL
                        fd.fail(f"{na} x {nb} bins: rc {rc}, expected PQPS_EINVAL")
                    cases += 1
            runs_dev, n_runs = C.c_void_p(), C.c_uint64()
            if L.pqps_group_pair_sort(ctx.h, a, 0, 0, b, 0, 5, None, n, ids, len(listed), base, C.byref(runs_dev), C.byref(n_runs), None) != -1:
                fd.fail("sort with n_a = 0: expected PQPS_EINVAL")
            cases += 1
        for _, _, ids, count in lists.values():
            ctx.free(ids)
            ctx.free(count)
        inp.free()
        print(f"pair: n={n} ok", flush=True)
    ctx.free(out)
    gpu.close()
    assert cases == planned_cases(), (cases, planned_cases())
    print(f"pair: {gpu.nt} cases={cases} kernels={len(gpu.kernels)}")
    for name in sorted(gpu.kernels):
        print("  " + name)
    print("OK")


@pytest.mark.gpu
@pytest.mark.parametrize("nt", ["0", "1"])
def test_pair_calls_at_the_shim(nt):
    p = subprocess.run([sys.executable, __file__, "run"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PQPS_NT_LOADS=nt), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    flavour = "NT=true" if nt == "1" else "NT=false"
    kernels = [ln.strip() for ln in p.stdout.splitlines() if ln.startswith("  ")]
    # both paths of all three value forms ran, in this flavour and in no other
    assert len(kernels) == len(set(kernels)) == 6 and all(flavour in k for k in kernels), kernels
    assert f"cases={planned_cases()} " in p.stdout


def test_shim_shapes_cover_the_path_switches():
    """CPU: the case lists hold both sides of every switch and every width in both positions."""
    ds = {s[2] * s[5] for s in SCAN_SHAPES}
    assert {16384, 16400, 65536, 2304, 2320} <= ds and max(ds) == 65536
    assert {path_of(d, None) for d in ds} == {path_of(d, "val_i32") for d in ds} == {"PAIR_LDS", "PAIR_GLOBAL"}
    for pos in (0, 3):
        assert {s[pos][-1] for s in SCAN_SHAPES if s[pos][0] != "dom_s4"} == {1, 2, 4, BIT}
        assert {s[pos][-1] for s in LIST_SHAPES if s[pos][0] != "dom_s4"} == {1, 2, 4}
    assert any(s[2] * s[5] == 1 << 32 for s in SORT_SHAPES) and all(a * b == 0 or a * b > 65536 or max(a, b) > 65536 for a, b in BAD_SHAPES)


if __name__ == "__main__":
    run()
