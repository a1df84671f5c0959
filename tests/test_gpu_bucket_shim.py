"""pqps_filter_group_buckets, pqps_group_buckets_list, pqps_filter_aggregate_buckets and pqps_aggregate_buckets_list called at
the shim, the way tests/test_gpu_group_pair_shim.py calls its family: under both load flavours -- each in its own process,
because the shim reads PQPS_NT_LOADS once (this file is its own driver: `python test_gpu_bucket_shim.py run N`) -- with the
predicates and padding of tests/fused_driver.py (rows in the readable padding match every predicate and carry an in-range
code), and compared word for word with numpy over the uploaded arrays: the bucket of a row is
numpy.searchsorted(bounds, bin, 'right') - 1, the counts numpy.bincount, the fields ufunc.at.  Nothing expected comes from the
library.

  * n in {1, 1023, 1024, 1025, 4097, 300 001}: the partial last step, one wave, one workgroup, several workgroups
  * group columns 1, 2 and 4 bytes wide, a signed column with a non-zero bin base; codes >= the domain are present and left out
  * 1, 2, 16, 17 buckets, both sides of every path limit (2047 | 2048 with a value, 8191 | 8192 without, 16 383 | 16 384 for
    the bounds in LDS) and 65 536; bounds with one code per bucket, with one bucket holding the whole domain, and random runs
  * no WHERE, a sparse, a dense and an empty selection, and one match in the last row
  * value columns: i32 with negatives, INT_MIN and INT_MAX; u64 above 2^63
  * the list calls over an ascending list, a shuffled one with duplicates and a row past n_rows, *count above, at and below
    the capacity, an id_base at the top of u32
  * after every fused call pqps_last_kernel() names the expected instance and this process's load flavour
  * n_buckets 0 or above 65 536, NULL bounds and a domain of 0 return PQPS_EINVAL from all four calls
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
U64 = fd.U64
SIZES = (1, 1023, 1024, 1025, 4097, 300_001)
VALS = (None, "val_i32", "val_u64")
VAL_NAME = {"val_i32": "i32", "val_u64": "u64"}
PREDS = fd.PRED_NAMES + ("last",)
SMALL, COUNT_LDS, AGG_LDS, BOUNDS_LDS, MAX = 16, 8191, 2047, 16383, 65536     # the limits of csrc/bins_kernels.hpp
# (group column width, buckets, kind, domain): "unit" one code per bucket, "whole" one bucket over the domain, "runs" random runs
SHAPES = (
    (1, 1, "whole", 200), (2, 1, "whole", 65536), (4, 1, "whole", 1 << 31),
    (1, 2, "runs", 256), (2, 2, "unit", 2),
    (2, 16, "unit", 16), (1, 16, "runs", 250), (4, 17, "unit", 17), (4, 17, "runs", 70000),
    ("s4", 17, "runs", 2000),
    (2, 2047, "unit", 2047), (4, 2048, "unit", 2048), (2, 2047, "runs", 60000),
    (4, 8191, "unit", 8191), (2, 8192, "unit", 8192), (4, 8191, "runs", 1 << 20),
    (2, 16383, "unit", 16383), (4, 16384, "unit", 16384), (4, 16383, "runs", 1 << 24),
    (2, 65536, "unit", 65536), (4, 65536, "unit", 65536), (4, 65536, "runs", 1 << 31),
)
BAD = ((0, 5, True), (65537, 70000, True), (5, 5, False), (5, 0, True))       # (n_buckets, domain, bounds given)


def planned_cases(n):
    per_shape = len(PREDS) + 2 * 2 + 3 * 2                       # COUNT scans, valued scans, list calls
    return len(SHAPES) * per_shape + (len(BAD) * 4 if n == SIZES[0] else 0)


def scan_path(nb, val):
    if val is None:
        path = "BUCKET_SMALL" if nb <= SMALL else "BUCKET_LDS" if nb <= COUNT_LDS else "BUCKET_GLOBAL"
        return f"bucket_scan_kernel<{path}, BLDS={'true' if nb <= BOUNDS_LDS else 'false'}, NT=?>"
    path = "BUCKET_LDS" if nb <= AGG_LDS else "BUCKET_GLOBAL"
    return f"bucket_agg_scan_kernel<{path}, BLDS={'true' if nb <= BOUNDS_LDS else 'false'}, {VAL_NAME[val]}, NT=?>"


def make_bounds(inp, shape):
    w, nb, kind, domain = shape
    if kind == "runs":
        rng = inp.rng(("bounds", shape))
        if domain <= 1 << 20:
            starts = np.sort(rng.choice(np.arange(1, domain, dtype=np.int64), nb - 1, replace=False))
        else:                                                    # distinct draws, a random nb - 1 of them
            starts = np.sort(rng.permutation(np.unique(rng.integers(1, domain, 2 * nb)))[:nb - 1])
        return np.concatenate([[0], starts, [domain]]).astype(np.uint32)
    return np.concatenate([np.arange(nb, dtype=np.int64), [domain]]).astype(np.uint32)


def group_column(inp, gpu, shape):
    """-> (Col, bin base): codes over the domain and an eighth beyond it, the domain's edges on rows that match, padding code 0"""
    w, nb, kind, domain = shape
    if w == "s4":
        return inp.column(("dom_s4",)), fd.SBASE
    top = fd.width_top(w)
    a = inp.rng(("codes", shape)).integers(0, min(top, domain + domain // 8 + 1), inp.pad, endpoint=True).astype(np.uint64)
    inp.plant(a, np.array([v for v in (0, domain - 1, domain, domain + 1, top) if v <= top], dtype=np.uint64))
    a[inp.n:] = 0
    return fd.Col(gpu, a.astype(fd.DT[w]), w, inp.n), 0


def reference(col, base, bounds, nb, vcol, rows):
    bucket = np.searchsorted(bounds, fd.bins_of(col, base, rows), "right").astype(np.int64) - 1
    ok = (bucket >= 0) & (bucket < nb)
    d = bucket[ok]
    if vcol is None:
        return np.bincount(d, minlength=nb).astype(np.uint32)
    wide, img = fd.agg_wide_image(vcol, rows)
    out = np.zeros(4 * nb, dtype=np.uint64)
    out[2 * nb:3 * nb] = U64
    out[:nb] = np.bincount(d, minlength=nb)
    np.add.at(out[nb:2 * nb], d, wide[ok])
    np.minimum.at(out[2 * nb:3 * nb], d, img[ok])
    np.maximum.at(out[3 * nb:], d, img[ok])
    return out


def run(n):
    gpu = fd.Gpu()
    L, ctx = gpu.L, gpu.ctx
    out = ctx.malloc(4 * MAX * 8 + 64)
    inp = fd.Inputs(n, gpu)
    # one match in the last row: a u32 column that is 7 there -- and in the padding behind it
    last = np.zeros(inp.pad, dtype=np.uint32)
    last[n - 1:] = 7
    last_col = fd.Col(gpu, last, 4, n)
    last_bound = (pq.column_array([(last_col.ptr, 4)]), 1, fd.make_pred([(0, 0, 7, 0)], 1, 0b10))
    sel = dict(inp.sel, last=np.array([n - 1]))

    def bound(pname):
        return (last_bound[0], last_bound[1], C.byref(last_bound[2])) if pname == "last" else inp.bound(pname)

    lists = {}
    for k, pname in enumerate(PREDS):
        rows = sel[pname]
        if k % 2 == 0:                                           # ascending, id_base 0
            listed, base = rows.astype(np.int64), 0
        else:                                                    # every seventh twice, shuffled, a row past n_rows, a high id_base
            rows = inp.rng(("bucketlist", pname)).permutation(np.concatenate([rows, rows[::7]]))
            listed, base = np.concatenate([rows, [n + 3], rows[:1]]).astype(np.int64), fd.HIGH_BASE
        lists[pname] = (listed, base, gpu.put((listed + base).astype(np.uint32)), gpu.put(np.array([len(listed)], dtype=np.uint64)))
    cases = 0
    for i, shape in enumerate(SHAPES):
        w, nb, kind, domain = shape
        col, base = group_column(inp, gpu, shape)
        bounds = make_bounds(inp, shape)
        assert len(bounds) == nb + 1 and bounds[0] == 0 and bounds[-1] == domain and (np.diff(bounds.astype(np.int64)) > 0).all()
        bounds_dev = gpu.put(bounds)
        for v, val in enumerate(VALS):
            vcol = inp.column((val,)) if val else None
            words, dt = (nb, np.uint32) if val is None else (4 * nb, np.uint64)
            scans = PREDS if val is None else tuple(PREDS[(i + v + j) % len(PREDS)] for j in (0, 2))
            for pname in scans:
                what = f"bucket scan n={n} val={val} pred={pname} shape={shape}"
                ctx.memset(out, 0xA5, words * np.dtype(dt).itemsize)                   # the call initialises its output
                cols, nc, pred = bound(pname)
                if val is None:
                    rc = L.pqps_filter_group_buckets(ctx.h, cols, nc, n, pred, col.ref(), base, bounds_dev, nb, domain, out, None)
                else:
                    rc = L.pqps_filter_aggregate_buckets(ctx.h, cols, nc, n, pred, vcol.ref(), col.ref(), base, bounds_dev, nb, domain, out, None)
                pq.check(rc, what)
                gpu.fused(scan_path(nb, val), what)
                fd.compare(what, {"out": gpu.get(out, dt, words)}, {"out": reference(col, base, bounds, nb, vcol, sel[pname])})
                cases += 1
            for j in range(2):
                pname = PREDS[(i + 2 * v + 3 * j + 1) % len(PREDS)]
                listed, id_base, ids, count = lists[pname]
                cap = (len(listed) // 2, len(listed), len(listed) + 5)[(i + v + j) % 3]    # *count_dev above / at / below the capacity
                what = f"bucket list n={n} val={val} pred={pname} cap={cap}/{len(listed)} shape={shape}"
                ctx.memset(out, 0xA5, words * np.dtype(dt).itemsize)
                if val is None:
                    rc = L.pqps_group_buckets_list(ctx.h, col.ref(), n, ids, count, cap, id_base, base, bounds_dev, nb, domain, out, None)
                else:
                    rc = L.pqps_aggregate_buckets_list(ctx.h, vcol.ref(), col.ref(), n, ids, count, cap, id_base, base, bounds_dev, nb, domain,
                                                       out, None)
                pq.check(rc, what)
                rows = listed[:cap]
                fd.compare(what, {"out": gpu.get(out, dt, words)}, {"out": reference(col, base, bounds, nb, vcol, rows[rows < n])})
                cases += 1
        if n == SIZES[0] and i == 0:
            cols, nc, pred = bound("all")
            listed, id_base, ids, count = lists["all"]
            vref = inp.column(("val_i32",)).ref()
            for bad_nb, bad_domain, given in BAD:
                b = bounds_dev if given else None
                for rc in (L.pqps_filter_group_buckets(ctx.h, cols, nc, n, pred, col.ref(), base, b, bad_nb, bad_domain, out, None),
                           L.pqps_group_buckets_list(ctx.h, col.ref(), n, ids, count, len(listed), id_base, base, b, bad_nb, bad_domain, out, None),
                           L.pqps_filter_aggregate_buckets(ctx.h, cols, nc, n, pred, vref, col.ref(), base, b, bad_nb, bad_domain, out, None),
                           L.pqps_aggregate_buckets_list(ctx.h, vref, col.ref(), n, ids, count, len(listed), id_base, base, b, bad_nb, bad_domain,
                                                         out, None)):
                    if rc != -1:                                 # PQPS_EINVAL
                        fd.fail(f"{bad_nb} buckets, domain {bad_domain}, bounds {given}: rc {rc}, expected PQPS_EINVAL")
                    cases += 1
        ctx.sync()
        ctx.free(bounds_dev)
        if w != "s4":
            ctx.free(col.ptr)
    for _, _, ids, count in lists.values():
        ctx.free(ids)
        ctx.free(count)
    ctx.free(last_col.ptr)
    inp.free()
    ctx.free(out)
    gpu.close()
    assert cases == planned_cases(n), (cases, planned_cases(n))
    print(f"buckets: n={n} {gpu.nt} cases={cases} kernels={len(gpu.kernels)}")
    for name in sorted(gpu.kernels):
        print("  " + name)
    print("OK")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nt", ["0", "1"])
def test_bucket_calls_at_the_shim(nt, n):
    p = subprocess.run([sys.executable, __file__, "run", str(n)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PQPS_NT_LOADS=nt), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    flavour = "NT=true" if nt == "1" else "NT=false"
    kernels = [ln.strip() for ln in p.stdout.splitlines() if ln.startswith("  ")]
    # the four COUNT instances and the three of either value width ran, in this flavour and in no other
    assert len(kernels) == len(set(kernels)) == 10 and all(flavour in k for k in kernels), kernels
    assert f"cases={planned_cases(n)} " in p.stdout


def test_shim_shapes_cover_the_path_switches():
    """CPU: the case list holds both sides of every limit, every width, and the three kinds of bounds."""
    nbs = {s[1] for s in SHAPES}
    assert {1, 2, 16, 17, AGG_LDS, AGG_LDS + 1, COUNT_LDS, COUNT_LDS + 1, BOUNDS_LDS, BOUNDS_LDS + 1, MAX} <= nbs and max(nbs) == MAX
    assert {s[0] for s in SHAPES} == {1, 2, 4, "s4"} and {s[2] for s in SHAPES} == {"unit", "whole", "runs"}
    assert len({scan_path(nb, None) for nb in nbs}) == 4 and len({scan_path(nb, "val_i32") for nb in nbs}) == 3
    # codes at or above the domain fit the column wherever the width has room for them
    assert any(s[3] < fd.width_top(s[0]) for s in SHAPES if s[0] != "s4")


if __name__ == "__main__":
    run(int(sys.argv[2]))
