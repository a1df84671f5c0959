"""pqps_remap_codes called alone at the shim and compared with numpy (lut[src], a code >= lut_count -> 0 and counted), exactly.

Every case checks the WHOLE destination buffer byte for byte -- the n codes, and the padding behind them, pre-filled with a
sentinel, of which no byte at or past n * dst_width may change -- the source unchanged when the call is out of place, and the
count of out-of-range codes.  The source's own padding holds codes that would be counted (and, looked up, would differ), so a
kernel that reads past n shows.

  * n around the kernel's edges: the 4-, 8- and 16-element chunk of a 16-byte load, the 256-lane workgroup, several workgroups
  * the six width pairs, out of place for all and in place for the equal ones
  * lut_count around the code widths and around PQPS_REMAP_LDS_CODES, both forms wherever legal
  * planted out-of-range codes (first, last and scattered elements) wherever the source width can express one
  * a column long enough that the lanes of the persistent grid take a second trip, both forms
  * the PQPS_EINVAL cases: nothing written
"""
import ctypes as C

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

N = (0, 1, 3, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4099, 70_001)
PAIRS = ((1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 4))
LUT_COUNTS = (1, 2, 255, 256, 257, pq.REMAP_LDS_CODES, pq.REMAP_LDS_CODES + 1, 65_536, 70_000)
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
GUARD = 64                                                        # elements behind the last chunk nobody may touch
EINVAL = -1
BAD_SENTINEL = 0x7777777777777777


def test_constants_match_the_header():
    assert pq.lib().pqps_remap_form(pq.REMAP_LDS_CODES) == pq.REMAP_LDS
    assert pq.lib().pqps_remap_form(pq.REMAP_LDS_CODES + 1) == pq.REMAP_GLOBAL
    assert pq.lib().pqps_remap_form(1) == pq.REMAP_LDS
    assert pq.REMAP_LDS_CODES <= 16_384


class Device:
    def __init__(self):
        self.ctx = pq.Context(0)
        self.bad = self.ctx.malloc(64)
        self.luts = {}

    def lut(self, count, dst_width):
        """(device pointer, host array) of a table of `count` random values that fit dst_width -- no identity, no order."""
        key = (count, dst_width)
        if key not in self.luts:
            rng = np.random.default_rng(count * 8 + dst_width)
            host = rng.integers(0, min(1 << (8 * dst_width), 1 << 32), count, dtype=np.uint64).astype(np.uint32)
            p = self.ctx.malloc(host.nbytes)
            self.ctx.upload(p, host.ctypes.data, host.nbytes)
            self.luts[key] = (p, host)
        return self.luts[key]

    def upload(self, array):
        p = self.ctx.malloc(array.nbytes)
        self.ctx.upload(p, array.ctypes.data, array.nbytes)
        return p

    def download(self, p, like):
        out = np.empty_like(like)
        self.ctx.download(out.ctypes.data, p, out.nbytes)
        return out

    def set_bad(self, value):
        w = np.array([value], dtype=np.uint64)
        self.ctx.upload(self.bad, w.ctypes.data, 8)

    def get_bad(self):
        w = np.zeros(1, dtype=np.uint64)
        self.ctx.download(w.ctypes.data, self.bad, 8)
        return int(w[0])

    def close(self):
        for p, _ in self.luts.values():
            self.ctx.free(p)
        self.ctx.free(self.bad)
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def room(n):
    return (n + 15) // 16 * 16 + GUARD


def source(rng, n, sw, lut_count, plant):
    """n codes below lut_count (as far as sw bytes can say them), `plant`: some at or past it; the padding 0x5A bytes."""
    a = np.full(room(n), 0x5A5A5A5A & ((1 << (8 * sw)) - 1), dtype=DTYPE[sw])
    top = min(lut_count, 1 << (8 * sw))
    a[:n] = rng.integers(0, top, n, dtype=np.uint64).astype(DTYPE[sw])
    if plant and n:
        where = np.unique(np.concatenate(([0, n - 1], rng.integers(0, n, max(1, n // 9)))))
        a[where] = rng.integers(lut_count, 1 << (8 * sw), len(where), dtype=np.uint64).astype(DTYPE[sw])
        a[n - 1] = (1 << (8 * sw)) - 1                            # the largest code there is
    return a


def run(dev, n, sw, dw, lut_count, form, in_place, plant, seed=0, count_bad=True):
    lut_dev, lut = dev.lut(lut_count, dw)
    rng = np.random.default_rng([n, sw, dw, lut_count, seed])
    src = source(rng, n, sw, lut_count, plant)
    codes = src[:n].astype(np.int64)
    inside = codes < lut_count
    want_codes = np.where(inside, lut[np.minimum(codes, lut_count - 1)], 0).astype(DTYPE[dw])
    src_dev = dev.upload(src)
    if in_place:
        dst, dst_dev = src.copy(), src_dev
    else:
        dst = np.full(room(n), 0xA5A5A5A5 & ((1 << (8 * dw)) - 1), dtype=DTYPE[dw])
        dst_dev = dev.upload(dst)
    want = dst.copy()
    want[:n] = want_codes
    try:
        dev.set_bad(BAD_SENTINEL)
        pq.remap_codes(dev.ctx, src_dev, sw, dst_dev, dw, n, lut_dev, lut_count, form, dev.bad if count_bad else None)
        dev.ctx.sync()
        got = dev.download(dst_dev, dst)
        what = (n, sw, dw, lut_count, form, in_place, plant)
        assert got.tobytes() == want.tobytes(), (what, np.flatnonzero(got != want)[:8])
        if not in_place:
            assert dev.download(src_dev, src).tobytes() == src.tobytes(), what
        if count_bad:
            assert dev.get_bad() == int(np.count_nonzero(~inside)), what
            assert plant or dev.get_bad() == 0
        else:
            assert dev.get_bad() == BAD_SENTINEL
    finally:
        dev.ctx.free(src_dev)
        if not in_place:
            dev.ctx.free(dst_dev)


def forms_of(lut_count):
    return (pq.REMAP_LDS, pq.REMAP_GLOBAL) if lut_count <= pq.REMAP_LDS_CODES else (pq.REMAP_GLOBAL,)


# every width pair with every table whose largest position fits the destination (the others are PQPS_EINVAL cases, below);
# 70 000 entries are reached in full by 4-byte sources only, narrower sources reach their own codes
CASES = [(sw, dw, count) for sw, dw in PAIRS for count in LUT_COUNTS if count <= 1 << (8 * dw)]


@pytest.mark.parametrize("sw, dw, lut_count", CASES)
def test_remap_matches_numpy(dev, sw, dw, lut_count):
    can_plant = lut_count < 1 << (8 * sw)
    for n in N:
        for form in forms_of(lut_count):
            for in_place in ((False, True) if sw == dw else (False,)):
                for plant in ((False, True) if can_plant else (False,)):
                    run(dev, n, sw, dw, lut_count, form, in_place, plant)


def test_without_a_bad_counter(dev):
    run(dev, 1025, 2, 2, 300, pq.REMAP_LDS, True, True, count_bad=False)
    run(dev, 1025, 1, 4, 200, pq.REMAP_GLOBAL, False, True, count_bad=False)


def test_the_form_the_engine_takes(dev):
    run(dev, 4099, 2, 2, 2000, None, True, True)
    run(dev, 4099, 2, 2, 5000, None, True, True)
    run(dev, 4099, 4, 4, 70_000, None, False, True)


def test_a_second_trip_of_the_persistent_grid(dev):
    """More chunks than the largest grid has lanes (8 workgroups of 256 per CU): some lanes take a second trip."""
    lanes = dev.ctx.info()[1] * 8 * 256
    run(dev, lanes * 4 + 4 * 256 * 3 + 3, 4, 4, 4000, pq.REMAP_LDS, True, True)
    run(dev, lanes * 4 + 4 * 256 * 3 + 1, 4, 4, 70_000, pq.REMAP_GLOBAL, False, True)
    run(dev, lanes * 8 + 8 * 256 + 5, 2, 4, 256, pq.REMAP_LDS, False, False)


def test_einval_writes_nothing(dev):
    n = 1000
    rng = np.random.default_rng(5)
    lut_dev, _ = dev.lut(256, 4)
    big_dev, _ = dev.lut(70_000, 4)
    src = source(rng, n, 4, 256, False)
    dst = np.full(room(n), 0xA5A5A5A5, dtype=np.uint32)
    src_dev, dst_dev = dev.upload(src), dev.upload(dst)
    L, ctx = pq.lib(), dev.ctx.h
    LDS, GLOBAL = pq.REMAP_LDS, pq.REMAP_GLOBAL
    cases = {
        "source not 16-byte aligned": (src_dev + 4, 1, dst_dev, 1, n, lut_dev, 256, LDS),
        "destination not 16-byte aligned": (src_dev, 1, dst_dev + 8, 1, n, lut_dev, 256, LDS),
        "narrower 2 -> 1": (src_dev, 2, dst_dev, 1, n, lut_dev, 256, LDS),
        "narrower 4 -> 2": (src_dev, 4, dst_dev, 2, n, lut_dev, 256, LDS),
        "narrower 4 -> 1": (src_dev, 4, dst_dev, 1, n, lut_dev, 256, LDS),
        "source width 3": (src_dev, 3, dst_dev, 4, n, lut_dev, 256, LDS),
        "source width 0": (src_dev, 0, dst_dev, 4, n, lut_dev, 256, LDS),
        "destination width 8": (src_dev, 4, dst_dev, 8, n, lut_dev, 256, LDS),
        "in place with different widths": (src_dev, 1, src_dev, 2, n, lut_dev, 256, LDS),
        "partial overlap, destination behind": (src_dev, 4, src_dev + 16, 4, n, lut_dev, 256, LDS),
        "partial overlap, destination in front": (src_dev + 16, 4, src_dev, 4, n, lut_dev, 256, LDS),
        "partial overlap, widening": (src_dev + 1024, 1, src_dev, 4, n, lut_dev, 256, LDS),
        "LDS form, table too large": (src_dev, 4, dst_dev, 4, n, big_dev, pq.REMAP_LDS_CODES + 1, LDS),
        "unknown form": (src_dev, 4, dst_dev, 4, n, lut_dev, 256, 2),
        "negative form": (src_dev, 4, dst_dev, 4, n, lut_dev, 256, -1),
        "empty table": (src_dev, 4, dst_dev, 4, n, lut_dev, 0, LDS),
        "257 codes into 1 byte": (src_dev, 1, dst_dev, 1, n, big_dev, 257, LDS),
        "65 537 codes into 2 bytes": (src_dev, 2, dst_dev, 2, n, big_dev, 65_537, GLOBAL),
        "NULL source": (None, 4, dst_dev, 4, n, lut_dev, 256, LDS),
        "NULL destination": (src_dev, 4, None, 4, n, lut_dev, 256, LDS),
        "NULL table": (src_dev, 4, dst_dev, 4, n, None, 256, LDS),
        "misaligned even with no rows": (src_dev + 2, 1, dst_dev, 1, 0, lut_dev, 256, LDS),
    }
    try:
        dev.set_bad(BAD_SENTINEL)
        for what, (s, sw, d, dw, k, lut, count, form) in cases.items():
            assert L.pqps_remap_codes(ctx, s, sw, d, dw, k, lut, count, form, dev.bad, None) == EINVAL, what
        assert L.pqps_remap_codes(None, src_dev, 4, dst_dev, 4, n, lut_dev, 256, LDS, dev.bad, None) == EINVAL
        dev.ctx.sync()
        assert dev.download(src_dev, src).tobytes() == src.tobytes()
        assert dev.download(dst_dev, dst).tobytes() == dst.tobytes()
        assert dev.get_bad() == BAD_SENTINEL
        # adjacent ranges do not overlap: the destination may begin where the source ends
        assert L.pqps_remap_codes(ctx, src_dev, 4, src_dev + 4 * 1024, 4, 16, lut_dev, 256, LDS, dev.bad, None) == 0
        dev.ctx.sync()
    finally:
        dev.ctx.free(src_dev)
        dev.ctx.free(dst_dev)
