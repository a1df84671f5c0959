"""pqps_bins_having (and pqps_bins_rows) called alone at the shim and compared with numpy, exactly.

  * n_bins in {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65 536, 65 537, 1 000 003}: one lane, a round that ends in its lower
    word, whole rounds, more than one workgroup, more rounds than the grid has waves
  * both bin layouts (u32 counts; the field-major [4][n_bins] u64), every field x every op
  * constants at the edges: 0 and 2^32 - 1 for counts; INT64_MIN, -1, 0, INT64_MAX for signed sums and the same bit patterns
    unsigned; the images of INT_MIN and INT_MAX for MIN and MAX -- the bins hold exactly those values too
  * a block of empty bins (count 0, sum 0, min image all ones, max image 0) stays unset under COUNT < 5, SUM = 0, MIN <= c and
    MAX >= c, all of which the empty fields satisfy
  * the output is pre-filled with 0xFF: the tail bits of the last word read 0, the guard word behind the bitmap is untouched
  * members == the popcount, and a NULL members is tolerated
  * every PQPS_EINVAL case returns before a launch: bitmap and members stay as they were
"""
import ctypes as C

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

N_BINS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65_536, 65_537, 1_000_003)
COUNT, SUM, MIN, MAX = 0, 1, 2, 3                      # PQPS_HAVING_COUNT .. _MAX
EQ, NE, LT, GT, LE, GE = range(6)                      # PQPS_HAVING_EQ .. _GE
EINVAL = -1
U64_MAX, M63 = 2**64 - 1, 1 << 63
INT64_EDGES = (-2**63, -1, 0, 2**63 - 1)
GUARD_WORDS = 4
SENTINEL = 0xDEADBEEF


def image(v):
    """the image of an i32 value in pqps_filter_aggregate's min / max fields"""
    return ((v & U64_MAX) ^ M63) & U64_MAX


IMG_EDGES = (image(-2**31), image(2**31 - 1), image(0))


def make_bins(n, seed):
    """-> (u32 counts, [4][n] u64 fields): about a third of the bins empty -- one contiguous block of them among those -- and
    the edge values of every field planted in bins that have rows."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 9, n).astype(np.uint64)
    cnt[rng.random(n) < 0.15] = 0
    lo, hi = n // 3, n // 3 + max(1, n // 5)
    if n >= 5:
        cnt[lo:hi] = 0                                                   # the block of empty bins
    if not cnt.any():
        cnt[0] = 3
    live = np.flatnonzero(cnt)
    sums = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True).view(np.uint64).copy()
    sums[rng.random(n) < 0.2] = 0
    vals_lo = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64, endpoint=True)
    vals_hi = np.maximum(vals_lo, rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64, endpoint=True))
    mins = (vals_lo.view(np.uint64) ^ np.uint64(M63))
    maxs = (vals_hi.view(np.uint64) ^ np.uint64(M63))
    cnt32 = cnt.copy()
    for k, b in enumerate(live[:12]):                                   # the edges, in bins that count
        sums[b] = np.int64(INT64_EDGES[k % 4]).view(np.uint64)
        mins[b] = IMG_EDGES[k % 3]
        maxs[b] = IMG_EDGES[(k + 1) % 3]
        cnt32[b] = (2**32 - 1, 5, 1)[k % 3]
        cnt[b] = (2**32 - 1, 2**40 + 1, 5)[k % 3]
    empty = cnt == 0
    sums[empty], mins[empty], maxs[empty] = 0, U64_MAX, 0
    fields = np.stack([cnt, sums, mins, maxs]).astype(np.uint64)
    return cnt32.astype(np.uint32), np.ascontiguousarray(fields)


def compare(x, op, c, signed):
    if signed:
        x, c = x.view(np.int64), np.uint64(c).view(np.int64)
    else:
        c = np.uint64(c)
    return (x == c, x != c, x < c, x > c, x <= c, x >= c)[op]


def expected(count, x, op, c, signed=False):
    return (count != 0) & compare(x, op, c, signed)


class Device:
    def __init__(self):
        self.ctx = pq.Context(0)
        n = max(N_BINS)
        self.bins = self.ctx.malloc(n * 32)
        self.bitmap = self.ctx.malloc(((n + 31) // 32 + GUARD_WORDS) * 4 + 8)
        self.members = self.ctx.malloc(8)
        self.loaded = None

    def load(self, key, array):
        if self.loaded != key:
            self.ctx.upload(self.bins, array.ctypes.data, array.nbytes)
            self.loaded = key

    def call(self, n, valued, field, op, c, signed=0, members=True, bins=True, bitmap_offset=0, have_bitmap=True):
        """-> (rc, the words + guard as downloaded, members word)"""
        ctx = self.ctx
        words = (n + 31) // 32 if n else 1
        before = np.full(words + GUARD_WORDS, 0xFFFFFFFF, dtype=np.uint32)
        ctx.upload(self.bitmap, before.ctypes.data, before.nbytes)
        sent = np.array([SENTINEL], dtype=np.uint64)
        ctx.upload(self.members, sent.ctypes.data, 8)
        rc = pq.lib().pqps_bins_having(ctx.h, self.bins if bins else None, n, valued, field, op, c, signed,
                                       (self.bitmap + bitmap_offset) if have_bitmap else None, self.members if members else None, None)
        ctx.sync()
        got = np.empty(words + GUARD_WORDS, dtype=np.uint32)
        ctx.download(got.ctypes.data, self.bitmap, got.nbytes)
        m = np.zeros(1, dtype=np.uint64)
        ctx.download(m.ctypes.data, self.members, 8)
        return rc, got, int(m[0])

    def having(self, n, valued, field, op, c, signed=0, members=True):
        """-> the n bits as bools; checks the tail bits, the guard and the members on the way"""
        rc, got, m = self.call(n, valued, field, op, c, signed, members)
        pq.check(rc, "pqps_bins_having")
        words = (n + 31) // 32
        assert np.all(got[words:] == 0xFFFFFFFF), "the guard words behind the bitmap are untouched"
        bits = np.unpackbits(got[:words].view(np.uint8), bitorder="little")
        assert not bits[n:].any(), "the tail bits of the last word are 0"
        assert m == (int(bits.sum()) if members else SENTINEL)
        return bits[:n].astype(bool)

    def close(self):
        for p in (self.bins, self.bitmap, self.members):
            self.ctx.free(p)
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@pytest.mark.parametrize("n", N_BINS)
def test_counts_layout(dev, n):
    cnt32, _ = make_bins(n, 0xC0 + n)
    dev.load(("c", n), cnt32)
    x = cnt32.astype(np.uint64)
    for op in range(6):
        for c in (0, 1, 5, 2**32 - 1, 2**32, U64_MAX):
            assert np.array_equal(dev.having(n, 0, COUNT, op, c), expected(x, x, op, c)), (op, c)
    assert np.array_equal(dev.having(n, 0, COUNT, GE, 1, members=False), x != 0)


@pytest.mark.parametrize("n", N_BINS)
def test_valued_layout(dev, n):
    _, f = make_bins(n, 0xF0 + n)
    dev.load(("v", n), f)
    cnt = f[0]
    for op in range(6):
        for c in (0, 5, 2**32 - 1, 2**40 + 1):
            assert np.array_equal(dev.having(n, 1, COUNT, op, c), expected(cnt, cnt, op, c)), ("count", op, c)
        for v in INT64_EDGES:
            c = v & U64_MAX
            assert np.array_equal(dev.having(n, 1, SUM, op, c, signed=1), expected(cnt, f[1], op, c, True)), ("sum i64", op, v)
            assert np.array_equal(dev.having(n, 1, SUM, op, c, signed=0), expected(cnt, f[1], op, c, False)), ("sum u64", op, v)
        for c in IMG_EDGES:
            # MIN and MAX compare images unsigned, whatever value_signed says
            assert np.array_equal(dev.having(n, 1, MIN, op, c, signed=op & 1), expected(cnt, f[2], op, c)), ("min", op, c)
            assert np.array_equal(dev.having(n, 1, MAX, op, c, signed=op & 1), expected(cnt, f[3], op, c)), ("max", op, c)
    assert np.array_equal(dev.having(n, 1, SUM, NE, 0, members=False), (cnt != 0) & (f[1] != 0))


@pytest.mark.parametrize("n", (65, 257, 65_537))
def test_empty_bins_are_never_members(dev, n):
    cnt32, f = make_bins(n, 0xE0 + n)
    empty = f[0] == 0
    lo, hi = n // 3, n // 3 + max(1, n // 5)
    assert empty[lo:hi].all() and (~empty).any()
    dev.load(("v", n, "e"), f)
    for field, op, c, row in ((COUNT, LT, 5, f[0]), (SUM, EQ, 0, f[1]), (MIN, LE, U64_MAX, f[2]), (MAX, GE, 0, f[3])):
        assert compare(row[empty], op, c, False).all(), "the empty fields satisfy the comparison by themselves"
        got = dev.having(n, 1, field, op, c, signed=int(field == SUM))
        assert not got[empty].any()
        assert np.array_equal(got, expected(f[0], row, op, c, field == SUM))
    dev.load(("c", n, "e"), cnt32)
    got = dev.having(n, 0, COUNT, LT, 5)
    assert not got[cnt32 == 0].any() and np.array_equal(got, (cnt32 != 0) & (cnt32 < 5))


def test_argument_errors_launch_nothing(dev):
    n = 257
    _, f = make_bins(n, 1)
    dev.load(("v", n, "x"), f)
    cases = [dict(n=0, valued=1, field=COUNT, op=EQ), dict(n=n, valued=1, field=-1, op=EQ), dict(n=n, valued=1, field=4, op=EQ),
             dict(n=n, valued=1, field=SUM, op=-1), dict(n=n, valued=1, field=SUM, op=6), dict(n=n, valued=0, field=SUM, op=EQ),
             dict(n=n, valued=0, field=MIN, op=EQ), dict(n=n, valued=0, field=MAX, op=EQ), dict(n=n, valued=1, field=COUNT, op=EQ, bins=False),
             dict(n=n, valued=1, field=COUNT, op=EQ, have_bitmap=False), dict(n=n, valued=1, field=COUNT, op=EQ, bitmap_offset=4)]
    for kw in cases:
        rc, got, m = dev.call(kw.pop("n"), kw.pop("valued"), kw.pop("field"), kw.pop("op"), 0, **kw)
        assert rc == EINVAL, kw
        assert np.all(got == 0xFFFFFFFF) and m == SENTINEL, "nothing was launched"
    assert pq.lib().pqps_bins_having(None, dev.bins, n, 1, COUNT, EQ, 0, 0, dev.bitmap, None, None) == EINVAL


@pytest.mark.parametrize("n", (1, 257, 65_537, 1_000_003))
def test_bins_rows(dev, n):
    cnt32, f = make_bins(n, 0xB0 + n)
    out = np.zeros(1, dtype=np.uint64)
    for valued, arr, want in ((0, cnt32, int(cnt32.astype(np.uint64).sum())), (1, f, int(f[0].sum(dtype=np.uint64)))):
        dev.load(("r", n, valued), arr)
        sent = np.array([SENTINEL], dtype=np.uint64)
        dev.ctx.upload(dev.members, sent.ctypes.data, 8)
        pq.check(pq.lib().pqps_bins_rows(dev.ctx.h, dev.bins, n, valued, dev.members, None), "pqps_bins_rows")
        dev.ctx.sync()
        dev.ctx.download(out.ctypes.data, dev.members, 8)
        assert int(out[0]) == want
    assert pq.lib().pqps_bins_rows(dev.ctx.h, dev.bins, 0, 0, dev.members, None) == EINVAL
    assert pq.lib().pqps_bins_rows(dev.ctx.h, None, n, 0, dev.members, None) == EINVAL
    assert pq.lib().pqps_bins_rows(dev.ctx.h, dev.bins, n, 0, None, None) == EINVAL
