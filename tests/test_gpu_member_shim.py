"""pqps_member_flags called alone at the shim and compared with numpy, exactly.

  * columns 1, 2, 4 and 8 bytes wide; n_rows in {1, 1023, 1024, 1025, 4097, 70 001}; both output forms
  * bitmap form: n_bits in {1, 32, 33, the LDS bound, the bound + 1, 2^20 + 5} (both placements of the bitmap), a non-zero base,
    values below the base (they wrap far past n_bits), values at n_bits and above, set bits behind n_bits in the last word
  * list form: 1, 2 and 4 097 values, lists that hold 0 and 2^64 - 1, an i32 column as its u32 bit pattern with negative values
  * the count equals the sum of the flags, plane bits from n_rows to the padded end are 0 although those rows hold members,
    and a guard region behind `out` stays as it was
  * the PQPS_EINVAL cases
"""
import ctypes as C

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

N_ROWS = (1, 1023, 1024, 1025, 4097, 70_001)
N_BITS = (1, 32, 33, pq.MEMBER_LDS_BITS, pq.MEMBER_LDS_BITS + 1, 2**20 + 5)
STEP = 1024
GUARD = 256
MAX_ROWS = (max(N_ROWS) + STEP - 1) // STEP * STEP
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
EINVAL = -1


class Device:
    """One context and buffers large enough for every case of this file."""

    def __init__(self):
        self.ctx = pq.Context(0)
        self.col = self.ctx.malloc(MAX_ROWS * 8)
        self.out = self.ctx.malloc(MAX_ROWS + GUARD)
        self.set = self.ctx.malloc(max((max(N_BITS) + 31) // 32 * 4, 4097 * 8))
        self.count = self.ctx.malloc(64)

    def run(self, values, n_rows, form, base=0, n_bits=0, words=None, values_list=None, out_form=pq.MEMBER_BYTES):
        """-> (flags of rows [0, n_rows), count); checks the padding bits, the guard and the count on the way."""
        ctx, width = self.ctx, values.dtype.itemsize
        padded = (n_rows + STEP - 1) // STEP * STEP
        assert len(values) == padded
        ctx.upload(self.col, values.ctypes.data, values.nbytes)
        host_set = words if form == pq.MEMBER_BITMAP else values_list
        if len(host_set):
            ctx.upload(self.set, host_set.ctypes.data, host_set.nbytes)
        out_bytes = padded // 8 if out_form == pq.MEMBER_PLANE else n_rows
        before = np.full(out_bytes + GUARD, 0xA5, dtype=np.uint8)
        ctx.upload(self.out, before.ctypes.data, before.nbytes)
        sentinel = np.array([0xDEADBEEF], dtype=np.uint64)
        ctx.upload(self.count, sentinel.ctypes.data, 8)
        col = pq.Column(self.col, width, 0)
        rc = pq.lib().pqps_member_flags(ctx.h, C.byref(col), n_rows, form, base, n_bits, self.set if form == pq.MEMBER_BITMAP else None,
                                        self.set if form == pq.MEMBER_LIST else None, 0 if values_list is None else len(values_list),
                                        out_form, self.out, self.count, None)
        pq.check(rc, "pqps_member_flags")
        ctx.sync()
        got = np.empty(out_bytes + GUARD, dtype=np.uint8)
        ctx.download(got.ctypes.data, self.out, got.nbytes)
        count = np.zeros(1, dtype=np.uint64)
        ctx.download(count.ctypes.data, self.count, 8)
        assert np.all(got[out_bytes:] == 0xA5), "the guard behind out is untouched"
        if out_form == pq.MEMBER_PLANE:
            bits = np.unpackbits(got[:out_bytes], bitorder="little")
            assert not bits[n_rows:].any(), "plane bits from n_rows to the padded end are 0"
            flags = bits[:n_rows]
        else:
            flags = got[:n_rows]
            assert set(np.unique(flags)) <= {0, 1}
        assert int(count[0]) == int(flags.sum())
        return flags.astype(bool), int(count[0])

    def close(self):
        for p in (self.col, self.out, self.set, self.count):
            self.ctx.free(p)
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def bitmap_reference(values, base, n_bits, words):
    x = values.astype(np.int64) & 0xFFFFFFFF
    idx = (x - base) & 0xFFFFFFFF
    ok = idx < n_bits
    safe = np.where(ok, idx, 0)
    return ok & (((words[safe >> 5] >> (safe & 31).astype(np.uint32)) & 1) != 0)


def bitmap_case(rng, width, n_bits, padded):
    """(values, base, words): a third of the values inside the window, the others around it -- below the base and at n_bits and above."""
    top = 1 << (8 * width)
    base = {1: 7, 2: 300, 4: 0xFFFFFF00}[width]                   # (4 bytes: the window crosses 2^32, i.e. from negative i32 values up)
    words = rng.integers(0, 2**32, (n_bits + 31) // 32, dtype=np.uint64).astype(np.uint32)
    words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n_bits % 32) if n_bits % 32 else np.uint32(0)      # set bits behind n_bits: never members
    words[0] |= np.uint32(1)
    if n_bits > 1:
        words[(n_bits - 1) >> 5] |= np.uint32(1) << np.uint32((n_bits - 1) & 31)
    inside = rng.integers(0, n_bits, padded)
    around = rng.integers(-40, 40, padded) + np.where(rng.integers(0, 2, padded) == 1, n_bits, 0)
    edge = rng.choice(np.array([-1, 0, n_bits - 1, n_bits, n_bits + 1]), padded)
    pick = rng.integers(0, 3, padded)
    off = np.where(pick == 0, inside, np.where(pick == 1, around, edge))
    values = ((base + off) % top).astype(DTYPE[width])
    return values, base, words


@pytest.mark.parametrize("out_form", [pq.MEMBER_BYTES, pq.MEMBER_PLANE], ids=["bytes", "plane"])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_bitmap_form(dev, width, out_form):
    rng = np.random.default_rng(100 * width + out_form)
    some_members = False
    for n_bits in N_BITS:
        for n_rows in N_ROWS:
            padded = (n_rows + STEP - 1) // STEP * STEP
            values, base, words = bitmap_case(rng, width, n_bits, padded)
            values[n_rows:] = base % (1 << (8 * width))             # the padding rows hold a member: the kernel has to trim them
            want = bitmap_reference(values, base, n_bits, words)
            assert want[n_rows:].all()
            got, count = dev.run(values, n_rows, pq.MEMBER_BITMAP, base, n_bits, words=words, out_form=out_form)
            assert np.array_equal(got, want[:n_rows]), (width, n_bits, n_rows)
            some_members |= 0 < count < n_rows
    assert some_members


def list_reference(values, values_list):
    x = (values.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) if values.dtype == np.int32 else values.astype(np.uint64)
    return np.isin(x, values_list)


@pytest.mark.parametrize("out_form", [pq.MEMBER_BYTES, pq.MEMBER_PLANE], ids=["bytes", "plane"])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_list_form(dev, width, out_form):
    rng = np.random.default_rng(200 * width + out_form)
    top = (1 << (8 * width)) - 1
    for n_list in (1, 2, 4097):
        # the domain the rows are drawn from: small enough that many rows are members, and its two ends are listed
        # (a list may hold values no row of a narrow column can carry: harmless)
        ends = np.array([0, top], dtype=np.uint64)
        domain = np.unique(np.concatenate([rng.integers(0, max(top, 1 << 15), 3 * n_list, dtype=np.uint64, endpoint=True), ends]))
        inner = rng.choice(np.setdiff1d(domain, ends), max(n_list - 2, 0), replace=False)
        values_list = np.sort(np.concatenate([inner, ends if n_list > 1 else ends[1:]]))
        assert len(values_list) == n_list == len(np.unique(values_list))
        for n_rows in N_ROWS:
            padded = (n_rows + STEP - 1) // STEP * STEP
            values = rng.choice(domain, padded).astype(DTYPE[width])
            values[rng.integers(0, padded, padded // 4 + 1)] = values_list[rng.integers(0, n_list, padded // 4 + 1)].astype(DTYPE[width])
            values[n_rows:] = top                                  # the padding rows hold a member
            want = list_reference(values, values_list)
            assert want[n_rows:].all()
            got, count = dev.run(values, n_rows, pq.MEMBER_LIST, values_list=values_list, out_form=out_form)
            assert np.array_equal(got, want[:n_rows]), (width, n_list, n_rows)
            assert n_rows < 1000 or 0 < count < n_rows


def test_list_form_takes_i32_values_as_their_bit_pattern(dev):
    rng = np.random.default_rng(5)
    listed = np.array([-2**31, -70000, -3, -1, 0, 1, 130, 2**31 - 1], dtype=np.int64)
    values_list = np.sort((listed & 0xFFFFFFFF).astype(np.uint64))          # negative values sort behind the others
    assert values_list[0] == 0 and values_list[-1] == 0xFFFFFFFF
    for n_rows in (1025, 70_001):
        padded = (n_rows + STEP - 1) // STEP * STEP
        values = rng.choice(np.concatenate([listed, listed + 1, listed[1:] - 1, np.array([5, -5, 2**31 - 2])]), padded).astype(np.int32)
        want = np.isin(values.astype(np.int64), listed)
        for out_form in (pq.MEMBER_BYTES, pq.MEMBER_PLANE):
            got, count = dev.run(values, n_rows, pq.MEMBER_LIST, values_list=values_list, out_form=out_form)
            assert np.array_equal(got, want[:n_rows]) and 0 < count < n_rows


def test_an_empty_list_and_an_empty_table(dev):
    values = np.arange(STEP, dtype=np.uint16)
    got, count = dev.run(values, 1000, pq.MEMBER_LIST, values_list=np.zeros(0, dtype=np.uint64), out_form=pq.MEMBER_PLANE)
    assert count == 0 and not got.any()
    # n_rows == 0: nothing is launched, nothing of `out` is written, the count is 0
    ctx = dev.ctx
    mark = np.full(64, 0x5A, dtype=np.uint8)
    ctx.upload(dev.out, mark.ctypes.data, 64)
    ctx.upload(dev.count, mark.ctypes.data, 8)
    col = pq.Column(dev.col, 2, 0)
    for out_form in (pq.MEMBER_BYTES, pq.MEMBER_PLANE):
        pq.check(pq.lib().pqps_member_flags(ctx.h, C.byref(col), 0, pq.MEMBER_LIST, 0, 0, None, None, 0, out_form, dev.out, dev.count, None))
        ctx.sync()
        got, count = np.zeros(64, dtype=np.uint8), np.ones(1, dtype=np.uint64)
        ctx.download(got.ctypes.data, dev.out, 64)
        ctx.download(count.ctypes.data, dev.count, 8)
        assert np.all(got == 0x5A) and count[0] == 0
    # the count may be left out
    pq.check(pq.lib().pqps_member_flags(ctx.h, C.byref(col), 1000, pq.MEMBER_LIST, 0, 0, None, None, 0, pq.MEMBER_BYTES, dev.out, None, None))
    ctx.sync()


def test_bad_arguments_are_einval(dev):
    L, ctx = pq.lib(), dev.ctx

    def call(width=2, form=pq.MEMBER_BITMAP, n_bits=64, bitmap=dev.set, lst=None, n_list=0, out_form=pq.MEMBER_BYTES, out=dev.out, data=dev.col):
        col = pq.Column(data, width, 0)
        return L.pqps_member_flags(ctx.h, C.byref(col), 1024, form, 0, n_bits, bitmap, lst, n_list, out_form, out, dev.count, None)

    assert call(width=pq.WIDTH_BITS) == EINVAL, "a bit plane is no member column"
    assert call(width=pq.WIDTH_BITS, form=pq.MEMBER_LIST, bitmap=None, lst=dev.set, n_list=1) == EINVAL
    assert call(width=8) == EINVAL, "an 8-byte column takes the list form"
    assert call(width=3) == EINVAL and call(width=0) == EINVAL and call(width=16) == EINVAL
    assert call(form=2) == EINVAL and call(form=-1) == EINVAL and call(out_form=2) == EINVAL
    assert call(bitmap=None) == EINVAL and call(n_bits=0) == EINVAL and call(n_bits=2**32 + 1) == EINVAL
    assert call(form=pq.MEMBER_LIST, bitmap=None, lst=None, n_list=3) == EINVAL
    assert call(out=None) == EINVAL and call(out=dev.out + 8) == EINVAL and call(data=dev.col + 4) == EINVAL
    assert b"" != L.pqps_last_error()
    ctx.sync()
    assert call() == 0                                            # ... and the same call with good arguments runs
    ctx.sync()
