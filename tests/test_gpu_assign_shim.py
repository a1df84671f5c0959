"""pqps_filter_assign and pqps_assign_flags called alone at the shim and compared with numpy (np.where(mask, value, old)), exactly.

Every case checks the WHOLE buffer of every target byte for byte -- the rows, the padding up to the PQPS_TILE_ROWS multiple
(pre-filled with a pattern, and selected by the predicate / the flags, so that trimming to n_rows is tested) and a guard behind
it -- every other column unchanged, and the matched count.

  * widths 1, 2, 4 and 8; n_rows around the kernel's edges: the 4-row lane chunk, the 256-row chunk, the 1024-row step, the
    4096-row padding
  * masks: no row, every row, every second row, row i % 4 == 3, one row in 1000, only the last row (empty, full and partial
    chunks, steps that are skipped)
  * a table of (waves of the grid) x 1024 + 1025 rows: some waves take a second step, the last step is partial
  * a target that is the predicate's own column, three targets of different widths in one launch, a predicate on a bit plane
    with the byte column as target
  * the PQPS_EINVAL cases
"""
import ctypes as C

import numpy as np
import pytest

import qpelib as q

pq = q.pq
pytestmark = pytest.mark.gpu

N_ROWS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
VALUE = {1: 0xC3, 2: 0xBEEF, 4: 0xDEADBEEF, 8: 0x0123456789ABCDEF}
GUARD = 64                                                        # rows behind the padding nobody may touch
EINVAL = -1
MASKS = {
    "none": lambda i, n: np.zeros(n, dtype=bool),
    "all": lambda i, n: np.ones(n, dtype=bool),
    "every second": lambda i, n: i % 2 == 1,
    "i % 4 == 3": lambda i, n: i % 4 == 3,
    "one in 1000": lambda i, n: i % 1000 == 0,
    "last row": lambda i, n: i == n - 1,
}


def padded_rows(n_rows):
    return (n_rows + pq.TILE_ROWS - 1) // pq.TILE_ROWS * pq.TILE_ROWS


def sel_spec():
    s = pq.SchemaSpec()
    for name, w in (("command_id", 8), ("exit_code", 4), ("user_id", 4), ("risk_level", 4), ("sudo_used", 1)):
        s.set_numeric(name, w)
    s.set_dict("shell_type", 1, [b"a", b"b", b"c", b"d", b"e", b"f"])
    s.set_dict("user_name", 2, [b"a", b"b", b"c", b"d", b"e", b"f"])
    return s


SPEC = sel_spec()


def sel_pred(_cache=[]):
    """`sel = 1`: one leaf on one 1-byte (or bit-plane) column."""
    if not _cache:
        _cache.append(pq.compile_where(SPEC, [("sudo_used", "=", "1")])[0])
    return _cache[0]


class Device:
    def __init__(self):
        self.ctx = pq.Context(0)
        self.count = self.ctx.malloc(64)
        self.bufs = []

    def upload(self, array):
        p = self.ctx.malloc(array.nbytes)
        self.bufs.append(p)
        self.ctx.upload(p, array.ctypes.data, array.nbytes)
        return p

    def download(self, p, like):
        out = np.empty_like(like)
        self.ctx.download(out.ctypes.data, p, out.nbytes)
        return out

    def release(self):
        for p in self.bufs:
            self.ctx.free(p)
        self.bufs = []

    def close(self):
        self.release()
        self.ctx.free(self.count)
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def old_values(rng, width, n_rows):
    """A column of `width` bytes: random rows, the padding and the guard filled with a pattern."""
    total = padded_rows(n_rows) + GUARD
    a = np.frombuffer(rng.bytes(total * width), dtype=DTYPE[width]).copy()
    a[n_rows:] = np.frombuffer(bytes([0x5A]) * ((total - n_rows) * width), dtype=DTYPE[width])
    return a


def run(dev, form, n_rows, mask, targets, pred=None, pred_cols=None, bystanders=()):
    """One launch.  form: "fused" (pqps_filter_assign over the predicate) or "flags" (pqps_assign_flags over the mask as
    flags).  targets: [(old array, value), ...]; pred / pred_cols: the predicate and its [(array, width)] columns -- by
    default `sel = 1` over a byte column that holds the mask (and 1 from n_rows on).  Checks everything the docstring of
    this file names."""
    total = padded_rows(n_rows) + GUARD
    sel = np.ones(total, dtype=np.uint8)
    sel[:n_rows] = mask
    ptrs = [dev.upload(old) for old, _ in targets]
    triples = [(p, old.dtype.itemsize, value) for p, (old, value) in zip(ptrs, targets)]
    others = [(a, dev.upload(a)) for a in bystanders]
    if form == "flags":
        flags = sel.copy()
        fptr = dev.upload(flags)
        others.append((flags, fptr))
        pq.assign_flags(dev.ctx, fptr, n_rows, triples)
        dev.ctx.sync()
    else:
        if pred is None:
            pred, pred_cols = sel_pred(), [(sel, 1)]
        held = []
        for a, w in pred_cols:
            mine = [p for p, (old, _) in zip(ptrs, targets) if old is a]
            if mine:
                held.append((mine[0], w))
            else:
                p = dev.upload(a)
                others.append((a, p))
                held.append((p, w))
        sentinel = np.array([0xDEADBEEF], dtype=np.uint64)
        dev.ctx.upload(dev.count, sentinel.ctypes.data, 8)
        pq.filter_assign(dev.ctx, pq.column_array(held), len(held), n_rows, pred, triples, dev.count)
        dev.ctx.sync()
        got = dev.download(dev.count, sentinel)
        assert int(got[0]) == int(np.count_nonzero(mask)), "matched count"
    full = np.zeros(total, dtype=bool)
    full[:n_rows] = mask
    for p, (old, value) in zip(ptrs, targets):
        want = np.where(full, np.array(value, dtype=np.uint64).astype(old.dtype), old)
        got = dev.download(p, old)
        assert got.tobytes() == want.tobytes(), f"target of width {old.dtype.itemsize}: rows, padding and guard"
    for a, p in others:
        assert dev.download(p, a).tobytes() == a.tobytes(), "a column that is no target is unchanged"
    dev.release()


@pytest.mark.parametrize("form", ["fused", "flags"])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_widths_sizes_and_masks(dev, width, form):
    rng = np.random.default_rng(10 * width + (form == "flags"))
    for n_rows in N_ROWS:
        i = np.arange(n_rows)
        for name, make in MASKS.items():
            bystander = old_values(rng, 4, n_rows)
            run(dev, form, n_rows, make(i, n_rows), [(old_values(rng, width, n_rows), VALUE[width])], bystanders=[bystander])


@pytest.mark.parametrize("form", ["fused", "flags"])
def test_random_masks_every_density(dev, form):
    rng = np.random.default_rng(77)
    for width in (1, 2, 4, 8):
        for density in (0.01, 0.3, 0.9):
            n_rows = 3 * 4096 + 1027
            run(dev, form, n_rows, rng.random(n_rows) < density, [(old_values(rng, width, n_rows), VALUE[width])])


@pytest.mark.parametrize("form", ["fused", "flags"])
def test_second_trip_of_the_grid_stride_loop(dev, form):
    """More steps than the grid has waves (a persistent grid of 8 workgroups of 4 waves per CU, never more than one step per
    wave): the first waves take a second step, and the table's last step is partial.  Steps without a match, full steps and
    mixed steps alternate."""
    cus = dev.ctx.info()[1]
    waves = cus * 8 * 4
    n_rows = waves * 1024 + 1025
    rng = np.random.default_rng(5)
    step = np.arange(n_rows) // 1024
    mask = np.where(step % 3 == 0, False, np.where(step % 3 == 1, True, rng.random(n_rows) < 0.4))
    mask[-1] = True
    run(dev, form, n_rows, mask, [(old_values(rng, 1, n_rows), VALUE[1])])


@pytest.mark.parametrize("column, width", [("shell_type", 1), ("user_name", 2), ("risk_level", 4), ("command_id", 8)])
def test_target_is_the_predicates_column(dev, column, width):
    """x = 3 -> x := 5 with rows that hold 5 already: a row is matched by its old value only, once."""
    rng = np.random.default_rng(width)
    literal = "d" if width < 4 else "3"                          # "d" is code 3 of the dictionaries
    pred, ids = pq.compile_where(SPEC, [(column, "=", literal)])
    assert ids == [pq.COL[column]]
    for n_rows in (5, 1025, 4097, 20_001):
        total = padded_rows(n_rows) + GUARD
        x = rng.integers(2, 7, total).astype(DTYPE[width])
        x[n_rows:] = 3                                           # the padding would match
        run(dev, "fused", n_rows, x[:n_rows] == 3, [(x, 5)], pred=pred, pred_cols=[(x, width)])


@pytest.mark.parametrize("form", ["fused", "flags"])
@pytest.mark.parametrize("widths", [(1, 2, 8), (4, 2, 1), (8, 4, 2)])
def test_three_targets_in_one_launch(dev, widths, form):
    rng = np.random.default_rng(sum(widths))
    for n_rows in (257, 4097, 9000):
        mask = rng.random(n_rows) < 0.5
        mask[n_rows // 2: n_rows // 2 + 300] = True              # full chunks too
        targets = [(old_values(rng, w, n_rows), VALUE[w] ^ k) for k, w in enumerate(widths)]
        run(dev, form, n_rows, mask, targets, bystanders=[old_values(rng, 2, n_rows)])


def test_predicate_on_the_bit_plane_byte_column_as_target(dev):
    """WHERE sudo_used = 1 read from the plane, SET sudo_used = 0 written to the bytes: the plane is left as it was."""
    rng = np.random.default_rng(9)
    for n_rows in (5, 1023, 4097, 33_333):
        total = padded_rows(n_rows) + GUARD
        sudo = (rng.random(total) < 0.4).astype(np.uint8)
        sudo[n_rows:] = 1
        plane = np.packbits(sudo[:padded_rows(n_rows)], bitorder="little")
        other = old_values(rng, 4, n_rows)
        run(dev, "fused", n_rows, sudo[:n_rows] == 1, [(sudo, 0), (other, 7)], pred=sel_pred(), pred_cols=[(plane, pq.WIDTH_BITS)])


def test_no_rows_launches_nothing(dev):
    rng = np.random.default_rng(1)
    old = old_values(rng, 4, 0)
    for form in ("fused", "flags"):
        run(dev, form, 0, np.zeros(0, dtype=bool), [(old, 9)])


def test_einval(dev):
    L, ctx = pq.lib(), dev.ctx
    buf = dev.upload(np.zeros(8192, dtype=np.uint64))
    cols = pq.column_array([(buf, 1)])
    good = [(buf + 4096, 4, 1)]

    def fused(triples, n=None):
        t = pq.assign_targets(triples)
        return L.pqps_filter_assign(ctx.h, cols, 1, 100, C.byref(sel_pred()), t, len(triples) if n is None else n, dev.count, None)

    def flags(triples, flags_ptr=buf):
        return L.pqps_assign_flags(ctx.h, flags_ptr, 100, pq.assign_targets(triples), len(triples), None)

    for call in (fused, flags):
        assert call(good) == 0
        assert call([]) == EINVAL                                                    # no target
        assert call([(buf + 4096, 3, 1)]) == EINVAL                                  # width
        assert call([(buf + 4096, pq.WIDTH_BITS, 1)]) == EINVAL                      # a bit plane is never a target
        assert call([(buf + 4100, 4, 1)]) == EINVAL                                  # alignment
        assert call([(None, 4, 1)]) == EINVAL
        assert call([(buf + 4096, 4, 1), (buf + 4096, 4, 2)]) == EINVAL              # the same column twice
        assert call([(buf + 4096 + 512 * k, 1, 1) for k in range(13)]) == EINVAL     # more than PQPS_MAX_COLUMNS
    assert fused(good, n=0) == EINVAL
    assert flags(good, flags_ptr=buf + 1) == EINVAL
    ctx.sync()
    dev.release()
