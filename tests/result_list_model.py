"""Index mode and the result-list tail, restated in numpy from the text of include/pqps_hip.h: what pqps_index_build,
pqps_index_probe, pqps_index_select / pqps_filter_gather (the append), pqps_gather_keys, pqps_project_column, pqps_merge_slots and
pqps_merge_index_slots must leave in device memory, word for word -- and the case lists tests/test_gpu_result_list_shim.py runs.

No function here copies a kernel's arithmetic: the probe is numpy.searchsorted, the index order is qpelib.host_index_order (a
stable argsort of the rows fed in descending order), the merges are concatenations and numpy.lexsort.  Every reference has a
row-by-row twin (`*_slow`) that tests/test_result_list_model.py compares it with, and that file checks every case list for the
edges it is there for.  Nothing here needs a GPU.
"""
import functools
import zlib

import numpy as np

import qpelib as q

U32, TOP32, U64 = 1 << 32, 0xFFFFFFFF, (1 << 64) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
PQPS_OK, PQPS_EINVAL, PQPS_EOVERFLOW = 0, -1, -5
HEADER_WORDS = 4                                # PQPS_SLOT_HEADER_WORDS: [u64 count][u64 reserved] in front of a slot's IDs
HIGH_BASE = 4_000_000_000                       # an id_base that puts every ID above 2^31
WRAP_BASE = U32 - 1000                          # ... and one past which row + id_base wraps (rows 1000 and up)
A5_32, A5_64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5   # what every output buffer holds before a call
MARK_ID, MARK_KEY = 0xDEADBEEF, 0x0123456789ABCDEF   # what a slot holds behind its count: never part of an answer
HUGE = 1 << 40                                  # a count far above any capacity

# key type -> (numpy type, key_kind of the header: 1 = signed i32)
TYPES = {"u8": (np.uint8, 0), "u16": (np.uint16, 0), "u32": (np.uint32, 0), "i32": (np.int32, 1), "u64": (np.uint64, 0)}
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def rng(*key):
    return np.random.default_rng([0x1DE7, zlib.crc32(repr(key).encode())])


def dtype_of(t):
    return TYPES[t][0]


def kind_of(t):
    return TYPES[t][1]


def width_of(t):
    return np.dtype(TYPES[t][0]).itemsize


def mask_of(t):
    return (1 << (8 * width_of(t))) - 1


def type_min(t):
    return int(np.iinfo(dtype_of(t)).min)


def type_max(t):
    return int(np.iinfo(dtype_of(t)).max)


def as_key(raw, t):
    """A raw 64-bit pattern as the key it stands for: its low `width` bytes, in the key's own type."""
    return np.array([raw & mask_of(t)], dtype=np.uint64).astype(UNSIGNED[width_of(t)]).view(dtype_of(t))[0]


def raw_zero(value, t):
    """A key as a raw pattern, zero-extended."""
    return int(value) & mask_of(t)


def raw_sign(value, t):
    """A key as a raw pattern, sign-extended (differs from raw_zero for negative i32 keys only)."""
    return int(value) & U64


def from_image(img, t):
    """Unsigned order-preserving images (u64) -> the keys in their own type."""
    raw = img ^ np.uint64(0x80000000) if kind_of(t) else img
    return raw.astype(UNSIGNED[width_of(t)]).view(dtype_of(t))


# ---- the references ---------------------------------------------------------------------------------------------------------
def index_order(keys):
    """Row numbers sorted by (key ascending, row DESCENDING); the sorted keys are keys[order]."""
    return q.host_index_order(keys)


def index_order_slow(keys):
    vals = keys.tolist()
    return np.array(sorted(range(len(vals)), key=lambda r: (vals[r], -r)), dtype=np.int64)


def probe(sorted_keys, lo, hi):
    """(first position with key >= lo, first position with key > hi, not below the former), compared in the keys' own type."""
    b = int(np.searchsorted(sorted_keys, sorted_keys.dtype.type(lo), side="left"))
    e = int(np.searchsorted(sorted_keys, sorted_keys.dtype.type(hi), side="right"))
    return b, max(b, e)


def probe_slow(sorted_keys, lo, hi):
    vals, lo, hi = sorted_keys.tolist(), int(lo), int(hi)
    b = next((i for i, v in enumerate(vals) if v >= lo), len(vals))
    e = next((i for i, v in enumerate(vals) if v > hi), len(vals))
    return b, e if e > b else b


def select_append(out, count, perm, b, e, passes, id_base, capacity):
    """One probe's rows appended: the rows of perm[b:e] that pass (`passes`: a mask over the table, None = all), + id_base
    mod 2^32, at out[count ...), cut at `capacity`; -> the new count, which advances by what there was.  `out` is written in place."""
    rows = perm[b:e].astype(np.int64)
    if passes is not None:
        rows = rows[passes[rows]]
    ids = ((rows + id_base) % U32).astype(np.uint32)
    room = min(max(capacity - count, 0), len(ids))
    out[count:count + room] = ids[:room]
    return count + len(ids)


def select_append_slow(out, count, perm, b, e, passes, id_base, capacity):
    for i in range(b, e):
        r = int(perm[i])
        if passes is None or passes[r]:
            if count < capacity:
                out[count] = (r + id_base) & TOP32
            count += 1
    return count


def key_image(values, signed):
    """The order-preserving u64 image of pqps_gather_keys: the value zero-extended, a signed i32 with its sign bit flipped."""
    if signed:
        return (values.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return values.astype(np.uint64)


def key_image_slow(values, signed):
    return np.array([int(v) + (1 << 31) if signed else int(v) for v in values.tolist()], dtype=np.uint64)


def project(col, ids, id_base, count, capacity):
    """out[i] = col[ids[i] - id_base] (32-bit arithmetic) for the first min(count, capacity) entries."""
    n = min(count, capacity)
    return col[(ids[:n].astype(np.int64) - id_base) % U32]


def project_slow(col, ids, id_base, count, capacity):
    vals, out = col.tolist(), []
    for i in range(len(ids)):
        if i < count and i < capacity:
            out.append(vals[(int(ids[i]) - id_base) & TOP32])
    return np.array(out, dtype=col.dtype)


def slot_reported(slots, world, stride):
    """The u64 counts at the head of `world` slots `stride` u32 words apart."""
    return [int(slots[r * stride:r * stride + 2].view(np.uint64)[0]) for r in range(world)]


def compact_slots(slots, key_slots, world, stride):
    """-> (IDs, keys or None, totals): the first min(reported, stride - 4) IDs of every slot in rank order, and the keys that go
    with them -- rank r's keys begin at key_slots[r * (stride - 4)]; totals = [IDs held, IDs reported (mod 2^64)]."""
    seg = stride - HEADER_WORDS
    reported = slot_reported(slots, world, stride)
    held = [min(c, seg) for c in reported]
    ids = [slots[r * stride + HEADER_WORDS:r * stride + HEADER_WORDS + held[r]] for r in range(world)]
    keys = None if key_slots is None else np.concatenate([key_slots[r * seg:r * seg + held[r]] for r in range(world)])
    return np.concatenate(ids), keys, np.array([sum(held), sum(reported) & U64], dtype=np.uint64)


def merge_slots(slots, world, stride, merged_capacity):
    """-> (what `merged` holds from word 0 on: the first merged_capacity IDs of the rank-order concatenation, totals)."""
    ids, _, totals = compact_slots(slots, None, world, stride)
    return ids[:merged_capacity], totals


def merge_slots_slow(slots, world, stride, merged_capacity):
    words, seg, out, held, raw = slots.tolist(), stride - HEADER_WORDS, [], 0, 0
    for r in range(world):
        reported = words[r * stride] | (words[r * stride + 1] << 32)
        raw += reported
        for i in range(seg):
            if i < reported:
                held += 1
                if len(out) < merged_capacity:
                    out.append(words[r * stride + HEADER_WORDS + i])
    return np.array(out, dtype=np.uint32), np.array([held, raw & U64], dtype=np.uint64)


def merge_index_slots(slots, key_slots, world, stride, merged_capacity):
    """-> (return code, merged or None, totals): the compacted IDs sorted by (key ascending, id DESCENDING), whatever order a
    slot holds them in; with more IDs than merged_capacity PQPS_EOVERFLOW, `merged` untouched (None), totals still written."""
    ids, keys, totals = compact_slots(slots, key_slots, world, stride)
    if len(ids) > merged_capacity:
        return PQPS_EOVERFLOW, None, totals
    order = np.lexsort((TOP32 - ids.astype(np.int64), keys))
    return PQPS_OK, ids[order], totals


def merge_index_slots_slow(slots, key_slots, world, stride, merged_capacity):
    words, keys, seg, pairs, raw = slots.tolist(), key_slots.tolist(), stride - HEADER_WORDS, [], 0
    for r in range(world):
        reported = words[r * stride] | (words[r * stride + 1] << 32)
        raw += reported
        for i in range(min(reported, seg)):
            pairs.append((keys[r * seg + i], -words[r * stride + HEADER_WORDS + i]))
    totals = np.array([len(pairs), raw & U64], dtype=np.uint64)
    if len(pairs) > merged_capacity:
        return PQPS_EOVERFLOW, None, totals
    return PQPS_OK, np.array([-p[1] for p in sorted(pairs)], dtype=np.uint32), totals


# ---- pqps_index_build: the case list ----------------------------------------------------------------------------------------
BUILD_NS = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, 70_001)
PATTERN = 0x5A5A5A5A5A5A5A5A


def build_contents(t):
    """equal (no pass); bytes 0 .. k differ, k = 0 .. width - 1 (k + 1 passes); only the top byte differs (`width` passes);
    full-range random with the type's minimum and maximum; heavy duplicates; for i32 both signs with the four named values."""
    return ("equal",) + tuple(("bytes", k) for k in range(width_of(t))) + ("top", "random", "dups") + (("signs",) if t == "i32" else ())


@functools.lru_cache(maxsize=None)
def build_keys(t, content, n):
    w, mask, r = width_of(t), mask_of(t), rng("build", t, content, n)
    if content == "equal":
        img = np.full(n, PATTERN & mask, dtype=np.uint64)
    elif content == "random":
        img = r.integers(0, mask, n, dtype=np.uint64, endpoint=True)
        if n >= 2:
            img[r.permutation(n)[:2]] = (0, mask)                # the type's minimum and maximum
    elif content == "dups":
        img = np.array([0, 1, mask // 2, mask - 1, mask], dtype=np.uint64)[r.integers(0, 5, n)]
    elif content == "signs":
        named = key_image(np.array([I32_MIN, -1, 0, I32_MAX], dtype=np.int32), True)
        img = np.where(r.random(n) < 0.5, named[r.integers(0, 4, n)], r.integers(0, mask, n, dtype=np.uint64, endpoint=True))
        if n >= 4:
            img[r.permutation(n)[:4]] = named
    else:
        low = 8 * (w - 1) if content == "top" else 0            # the first bit that varies
        high = 8 * w if content == "top" else 8 * (content[1] + 1)
        span = ((1 << high) - 1) & ~((1 << low) - 1)
        img = np.uint64(PATTERN & mask & ~span) | (r.integers(0, (1 << (high - low)) - 1, n, dtype=np.uint64, endpoint=True) << np.uint64(low))
        if n >= 2:                                               # the highest varying byte does differ
            at = r.permutation(n)[:2]
            img[at[0]], img[at[1]] = PATTERN & mask & ~span, (PATTERN & mask & ~span) | span
    keys = from_image(img.astype(np.uint64), t)
    keys.setflags(write=False)
    return keys


def sort_passes(keys, t):
    """Passes of an 8-bit LSD sort that skips the bytes above the highest one in which two keys differ."""
    if len(keys) < 2:
        return 0
    img = key_image(keys, kind_of(t) == 1)
    return (int(img.min() ^ img.max()).bit_length() + 7) // 8


def build_cases(t):
    return tuple((content, n) for content in build_contents(t) for n in BUILD_NS)


# ---- pqps_index_probe: the case list ------------------------------------------------------------------------------------------
PROBE_NS = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 262_143, 262_144, 262_145)


def probe_kinds(t):
    """arange(n): every position a boundary; arange(n) // 3: runs of equal keys; for i32 also arange(n) - n // 2: both signs."""
    return ("arange", "thirds") + (("centred",) if t == "i32" else ())


@functools.lru_cache(maxsize=None)
def probe_index(t, kind, n):
    """The sorted keys of the index (values modulo the type's range)."""
    a = np.arange(n, dtype=np.int64)
    a = a // 3 if kind == "thirds" else a - n // 2 if kind == "centred" else a
    raw = a if width_of(t) == 8 else a % (mask_of(t) + 1)          # (a negative key: its two's complement pattern)
    keys = np.sort(raw.astype(np.uint64).astype(UNSIGNED[width_of(t)]).view(dtype_of(t)))
    keys.setflags(write=False)
    return keys


def probe_positions(n):
    c = (n + 63) // 64
    return sorted({p for p in (0, 1, 62, 63, 64, 65, c - 1, c, c + 1, n - 2, n - 1) if 0 <= p < n})


@functools.lru_cache(maxsize=None)
def probe_windows(t, kind, n):
    """(key_lo, key_hi) as raw 64-bit patterns: every pair of the keys at the named positions (lo > hi among them); a key below
    the smallest and one above the largest; the type's extremes, for i32 zero- and sign-extended."""
    keys, out = probe_index(t, kind, n), []
    at = [int(keys[p]) for p in probe_positions(n)]
    out += [(raw_zero(a, t), raw_zero(b, t)) for a in at for b in at]
    lo, hi = (int(keys[0]), int(keys[-1])) if n else (5, 5)
    if lo > type_min(t):
        out += [(raw_zero(lo - 1, t), raw_zero(lo - 1, t)), (raw_sign(lo - 1, t), raw_zero(lo, t))]
    if hi < type_max(t):
        out += [(raw_zero(hi + 1, t), raw_zero(hi + 1, t)), (raw_zero(hi, t), raw_sign(hi + 1, t)), (raw_zero(lo, t), raw_zero(hi + 1, t))]
    mn, mx = type_min(t), type_max(t)
    for ext in (raw_zero, raw_sign):
        out += [(ext(mn, t), ext(mx, t)), (ext(mx, t), ext(mn, t)), (ext(mn, t), ext(mn, t)), (ext(mx, t), ext(mx, t))]
        out += [(ext(mn, t), raw_zero(lo, t)), (raw_zero(hi, t), ext(mx, t)), (ext(mx, t), raw_zero(lo, t))]
    return tuple(dict.fromkeys(out))


def probe_cases(t):
    return tuple((kind, n) for kind in probe_kinds(t) for n in PROBE_NS)


# ---- select / append: the case list ---------------------------------------------------------------------------------------------
SELECT_TABLES = ("i32", "u8")                                    # a 70 001-row i32 index with both signs, a 1 025-row u8 index
SELECT_LENGTHS = tuple(range(10)) + (1023, 1024, 1025)
SELECT_PRESETS = (0, 1, 3, 1000)
SELECT_BASES = (0, HIGH_BASE)
SELECT_PLACES = ("below", "equal", "inside", "end", "beyond")
SELECT_PATHS = ("gather", "gather_flag", "copy")                 # probe + filter_gather (the probed comparison; a flag column); index_select


@functools.lru_cache(maxsize=None)
def select_table(name):
    """-> (key type, key column, flag column (u8, 0 / 1), perm, sorted keys)."""
    r = rng("select", name)
    if name == "i32":                                            # distinct keys three apart: every [b, e) is a window, every gap an empty one
        n = 70_001
        keys = ((r.permutation(n) - 35_000) * 3).astype(np.int64)
        keys[np.argmin(keys)], keys[np.argmax(keys)] = I32_MIN, I32_MAX
        keys = keys.astype(np.int32)
    else:                                                        # twenty single rows, one run of 1003, two single rows
        counts = {v: 1 for v in range(20)}
        counts.update({200: 1003, 254: 1, 255: 1})
        keys = r.permutation(np.repeat(np.array(list(counts), dtype=np.uint8), list(counts.values())))
    flag = r.integers(0, 2, len(keys)).astype(np.uint8)
    order = index_order(keys)
    for a in (keys, flag, order):
        a.setflags(write=False)
    return name, keys, flag, order.astype(np.uint32), keys[order]


@functools.lru_cache(maxsize=None)
def select_windows(name):
    """(key_lo, key_hi, b, e): raw patterns and the positions they select; lo <= hi in every one (an empty window lies in a gap)."""
    t, _, _, _, skeys = select_table(name)
    n, out = len(skeys), []
    if name == "i32":
        spans = [(b, b + ln) for ln in SELECT_LENGTHS for b in (2, 7, 12, n - ln - 1, n - ln) if ln or b < n] + [(0, n)]
        for i, (b, e) in enumerate(dict.fromkeys(spans)):
            lo, hi = (int(skeys[b]), int(skeys[e - 1])) if e > b else (int(skeys[b]) - 2, int(skeys[b]) - 1)
            ext = raw_sign if i % 2 else raw_zero
            out.append((ext(lo, t), ext(hi, t), b, e))
    else:
        edges = list(range(22)) + [100, 150, 199, 200, 201, 253, 254, 255]
        for lo in edges:
            for hi in edges:
                b, e = probe(skeys, lo, hi)
                if lo <= hi and e - b in SELECT_LENGTHS:
                    out.append((lo, hi, b, e))
    assert all(probe(skeys, as_key(lo, t), as_key(hi, t)) == (b, e) and as_key(lo, t) <= as_key(hi, t) for lo, hi, b, e in out)
    return tuple(out)


def place_capacity(place, preset, rows):
    """out_capacity for a probe that appends `rows` IDs at `preset`; None where the place does not exist."""
    if place == "below":
        return preset - 1 if preset else None
    if place == "inside":
        return preset + rows // 2 if rows >= 2 else None
    return {"equal": preset, "end": preset + rows, "beyond": preset + rows + 7}[place]


@functools.lru_cache(maxsize=None)
def select_cases(name):
    """Single probes: every window x preset count x capacity place, id_base in turn -> (window index, preset, id_base, place)."""
    out, i = [], 0
    for wi in range(len(select_windows(name))):
        for pi, preset in enumerate(SELECT_PRESETS):
            for place in SELECT_PLACES:
                out.append((wi, preset, SELECT_BASES[(wi + pi + i // 3) % 2], place))
                i += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def select_sequences(name):
    """Three probes into one buffer -> (three window indexes, preset, id_base, place): the capacity is placed by the SECOND probe's rows
    (`below`: inside the first's), so that the probes behind it append nothing and still count."""
    r, ws, out = rng("sequences", name), select_windows(name), []
    some = [i for i, w in enumerate(ws) if 2 <= w[3] - w[2] <= 1025]
    for k, place in enumerate(("below", "equal", "inside", "end", "beyond") * 4):
        out.append((tuple(int(x) for x in r.choice(some, 3)), SELECT_PRESETS[k % 4], SELECT_BASES[(k // 4) % 2], place))
    return tuple(out)


def sequence_capacity(place, preset, rows):
    """rows = what each of the three probes appends."""
    first = preset + rows[0]
    if place == "below":
        return preset + rows[0] // 2
    return {"equal": first, "inside": first + rows[1] // 2, "end": first + rows[1], "beyond": first + sum(rows[1:]) + 7}[place]


# ---- pqps_gather_keys / pqps_project_column: the case list -----------------------------------------------------------------------
LIST_ROWS = 5000
LIST_MS = (0, 1, 255, 256, 257)                                   # + one list longer than the capped grid (CUs known on the device only)
LIST_BASES = (0, HIGH_BASE, WRAP_BASE)
LIST_COUNTS = ("below", "equal", "huge")                          # *count_dev against capacity = the list's length


@functools.lru_cache(maxsize=None)
def list_column(t):
    """5 000 rows, full-range random, with the type's extremes (for i32: INT_MIN, -1, 0, INT_MAX) in several rows."""
    r, mask = rng("column", t), mask_of(t)
    img = r.integers(0, mask, LIST_ROWS, dtype=np.uint64, endpoint=True)
    col = from_image(img, t).copy()
    named = [type_min(t), type_max(t)] + ([-1, 0, 1] if t == "i32" else [1])
    col[r.permutation(LIST_ROWS)[:20 * len(named)]] = np.array([v & mask for v in named] * 20, dtype=np.uint64).astype(UNSIGNED[width_of(t)]).view(dtype_of(t))
    col.setflags(write=False)
    return col


@functools.lru_cache(maxsize=None)
def list_rows(m):
    """m rows of the column in shuffled order, every fifth listed twice; the named rows among them."""
    r = rng("rows", m)
    rows = r.integers(0, LIST_ROWS, m)
    rows[::5] = rows[r.integers(0, max(m, 1), len(rows[::5]))] if m else rows[::5]
    if m >= 255:
        rows[r.permutation(m)[:4]] = (0, 999, 1000, LIST_ROWS - 1)   # both sides of the row at which WRAP_BASE wraps
    rows.setflags(write=False)
    return rows


def list_ids(m, id_base):
    return ((list_rows(m) + id_base) % U32).astype(np.uint32)


def long_list(grid_blocks_per_cu, cus):
    """The shortest list that takes a grid-stride turn: blocks capped at grid_blocks_per_cu x CUs, 256 entries each, plus one."""
    return grid_blocks_per_cu * cus * 256 + 1


def list_count(how, m):
    return {"below": max(m - 1, 0), "equal": m, "huge": HUGE}[how]


def list_cases(long_m):
    """-> (m, id_base, count): the short lists with every base and count, the long one with every count (bases in turn)."""
    out = [(m, base, how) for m in LIST_MS for base in LIST_BASES for how in LIST_COUNTS]
    return tuple(out + [(long_m, LIST_BASES[i], how) for i, how in enumerate(LIST_COUNTS)])


# ---- the two merges: the case lists ------------------------------------------------------------------------------------------------
MERGE_LAYOUTS = ((1, 6), (2, 6), (3, 258), (8, 4100), (1024, 10), (2, 262_144 + 260))       # (world, slot_stride)
INDEX_LAYOUTS = tuple((w, 8) if w == 1024 else (w, s) for w, s in MERGE_LAYOUTS)
COUNT_PATTERNS = ("empty", "first_empty", "middle_empty", "last_empty", "full", "over_one", "over_huge", "below_full", "mixed", "ones")
CAPACITY_PLACES = ("zero", "short", "exact", "spare")             # merged_capacity 0, total - 1, total, total + 7
KEY_SETS = ("equal", "byte0", "bytes01", "byte7", "random", "signed5")
ID_MODES = ("leaf", "leaf_high", "shuffled", "shuffled_high")     # the order inside a slot; IDs below / above 2^31
INDEX_TOTALS = (0, 1, 2, 4095, 4096, 4097, 70_001)


def pattern_counts(pattern, world, stride, seed=0):
    """The reported count of every slot; the values come from {0, 1, seg_cap - 1, seg_cap, seg_cap + 1, 2^40}."""
    seg = stride - HEADER_WORDS
    values = (0, 1, seg - 1, seg, seg + 1, HUGE)
    c = [seg] * world
    if pattern == "empty":
        c = [0] * world
    elif pattern == "first_empty":
        c[0] = 0
    elif pattern == "middle_empty":
        c[world // 2] = 0
        if world > 4:
            c[world // 2 - 1] = 0
    elif pattern == "last_empty":
        c[-1] = 0
    elif pattern == "over_one":
        c = [seg - 1] * world
        c[world // 2] = seg + 1
    elif pattern == "over_huge":
        c = [1] * world
        c[0] = HUGE
    elif pattern == "below_full":
        c = [seg - 1] * world
    elif pattern == "ones":
        c = [1] * world
    elif pattern == "mixed":
        c = [values[i] for i in rng("mixed", world, stride, seed).integers(0, 6, world)]
    return tuple(c)


def capacity_of(place, total):
    return {"zero": 0, "short": max(total - 1, 0), "exact": total, "spare": total + 7}[place]


def merge_cases():
    """-> (world, stride, counts, capacity place, totals given)."""
    out = []
    for world, stride in MERGE_LAYOUTS:
        for pattern in COUNT_PATTERNS:
            for place in CAPACITY_PLACES:
                for given in (True, False):
                    out.append((world, stride, pattern_counts(pattern, world, stride), place, given))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plain_slots(world, stride, counts):
    """`world` slots of random IDs (never a marker, never the fill); MARK_ID in the reserved words and behind every count."""
    r = rng("slots", world, stride, counts)
    seg = stride - HEADER_WORDS
    slots = np.full(world * stride, MARK_ID, dtype=np.uint32)
    for k, c in enumerate(counts):
        slots[k * stride:k * stride + 2] = np.array([c], dtype=np.uint64).view(np.uint32)
        held = min(c, seg)
        slots[k * stride + HEADER_WORDS:k * stride + HEADER_WORDS + held] = r.integers(0, 0xA0000000, held, dtype=np.uint32)
    slots.setflags(write=False)
    return slots


@functools.lru_cache(maxsize=None)
def key_column(key_set, n_rows):
    """The keys of a table of n_rows rows as images (u64); for signed5 also the i32 column pqps_gather_keys makes them from."""
    r = rng("keys", key_set, n_rows)
    if key_set == "signed5":
        col = np.array([I32_MIN, -1, 0, 1, I32_MAX], dtype=np.int32)[r.integers(0, 5, n_rows)]
        return key_image(col, True), col
    if key_set == "equal":
        img = np.full(n_rows, PATTERN, dtype=np.uint64)
    elif key_set == "random":
        img = r.integers(0, U64, n_rows, dtype=np.uint64, endpoint=True)
        img[r.permutation(n_rows)[:2]] = (0, U64)
    else:
        low, high = {"byte0": (0, 8), "bytes01": (0, 16), "byte7": (56, 64)}[key_set]
        span = ((1 << high) - 1) & ~((1 << low) - 1)
        img = np.uint64(PATTERN & ~span) | (r.integers(0, 1 << (high - low), n_rows, dtype=np.uint64) << np.uint64(low))
        img[r.permutation(n_rows)[:2]] = (PATTERN & ~span, PATTERN | span)
    return img, None


def index_slots(world, stride, counts, key_set, id_mode):
    """-> (slots, key_slots, id_base, the i32 column or None).  Rank r holds rows of [r * seg_cap, (r + 1) * seg_cap): a higher
    rank's rows are higher rows.  Inside a slot the rows are in leaf order (key ascending, row descending) or shuffled.  Behind a
    slot's count: MARK_ID and MARK_KEY.  key_slots is `world` x seg_cap u64, a rank's keys seg_cap apart."""
    r = rng("index_slots", world, stride, counts, key_set, id_mode)
    seg = stride - HEADER_WORDS
    id_base = HIGH_BASE if id_mode.endswith("high") else 0
    img, col = key_column(key_set, world * seg)
    slots = np.full(world * stride, MARK_ID, dtype=np.uint32)
    key_slots = np.full(world * seg, MARK_KEY, dtype=np.uint64)
    for k, c in enumerate(counts):
        slots[k * stride:k * stride + 2] = np.array([c], dtype=np.uint64).view(np.uint32)
        held = min(c, seg)
        rows = k * seg + r.permutation(seg)[:held]
        if id_mode.startswith("leaf"):
            rows = rows[np.lexsort((-rows, img[rows]))]
        slots[k * stride + HEADER_WORDS:k * stride + HEADER_WORDS + held] = rows + id_base
        key_slots[k * seg:k * seg + held] = img[rows]
    slots.setflags(write=False)
    key_slots.setflags(write=False)
    return slots, key_slots, id_base, col


def total_counts(total, world, stride):
    """Counts of `world` slots that hold `total` IDs together: the first and the last slot half each where one slot could hold
    them all, the slots filled in turn otherwise."""
    seg = stride - HEADER_WORDS
    if world > 1 and total <= seg:
        return (total // 2,) + (0,) * (world - 2) + (total - total // 2,)
    c = tuple(min(seg, max(total - k * seg, 0)) for k in range(world))
    assert sum(c) == total, (total, world, stride)
    return c


def index_merge_cases():
    """-> (world, stride, counts, key set, id mode, capacity place).  Small layouts: every pattern x key set x id mode at `exact`
    and the other places in turn; the 262 400-ID layout: every pattern once, key sets and id modes in turn; the named totals."""
    out, i = [], 0
    for world, stride in INDEX_LAYOUTS:
        big = stride > 100_000
        for pattern in COUNT_PATTERNS:
            counts = pattern_counts(pattern, world, stride)
            for ki, key_set in enumerate(KEY_SETS):
                for mi, id_mode in enumerate(ID_MODES):
                    if big and (ki, mi) != (i % len(KEY_SETS), i % len(ID_MODES)):
                        continue
                    out.append((world, stride, counts, key_set, id_mode, ("exact", "spare", "exact", "short", "exact", "zero")[(i + ki + mi) % 6]))
            i += 1
    for total, (world, stride) in ((0, (2, 6)), (1, (2, 6)), (2, (2, 6)), (1, (3, 258)), (2, (3, 258)), (4095, (8, 4100)), (4096, (8, 4100)),
                                   (4097, (8, 4100)), (4095, (1024, 8)), (4096, (1024, 8)), (4097, (2, 262_404)), (70_001, (2, 262_404))):
        for ki, key_set in enumerate(KEY_SETS):
            out.append((world, stride, total_counts(total, world, stride), key_set, ID_MODES[(ki + total) % 4], "exact"))
    return tuple(out)
