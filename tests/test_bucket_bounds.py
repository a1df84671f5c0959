"""hipBucketBounds (engine/hip/hipPredicate.c), the buckets of GROUP BY PREFIX(k) / WIDTH(w), checked on the CPU against plain
Python: a prefix bucket is a run of itertools.groupby over the sorted dictionary truncated as bytes, a width bucket is Python's
floor division -- and every refusal."""
import itertools

import pytest

import qpelib as q

pq = q.pq
PREFIXES = (1, 4, 7, 10, 13, 24, 2000)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
_dicts = {}


def dictionaries(csv):
    """column -> the sorted distinct values (bytes) of every string column of a golden CSV"""
    if csv not in _dicts:
        t = q.OracleTable(q.GOLDEN / csv, [])
        _dicts[csv] = {c: sorted({t.cell(r, c).encode("latin-1") for r in range(t.n)}) for c in q.ORC_STR}
    return _dicts[csv]


def prefix_model(values, k):
    """(bounds, keys, key texts) of PREFIX(k) over an ascending dictionary"""
    bounds, texts, at = [], [], 0
    for text, run in itertools.groupby(values, key=lambda v: v[:k]):
        bounds.append(at)
        texts.append(text)
        at += len(list(run))
    return bounds + [len(values)], bounds, texts


def check_shape(bounds, keys, domain):
    assert bounds[0] == 0 and bounds[-1] == domain and len(bounds) == len(keys) + 1
    assert all(a < b for a, b in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("csv", ["commands_2k.csv", "edge_cases.csv"])
@pytest.mark.parametrize("k", PREFIXES)
def test_prefix_buckets_of_the_golden_dictionaries(csv, k):
    for column, values in dictionaries(csv).items():
        want_bounds, want_keys, texts = prefix_model(values, k)
        bounds, keys = pq.bucket_bounds(column, pq.BUCKET_PREFIX, k, dictionary=values)
        assert (bounds, keys) == (want_bounds, want_keys), column
        check_shape(bounds, keys, len(values))
        assert [values[c][:k] for c in keys] == texts and texts == sorted(set(texts))


def test_days_and_hours_of_the_golden_timestamps():
    """The file holds 2 000 distinct timestamps over 13 months, 364 days and 1 802 hours (counted with Python sets of the
    truncated strings, which the test repeats)."""
    values = dictionaries("commands_2k.csv")["timestamp"]
    assert len(values) == 2000
    for k, n in ((7, 13), (10, 364), (13, 1802)):
        assert len({v[:k] for v in values}) == n
        assert len(pq.bucket_bounds("timestamp", pq.BUCKET_PREFIX, k, dictionary=values)[1]) == n
    # a prefix longer than every string: one bucket per value
    assert pq.bucket_bounds("timestamp", pq.BUCKET_PREFIX, 2000, dictionary=values)[0] == list(range(2001))


HAND = sorted([b"a", b"ab", b"aba", b"abb", b"abc\xc3\xa9", b"b", b"ba", b"z\x80", b"z\x80\xff", b"z\xfe", b"\x80", b"\xff\xff\xff"])


@pytest.mark.parametrize("k", (1, 2, 3, 4, 5, 100))
def test_prefix_buckets_of_a_hand_made_dictionary(k):
    """strings shorter than k, a string that is another's prefix, bytes >= 0x80 (strcmp compares unsigned bytes)"""
    want_bounds, want_keys, texts = prefix_model(HAND, k)
    bounds, keys = pq.bucket_bounds("user_name", pq.BUCKET_PREFIX, k, dictionary=HAND)
    assert (bounds, keys) == (want_bounds, want_keys)
    check_shape(bounds, keys, len(HAND))
    if k == 2:
        # "a" alone, then "ab" with "aba", "abb" and "abc.."; "b" alone before "ba"
        assert [HAND[c][:k] for c in keys][:4] == [b"a", b"ab", b"b", b"ba"]


def width_model(lo, hi, w):
    qs = range(lo // w, hi // w + 1)
    keys = [qq * w for qq in qs]
    return [max(kk, lo) - lo for kk in keys] + [hi - lo + 1], keys


WIDTH_CASES = [(-7, 9, 1), (-7, 9, 2), (-7, 9, 5), (-7, 9, 100), (INT_MIN, INT_MIN + 10, 1), (INT_MIN, INT_MIN + 10, 3),
               (INT_MIN, INT_MIN + 10, 7), (INT_MIN, INT_MIN + 10, 1 << 40), (INT_MAX - 10, INT_MAX, 1), (INT_MAX - 10, INT_MAX, 4),
               (INT_MAX - 10, INT_MAX, INT_MAX), (-70000, 70000, 3), (-70000, 70000, 1000), (-70000, 70000, 140001), (5, 5, 1),
               (0, 65535, 1), (-1, -1, 10)]


@pytest.mark.parametrize("lo,hi,w", WIDTH_CASES)
def test_width_buckets(lo, hi, w):
    want_bounds, want_keys = width_model(lo, hi, w)
    bounds, keys = pq.bucket_bounds("user_id", pq.BUCKET_WIDTH, w, lo=lo, hi=hi)
    assert (bounds, keys) == (want_bounds, want_keys)
    check_shape(bounds, keys, hi - lo + 1)
    assert len(keys) == hi // w - lo // w + 1
    # every value of the range lands in the bucket of its floor division
    for v in {lo, hi, (lo + hi) // 2, min(hi, lo + 1), max(lo, hi - 1)}:
        b = max(j for j in range(len(keys)) if bounds[j] <= v - lo)
        assert keys[b] == v // w * w


def test_a_lower_bound_below_int_min():
    bounds, keys = pq.bucket_bounds("exit_code", pq.BUCKET_WIDTH, 1000, lo=INT_MIN, hi=INT_MIN + 10)
    assert keys == [INT_MIN // 1000 * 1000] and keys[0] < INT_MIN and bounds == [0, 11]


def test_the_bucket_limit():
    """[-70000, 70000]: w = 2 gives 70 001 buckets and is refused, w = 3 gives 46 668 and is accepted"""
    with pytest.raises(pq.PqpsError):
        pq.bucket_bounds("user_id", pq.BUCKET_WIDTH, 2, lo=-70000, hi=70000)
    assert len(pq.bucket_bounds("user_id", pq.BUCKET_WIDTH, 3, lo=-70000, hi=70000)[1]) == 46668
    big = [b"%06d" % i for i in range(65537)]
    with pytest.raises(pq.PqpsError):
        pq.bucket_bounds("timestamp", pq.BUCKET_PREFIX, 6, dictionary=big)
    assert len(pq.bucket_bounds("timestamp", pq.BUCKET_PREFIX, 6, dictionary=big[:65536])[1]) == 65536
    assert len(pq.bucket_bounds("timestamp", pq.BUCKET_PREFIX, 5, dictionary=big)[1]) == 6554


REFUSED = {
    "k < 1": ("user_name", pq.BUCKET_PREFIX, 0, dict(dictionary=HAND)),
    "k negative": ("user_name", pq.BUCKET_PREFIX, -3, dict(dictionary=HAND)),
    "w < 1": ("user_id", pq.BUCKET_WIDTH, 0, dict(lo=0, hi=9)),
    "w negative": ("user_id", pq.BUCKET_WIDTH, -100, dict(lo=0, hi=9)),
    "PREFIX on a number": ("user_id", pq.BUCKET_PREFIX, 3, dict(dictionary=HAND)),
    "PREFIX on a boolean": ("sudo_used", pq.BUCKET_PREFIX, 1, dict(dictionary=HAND)),
    "WIDTH on a string": ("timestamp", pq.BUCKET_WIDTH, 10, dict(lo=0, hi=9)),
    "WIDTH on a boolean": ("sudo_used", pq.BUCKET_WIDTH, 1, dict(lo=0, hi=1)),
    "command_id, PREFIX": ("command_id", pq.BUCKET_PREFIX, 3, dict(dictionary=HAND)),
    "command_id, WIDTH": ("command_id", pq.BUCKET_WIDTH, 100, dict(lo=0, hi=9)),
    "an unknown column": ("no_such_column", pq.BUCKET_WIDTH, 100, dict(lo=0, hi=9)),
    "an unknown mode": ("user_id", 3, 100, dict(lo=0, hi=9)),
    "the whole i32 range": ("user_id", pq.BUCKET_WIDTH, 1 << 20, dict(lo=INT_MIN, hi=INT_MAX)),
    "an empty range": ("user_id", pq.BUCKET_WIDTH, 10, dict(lo=5, hi=4)),
    "an empty dictionary": ("user_name", pq.BUCKET_PREFIX, 3, dict(dictionary=[])),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals(case, capfd):
    column, mode, arg, kw = REFUSED[case]
    with pytest.raises(pq.PqpsError):
        pq.bucket_bounds(column, mode, arg, **kw)
    assert "HIP engine: buckets of" in capfd.readouterr().err     # the reason, like the other compile refusals
