"""The numpy model of the 12-bit packed layout (tests/pack12_model.py) against a bit-by-bit reference.

The reference writes every bit of every field on its own into one Python integer -- bit 12 r + i of the buffer is bit i
of row r -- and knows nothing of bytes, pairs or dwords, so the fields that straddle a byte (every odd row) and a dword
(rows 2 and 5 of every 8) are covered by construction."""
import numpy as np
import pytest

import pack12_model as m


def reference_pack(codes, rows):
    big = 0
    for r, c in enumerate(codes):
        for i in range(12):
            if (int(c) >> i) & 1:
                big |= 1 << (12 * r + i)
    return np.frombuffer(big.to_bytes(rows * 3 // 2, "little"), dtype=np.uint8)


def reference_unpack(packed, n):
    big = int.from_bytes(bytes(packed), "little")
    return np.array([sum(((big >> (12 * r + i)) & 1) << i for i in range(12)) for r in range(n)], dtype=np.uint16)


CASES = {
    "zeros": np.zeros(19, dtype=np.uint16),
    "all_4095": np.full(24, 4095, dtype=np.uint16),
    "alternating_fff_0": np.tile(np.array([0xFFF, 0], dtype=np.uint16), 20),
    "alternating_0_fff": np.tile(np.array([0, 0xFFF], dtype=np.uint16), 20)[:37],
    "one_bit_walk": np.array([1 << (r % 12) for r in range(48)], dtype=np.uint16),
    "straddlers_only": np.array([0xFFF if r % 8 in (2, 5) else 0 for r in range(64)], dtype=np.uint16),
    "straddlers_clear": np.array([0 if r % 8 in (2, 5) else 0xFFF for r in range(64)], dtype=np.uint16),
    "edges": np.array([0, 4095, 1, 4094, 2048, 2047, 0xA5A, 0x5A5, 4095, 0], dtype=np.uint16),
    "single": np.array([0xABC], dtype=np.uint16),
    "random_1025": np.random.default_rng(12).integers(0, 4096, 1025).astype(np.uint16),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pack_and_unpack_match_the_bit_reference(name):
    codes = CASES[name]
    rows = m.padded_rows(codes.size)
    packed = m.pack(codes)
    assert packed.dtype == np.uint8 and packed.size == rows * 3 // 2
    assert np.array_equal(packed, reference_pack(codes, rows))
    assert np.array_equal(m.unpack(packed, codes.size), codes)
    assert np.array_equal(reference_unpack(packed, codes.size), codes)
    assert not m.unpack(packed, rows)[codes.size:].any()          # the padding's fields are zero


def test_eight_rows_are_three_dwords():
    codes = np.array([0x001, 0x002, 0xF03, 0x004, 0x005, 0xA06, 0x007, 0x008], dtype=np.uint16)
    d = m.pack(codes, rows=8).view("<u4")
    assert d.size == 3
    assert d[0] == (0x001 | 0x002 << 12 | (0xF03 & 0xFF) << 24)                       # row 2 straddles dwords 0 and 1
    assert d[1] == (0xF03 >> 8 | 0x004 << 4 | 0x005 << 16 | (0xA06 & 0xF) << 28)      # row 5 straddles dwords 1 and 2
    assert d[2] == (0xA06 >> 4 | 0x007 << 8 | 0x008 << 20)


def test_values_are_masked_to_twelve_bits():
    codes = np.array([0x1FFF, 0xF000, 0x8001], dtype=np.uint16)
    assert np.array_equal(m.unpack(m.pack(codes), 3), codes & 0xFFF)


def test_padded_rows():
    assert [m.padded_rows(n) for n in (0, 1, 1023, 1024, 1025)] == [1024, 1024, 1024, 1024, 2048]
    assert m.padded_rows(4097, 4096) == 8192
