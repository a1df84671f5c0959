"""numpy model of the 12-bit packed column layout (PQPS_WIDTH_P12, include/pqps_hip.h).

Row r occupies the 12 bits at bit offset 12 r of the buffer, little-endian: 8 rows are exactly 3 dwords (12 bytes).  The
buffer covers the rows rounded up to a whole number of 1024-row steps; the fields of rows at and past n are zero."""
import numpy as np

STEP_ROWS = 1024


def padded_rows(n, unit=STEP_ROWS):
    return max((n + unit - 1) // unit, 1) * unit


def pack(codes, rows=None):
    """u16 codes (each below 4096 after masking) -> the packed bytes of `rows` rows (default: n rounded up to a step)."""
    codes = np.asarray(codes, dtype=np.uint16)
    rows = padded_rows(codes.size) if rows is None else rows
    assert rows % 8 == 0 and rows >= codes.size
    v = np.zeros(rows, dtype=np.uint32)
    v[:codes.size] = codes & 0xFFF
    a, b = v[0::2], v[1::2]                                  # two rows = three bytes
    out = np.empty((rows // 2, 3), dtype=np.uint8)
    out[:, 0] = a & 0xFF
    out[:, 1] = (a >> 8) | ((b & 0xF) << 4)
    out[:, 2] = b >> 4
    return out.reshape(-1)


def unpack(packed, n):
    """The first n rows of a packed buffer as u16."""
    p = np.asarray(packed, dtype=np.uint8)[:(n + 1) // 2 * 3].reshape(-1, 3).astype(np.uint16)
    v = np.empty(p.shape[0] * 2, dtype=np.uint16)
    v[0::2] = p[:, 0] | ((p[:, 1] & 0xF) << 8)
    v[1::2] = (p[:, 1] >> 4) | (p[:, 2] << 4)
    return v[:n]
