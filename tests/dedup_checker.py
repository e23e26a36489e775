"""An independent restatement of exact row deduplication (include/tgx.h: the dedup block): first[k] from a Python dict
keyed by the row's bytes, and tgx_row_hash with Python integers masked to 64 bits.  Nothing here goes through the library."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0xA0761D6478BD642F


def row_bytes(data: np.ndarray, offs: np.ndarray) -> list:
    """the rows of data (u8 or u32) at offs (in elements) as bytes objects: a row of ids is its little-endian u32 bytes"""
    raw = np.ascontiguousarray(data).astype(data.dtype.newbyteorder("<"), copy=False).tobytes()
    w = data.dtype.itemsize
    return [raw[int(offs[k]) * w:int(offs[k + 1]) * w] for k in range(len(offs) - 1)]


def first_equal(data: np.ndarray, offs: np.ndarray):
    """-> (first int64[S], n_unique)"""
    seen = {}
    first = [seen.setdefault(row, k) for k, row in enumerate(row_bytes(data, offs))]
    return np.asarray(first, np.int64), len(seen)


def _mix(x: int) -> int:
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def row_hash(row: bytes, seed: int = 0) -> int:
    s = _mix((seed ^ SALT) & M64)
    n = len(row)
    acc = 0
    for j in range((n + 7) // 8):
        w = int.from_bytes(row[8 * j:8 * j + 8], "little")   # (a short last word: the missing bytes are zero)
        acc = (acc + _mix(w ^ ((j + 1) * 0x9E3779B97F4A7C15 & M64) ^ s)) & M64
    return _mix(acc ^ (n * 0xC2B2AE3D27D4EB4F & M64) ^ s)
