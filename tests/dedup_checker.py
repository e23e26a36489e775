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


# ---- the same for many rows at once: numpy uint64 arithmetic, which wraps at 2^64 -------------------------------------

def mix_np(x: np.ndarray) -> np.ndarray:
    """_mix of every element of a uint64 array"""
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def row_hash_equal_length(rows: np.ndarray, seed: int = 0) -> np.ndarray:
    """tgx_row_hash of every row of rows, uint8[n, n_bytes] (rows of one length) -> uint64[n]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, n_bytes = rows.shape
    W = (n_bytes + 7) // 8
    s = np.uint64(_mix((seed ^ SALT) & M64))
    padded = np.zeros((n, 8 * W), np.uint8)          # (a short last word: the missing bytes are zero)
    padded[:, :n_bytes] = rows
    words = padded.view("<u8").astype(np.uint64)     # [n, W]
    with np.errstate(over="ignore"):
        place = np.arange(1, W + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        acc = mix_np(words ^ place[None, :] ^ s).sum(axis=1, dtype=np.uint64) if W else np.zeros(n, np.uint64)
        return mix_np(acc ^ np.uint64(n_bytes * 0xC2B2AE3D27D4EB4F & M64) ^ s)


def row_hashes(data: np.ndarray, offs: np.ndarray, seed: int = 0) -> np.ndarray:
    """tgx_row_hash of every row of data (u8 or u32) at offs (in elements) -> uint64[S]: the rows are grouped by their
    length and each group goes through row_hash_equal_length (a row of ids is its little-endian u32 bytes)"""
    raw = np.frombuffer(np.ascontiguousarray(data).astype(data.dtype.newbyteorder("<"), copy=False).tobytes(), np.uint8)
    w = data.dtype.itemsize
    begin = offs[:-1].astype(np.int64) * w
    lens = np.diff(offs.astype(np.int64)) * w
    out = np.empty(lens.size, np.uint64)
    for n_bytes in np.unique(lens):
        rows = np.flatnonzero(lens == n_bytes)
        at = begin[rows][:, None] + np.arange(int(n_bytes), dtype=np.int64)[None, :]
        out[rows] = row_hash_equal_length(raw[at], seed)
    return out
