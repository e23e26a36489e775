"""Row selection and the seeded permutation as include/tgx.h states them (tgx_result_select, tgx_corpus_select,
tgx_shuffle_key), restated independently of csrc/select.h: a per-row slice-and-concatenate, and a stable argsort over keys
computed with numpy's wrapping uint64 arithmetic."""
import numpy as np

SALT = 0xD6E8FEB86659FD93
MASK = 2**64 - 1


def select(data, offs, rows):
    """-> (the selected rows back to back, offsets u64[M+1]); every index must be a row"""
    o = [int(x) for x in offs]
    rows = [int(r) for r in rows]
    assert all(0 <= r < len(o) - 1 for r in rows)
    parts = [data[o[r]:o[r + 1]] for r in rows]
    out = np.concatenate(parts) if parts else data[:0]
    out_offs = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        np.cumsum([o[r + 1] - o[r] for r in rows], out=out_offs[1:])
    return out.astype(data.dtype), out_offs


def keys(n, seed):
    """tgx_shuffle_key(seed, g) for g < n as uint64[n]"""
    g = np.arange(n, dtype=np.uint64)
    x = np.full(n, seed & MASK, np.uint64) ^ np.uint64(SALT) ^ (g * np.uint64(0x9E3779B97F4A7C15))
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def key(seed, g):
    """one key, in Python integers"""
    x = (seed ^ SALT ^ (g * 0x9E3779B97F4A7C15)) & MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def shuffled_rows(n, seed):
    """0 .. n-1 sorted ascending by (key, index)"""
    return np.argsort(keys(n, seed), kind="stable").astype(np.int64)
