"""An independent restatement of the shared n-grams (include/tgx.h: the gram block): grams as tuples in Python sets, keys
from dedup_checker.row_hash_equal_length over the stacked grams, sets with np.unique and membership with np.isin.
Nothing here goes through the library or csrc/gram.h."""
import numpy as np

import dedup_checker as dc

MINHASH_SALT = 0xD6E8FEB86659FD93


def rows_of(data: np.ndarray, offs: np.ndarray) -> list:
    return [tuple(int(x) for x in data[int(offs[k]):int(offs[k + 1])]) for k in range(len(offs) - 1)]


def row_of_element(offs: np.ndarray) -> np.ndarray:
    """-> int64[n_elems]: the row that owns every element"""
    lens = np.diff(offs.astype(np.int64))
    return np.repeat(np.arange(lens.size, dtype=np.int64), lens)


def validity(offs: np.ndarray, w: int) -> np.ndarray:
    """-> bool[n_elems]: the gram at element e is valid iff e + w <= the end of e's row"""
    lens = np.diff(offs.astype(np.int64))
    ends = np.repeat(offs[1:].astype(np.int64), lens)
    return np.arange(ends.size, dtype=np.int64) + w <= ends


def keys_at(data: np.ndarray, offs: np.ndarray, w: int, seed: int):
    """-> (valid bool[n_elems], keys uint64[valid.sum()]): the key of every valid gram, in element order"""
    valid = validity(offs, w)
    eb = data.dtype.itemsize
    raw = np.frombuffer(np.ascontiguousarray(data).astype(data.dtype.newbyteorder("<"), copy=False).tobytes(), np.uint8).reshape(-1, eb)
    at = np.flatnonzero(valid)[:, None] + np.arange(w, dtype=np.int64)[None, :]
    stacked = raw[at].reshape(at.shape[0], w * eb)
    return valid, dc.row_hash_equal_length(stacked, (seed ^ MINHASH_SALT) & dc.M64)


def keys_of(data: np.ndarray, offs: np.ndarray, w: int, seed: int = 0) -> np.ndarray:
    """the gram set of a source: ascending, distinct uint64 keys"""
    return np.unique(keys_at(data, offs, w, seed)[1])


def hits(data: np.ndarray, offs: np.ndarray, w: int, seed: int, keys: np.ndarray):
    """-> (count int64[S], mask uint8[n_elems]) of the source against a set of keys (any order)"""
    valid, mine = keys_at(data, offs, w, seed)
    mask = np.zeros(valid.size, np.uint8)
    mask[np.flatnonzero(valid)[np.isin(mine, np.asarray(keys, np.uint64))]] = 1
    count = np.bincount(row_of_element(offs)[mask == 1], minlength=len(offs) - 1).astype(np.int64)
    return count, mask


def grams_of(rows: list, w: int) -> set:
    return {r[t:t + w] for r in rows for t in range(len(r) - w + 1)}


def true_hits(data: np.ndarray, offs: np.ndarray, w: int, eval_data: np.ndarray, eval_offs: np.ndarray):
    """-> (count, mask) by tuple membership, with no hash: what the keys stand for"""
    wanted = grams_of(rows_of(eval_data, eval_offs), w)
    count = np.zeros(len(offs) - 1, np.int64)
    mask = np.zeros(int(offs[-1]), np.uint8)
    for i, r in enumerate(rows_of(data, offs)):
        for t in range(len(r) - w + 1):
            if r[t:t + w] in wanted:
                mask[int(offs[i]) + t] = 1
                count[i] += 1
    return count, mask


def distinct_grams_have_distinct_keys(sources: list, w: int, seed: int) -> bool:
    """sources: (data, offs) pairs.  No two distinct grams among them share a key: then key membership is gram membership"""
    grams, keys = set(), []
    for data, offs in sources:
        grams |= grams_of(rows_of(data, offs), w)
        keys.append(keys_at(data, offs, w, seed)[1])
    return np.unique(np.concatenate(keys)).size == len(grams) if keys else True
