"""An independent restatement of the near-duplicate block of include/tgx.h, straight from its definitions: shingles are
slices of a row (no tiles, no chunks), the shingle hash is dedup_checker.row_hash (Python integers masked to 64 bits),
the permutations are numpy uint64 arithmetic (which wraps at 2^64), the buckets are dicts and the chains are followed one
step at a time.  It also gives the true Jaccard similarity of two rows' shingle sets.  Nothing here goes through the
library."""
import numpy as np

from dedup_checker import M64, _mix, row_hash, row_hash_equal_length

SALT = 0xD6E8FEB86659FD93
G = 0x9E3779B97F4A7C15


def rows_of(data, offs):
    """the rows of data at offs (in elements) as tuples of ints"""
    flat = [int(x) for x in data]
    return [tuple(flat[int(offs[k]):int(offs[k + 1])]) for k in range(len(offs) - 1)]


def shingles(row, w):
    """the shingles of a row, in order: m = max(1, n - w + 1) slices of min(w, n) elements"""
    n = len(row)
    return [tuple(row)] if n < w else [tuple(row[t:t + w]) for t in range(n - w + 1)]


def jaccard(row_a, row_b, w):
    a, b = set(shingles(row_a, w)), set(shingles(row_b, w))
    return len(a & b) / len(a | b)


def shingle_hash(sh, elem_bytes, seed=0):
    return row_hash(b"".join(int(x).to_bytes(elem_bytes, "little") for x in sh), (seed ^ SALT) & M64)


def perms(n_perm, seed=0):
    """-> (a, b): uint64[K] each"""
    s = _mix((seed ^ SALT) & M64)
    a = [_mix(s ^ ((2 * k + 1) * G & M64)) | 1 for k in range(n_perm)]
    b = [_mix(s ^ ((2 * k + 2) * G & M64)) for k in range(n_perm)]
    return np.asarray(a, np.uint64), np.asarray(b, np.uint64)


def value(h, k, seed=0):
    s = _mix((seed ^ SALT) & M64)
    a = _mix(s ^ ((2 * k + 1) * G & M64)) | 1
    b = _mix(s ^ ((2 * k + 2) * G & M64))
    return ((a * h + b) & M64) >> 32


def signatures(data, offs, w, n_perm, seed=0):
    """-> uint32[S, K]"""
    elem_bytes = np.asarray(data).dtype.itemsize
    a, b = perms(n_perm, seed)
    seen = {}
    sig = np.empty((len(offs) - 1, n_perm), np.uint32)
    with np.errstate(over="ignore"):
        for i, row in enumerate(rows_of(data, offs)):
            hs = []
            for sh in set(shingles(row, w)):
                if sh not in seen:
                    seen[sh] = shingle_hash(sh, elem_bytes, seed)
                hs.append(seen[sh])
            h = np.asarray(hs, np.uint64)
            v = (a[None, :] * h[:, None] + b[None, :]) >> np.uint64(32)
            sig[i] = v.min(axis=0).astype(np.uint32)
    return sig


def band_keys(sig, bands, seed=0):
    """-> uint64[S, B]"""
    S, K = sig.shape
    r = K // bands
    keys = np.empty((S, bands), np.uint64)
    for i in range(S):
        for b in range(bands):
            raw = sig[i, b * r:(b + 1) * r].astype("<u4").tobytes()
            keys[i, b] = row_hash(raw, ((seed ^ SALT) + b + 1) & M64)
    return keys


def heads_of(keys):
    """-> int64[S, B]: the first row with the same key in the band"""
    S, B = keys.shape
    heads = np.empty((S, B), np.int64)
    for b in range(B):
        seen = {}
        for i in range(S):
            heads[i, b] = seen.setdefault(int(keys[i, b]), i)
    return heads


def near_first(sig, heads, min_agree):
    """-> (first int64[S], n_clusters, first0)"""
    S, _ = sig.shape
    first0 = np.arange(S, dtype=np.int64)
    for i in range(S):
        ok = [int(j) for j in set(heads[i].tolist()) if j < i and int((sig[i] == sig[j]).sum()) >= min_agree]
        first0[i] = min([i] + ok)
    first = first0.copy()
    for i in range(S):
        j = i
        while first0[j] != j:
            j = int(first0[j])
        first[i] = j
    return first, int((first == np.arange(S)).sum()), first0


# ---- the same for many rows at once: numpy uint64 arithmetic, which wraps at 2^64 -------------------------------------

def band_keys_np(sig, bands, seed=0):
    """band_keys, a band of every row at a time -> uint64[S, B]"""
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    S, K = sig.shape
    r = K // bands
    keys = np.empty((S, bands), np.uint64)
    for b in range(bands):
        raw = np.ascontiguousarray(sig[:, b * r:(b + 1) * r].astype("<u4")).view(np.uint8).reshape(S, 4 * r)
        keys[:, b] = row_hash_equal_length(raw, ((seed ^ SALT) + b + 1) & M64)
    return keys


def heads_of_np(keys):
    """heads_of -> int64[S, B]: numpy's unique gives the first row of every key"""
    S, B = keys.shape
    heads = np.empty((S, B), np.int64)
    for b in range(B):
        _, first_row, inverse = np.unique(keys[:, b], return_index=True, return_inverse=True)
        heads[:, b] = first_row[inverse.reshape(-1)]
    return heads


def near_first_memo(sig, heads, min_agree):
    """near_first for many rows -> (first int64[S], n_clusters, first0): first0 a band of every row at a time, and the
    roots in ascending order of the rows, each from the root of the earlier row it points to (first0[i] <= i).  A head
    that is no row before i is not followed, whatever its value."""
    sig = np.asarray(sig)
    heads = np.asarray(heads, np.int64)
    S, _ = sig.shape
    me = np.arange(S, dtype=np.int64)
    first0 = me.copy()
    for b in range(heads.shape[1]):
        h = heads[:, b]
        before = (h >= 0) & (h < me)
        j = np.where(before, h, 0)
        takes = before & ((sig == sig[j]).sum(axis=1) >= min_agree)
        first0 = np.minimum(first0, np.where(takes, h, me))
    root = first0.tolist()
    for i in range(S):
        if root[i] != i:
            root[i] = root[root[i]]
    first = np.asarray(root, np.int64).reshape(S)
    return first, int((first == me).sum()), first0
