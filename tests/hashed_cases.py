"""The one batch and the one reference of the hashed n-gram feature tests (include/tgx_hashed.h; csrc/hashed.hip,
csrc/hashed.h).  The reference is numpy: per distinct gram _lib.gram_key on the gram's bytes, the bucket from Python
integers, np.add.at for the accumulation."""
import functools

import numpy as np

from tokengeex_amd import _lib

KINDS = ("ids", "bytes")
DTYPE = {"ids": np.uint32, "bytes": np.uint8}
SEED = 0xC0FFEE1234567890
V = 50  # ids below it; the text's bytes come from as many letters

# Row lengths, in elements; a wave takes 64 consecutive elements.  Empty rows and rows shorter than some or every width;
# a filler to element 64; 64 one-element rows that are one chunk; a row of 64 that ends on a chunk edge (192), of 63 that
# ends before one (255), of 65 that crosses 256 and ends on 320; rows of 65 and 63 that end after (385) and on (448) an
# edge; a row of 700, eleven chunks; short rows and a last chunk of 6 elements.
LENGTHS = [0, 0, 1, 2, 4, 57] + [1] * 64 + [64, 63, 0, 65, 65, 63, 700, 3, 0, 5, 2, 0]


@functools.lru_cache(maxsize=None)
def batch(kind, lengths=tuple(LENGTHS), alphabet=V):
    """(data, offs) of the rows; read-only"""
    rng = np.random.default_rng(7)
    offs = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    data = rng.integers(0, alphabet, int(offs[-1]))
    data = data.astype(np.uint32) if kind == "ids" else (data + ord("A")).astype(np.uint8)
    data.setflags(write=False)
    offs.setflags(write=False)
    return data, offs


@functools.lru_cache(maxsize=None)
def weights(B, K):
    """Q int32[K, B] over the whole range of an i32, its ends included"""
    q = np.random.default_rng(B * 31 + K).integers(-2**31, 2**31, (K, B)).astype(np.int32)
    q.reshape(-1)[:2] = (2**31 - 1, -2**31)[:min(2, q.size)]
    q.setflags(write=False)
    return q


def reference(data, offs, widths, B, seed, q=None):
    """counts int64[B] and, under q int32[K, B], scores int64[S, K] (else None)"""
    S = len(offs) - 1
    ends = offs[1:].astype(np.int64)
    row_of = np.repeat(np.arange(S), np.diff(offs.astype(np.int64)))
    counts = np.zeros(B, np.int64)
    scores = None if q is None else np.zeros((S, q.shape[0]), np.int64)
    for w in widths:
        if data.size < w:
            continue
        win = np.lib.stride_tricks.sliding_window_view(data, w)
        ok = np.flatnonzero(np.arange(win.shape[0]) + w <= ends[row_of[:win.shape[0]]])  # the gram stays inside its row
        grams, inv = np.unique(win[ok], axis=0, return_inverse=True)
        b = np.array([(_lib.gram_key(g.tobytes(), seed) * B) >> 64 for g in grams], np.int64)[inv.reshape(-1)]
        np.add.at(counts, b, 1)
        if q is not None:
            np.add.at(scores, row_of[ok], q[:, b].T.astype(np.int64))
    return counts, scores
