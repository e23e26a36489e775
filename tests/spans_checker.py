"""Token spans restated in plain numpy / Python with per-row loops: the checker of test_spans_cpu.py / test_spans_gpu.py.
It follows the normative text of include/tgx.h (tgx_result_spans_device, tgx_result_pad_spans_device) line by line from
the tokens' bytes and shares nothing with csrc/spans.h.  The padded placement goes through layout_checker.padded.

`token_bytes(x)` gives the bytes of id x (special tokens included); row i has the tokens ids[offs[i]:offs[i+1]].
"""
import numpy as np

import layout_checker as lc


def _is_cont(b):
    return 0x80 <= b <= 0xBF


def row_spans(tokens, unit):
    """tokens: the row's tokens as bytes -> ([(start, end)], the row's raw text)"""
    text = b"".join(tokens)
    # c(p) = the bytes not in 80..BF among the first p bytes of the row's raw text
    c = [0] * (len(text) + 1)
    for p, byte in enumerate(text):
        c[p + 1] = c[p] + (0 if _is_cont(byte) else 1)
    out, b = [], 0
    for t in tokens:
        e = b + len(t)
        if unit == "byte":
            out.append((b, e))
        elif len(t) == 0:
            out.append((c[b], c[b]))
        else:
            out.append((c[b] - (1 if _is_cont(t[0]) else 0), c[e]))
        b = e
    return out, text


def flat(ids, offs, token_bytes, unit, dtype=np.int64):
    """-> [T, 2] of dtype"""
    S = len(offs) - 1
    out = np.zeros((int(offs[-1]) if S else 0, 2), np.int64)
    for i in range(S):
        lo, hi = int(offs[i]), int(offs[i + 1])
        sp, _ = row_spans([token_bytes(int(x)) for x in ids[lo:hi]], unit)
        if sp:
            out[lo:hi] = sp
    assert np.array_equal(out.astype(dtype), out)
    return out.astype(dtype)


def padded(ids, offs, token_bytes, unit, L, bos=None, eos=None, pad_left=False, trunc_left=False, dtype=np.int64, flat_spans=None):
    """-> [S, L, 2] of dtype: cell (i, c) holds the span of the token tgx_result_pad_device puts there, (0, 0) elsewhere.
    flat_spans: what flat(ids, offs, token_bytes, unit) returned, when the caller has it already."""
    T = int(offs[-1])
    if flat_spans is None:
        flat_spans = flat(ids, offs, token_bytes, unit)
    sp = np.concatenate([flat_spans.astype(np.int64), np.zeros((1, 2), np.int64)])   # entry T: bos, eos and padding
    where = lc.padded(np.arange(T, dtype=np.int64), offs, L, T, T if bos is not None else None, T if eos is not None else None,
                      pad_left, trunc_left, np.int64)[0]
    return sp[where].astype(dtype)


def vocab_lookup(tokens, specials=()):
    tokens, specials = list(tokens), list(specials)
    V = len(tokens)
    return lambda x: tokens[x] if x < V else specials[x - V]
