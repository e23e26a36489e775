"""The padded and packed layouts of encoded ids, restated in plain numpy with per-row loops: the checker of
test_layout_cpu.py / test_layout_gpu.py.  It follows the normative text of include/tgx.h (tgx_result_pad_device,
tgx_result_pack_device) line by line and shares nothing with csrc/layout.h.

Row i has the tokens ids[offs[i]:offs[i+1]].  bos / eos: None = absent; A = how many are present.
"""
import numpy as np


def _seq(tokens, bos, eos):
    return ([bos] if bos is not None else []) + [int(t) for t in tokens] + ([eos] if eos is not None else [])


def padded(ids, offs, L, pad, bos=None, eos=None, pad_left=False, trunc_left=False, dtype=np.int32):
    """-> (out [S, L] dtype, mask [S, L] u8, lengths [S] i32, n_truncated)"""
    S = len(offs) - 1
    A = (bos is not None) + (eos is not None)
    assert L >= 1 and L >= A
    out = np.full((S, L), pad, dtype=dtype)
    mask = np.zeros((S, L), np.uint8)
    lengths = np.zeros(S, np.int32)
    n_truncated = 0
    for i in range(S):
        t = ids[int(offs[i]):int(offs[i + 1])]
        n = len(t)
        keep = min(n, L - A)
        kept = t[n - keep:] if trunc_left else t[:keep]
        seq = _seq(kept, bos, eos)
        ln = keep + A
        assert len(seq) == ln
        lengths[i] = ln
        if n > L - A:
            n_truncated += 1
        if pad_left:
            out[i, L - ln:L] = seq
            mask[i, L - ln:L] = 1
        else:
            out[i, 0:ln] = seq
            mask[i, 0:ln] = 1
    return out, mask, lengths, n_truncated


def packed(ids, offs, L, pad, bos=None, eos=None, dtype=np.int32):
    """-> (out [B, L] dtype, doc [B, L] i32, pos [B, L] i32)"""
    S = len(offs) - 1
    assert L >= 1
    stream, doc, pos = [], [], []
    for i in range(S):
        seq = _seq(ids[int(offs[i]):int(offs[i + 1])], bos, eos)
        stream += seq
        doc += [i] * len(seq)
        pos += list(range(len(seq)))
    n_stream = len(stream)
    A = (bos is not None) + (eos is not None)
    assert n_stream == int(offs[-1]) + S * A
    B = -(-n_stream // L)
    tail = B * L - n_stream
    out = np.array(stream + [pad] * tail, dtype=dtype).reshape(B, L)
    doc = np.array(doc + [-1] * tail, dtype=np.int32).reshape(B, L)
    pos = np.array(pos + [0] * tail, dtype=np.int32).reshape(B, L)
    return out, doc, pos


def packed_fast(ids, offs, L, pad, bos=None, eos=None, dtype=np.int32):
    """`packed` for streams of millions of elements (np.repeat instead of Python lists); test_layout_cpu.py pins it to
    `packed` on the small cases."""
    ids = np.asarray(ids, np.int64)
    offs = np.asarray(offs, np.int64)
    S = len(offs) - 1
    A = (bos is not None) + (eos is not None)
    n = np.diff(offs)
    seq_len = n + A
    P = np.concatenate([[0], np.cumsum(seq_len)])
    n_stream = int(P[-1])
    doc = np.repeat(np.arange(S, dtype=np.int64), seq_len)
    pos = np.arange(n_stream, dtype=np.int64) - P[:-1][doc]
    has_bos = 1 if bos is not None else 0
    k = pos - has_bos
    is_tok = (k >= 0) & (k < n[doc])
    out = np.empty(n_stream, np.int64)
    out[is_tok] = ids[(offs[:-1][doc] + k)[is_tok]]
    if bos is not None:
        out[pos == 0] = bos
    if eos is not None:
        out[k == n[doc]] = eos
    B = -(-n_stream // L)
    tail = B * L - n_stream
    out = np.concatenate([out, np.full(tail, pad, np.int64)]).astype(dtype).reshape(B, L)
    doc = np.concatenate([doc, np.full(tail, -1, np.int64)]).astype(np.int32).reshape(B, L)
    pos = np.concatenate([pos, np.zeros(tail, np.int64)]).astype(np.int32).reshape(B, L)
    return out, doc, pos
