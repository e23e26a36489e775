"""Overflow windows restated in plain numpy / Python: the checker of test_windows_cpu.py / test_windows_gpu.py.  It follows
the normative text of include/tgx.h (tgx_result_window_pad_device, tgx_result_window_spans_device) line by line and
shares nothing with csrc/layout.h.

Row i has the tokens ids[offs[i]:offs[i+1]].  bos / eos: None = absent; A = how many are present; room = L - A tokens
fit a window and step = room - stride is how far the next window moves on.

`windows_by_row` is the definition as one Python loop per row and window; `windows` says the same with whole-array numpy
for inputs of many thousand windows (test_windows_cpu.py pins the two to each other on the small cases).
"""
import numpy as np


def valid(L, stride, bos=None, eos=None):
    A = (bos is not None) + (eos is not None)
    return L >= A + 1 and 0 <= stride < L - A


def row_windows(n, room, stride, trunc_left=False):
    """The windows of a row of n tokens -> [(first kept index, kept count)], k = 0 .. nw - 1"""
    step = room - stride
    assert room >= 1 and step >= 1
    nw = 1 if n <= room else 1 + -(-(n - room) // step)
    out = []
    for k in range(nw):
        reach = min(n, k * step + room)
        lo, hi = (n - reach, n - k * step) if trunc_left else (k * step, reach)
        out.append((lo, hi - lo))
    return out


def windows_by_row(ids, offs, L, stride, pad, bos=None, eos=None, pad_left=False, trunc_left=False, dtype=np.int32):
    """-> (out [W, L] dtype, mask [W, L] u8, lengths [W] i32, window_row [W] i32, window_first [W] i32)"""
    assert valid(L, stride, bos, eos)
    S = len(offs) - 1
    A = (bos is not None) + (eos is not None)
    rows_out, rows_mask, lengths, window_row, window_first = [], [], [], [], []
    for i in range(S):
        t = [int(x) for x in ids[int(offs[i]):int(offs[i + 1])]]
        for first, keep in row_windows(len(t), L - A, stride, trunc_left):
            seq = ([bos] if bos is not None else []) + t[first:first + keep] + ([eos] if eos is not None else [])
            fill = [pad] * (L - len(seq))
            rows_out.append(fill + seq if pad_left else seq + fill)
            rows_mask.append([0] * len(fill) + [1] * len(seq) if pad_left else [1] * len(seq) + [0] * len(fill))
            lengths.append(keep + A)
            window_row.append(i)
            window_first.append(first)
    W = len(rows_out)
    return (np.array(rows_out, dtype=dtype).reshape(W, L), np.array(rows_mask, dtype=np.uint8).reshape(W, L),
            np.array(lengths, np.int32), np.array(window_row, np.int32), np.array(window_first, np.int32))


def n_windows(offs, L, stride, bos=None, eos=None):
    A = (bos is not None) + (eos is not None)
    room, step = L - A, L - A - stride
    n = np.diff(np.asarray(offs, np.int64))
    return int(np.where(n <= room, 1, 1 + -(-(n - room) // step)).sum())


def windows(ids, offs, L, stride, pad, bos=None, eos=None, pad_left=False, trunc_left=False, dtype=np.int32):
    """windows_by_row without Python loops"""
    assert valid(L, stride, bos, eos)
    ids = np.asarray(ids, np.int64)
    offs = np.asarray(offs, np.int64)
    S = len(offs) - 1
    A = (bos is not None) + (eos is not None)
    room, step = L - A, L - A - stride
    n = np.diff(offs)
    nw = np.where(n <= room, 1, 1 + -(-(n - room) // step))
    Wo = np.concatenate([[0], np.cumsum(nw)])
    W = int(Wo[-1])
    row = np.repeat(np.arange(S, dtype=np.int64), nw)
    k = np.arange(W, dtype=np.int64) - Wo[:-1][row]
    reach = np.minimum(n[row], k * step + room)
    if trunc_left:
        first, keep = n[row] - reach, reach - k * step
    else:
        first, keep = k * step, reach - k * step
    ln = keep + A
    col0 = (L - ln) if pad_left else np.zeros(W, np.int64)
    q = np.arange(L, dtype=np.int64)[None, :] - col0[:, None]       # index into [bos] + kept + [eos]
    on_seq = (q >= 0) & (q < ln[:, None])
    t = q - (1 if bos is not None else 0)                           # index into the kept tokens
    is_tok = on_seq & (t >= 0) & (t < keep[:, None])
    out = np.full((W, L), pad, np.int64)
    src = (offs[:-1][row] + first)[:, None] + t
    out[is_tok] = ids[src[is_tok]]
    if bos is not None:
        out[on_seq & (q == 0)] = bos
    if eos is not None:
        out[on_seq & (t == keep[:, None])] = eos
    return out.astype(dtype), on_seq.astype(np.uint8), ln.astype(np.int32), row.astype(np.int32), first.astype(np.int32)


def window_spans(offs, flat_spans, L, stride, bos=None, eos=None, pad_left=False, trunc_left=False, dtype=np.int64):
    """-> [W, L, 2] of dtype: cell (w, c) holds the span of the token tgx_result_window_pad_device puts there, (0, 0)
    elsewhere.  flat_spans: [T, 2], every token's span in its row's text (spans_checker.flat)."""
    T = int(offs[-1])
    sp = np.concatenate([np.asarray(flat_spans, np.int64).reshape(T, 2), np.zeros((1, 2), np.int64)])   # entry T: bos, eos, padding
    where = windows(np.arange(T, dtype=np.int64), offs, L, stride, T, T if bos is not None else None, T if eos is not None else None,
                    pad_left, trunc_left, np.int64)[0]
    return sp[where].astype(dtype)
