"""Fill-in-the-middle as include/tgx.h states it (tgx_result_fim), restated independently of csrc/fim.h: the uniform on
Python integers, one Python loop over the rows, list slices for the pieces.  `invert_row` undoes a row from its
(mode, a, b) alone."""
import numpy as np

MASK = 2**64 - 1
SALT = 0xA0761D6478BD642F
COPY, PSM, SPM = 0, 1, 2


def u01(seed, row, draw):
    x = (seed ^ SALT ^ (row * 0x9E3779B97F4A7C15) ^ (draw * 0xC2B2AE3D27D4EB4F)) & MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return float(x >> 11) * 2.0 ** -53   # both steps exact: an integer below 2^53, times a power of two


def cut(seed, g, n, d):
    return min(n, int(u01(seed, g, d) * float(n + 1)))


def row_plan(seed, g, n, rate, spm_rate):
    """-> (mode, a, b) of row g with n tokens"""
    g &= MASK
    if n < 1 or not u01(seed, g, 0) < rate:
        return COPY, 0, 0
    mode = SPM if u01(seed, g, 1) < spm_rate else PSM
    c2, c3 = cut(seed, g, n, 2), cut(seed, g, n, 3)
    return mode, min(c2, c3), max(c2, c3)


def fim_row(t, mode, a, b, pre, suf, mid):
    t = list(t)
    prefix, middle, suffix = t[:a], t[a:b], t[b:]
    if mode == COPY:
        return t
    if mode == PSM:
        return [pre] + prefix + [suf] + suffix + [mid] + middle
    return [pre, suf] + suffix + [mid] + prefix + middle


def invert_row(row, mode, a, b):
    """the input row of an output row, from (mode, a, b) alone"""
    row = list(row)
    if mode == COPY:
        return row
    n = len(row) - 3
    ns = n - b
    if mode == PSM:
        prefix, suffix, middle = row[1:1 + a], row[a + 2:a + 2 + ns], row[a + 3 + ns:]
    else:
        suffix, prefix, middle = row[2:2 + ns], row[3 + ns:3 + ns + a], row[3 + ns + a:]
    return prefix + middle + suffix


def fim(ids, offs, vocab_size, pre, suf, mid, rate=1.0, spm_rate=0.5, seed=0, first_row=0):
    """-> (ids u32[T'], offsets u64[S+1], vocab_size, mode u8[S], cuts u64[S, 2], n_applied)"""
    S = len(offs) - 1
    out, out_offs = [], [0]
    mode = np.zeros(S, np.uint8)
    cuts = np.zeros((S, 2), np.uint64)
    n_applied = 0
    for i in range(S):
        t = ids[int(offs[i]):int(offs[i + 1])].tolist()
        m, a, b = row_plan(seed, first_row + i, len(t), rate, spm_rate)
        mode[i], cuts[i, 0], cuts[i, 1] = m, a, b
        n_applied += m != COPY
        out.extend(fim_row(t, m, a, b, pre, suf, mid))
        out_offs.append(len(out))
    return (np.asarray(out, np.uint32).reshape(-1), np.asarray(out_offs, np.uint64), max(vocab_size, 1 + max(pre, suf, mid)), mode, cuts,
            n_applied)
