"""The assembly of a sample-level result from the result over the non-special segments and the split plan, restated in
plain numpy with per-segment loops: the checker of test_assemble_cpu.py / test_assemble_gpu.py.  It follows the normative
text of include/tgx.h (tgx_assemble_result) line by line, does not call the library and shares nothing with
csrc/assemble.h.

ids / id_offs: the result over E encoded segments (offsets o[0..E]).  seg_offs u64[S+1]: sample i owns segments
[seg_offs[i], seg_offs[i+1]).  seg_special i32[K]: >= 0 an index into the special tokens, negative "the next encoded
segment".  V: the base vocabulary size.
"""
import numpy as np


def assemble(ids, id_offs, seg_offs, seg_special, V):
    """-> (out_ids u32[T'], out_offs u64[S+1])"""
    ids = np.asarray(ids, np.int64)
    o = [0] if id_offs is None else [int(x) for x in id_offs]
    E, T = len(o) - 1, o[-1]
    seg_offs = [int(x) for x in seg_offs]
    seg_special = [int(x) for x in seg_special]
    S, K = len(seg_offs) - 1, seg_offs[-1]
    assert len(seg_special) == K
    enc = [sp < 0 for sp in seg_special]
    r = [0] * (K + 1)                      # r_k = the number of k' < k with enc(k')
    for k in range(K):
        r[k + 1] = r[k] + (1 if enc[k] else 0)
    assert r[K] == E
    D = [o[r[k]] + (k - r[k]) for k in range(K + 1)]
    assert D[K] == T + (K - E)
    out = np.zeros(D[K], np.uint32)
    written = np.zeros(D[K], bool)
    for k in range(K):
        for j in range(D[k], D[k + 1]):
            out[j] = ids[o[r[k]] + (j - D[k])] if enc[k] else V + seg_special[k]
            written[j] = True
    assert written.all()                   # every position has exactly one owner
    out_offs = np.array([D[seg_offs[i]] for i in range(S + 1)], np.uint64)
    return out, out_offs
