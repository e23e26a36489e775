"""Python restatement of sampling a segmentation from the Unigram lattice (tgx_encode_batch_sample), the checker of
tests/test_sample_cpu.py and tests/test_sample_gpu.py.  Matches come from the CPU oracle's common prefix search; nothing
here calls the library's kernels.

Per sample: A[0] = 0, A[p] = logsumexp over the matches (q, len), q + len = p, of A[q] + alpha * score (f64); the token
ending at p is the match with the largest key A[q] + alpha * score - log(-log u), u = sample_u01(seed, sample, q, len),
ties to the longer token; the path is the back-trace from n."""
from __future__ import annotations

import math

M64 = (1 << 64) - 1
NINF = float("-inf")


def sample_u01(seed: int, sample: int, pos: int, length: int) -> float:
    x = (seed ^ 0xD6E8FEB86659FD93 ^ (sample * 0x9E3779B97F4A7C15) ^ (pos * 0xC2B2AE3D27D4EB4F)
         ^ (length * 0x165667B19E3779F9)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    u = (float(x >> 11) + 0.5) * 2.0 ** -53
    return u if u < 1.0 else 1.0 - 2.0 ** -53


def incoming(oracle, text: bytes, max_len: int) -> list[list[tuple[int, int]]]:
    """inc[p] = [(q, id), ...] of the matches ending at p, ascending q (the longer token first)."""
    n = len(text)
    inc: list[list[tuple[int, int]]] = [[] for _ in range(n + 1)]
    for q in range(n):
        for tid, ln in oracle.common_prefix_search(text[q:q + max_len]):
            inc[q + ln].append((q, tid))
    return inc


def check_sample(inc, scores, n: int, alpha: float, seed: int, sample: int, viterbi: bool = False):
    """-> dict(logz, ids, gap, vgap, vids): log Z = A[n] (-inf: no path), the sampled ids, the smallest key gap (best minus
    runner-up) along the sampled path; with viterbi=True also the Viterbi ids and the smallest score gap along them."""
    A = [NINF] * (n + 1)
    A[0] = 0.0
    bp = [(-1, -1)] * (n + 1)
    gp = [math.inf] * (n + 1)
    V = [NINF] * (n + 1) if viterbi else None
    if viterbi:
        V[0] = 0.0
    vbp = [(-1, -1)] * (n + 1)
    vgp = [math.inf] * (n + 1)
    for p in range(1, n + 1):
        best = second = NINF
        arg = (-1, -1)
        cands = []
        vb = vs = NINF
        varg = (-1, -1)
        for q, tid in inc[p]:
            a = A[q]
            if a == NINF:
                continue
            s = alpha * float(scores[tid])
            c = a + s
            cands.append(c)
            k = c - math.log(-math.log(sample_u01(seed, sample, q, p - q)))
            if k > best:
                second, best, arg = best, k, (q, tid)
            elif k > second:
                second = k
            if viterbi:
                v = V[q] + float(scores[tid])
                if v > vb:
                    vs, vb, varg = vb, v, (q, tid)
                elif v > vs:
                    vs = v
        if cands:
            m = max(cands)
            A[p] = m + math.log(math.fsum(math.exp(c - m) for c in cands))
            bp[p] = arg
            gp[p] = best - second
            if viterbi:
                V[p], vbp[p], vgp[p] = vb, varg, vb - vs
    out = {"logz": A[n], "ids": None, "gap": math.inf}
    if A[n] == NINF:
        return out
    ids, gap, p = [], math.inf, n
    while p > 0:
        q, tid = bp[p]
        ids.append(tid)
        gap = min(gap, gp[p])
        p = q
    out["ids"], out["gap"] = ids[::-1], gap
    if viterbi:
        vids, vgap, p = [], math.inf, n
        while p > 0:
            q, tid = vbp[p]
            vids.append(tid)
            vgap = min(vgap, vgp[p])
            p = q
        out["vids"], out["vgap"] = vids[::-1], vgap
    return out


def enumerate_segmentations(inc, n: int):
    """Every path 0 -> n as a tuple of ids (tiny strings only)."""
    paths = {0: [()]}
    for p in range(1, n + 1):
        paths[p] = [path + (tid,) for q, tid in inc[p] for path in paths.get(q, [])]
    return paths[n]


def segmentation_probs(inc, scores, n: int, alpha: float) -> dict:
    segs = enumerate_segmentations(inc, n)
    w = [alpha * sum(float(scores[t]) for t in s) for s in segs]
    m = max(w)
    z = math.fsum(math.exp(x - m) for x in w)
    return {s: math.exp(x - m) / z for s, x in zip(segs, w)}, m + math.log(z)
