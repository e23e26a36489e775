"""The batches that tests/test_fim_cpu.py hands the host twin and tests/test_fim_gpu.py the kernels: seeded, so both see
the same ones.

Row lengths come from {0, 1, 2, 3, 1019 .. 1029, 4093 .. 4100}: around one and four of the fill kernel's tiles of 1024
positions.  Every batch has a run of empty rows in the middle and, most of them, one at the start and one at the end.  One
row is sized so that T' lands on 1024·k + d, d = -3 .. 3: the last tile holds 1021 .. 1023, 1024 or 1 .. 3 positions, so
its last thread slot is partial unless d = 0."""
import numpy as np

import fim_checker as fc

LENGTHS = [0, 1, 2, 3] + list(range(1019, 1030)) + list(range(4093, 4101))
RATES = (0.0, 0.5, 1.0)
V = 1000
N_BATCHES = 198   # 22 rounds over the 9 pairs of rates


def batch(k):
    """-> dict(ids, offs, vocab_size, pre, suf, mid, rate, spm_rate, seed, first_row)"""
    rng = np.random.default_rng(5000 + k)
    rate, spm_rate = RATES[k % 3], RATES[(k // 3) % 3]
    seed = (0, 2**64 - 1)[k % 2] if k < 4 else int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2))
    first_row = (0, 1, 12345, 2**64 - 2)[int(rng.integers(0, 4))]   # the last one wraps inside the batch
    body = [int(x) for x in rng.choice(LENGTHS, int(rng.integers(2, 7)))]
    mid_at = int(rng.integers(1, len(body)))
    lens = [0] * int(rng.integers(0, 3)) + body[:mid_at] + [0] * int(rng.integers(1, 4)) + body[mid_at:]
    # the row that puts T' where it is wanted
    cur = sum(n + (3 if fc.row_plan(seed, first_row + i, n, rate, spm_rate)[0] else 0) for i, n in enumerate(lens))
    d = k % 7 - 3
    extra = 3 if fc.u01(seed, (first_row + len(lens)) & fc.MASK, 0) < rate else 0
    target = (cur + extra + 1 + 3 + 1023) // 1024 * 1024 + d
    lens += [target - cur - extra] + [0] * int(rng.integers(0, 3))
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(0, V, int(offs[-1])).astype(np.uint32)
    pre, suf, mid = [(V, V + 1, V + 2), (V + 5, V + 1, V + 3), (3, 1, 2), (V - 1, V, 7)][int(rng.integers(0, 4))]
    case = dict(ids=ids, offs=offs, vocab_size=V, pre=pre, suf=suf, mid=mid, rate=rate, spm_rate=spm_rate, seed=seed, first_row=first_row)
    case["want_total"] = target
    return case


def long_row():
    """one row of 70 000 tokens (about 69 tiles) between two short ones and empty rows"""
    rng = np.random.default_rng(77)
    lens = [0, 5, 70_000, 0, 0, 1026, 0]
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(0, V, int(offs[-1])).astype(np.uint32)
    return dict(ids=ids, offs=offs, vocab_size=V, pre=V + 2, suf=V, mid=V + 1, rate=1.0, spm_rate=0.5, seed=99, first_row=3)


def args(case):
    """the keyword arguments of _lib.fim_host / NativeResult.fim / fim_checker.fim"""
    return dict(rate=case["rate"], spm_rate=case["spm_rate"], seed=case["seed"], first_row=case["first_row"])
