"""The batches that tests/test_select_cpu.py hands the host twins and tests/test_select_gpu.py the kernels: seeded, so
both see the same ones.

Row lengths come from {0, 1, 2, 3, 1019 .. 1029, 4093 .. 4100} for ids (around one and four of the fill kernel's tiles of
1024 ids); the byte batches add {13 .. 19, 4090 .. 4102} (around a slot of 16 bytes and a tile of 4096), so that every
source and destination residue mod 16 occurs and slots straddle row boundaries.  Every source has runs of empty rows at
its start, in its middle and at its end.  The index patterns rotate through identity, reverse, a strict subset, one row
repeated so that M > S, only empty rows, and a seeded random multiset.  The source's last non-empty row is selected exactly
once (except by "only empty rows") and sized so that T' lands on tile·k + d, d = -3 .. 3."""
import numpy as np

ID_LENGTHS = [0, 1, 2, 3] + list(range(1019, 1030)) + list(range(4093, 4101))
BYTE_LENGTHS = ID_LENGTHS + list(range(13, 20)) + list(range(4090, 4103))
PATTERNS = ("identity", "reverse", "subset", "repeat", "empty", "multiset")
TILE = {"ids": 1024, "bytes": 4096}
V = 1000
N_BATCHES = 96   # 16 rounds over the 6 patterns, for each kind


def batch(k, kind):
    """kind "ids" or "bytes" -> dict(data, offs, rows, pattern, want_total[, vocab_size])"""
    rng = np.random.default_rng((9000 if kind == "ids" else 19000) + k)
    lengths = ID_LENGTHS if kind == "ids" else BYTE_LENGTHS
    tile = TILE[kind]
    body = [int(x) for x in rng.choice(lengths, int(rng.integers(3, 8)))]
    if kind == "bytes":
        body[0] = 13 + k % 7 if k % 2 else body[0]   # a short row early on: the rows behind it start off a slot's edge
    mid_at = int(rng.integers(1, len(body)))
    body[mid_at - 1], body[mid_at] = body[mid_at - 1] or 2, body[mid_at] or 3   # the middle run lies between rows that have elements
    lens =[0] * int(rng.integers(1, 3)) + body[:mid_at] + [0] * int(rng.integers(1, 4)) + body[mid_at:]
    special = len(lens)                     # the row that puts T' where it is wanted
    lens += [1] + [0] * int(rng.integers(1, 3))
    S = len(lens)
    others = [i for i in range(S) if i != special]
    pattern = PATTERNS[k % 6]
    if pattern == "identity":
        rows = list(range(S))
    elif pattern == "reverse":
        rows = list(range(S))[::-1]
    elif pattern == "subset":
        keep = rng.random(S) < 0.6
        keep[special] = True
        keep[others[int(rng.integers(0, len(others)))]] = False
        rows = [i for i in range(S) if keep[i]]
    elif pattern == "repeat":
        rep = others[int(np.argmax([lens[i] for i in others]))] if k % 12 < 6 else others[int(rng.integers(0, len(others)))]
        rows = list(range(S)) + [rep] * (2 + k % 3)
        rows = [rows[i] for i in rng.permutation(len(rows))] if k % 4 == 3 else rows
    elif pattern == "empty":
        rows = [i for i in range(S) if lens[i] == 0 and i != special] * (1 + k % 3)
    else:
        rows = [others[int(x)] for x in rng.integers(0, len(others), int(rng.integers(1, 2 * S)))]
        rows.insert(int(rng.integers(0, len(rows) + 1)), special)
    if pattern == "empty":
        want_total = 0
    else:
        assert rows.count(special) == 1
        cur = sum(lens[r] for r in rows if r != special)
        d = k % 7 - 3
        want_total = (cur + 1 + 3 + tile - 1) // tile * tile + d
        lens[special] = want_total - cur
    offs = np.zeros(S + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    if kind == "ids":
        data = rng.integers(0, V, int(offs[-1])).astype(np.uint32)
    else:
        data = rng.integers(1, 256, int(offs[-1])).astype(np.uint8)
    case = dict(data=data, offs=offs, rows=np.asarray(rows, np.int64), pattern=pattern, want_total=want_total)
    if kind == "ids":
        case["vocab_size"] = V
    return case


def long_row(kind):
    """one row of 70 000 elements (about 69 tiles of ids, 18 of bytes) between short and empty rows, selected three times"""
    rng = np.random.default_rng(78)
    lens = [0, 5, 70_000, 0, 0, 1026, 0]
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    n = int(offs[-1])
    data = rng.integers(0, V, n).astype(np.uint32) if kind == "ids" else rng.integers(1, 256, n).astype(np.uint8)
    case = dict(data=data, offs=offs, rows=np.asarray([2, 1, 2, 3, 0, 2, 5, 6], np.int64), pattern="long", want_total=3 * 70_000 + 5 + 1026)
    if kind == "ids":
        case["vocab_size"] = V
    return case
