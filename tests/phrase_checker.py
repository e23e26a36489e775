"""An independent restatement of include/tgx_phrases.h from its text: naive slicing of every row at every element and set
lookups by phrase length.  No trie, no filter, no chunks, and it does not call the library.

hits_of(data, offs, phrases, fold_case, whole_word) -> (count int64[S], longest uint8[n_elems], per_phrase int64[P]) over
data u8[N] (phrases: bytes) or u32[T] (phrases: sequences of ids) and offsets u64[S+1] in elements."""
import numpy as np

MAX_LEN, MAX_BYTES = 255, 256
_FOLD = bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))
_WORD = frozenset(b for b in range(256) if 0x30 <= b <= 0x39 or 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A or b == 0x5F or b >= 0x80)


def fold(b: bytes, fold_case: bool) -> bytes:
    return b.translate(_FOLD) if fold_case else b


def phrase_bytes(p, eb: int) -> bytes:
    return bytes(p) if eb == 1 else np.asarray(list(p), dtype="<u4").tobytes()


def valid(p, eb: int) -> bool:
    n = len(p)
    return 1 <= n <= MAX_LEN and n * eb <= MAX_BYTES


def hits_of(data, offs, phrases, fold_case=False, whole_word=False):
    data = np.ascontiguousarray(data)
    eb = data.dtype.itemsize
    assert eb in (1, 4) and not ((fold_case or whole_word) and eb == 4)
    S = len(offs) - 1
    first = {}  # folded bytes -> the lowest index among the phrases equal to them
    for k, p in enumerate(phrases):
        assert valid(p, eb)
        first.setdefault(fold(phrase_bytes(p, eb), fold_case), k)
    by_len = {}
    for key in first:
        by_len.setdefault(len(key) // eb, set()).add(key)
    count = np.zeros(S, np.int64)
    longest = np.zeros(data.size, np.uint8)
    per = np.zeros(len(phrases), np.int64)
    for i in range(S):
        a, z = int(offs[i]), int(offs[i + 1])
        raw = data[a:z].astype(data.dtype.newbyteorder("<")).tobytes()
        text = fold(raw, fold_case)
        n = z - a
        for L, keys in by_len.items():
            nb = L * eb
            for e in range(n - L + 1):
                key = text[e * eb:e * eb + nb]
                if key not in keys:
                    continue
                if whole_word:   # (eb = 1) the neighbours inside this row only
                    if e > 0 and raw[e - 1] in _WORD:
                        continue
                    if e + L < n and raw[e + L] in _WORD:
                        continue
                count[i] += 1
                per[first[key]] += 1
                longest[a + e] = max(int(longest[a + e]), L)
    return count, longest, per


def cover_of(longest):
    """the elements inside some occurrence, by a loop"""
    out = np.zeros(len(longest), bool)
    for e, L in enumerate(longest):
        out[e:e + int(L)] = True
    return out
