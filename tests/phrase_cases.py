"""The batches that tests/test_phrase_cpu.py hands the host twin and tests/test_phrase_gpu.py the kernel: seeded, so both
see the same ones, for both kinds where a case applies ("bytes": the rows of a corpus, "ids": the rows of a result).

The kernel lays the ELEMENTS of all rows end to end, a lane a start position: a wave takes a chunk of 64, a block a tile of
256 (staged in LDS with a halo of the longest phrase) and, past the grid's cap, a run of consecutive tiles; a first-level
filter over the first two BYTES ends most lanes, the others walk a byte trie.  So the shapes are the smallest at which
that can go wrong: phrases of 1, 2 and 3 elements (the filter's level boundary); a phrase of the greatest length from
starts that span four chunk edges and reach the end of a tile's halo; phrases inside phrases and duplicates; occurrences
at and across a row's end, rows shorter than every phrase, runs of empty rows; starts 1 to 3 elements on either side of
a chunk's edge, a tile's and two tiles'; a batch past the grid's cap; all 256 byte values; the fold's and the word
bytes' neighbours; id phrases whose bytes also lie at byte offsets that are no multiple of 4; a set of 50 000 phrases;
the empty set, no rows, no elements.

case(name, kind) -> dict(name, kind, data, offs, phrases, combos, vocab_size); combos: the (fold_case, whole_word) pairs
the case runs under."""
import numpy as np

import gram_cases

KINDS = ("bytes", "ids")
CHUNK, TILE = 64, 256
DTYPE = {"bytes": np.uint8, "ids": np.uint32}
V = 1 << 25                      # the ids' vocabulary: ids of 2^24 and more exist
MAX_LEN = {"bytes": 255, "ids": 64}
PLAIN = ((False, False),)
ALL_FLAGS = ((False, False), (True, False), (False, True), (True, True))
BOTH = ("lens123", "max_len", "nested", "row_ends", "edges", "past_cap", "large_set", "empty_set", "no_rows", "no_elems")
BYTES_ONLY = ("all_bytes", "fold", "whole_word")
IDS_ONLY = ("ids_offsets",)


def all_cases():
    return [(n, k) for n in BOTH for k in KINDS] + [(n, "bytes") for n in BYTES_ONLY] + [(n, "ids") for n in IDS_ONLY]


def pack(rows, kind):
    offs = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.asarray([x for r in rows for x in r], dtype=DTYPE[kind]), offs


def _conv(rows, kind):
    """rows written as bytes -> the kind's rows: a byte b becomes the id _id(b) (distinct, some of them 2^24 and more)"""
    if kind == "bytes":
        return [list(r) for r in rows]
    return [[_id(b) for b in r] for r in rows]


def _id(b):
    return (b * 0x00810203 + b) % V


def _phr(p, kind):
    return bytes(p) if kind == "bytes" else [_id(b) for b in p]


def _done(name, kind, rows, phrases, combos=None):
    """rows and phrases are written in bytes and converted for the kind"""
    data, offs = pack(_conv(rows, kind), kind)
    if combos is None:
        combos = ALL_FLAGS if kind == "bytes" else PLAIN
    return dict(name=name, kind=kind, data=data, offs=offs, phrases=[_phr(p, kind) for p in phrases], combos=combos, vocab_size=V)


def _text(rng, n, alphabet=b"abAB c_1"):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def case(name, kind):
    rng = np.random.default_rng(9100 + 100 * (BOTH + BYTES_ONLY + IDS_ONLY).index(name) + KINDS.index(kind))
    if name == "lens123":     # every row length 0 .. 5 over a small alphabet, and a longer row: phrases of 1, 2 and 3 elements
        rows = [b"", b""] + [_text(rng, n, b"abc") for n in (0, 1, 2, 3, 4, 5, 1, 2, 3)] + [b""] + [_text(rng, 300, b"abcd")] + [b"a", b"ab", b"abc", b""]
        return _done(name, kind, rows, [b"a", b"ab", b"abc", b"b", b"ca", b"cab", b"d", b"dd", b"ddd"])
    if name == "max_len":     # the longest phrase from starts that span four chunk edges and from a tile's last start
        L = MAX_LEN[kind]
        long = bytes(rng.integers(1, 200, L).astype(np.uint8))
        miss = long[:-1] + bytes([long[-1] ^ 1])
        rows = [_text(rng, 60)]                                   # the next row starts at element 60
        rows.append(long + _text(rng, 7))                         # 60 .. 60 + L: over the edges 64, 128, 192, 256 (bytes)
        cum = 60 + L + 7
        rows.append(_text(rng, 2 * TILE - 1 - cum))               # the next row starts at a tile's last element
        rows.append(long)                                         # ... and ends with the row: the halo's last byte
        rows.append(miss + long[:L - 1])                          # the last element differs; then the row ends one element early
        rows.append(b"")
        rows.append(_text(rng, 3) + long + long)                  # back to back
        return _done(name, kind, rows, [long, long[:100 if kind == "bytes" else 30], long[5:50], long[L - 2:]])
    if name == "nested":      # a prefix, a suffix and an infix of another phrase; "aa" in "aaaa"; duplicates
        rows = [b"aaaa", b"abcde", b"xabcdex", b"abcd", b"bcde", b"", b"aaaaaaa", _text(rng, 200, b"abcde"), b"abcdeabcde"]
        return _done(name, kind, rows, [b"abcde", b"ab", b"de", b"bcd", b"aa", b"aa", b"abcde", b"e", b"aaa"])
    if name == "row_ends":    # at a row's end; completed only by the next row; rows shorter than every phrase; empty runs
        rows = [b"", b"", b"", b"xxhello", b"hel", b"lo", b"hell", b"o", b"", b"", b"h", b"he", b"hello", b"", b"hellohello", b"hellohell", b"ohello",
                b"", b""]
        return _done(name, kind, rows, [b"hello", b"lohe", b"hellohellohello"])
    if name == "edges":       # an occurrence beginning 1 .. 3 elements on either side of the edges 64, 256 and 512, in rows that cross them
        p, q = b"edge!", b"ge"
        rows, cum = [], 0
        for edge in (CHUNK, TILE, 2 * TILE):
            for d in (-3, -2, -1, 0, 1, 2, 3):
                base = (cum // (2 * TILE) + 1) * 2 * TILE          # a fresh pair of tiles
                rows.append(_text(rng, base - cum, b"edg!x"))
                cum = base
                row = bytearray(_text(rng, edge + 40, b"edg!x"))
                row[edge + d:edge + d + len(p)] = p
                rows.append(bytes(row))
                cum += len(row)
                if d == 0:                                          # a row that ends exactly at the edge, with the phrase last
                    fill = (cum // (2 * TILE) + 1) * 2 * TILE - cum
                    rows.append(_text(rng, fill + edge - len(p), b"edg!x") + p)
                    cum += fill + edge
        return _done(name, kind, rows, [p, q, b"!"])
    if name == "past_cap":    # gram_cases.past_cap_case's batch: over 2048 tiles, a row from one block's run into the next
        c = gram_cases.past_cap_case(kind)
        ev = [[int(x) for x in c["eval_data"][int(c["eval_offs"][k]):int(c["eval_offs"][k + 1])]] for k in range(len(c["eval_offs"]) - 1)]
        phrases = [r[:n] for r in ev if len(r) >= 16 for n in (3, 16)] + [r[:5] for r in ev if len(r) >= 5]
        phrases = [bytes(p) if kind == "bytes" else p for p in phrases]
        return dict(name=name, kind=kind, data=c["data"], offs=c["offs"], phrases=phrases, combos=PLAIN, vocab_size=gram_cases.V, where=c["where"])
    if name == "large_set":   # 50 000 phrases of 2 .. 24 elements: half cut from the text, half random
        n = 12000
        flat = rng.integers(0, 256, n).astype(np.uint8)
        cuts = rng.integers(400, 900, 20).cumsum()
        rows = [bytes(r) for r in np.split(flat, cuts[cuts < n])] + [b""]
        phrases = []
        for k in range(50000):
            L = int(rng.integers(2, 25))
            if k % 2:
                a = int(rng.integers(0, n - L))
                phrases.append(bytes(flat[a:a + L]))
            else:
                phrases.append(bytes(rng.integers(0, 256, L).astype(np.uint8)))
        return _done(name, kind, rows, phrases, ((False, False), (True, True)) if kind == "bytes" else PLAIN)
    if name == "empty_set":
        return _done(name, kind, [b"", b"abc", _text(rng, 300), b""], [])
    if name == "no_rows":
        return _done(name, kind, [], [b"a", b"bc"])
    if name == "no_elems":
        return _done(name, kind, [b""] * 5, [b"a", b"bc"])
    if name == "all_bytes":   # all 256 byte values; 0x00, 0xFE and 0xFF as first, middle and last bytes
        special = (0x00, 0xFE, 0xFF)
        phrases = [bytes([a, b, c]) for a in special for b in special for c in special]
        phrases += [bytes([b, (7 * b + 3) & 255, 255 - b]) for b in range(256)] + [bytes([b, b ^ 0x55]) for b in range(256)]
        phrases += [b"\x00", b"\xff", b"\xfe", b"\x00\x00", b"\xff\xff", b"\xfe\xff", b"\xff\xfe", b"\x00\xff\x00\xfe\x00"]
        flat = bytearray(rng.integers(0, 256, 6000).astype(np.uint8).tobytes())
        for k, p in enumerate(phrases):
            at = 9 * k + 3
            flat[at:at + len(p)] = p
        flat += bytes([0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFE, 0xFE, 0xFF, 0x00])
        cuts = [0, 1000, 1000, 2500, 5999, len(flat)]
        rows = [bytes(flat[a:z]) for a, z in zip(cuts, cuts[1:])]
        return _done(name, kind, rows, phrases)
    if name == "fold":        # duplicates only after folding; the four bytes next to A-Z / a-z; bytes >= 0x80
        rows = [b"Hello hELLO hello HELLO", b"@[`{ @[`{", b"`{@[", "École école".encode(), b"\xc1\xe1\xc1", b"Az aZ AZ az", b"",
                _text(rng, 300, b"heloHELO @[`{"), bytes(range(0x3F, 0x7D)), bytes(range(0x80, 0x100))]
        phrases = [b"Hello", b"hello", b"HELLO", b"@[", b"`{", b"@", b"`", b"[", b"{", "École".encode(), "école".encode(), b"\xc1", b"\xe1", b"az", b"AZ",
                   b"Az", b"lo h", b"LO H"]
        return _done(name, kind, rows, phrases)
    if name == "whole_word":  # the neighbours _, a digit, 0x80 and a space; a row's first and last element; the adjacent row's word byte
        rows = [b"cat", b"cat", b"a cat sat", b"_cat cat_ cat1 1cat", b"\x80cat cat\x80 cat", b"concat", b"cat", b"s cat", b"cats", b"x", b"cat",
                b"cat.cat,cat;(cat)", b"", b"tom cat", b"cat nip", b"tom cat nip", b"Cat CAT cAt", _text(rng, 300, b"cat _1.")]
        return _done(name, kind, rows, [b"cat", b"tom cat", b"cat nip", b"a", b"c", b"t", b" cat", b"cat ", b".", b"CAT"])
    if name == "ids_offsets":  # an id phrase whose bytes also lie at byte offsets 1, 2 and 3 modulo 4; ids 0, >= 2^24 and V - 1
        p = [0x01010001, 0x00010100]   # (every byte 0 or 1: shifted by one to three bytes they still are ids below V)
        raw = np.asarray(p, "<u4").tobytes()
        rows = []
        for shift in (0, 1, 2, 3):   # the phrase's 8 bytes from byte `shift` of a row of three or four ids on
            b = bytes(shift) + raw + bytes((-shift) % 4)
            rows.append([int(x) for x in np.frombuffer(b, "<u4")])
        rows += [[0, 0, V - 1, 0], [V - 1], [1 << 24, (1 << 24) + 1, 0], p + p, [], [0]]
        data, offs = pack(rows, kind)
        phrases = [p, [0], [0, 0], [V - 1], [1 << 24, (1 << 24) + 1], [V - 1, 0], [(1 << 24) + 1, 0]]
        return dict(name=name, kind=kind, data=data, offs=offs, phrases=phrases, combos=PLAIN, vocab_size=V)
    raise KeyError(name)
