"""Inputs of the normalisation tests (tgx_normalize_host, tgx_corpus_normalize): what test_norm_cpu.py and
test_norm_gpu.py both feed, and the truth they compare with (normalize_flat; unicodedata for rows that are UTF-8)."""
import functools
import unicodedata as ud

import numpy as np

from tokengeex_amd import _lib, synth

FORMS = ("nfd", "nfc", "nfkd", "nfkc")
SLOT, TILE = 16, 4096   # csrc/front.h: a thread slot's bytes and a tile's

# test_unicode_norm_cpu.py::test_bytes_that_are_not_utf8_pass_through
INVALID = [b"\xff\xfea\xcc\x81", b"\xe4\xb8", b"abc\x80\x80def", b"\xf5\x80\x80\x80", b"\xed\xa0\x80x", b"e\xcc\x81\xc0\xaf"]


def filler(n: int, salt: int) -> bytes:
    return bytes(ord("a") + (i * 7 + salt) % 23 for i in range(n))


def truth(form: str, rows: list[bytes]):
    """normalize_flat's (flat, offs); every row that is UTF-8 is also what unicodedata makes of it"""
    flat, offs = _lib.pack(rows)
    f, o = _lib.normalize_flat(form, flat, offs)
    for i, r in enumerate(rows):
        try:
            t = r.decode("utf-8")
        except UnicodeDecodeError:
            continue
        assert bytes(f[int(o[i]):int(o[i + 1])]) == ud.normalize(form.upper(), t).encode("utf-8"), (form, i, r)
    return f, o


class _Batch:
    """rows appended to one packed text, with ASCII in front of an event so that it falls where it is asked to"""

    def __init__(self):
        self.rows, self.n = [], 0

    def add(self, *rows: bytes):
        for r in rows:
            self.rows.append(r)
            self.n += len(r)

    def pad_to(self, mod: int, k: int) -> bytes:
        """ASCII after which the next byte stands k bytes in front of a multiple of mod"""
        return filler((-k - self.n) % mod, self.n)


@functools.lru_cache(maxsize=None)
def edge_batch() -> tuple[bytes, ...]:
    """Heads, active scalars, row ends and cut sequences at byte 15/16 of a slot and at byte 4095/4096 of a tile, empty rows
    between them, and a piece that ends the text."""
    b = _Batch()
    acute, jamo_v, wide_a, ga = "\u0301".encode(), "\u1161".encode(), "\uff21".encode(), "\uac00".encode()
    for mod in (SLOT, TILE):
        # a head as the last byte in front of the boundary, its mark behind it
        b.add(b.pad_to(mod, 1) + b"e" + acute + b"xyz", b"")
        assert (b.n - 5) % mod == 0
        # an active scalar whose lead byte is the last byte in front of the boundary (2, 3 and 4 bytes long; the head inert)
        b.add(b.pad_to(mod, 1 + 1) + b"a" + acute + b"b")
        b.add(b"", b.pad_to(mod, 1 + 3) + ga + jamo_v + b"z")
        b.add(b.pad_to(mod, 2 + 3) + ga + jamo_v + jamo_v)
        b.add(b.pad_to(mod, 1 + 1) + b"q" + "\U0001d165".encode() + b"r", b"", b"")
        # ... and one that changes alone, with nothing active around it
        b.add(b.pad_to(mod, 1) + wide_a + b"k", b.pad_to(mod, 2) + "\u00c5".encode() + "A\u030a".encode())
        # a row end between 'e' and its mark: the mark heads the next row and does not compose
        b.add(b.pad_to(mod, 1) + b"e", acute + b"abc", b"")
        # a row end inside CC 81: raw bytes on both sides, both rows unchanged
        b.add(b.pad_to(mod, 2) + b"e\xcc", b"\x81abc")
        b.add(b.pad_to(mod, 2) + ga[:2], ga[2:] + jamo_v, b"")
        # an inert head that is not ASCII, a raw byte in front of a mark, marks that change places, a mark after a cut
        b.add(b.pad_to(mod, 3) + "\u4e2d".encode() + acute + b"\xff" + acute + b"o" + "\u0301\u0316\u0323".encode())
        b.add(b.pad_to(mod, 2) + "\u0101".encode() + "\u0301\u0328".encode(), "\u09c7\u09be".encode(), "\u1100\u1161\u11a8".encode())
        # rows that end exactly at the boundary, with and without a piece at their end
        b.add(b.pad_to(mod, 3) + b"e" + acute, b"", b.pad_to(mod, 0), jamo_v + b"!")
    for raw in INVALID:
        b.add(raw, b.pad_to(SLOT, 2) + raw, b.pad_to(TILE, 3) + raw)
    b.add(b"", b"", filler(40, 1) + b"u" + "\u0308\u0301".encode())   # a piece ends the text
    return tuple(b.rows)


@functools.lru_cache(maxsize=None)
def random_rows(n: int = 20000, seed: int = 7) -> tuple[bytes, ...]:
    """test_unicode_norm_cpu.py::test_random_sequences_with_combining_marks' generator"""
    rng = np.random.default_rng(seed)
    marks = [cp for cp in range(0x300, 0x1E8D7) if ud.combining(chr(cp))]
    starters = list(range(0x41, 0x5B)) + list(range(0xC0, 0x250)) + list(range(0x391, 0x3CA)) + list(range(0x1100, 0x1113)) + \
        list(range(0x1161, 0x1176)) + list(range(0x11A8, 0x11C3)) + list(range(0xAC00, 0xAC00 + 600)) + [0x0F71, 0x0F72, 0x0F74, 0x1100, 0x09C7, 0x09BE, 0x0B47, 0x0B56]
    compat = [cp for cp in range(0xA0, 0x30000) if ud.decomposition(chr(cp)).startswith("<")][::7]
    texts = []
    for _ in range(n):
        s = []
        for _ in range(int(rng.integers(1, 12))):
            r = rng.random()
            pool = marks if r < 0.45 else starters if r < 0.85 else compat
            s.append(chr(pool[int(rng.integers(len(pool)))]))
        texts.append("".join(s).encode("utf-8"))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def descending_marks(n: int) -> str:
    """n combining marks that do not decompose, each of a lower class than the one in front of it (the sort has to turn them round)"""
    by_class = {}
    for cp in range(0x300, 0x1E8D7):
        if ud.combining(chr(cp)) and not ud.decomposition(chr(cp)):
            by_class.setdefault(ud.combining(chr(cp)), cp)
    picked = [by_class[c] for c in sorted(by_class, reverse=True)][:n]
    assert len(picked) == n
    return "".join(chr(cp) for cp in picked)


@functools.lru_cache(maxsize=None)
def mixed_rows() -> tuple[bytes, ...]:
    """48 KiB of the benchmark's mixed corpus: ASCII, CJK ideographs and fullwidth punctuation"""
    flat, offs = synth.make_corpus(48 << 10, "mixed", max_len=4096, seed_offset=3)
    return tuple(bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1))


# ---- one corpus past the caps of csrc/norm.hip's grids ------------------------------------------------------------------

CAP = 4096            # csrc/norm.hip: kNormMaxBlocks, of the kernels over tiles, over rows and over pieces
BLOCK = 256           # threads of a block of the kernels with a thread per row
PIECE_BLOCK = 64      # csrc/norm.hip: kPieceBlock, pieces per block of the kernels with a thread per piece


@functools.lru_cache(maxsize=None)
def past_cap_corpus():
    """-> (flat, offs): rounds of edge_batch() and of the first 3 000 random_rows(), two empty rows behind each of those,
    over the first 4096·4096 bytes and a little more: the kernels over tiles (norm_mark, norm_pieces, norm_places) go round
    twice, there are over 256·4096 rows and over 64·4096 pieces.  A round is no multiple of a tile, so every round puts its
    heads, marks and row ends at other places of the slots and tiles.  Behind them, in the second trip's tiles, a row of
    three tiles of ASCII (tiles without a piece: norm_pieces_kernel's `continue`) and one more round."""
    rows = list(edge_batch())
    for r in random_rows()[:3000]:
        rows += [r, b"", b""]
    unit, unit_offs = _lib.pack(rows)
    unit = np.ascontiguousarray(unit)
    unit_lens = np.diff(unit_offs.astype(np.int64))
    reps = CAP * TILE // unit.size + 1
    plain = np.frombuffer(filler(3 * TILE, 3), np.uint8)
    flat = np.concatenate([np.tile(unit, reps), plain, unit])
    lens = np.concatenate([np.tile(unit_lens, reps), [plain.size], unit_lens])
    offs = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    for a in (flat, offs):
        a.setflags(write=False)
    return flat, offs
