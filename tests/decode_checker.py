"""Plain per-row restatement of the decode semantics of include/tgx.h (tgx_decode_result / tgx_decode_padded): what the
padded form is checked against.  Nothing here shares code with the library."""
import numpy as np

REPLACEMENT = "\ufffd"
# every boundary of the byte classes of well-formed UTF-8
ALPHABET = bytes.fromhex("00 41 7F 80 8F 90 9F A0 BF C0 C1 C2 DF E0 E1 EC ED EE EF F0 F1 F3 F4 F5 FF")
# an empty special token, one that is not UTF-8 (it must come out verbatim) and two ordinary ones
MIXED_SPECIALS = [b"<s>", b"", b"\xff<bad\x80>", "<|\u00e9|>".encode()]


def mixed_tokens():
    """a vocabulary for the decode tests: an empty token, tokens of 1, 15, 16, 17, 63 and 64 bytes, UTF-8 characters split
    across tokens, invalid bytes"""
    euro, smile, e = "\u20ac".encode(), "\U0001f600".encode(), "\u00e9".encode()
    return [b"", b"a", b" ", b"\n", b"the", b" and", b"x" * 15, b"y" * 16, b"z" * 17, b"p" * 63, b"q" * 64,
            euro, euro[:1], euro[1:], euro[:2], euro[2:], smile, smile[:1], smile[1:], smile[:2], smile[2:], smile[:3], smile[3:],
            e, e[:1], e[1:], b"\x80", b"\xff", b"\xc0\xaf", b"\xed\xa0\x80", b"ab" + euro[:2], euro[2:] + b"cd",
            e * 8, (e * 8)[:-1], b"seventeen: " + e * 2 + euro[:2], euro[2:] + b" the tail of the euro sign" + b"!" * 20]


class OutOfBounds(Exception):
    def __init__(self, row, value):
        super().__init__(f"token id {value} is out of bounds")
        self.row, self.value = row, value


def live_rows(ids, mask=None, lengths=None, skip_id=None):
    """ids [S, L] -> per row the list of its live elements (Python ints), in order"""
    ids = np.asarray(ids)
    rows = []
    for i in range(ids.shape[0]):
        row = []
        for c in range(ids.shape[1]):
            x = int(ids[i, c])
            if mask is not None and not int(mask[i][c]):
                continue
            if lengths is not None and c >= max(0, int(lengths[i])):
                continue
            if skip_id is not None and x == int(skip_id):
                continue
            row.append(x)
        rows.append(row)
    return rows


def decode_rows(rows, tokens, specials, include_special):
    """rows: lists of ints; tokens: list[bytes]; specials: list[bytes] -> (bytes, offsets u64[S+1], n_replaced).
    Raises OutOfBounds for the lowest row with an element that is neither, naming the first such element of that row."""
    V, out, offs, replaced = len(tokens), bytearray(), [0], 0

    def flush(run):
        nonlocal replaced
        raw = b"".join(run)
        text = raw.decode("utf-8", "replace")
        # the replacement characters written: those in the output that were not already in the input
        replaced += text.count(REPLACEMENT) - raw.decode("utf-8", "ignore").count(REPLACEMENT)
        out.extend(text.encode("utf-8"))

    for i, row in enumerate(rows):
        for x in row:
            if not 0 <= x < V + len(specials):
                raise OutOfBounds(i, x)
        run = []
        for x in row:
            if x < V:
                run.append(tokens[x])
                continue
            flush(run)
            run = []
            if include_special:
                out.extend(specials[x - V])
        flush(run)
        offs.append(len(out))
    return np.frombuffer(bytes(out), np.uint8), np.asarray(offs, np.uint64), replaced


def decode_padded(ids, tokens, specials, include_special, mask=None, lengths=None, skip_id=None):
    return decode_rows(live_rows(ids, mask, lengths, skip_id), tokens, specials, include_special)
