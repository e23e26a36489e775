"""An independent checker of the per-row text statistics and the line view (include/tgx.h: tgx_corpus_text_stats_device,
tgx_corpus_lines).  It knows nothing of chunks, tiles or carries: per row it splits the bytes at b"\\n", drops the empty
last piece after a trailing '\\n' and counts with numpy.  For rows that are valid UTF-8 `second_truth` counts once more
with Python's own strings: len(line) over text.split("\\n"), and len(text)."""
import numpy as np

NAMES = ("bytes", "chars", "newlines", "lines", "max_line", "long_lines", "alpha", "digit", "space", "non_ascii", "control")
N = len(NAMES)
UNITS = ("char", "byte")

_B = np.arange(256)
IS_CHAR = (_B & 0xC0) != 0x80
IS_ALPHA = ((_B >= ord("A")) & (_B <= ord("Z"))) | ((_B >= ord("a")) & (_B <= ord("z")))
IS_DIGIT = (_B >= ord("0")) & (_B <= ord("9"))
IS_SPACE = (_B == 0x20) | ((_B >= 0x09) & (_B <= 0x0D))
IS_NON_ASCII = _B >= 0xC0
IS_CONTROL = ((_B < 0x20) & ~IS_SPACE) | (_B == 0x7F)


def pieces_of(raw: bytes):
    """the lines of a row without their terminators"""
    if not raw:
        return []
    pieces = raw.split(b"\n")
    if raw.endswith(b"\n"):
        pieces.pop()
    return pieces


def _units(piece: bytes, unit: str) -> int:
    return len(piece) if unit == "byte" else int(IS_CHAR[np.frombuffer(piece, np.uint8)].sum())


def rows_of(text, offs):
    raw = np.asarray(text, np.uint8).tobytes()
    o = [int(x) for x in offs]
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def stats_of(text, offs, line_limit: int, unit: str):
    """-> (stats int64[11, S], line_start uint8[N])"""
    rows = rows_of(text, offs)
    stats = np.zeros((N, len(rows)), np.int64)
    marks = np.zeros(int(offs[-1]) if len(offs) else 0, np.uint8)
    for i, raw in enumerate(rows):
        a = np.frombuffer(raw, np.uint8)
        lens = [_units(p, unit) for p in pieces_of(raw)]
        stats[:, i] = (len(raw), IS_CHAR[a].sum(), (a == 10).sum(), len(lens), max(lens, default=0), sum(n > line_limit for n in lens),
                       IS_ALPHA[a].sum(), IS_DIGIT[a].sum(), IS_SPACE[a].sum(), IS_NON_ASCII[a].sum(), IS_CONTROL[a].sum())
        at = int(offs[i])
        for p in pieces_of(raw):
            marks[at] = 1
            at += len(p) + 1
    return stats, marks


def second_truth(raw: bytes):
    """-> (characters, [the lines' lengths in characters]) of a row by Python's own strings, or None for invalid UTF-8"""
    try:
        text = raw.decode("utf-8")
    except UnicodeDecodeError:
        return None
    lines = text.split("\n") if text else []
    if text.endswith("\n"):
        lines.pop()
    return len(text), [len(line) for line in lines]


def lines_of(text, offs):
    """-> (offsets uint64[n_lines + 1] of the line view, line_row int64[n_lines])"""
    starts, line_row = [], []
    for i, raw in enumerate(rows_of(text, offs)):
        at = int(offs[i])
        for p in pieces_of(raw):
            starts.append(at)
            line_row.append(i)
            at += len(p) + 1
    return np.asarray(starts + [int(offs[-1]) if len(offs) else 0], np.uint64), np.asarray(line_row, np.int64)


def keep_list(text, offs, max_line=1000, mean_line=100.0, min_alnum=0.25, unit="char"):
    """-> the ascending rows that quality_rows keeps, from this checker's statistics"""
    s, _ = stats_of(text, offs, max_line, unit)
    d = dict(zip(NAMES, s))
    units = d["chars"] if unit == "char" else d["bytes"]
    keep = [i for i in range(s.shape[1])
            if d["max_line"][i] <= max_line and float(units[i] - d["newlines"][i]) <= float(mean_line) * float(d["lines"][i])
            and float(d["alpha"][i] + d["digit"][i]) >= float(min_alnum) * float(d["chars"][i])]
    return np.asarray(keep, np.int64)
