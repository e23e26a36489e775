"""An independent checker of the per-row word statistics (include/tgx_words.h: tgx_corpus_word_stats_device).  It knows
nothing of chunks, carries or tails: per row it takes the words of bytes.split(), the ellipses of a regular expression,
the lines of textstat_checker.pieces_of with lstrip / startswith / endswith, and bytes.lower() for the fold."""
import re

import numpy as np

from textstat_checker import IS_CHAR, pieces_of, rows_of

NAMES = ("words", "word_units", "max_word", "long_words", "alpha_words", "alpha_wide_words", "hash", "ellipsis", "lines", "bullet_lines",
         "ellipsis_lines", "punct_lines", "stop_words", "stop_mask")
N = len(NAMES)
UNITS = ("char", "byte")
SPACES = b" \t\n\r\x0b\x0c"
BULLETS = (b"-", b"*", "•".encode())
ELLIPSES = (b"...", "…".encode())
GOPHER = (b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with")
MARK_START, MARK_END, MARK_STOP, MARK_BULLET = 1, 2, 4, 8


def _units(word: bytes, unit: str) -> int:
    return len(word) if unit == "byte" else int(IS_CHAR[np.frombuffer(word, np.uint8)].sum())


def row_stats(raw: bytes, word_limit: int, stops, unit: str, fold: bool):
    """-> the fourteen statistics of one row"""
    words = raw.split()
    lens = [_units(w, unit) for w in words]
    lines = pieces_of(raw)
    seen = [(w.lower() if fold else w) for w in words]
    found = [stops.index(w) for w in seen if w in stops]
    return (len(words), sum(lens), max(lens, default=0), sum(n > word_limit for n in lens),
            sum(re.search(rb"[A-Za-z]", w) is not None for w in words), sum(re.search(rb"[A-Za-z\x80-\xff]", w) is not None for w in words),
            raw.count(b"#"), len(re.findall(rb"\.{3,}", raw)) + raw.count(ELLIPSES[1]), len(lines),
            sum(p.lstrip(SPACES).startswith(BULLETS) for p in lines), sum(p.endswith(ELLIPSES) for p in lines),
            sum(p[-1:] in (b".", b"!", b"?", b'"') for p in lines), len(found), sum(1 << k for k in set(found)))


def row_marks(raw: bytes, stops, fold: bool) -> np.ndarray:
    marks = np.zeros(len(raw), np.uint8)
    for m in re.finditer(rb"[^ \t\n\r\x0b\x0c]+", raw):
        marks[m.start()] |= MARK_START
        marks[m.end() - 1] |= MARK_END
        if (m.group().lower() if fold else m.group()) in stops:
            marks[m.end() - 1] |= MARK_STOP
    at = 0
    for p in pieces_of(raw):
        rest = p.lstrip(SPACES)
        if rest.startswith(BULLETS):
            marks[at + len(p) - len(rest) + (2 if rest.startswith(BULLETS[2]) else 0)] |= MARK_BULLET
        at += len(p) + 1
    return marks


def stats_of(text, offs, word_limit: int, stops=GOPHER, unit: str = "char", fold: bool = True):
    """-> (stats int64[14, S], marks uint8[N])"""
    stops = list(stops)
    rows = rows_of(text, offs)
    stats = np.zeros((N, len(rows)), np.int64)
    marks = [np.zeros(0, np.uint8)]
    for i, raw in enumerate(rows):
        stats[:, i] = row_stats(raw, word_limit, stops, unit, fold)
        marks.append(row_marks(raw, stops, fold))
    return stats, np.concatenate(marks)


def keep_of(stats, min_words=50, max_words=100_000, mean_word=(3, 10), max_symbol_ratio=0.1, max_bullet_lines=0.9, max_ellipsis_lines=0.3,
            min_alpha_words=0.8, min_stop_words=2, wide_is_alpha=True):
    """-> the ascending rows that gopher_quality_rows keeps, decided row by row from this checker's statistics"""
    keep = []
    for i in range(stats.shape[1]):
        d = {name: int(v) for name, v in zip(NAMES, stats[:, i])}
        w, ln = float(d["words"]), float(d["lines"])
        alpha = d["alpha_wide_words"] if wide_is_alpha else d["alpha_words"]
        if (min_words <= d["words"] <= max_words and float(mean_word[0]) * w <= d["word_units"] <= float(mean_word[1]) * w
                and d["hash"] <= max_symbol_ratio * w and d["ellipsis"] <= max_symbol_ratio * w and d["bullet_lines"] <= max_bullet_lines * ln
                and d["ellipsis_lines"] <= max_ellipsis_lines * ln and alpha >= min_alpha_words * w and bin(d["stop_mask"]).count("1") >= min_stop_words):
            keep.append(i)
    return np.asarray(keep, np.int64)
