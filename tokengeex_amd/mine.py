"""Idiom mining: the `mine` stage of the reference's training pipeline (src/mine.rs: IdiomMiner) on the device.

    miner = IdiomMiner(1000, [r" ?[A-Za-z_][A-Za-z0-9_]*", r"[0-9]{1,3}", r"\\n[ ]+"])
    idioms = miner.mine(samples)        # [(bytes, count)], the most frequent distinct matches: suggested tokens for `generate`

The reference runs a regex's find_iter over every sample and keeps the num_idioms most frequent matches.  Here the
pattern is compiled to the leftmost-first automaton of patterns.compile_pattern(..., find=True) and the matches are found,
keyed, counted and ranked by tensors.mine_idioms (csrc/find.hip; include/tgx_find.h).  Two things
differ from the reference, both on purpose: ties are ordered by first occurrence, where the reference leaves them to a
hash map's iteration order; and a match is at most max_len <= 64 bytes, so a longer one is cut there, which mine() reports
as an error unless it is told that this is fine."""
from __future__ import annotations

from . import _lib, patterns, tensors


class IdiomMiner:
    """IdiomMiner(num_idioms, pattern): pattern is a regex (str or bytes) in the syntax of patterns.compile_pattern, a
    list of them (their alternation in list order), or a BytePattern compiled with find=True."""

    def __init__(self, num_idioms: int, pattern, max_len: int = 64, device: int = 0):
        if int(num_idioms) < 1:
            raise ValueError("num_idioms must be at least 1")
        self.num_idioms, self.max_len, self.device = int(num_idioms), int(max_len), device
        self.pattern = pattern if isinstance(pattern, patterns.BytePattern) else patterns.compile_pattern(pattern, find=True)

    def mine(self, samples, allow_truncated: bool = False) -> "list[tuple[bytes, int]]":
        """samples: a list of str / bytes, or a resident NativeCorpus -> the num_idioms most frequent matches with their
        counts, by count descending and then by first occurrence.  ValueError when a match of some row was cut at max_len
        bytes, unless allow_truncated."""
        corpus = samples if isinstance(samples, _lib.NativeCorpus) else _lib.NativeCorpus(*_lib.pack([s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in samples]), device=self.device)
        try:
            if not allow_truncated:
                _, truncated = tensors.find_matches(corpus, self.pattern, self.max_len, return_truncated=True)
                rows = int((truncated != 0).sum())
                if rows:
                    raise ValueError(f"{rows} rows hold a match that goes on past max_len={self.max_len} bytes (the first: row {int(truncated.nonzero()[0])}); "
                                     "pass allow_truncated=True to count the cut matches")
            return tensors.mine_idioms(corpus, self.pattern, self.num_idioms, self.max_len)
        finally:
            if corpus is not samples:
                corpus.free()
