"""`import tokengeex` — the import name of the reference's Python package (bindings/python: module
`tokengeex`, classes `Tokenizer` and `TokenGeeXError`, stub bindings/python/tokengeex.pyi:3-255), served by
the MI355X implementation in `tokengeex_amd`: code written against the reference's package runs unchanged.
(The reference creates TokenGeeXError but never adds it to its module, bindings/python/src/lib.rs:226-233;
it is exported here, as its stub promises.)"""
from tokengeex_amd import LatticeStats, TokenGeeXError, Tokenizer  # noqa: F401  (LatticeStats: what Tokenizer.lattice_stats returns)
from tokengeex_amd import GOPHER_STOP_WORDS, WordStats, gopher_quality_keep, gopher_quality_rows, word_stats  # noqa: F401  (the Gopher quality filters of a resident corpus)

__all__ = ["Tokenizer", "TokenGeeXError", "LatticeStats", "word_stats", "WordStats", "gopher_quality_keep", "gopher_quality_rows", "GOPHER_STOP_WORDS"]
