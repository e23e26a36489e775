"""`import tokengeex` — the import name of the reference's Python package (bindings/python: module
`tokengeex`, classes `Tokenizer` and `TokenGeeXError`, stub bindings/python/tokengeex.pyi:3-255), served by
the MI355X implementation in `tokengeex_amd`: code written against the reference's package runs unchanged.
(The reference creates TokenGeeXError but never adds it to its module, bindings/python/src/lib.rs:226-233;
it is exported here, as its stub promises.)"""
from tokengeex_amd import LatticeStats, TokenGeeXError, Tokenizer  # noqa: F401  (LatticeStats: what Tokenizer.lattice_stats returns)
from tokengeex_amd import GOPHER_STOP_WORDS, WordStats, gopher_quality_keep, gopher_quality_rows, word_stats  # noqa: F401  (the Gopher quality filters of a resident corpus)
from tokengeex_amd import word_id, word_rows  # noqa: F401  (a resident corpus's words as rows of a result: word-level n-gram passes)
from tokengeex_amd import BytePattern, compile_pattern, pattern_hits, pattern_rows  # noqa: F401  (regex-class filters of a resident corpus as a scanned DFA)
from tokengeex_amd import pattern_cover, redact, redact_patterns  # noqa: F401  (the bytes inside a match, and their replacement in a new resident corpus)
from tokengeex_amd import ShapePattern, compile_shapes, shape_cover, shape_hits, shape_rows  # noqa: F401  (fixed-length class sequences, API keys and tokens, as a windowed bit scan)
from tokengeex_amd import IdiomMiner, find_matches, mine_idioms  # noqa: F401  (re.finditer on the device, and the reference's idiom miner over it)
from tokengeex_amd import DupSpans, dedup_spans, dup_spans, span_keep, span_rows  # noqa: F401  (spans that occurred earlier in the corpus, verified against the elements, and their deletion)

__all__ = ["Tokenizer", "TokenGeeXError", "LatticeStats", "find_matches", "mine_idioms", "IdiomMiner","word_stats", "WordStats", "gopher_quality_keep", "gopher_quality_rows", "GOPHER_STOP_WORDS", "word_rows", "word_id",
           "compile_pattern", "BytePattern", "pattern_hits", "pattern_rows", "pattern_cover", "redact", "redact_patterns",
           "compile_shapes", "ShapePattern", "shape_hits", "shape_rows", "shape_cover",
           "dup_spans", "DupSpans", "span_keep", "span_rows", "dedup_spans"]
