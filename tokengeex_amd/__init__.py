"""tokengeex_amd — MI355X-native (gfx950) implementation of TokenGeeX's Unigram
encode / E-step hot path behind the reference's Tokenizer API.

Importing this package loads tokengeex_amd/libtgx.so (HIP kernels + C ABI); the
import fails if the extension has not been built.  See include/tgx.h for the ABI
and DESIGN.md for the path and its boundary.
"""
from ._lib import (ESTEP_SNIPPET_LEN, MAX_TOKEN_LEN, LatticeStats, NativeCorpus, NativeModel, NativeResult, NativeText,
                   TokenGeeXError, device_count, pack, pool_filled_bytes, pool_trim)
from . import tensors  # torch is imported inside its functions
from .tensors import (clean_rows, first_equal, gram_hits, gram_set, line_repetition_rows, line_rows, quality_rows, repeat_stats, repetition_rows, text_stats, minhash, minhash_bands, near_first, near_unique_rows, row_hashes, row_lengths, select, shuffled_rows, to_packed, to_padded, to_padded_spans, to_spans,
                      to_window_spans, to_windows, unique_rows,
                      GOPHER_STOP_WORDS, WordStats, gopher_quality_keep, gopher_quality_rows, word_stats)
from .tokenizer import CrlfProcessor, Tokenizer, UnicodeProcessor, split_special_tokens

__all__ = ["Tokenizer", "TokenGeeXError", "NativeModel", "NativeCorpus", "NativeResult", "NativeText", "LatticeStats",
           "CrlfProcessor", "UnicodeProcessor", "split_special_tokens", "device_count", "pack", "pool_trim", "pool_filled_bytes",
           "MAX_TOKEN_LEN", "ESTEP_SNIPPET_LEN", "tensors", "to_padded", "to_packed", "to_spans", "to_padded_spans",
           "to_windows", "to_window_spans", "select", "row_lengths", "shuffled_rows", "first_equal", "unique_rows",
           "row_hashes", "minhash", "minhash_bands", "near_first", "near_unique_rows",
           "gram_set", "gram_hits", "clean_rows", "text_stats", "quality_rows", "line_rows",
           "repeat_stats", "repetition_rows", "line_repetition_rows",
           "word_stats", "WordStats", "gopher_quality_keep", "gopher_quality_rows", "GOPHER_STOP_WORDS"]
