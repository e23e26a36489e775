"""Encoded ids as PyTorch tensors on the device that produced them.

A NativeResult (of encode, sampling or n-best: n-best rows are just rows) holds flat u32 ids and u64 offsets in HBM.
`to_padded` and `to_packed` lay them out for a model — [S, L] `input_ids` with `attention_mask`, or the documents
concatenated and cut into [B, L] blocks — with the kernels of csrc/layout.hip, straight into tensors allocated with
`torch.empty`: the ids never visit the host.  `to_spans` and `to_padded_spans` give the offsets mapping the same way:
the part of its row's text that every token covers, in bytes or characters (csrc/spans.hip).  `to_windows` and
`to_window_spans` keep every token of a row longer than `max_length`: overlapping [W, L] windows, each tagged with the row
it came from (HF's `return_overflowing_tokens` with a `stride`).

The kernels are queued on `torch.cuda.current_stream(device)`, the stream torch's caching allocator orders the
tensors' memory on, and the call returns once that stream has reached its end: the tensors can be used by any torch op
right away, and the result may be freed right away.  The current device is not changed.

torch is imported inside the functions: `import tokengeex_amd` stays torch-free.
"""
from __future__ import annotations

from . import _lib


def _np_dtype(torch, dtype):
    import numpy as np
    if dtype == torch.int64:
        return np.int64
    if dtype == torch.int32:
        return np.int32
    raise ValueError(f"dtype must be torch.int32 or torch.int64 (got {dtype})")


def _check_dest(torch, name: str, t, device, dtype, numel: int) -> int:
    """A destination must be a contiguous tensor of `dtype` on `device` with room for numel elements -> its data_ptr()."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the result on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.numel() < numel:
        raise ValueError(f"{name} has room for {t.numel()} elements, {numel} are written")
    return t.data_ptr() if numel else 0


def _device_of(torch, result):
    if not torch.cuda.is_available():
        # libtgx.so produced the result, so a GPU is there: torch is looking through a HIP runtime of its own
        raise _lib.TokenGeeXError("torch sees no GPU although libtgx.so does: two HIP runtimes in one process "
                                  "(TGX_HIP_RUNTIME=system set? then import torch before tokengeex_amd)", _lib.ERR_DEVICE)
    return torch.device("cuda", result.device)


def pad_into(result: "_lib.NativeResult", input_ids, attention_mask=None, lengths=None, *, row_len: int, pad_id: int,
             bos_id: int | None = None, eos_id: int | None = None, padding_side: str = "right",
             truncation_side: str = "right") -> int:
    """The padded layout written into tensors the caller owns (input_ids: int32 or int64, at least S·row_len elements;
    attention_mask: uint8, the same count; lengths: int32, S): each must be contiguous and on the result's device, which
    is checked before anything is launched.  -> number of truncated rows."""
    import torch
    dev = _device_of(torch, result)
    S, L = result.num_samples, int(row_len)
    if not isinstance(input_ids, torch.Tensor):
        raise TypeError("input_ids must be a torch.Tensor")
    flags = _lib.layout_flags(padding_side, truncation_side, _np_dtype(torch, input_ids.dtype))
    p_ids = _check_dest(torch, "input_ids", input_ids, dev, input_ids.dtype, S * L)
    p_mask = 0 if attention_mask is None else _check_dest(torch, "attention_mask", attention_mask, dev, torch.uint8, S * L)
    p_len = 0 if lengths is None else _check_dest(torch, "lengths", lengths, dev, torch.int32, S)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return result.pad_device(L, pad_id, p_ids, mask_ptr=p_mask, lengths_ptr=p_len, bos_id=bos_id, eos_id=eos_id, flags=flags,
                             stream=stream)


def pack_into(result: "_lib.NativeResult", input_ids, doc_ids=None, positions=None, *, block_len: int, pad_id: int,
              bos_id: int | None = None, eos_id: int | None = None) -> int:
    """The packed layout written into tensors the caller owns (input_ids: int32 or int64; doc_ids, positions: int32; each
    at least n_blocks·block_len elements, n_blocks = ceil(result.layout_info(bos_id, eos_id)[1] / block_len)); checked
    as in pad_into.  -> n_blocks."""
    import torch
    dev = _device_of(torch, result)
    L = int(block_len)
    if L < 1:
        raise _lib.TokenGeeXError("block_len must be at least 1", _lib.ERR_INVALID)
    if not isinstance(input_ids, torch.Tensor):
        raise TypeError("input_ids must be a torch.Tensor")
    flags = _lib.layout_flags(dtype=_np_dtype(torch, input_ids.dtype))
    n_out = -(-result.layout_info(bos_id, eos_id)[1] // L) * L
    p_ids = _check_dest(torch, "input_ids", input_ids, dev, input_ids.dtype, n_out)
    p_doc = 0 if doc_ids is None else _check_dest(torch, "doc_ids", doc_ids, dev, torch.int32, n_out)
    p_pos = 0 if positions is None else _check_dest(torch, "positions", positions, dev, torch.int32, n_out)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return result.pack_device(L, pad_id, p_ids, doc_ptr=p_doc, pos_ptr=p_pos, bos_id=bos_id, eos_id=eos_id, flags=flags,
                              stream=stream)


def to_padded(result: "_lib.NativeResult", *, max_length: int | None = None, pad_id: int, bos_id: int | None = None,
              eos_id: int | None = None, padding_side: str = "right", truncation_side: str = "right", dtype=None,
              return_lengths: bool = False) -> dict:
    """-> {"input_ids": [S, L] of dtype (torch.int64 by default, or torch.int32), "attention_mask": [S, L] torch.uint8
    [, "lengths": [S] torch.int32]} on torch.device("cuda", result.device).

    Every row is [bos] + its tokens + [eos], cut to L (truncation_side: which end of the TOKENS goes; bos and eos
    stay) and filled up with pad_id on padding_side.  max_length=None: L = the longest row with its bos / eos (at
    least 1), so nothing is truncated."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    _np_dtype(torch, dtype)
    dev = _device_of(torch, result)
    if max_length is None:
        L = max(1, result.layout_info(bos_id, eos_id)[0])
    else:
        L = int(max_length)
        if L < 1:
            raise _lib.TokenGeeXError("max_length must be at least 1", _lib.ERR_INVALID)
    S = result.num_samples
    out = {"input_ids": torch.empty((S, L), dtype=dtype, device=dev),
           "attention_mask": torch.empty((S, L), dtype=torch.uint8, device=dev)}
    if return_lengths:
        out["lengths"] = torch.empty((S,), dtype=torch.int32, device=dev)
    pad_into(result, out["input_ids"], out["attention_mask"], out.get("lengths"), row_len=L, pad_id=pad_id, bos_id=bos_id,
             eos_id=eos_id, padding_side=padding_side, truncation_side=truncation_side)
    return out


def to_packed(result: "_lib.NativeResult", block_len: int, *, pad_id: int, bos_id: int | None = None, eos_id: int | None = None,
              dtype=None, return_doc: bool = False, drop_last: bool = False) -> dict:
    """The LM-pretraining layout -> {"input_ids": [B, block_len] of dtype [, "doc_ids", "positions": [B, block_len]
    torch.int32]}: the rows' sequences [bos] + tokens + [eos] concatenated and cut into blocks; doc_ids names the row
    an element came from, positions its index in that row's sequence; the tail of the last block holds pad_id, doc -1,
    position 0.  drop_last leaves a partly filled last block out (a view of the same memory)."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    _np_dtype(torch, dtype)
    dev = _device_of(torch, result)
    L = int(block_len)
    if L < 1:
        raise _lib.TokenGeeXError("block_len must be at least 1", _lib.ERR_INVALID)
    n_stream = result.layout_info(bos_id, eos_id)[1]
    B = -(-n_stream // L)
    out = {"input_ids": torch.empty((B, L), dtype=dtype, device=dev)}
    if return_doc:
        out["doc_ids"] = torch.empty((B, L), dtype=torch.int32, device=dev)
        out["positions"] = torch.empty((B, L), dtype=torch.int32, device=dev)
    pack_into(result, out["input_ids"], out.get("doc_ids"), out.get("positions"), block_len=L, pad_id=pad_id, bos_id=bos_id,
              eos_id=eos_id)
    if drop_last and n_stream % L:
        out = {k: v[:B - 1] for k, v in out.items()}
    return out


# ---- rows selected and reordered on the device (csrc/select.hip) ---------------------------------------------------------

def select(obj, rows):
    """A NativeResult or NativeCorpus whose row k is row rows[k] of `obj` (any order, any subset, repeats allowed), moved
    on the device.  rows: a torch tensor of indices or a boolean mask (on obj's device: read in place, in the order of
    torch.cuda.current_stream; on the host: uploaded), a list or a numpy array."""
    return obj.select(rows)


def row_lengths(result: "_lib.NativeResult"):
    """-> [S] torch.int64 on the result's device: the rows' token counts, for filtering and sorting without a host trip."""
    import torch
    dev = _device_of(torch, result)
    out = torch.empty((result.num_samples,), dtype=torch.int64, device=dev)
    result.lengths_device(out.data_ptr() if out.numel() else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def shuffled_rows(n: int, seed: int, device=0):
    """-> [n] torch.int64 on `device` (an index, or a torch.device): the seeded permutation of 0 .. n-1, the same on
    every machine and on the host (_lib.shuffled_rows_host): the rows sorted by (tgx_shuffle_key(seed, row), row)."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.TokenGeeXError("torch sees no GPU", _lib.ERR_DEVICE)
    dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    index = torch.cuda.current_device() if dev.index is None else dev.index
    dev = torch.device("cuda", index)
    out = torch.empty((int(n),), dtype=torch.int64, device=dev)
    _lib.shuffled_rows_device(index, int(n), seed, out.data_ptr() if out.numel() else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- exact row deduplication on the device (csrc/dedup.hip) --------------------------------------------------------------

def first_equal(obj):
    """-> [S] torch.int64 on obj's device (a NativeResult or NativeCorpus): first[k] = the first row with exactly row k's
    content, so first[k] == k marks the rows to keep and torch.bincount(first) gives the group sizes.  Exact: a hash
    finds the candidates, an element-by-element comparison decides."""
    import torch
    dev = _device_of(torch, obj)
    out = torch.empty((obj.num_samples,), dtype=torch.int64, device=dev)
    obj.first_equal(out.data_ptr() if out.numel() else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def unique_rows(obj):
    """-> torch.int64 indices, ascending, of the rows of obj that no earlier row equals: what `select` takes to drop the
    duplicates (of a corpus and, with the same indices, of its encoded result)."""
    import torch
    first = first_equal(obj)
    return (first == torch.arange(first.shape[0], dtype=torch.int64, device=first.device)).nonzero().reshape(-1)


def row_hashes(obj, seed: int = 0):
    """-> [S] torch.int64 on obj's device holding the u64 bits of tgx_row_hash(row, seed) of every row: the same on every
    machine, for a deduplication across ranks after an all-gather (probabilistic, unlike first_equal)."""
    import torch
    dev = _device_of(torch, obj)
    out = torch.empty((obj.num_samples,), dtype=torch.int64, device=dev)
    obj.row_hashes(out.data_ptr() if out.numel() else 0, seed, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- near-duplicate rows on the device (csrc/minhash.hip) ----------------------------------------------------------------

def minhash(obj, width: int = 5, n_perm: int = 128, seed: int = 0):
    """-> [S, n_perm] torch.int32 on obj's device (a NativeResult: token n-grams of `width` ids; a NativeCorpus: shingles
    of `width` bytes) holding the u32 bits of every row's MinHash signature, the same on every machine.  The share of
    equal entries of two signatures estimates the Jaccard similarity of the two rows' shingle sets."""
    import torch
    dev = _device_of(torch, obj)
    out = torch.empty((obj.num_samples, int(n_perm)), dtype=torch.int32, device=dev)
    obj.minhash(out.data_ptr() if out.numel() else 0, width, n_perm, seed, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def _check_sig(torch, sig):
    if not isinstance(sig, torch.Tensor) or sig.dtype != torch.int32 or sig.dim() != 2 or not sig.is_cuda:
        raise TypeError("sig must be a [S, K] torch.int32 tensor on a GPU, as minhash returns it")
    return sig.contiguous()


def minhash_bands(sig, bands: int, seed: int = 0):
    """-> (keys, heads), both [S, bands] torch.int64 on sig's device: the u64 bits of every band's key (what ranks
    all-gather for a pass across them) and head[i][b], the first row in row i's bucket of band b.  bands must divide K."""
    import torch
    sig = _check_sig(torch, sig)
    S, K = sig.shape
    keys = torch.empty((S, int(bands)), dtype=torch.int64, device=sig.device)
    heads = torch.empty((S, int(bands)), dtype=torch.int64, device=sig.device)
    spare = torch.empty(1, dtype=torch.int64, device=sig.device)  # (no row: the pointers still say that both are asked for)
    _lib.minhash_bands(sig.device.index, sig.data_ptr() if S else 0, S, K, bands, seed, (keys if S else spare).data_ptr(),
                       (heads if S else spare).data_ptr(), stream=torch.cuda.current_stream(sig.device).cuda_stream)
    return keys, heads


def near_first(sig, bands: int, threshold: float, seed: int = 0):
    """-> [S] torch.int64 on sig's device: first[i] = the root of row i's near-duplicate cluster, so first[i] == i marks
    the rows to keep.  Rows that share a bucket in one of `bands` bands are candidates; a row joins its bucket's head when
    at least ceil(threshold·K) of their K signature values agree.  A star per bucket: a row is compared with the bucket's
    head only, and clusters join through chains of heads."""
    import math
    import torch
    sig = _check_sig(torch, sig)
    S, K = sig.shape
    if not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"threshold must be in (0, 1] (got {threshold})")
    min_agree = max(1, math.ceil(float(threshold) * K))
    _, heads = minhash_bands(sig, bands, seed)
    first = torch.empty((S,), dtype=torch.int64, device=sig.device)
    _lib.minhash_near_first(sig.device.index, sig.data_ptr() if S else 0, S, K, heads.data_ptr() if S else 0, bands, min_agree,
                            first.data_ptr() if S else 0, stream=torch.cuda.current_stream(sig.device).cuda_stream)
    return first


def near_unique_rows(sig, bands: int, threshold: float, seed: int = 0):
    """-> torch.int64 indices, ascending, of the rows that are the root of their near-duplicate cluster: what `select`
    takes to drop the near-copies (of a corpus and, with the same indices, of its encoded result)."""
    import torch
    first = near_first(sig, bands, threshold, seed)
    return (first == torch.arange(first.shape[0], dtype=torch.int64, device=first.device)).nonzero().reshape(-1)


# ---- shared n-grams on the device: decontamination (csrc/gram.hip) -------------------------------------------------------

def gram_set(obj, width: int, seed: int = 0):
    """-> a NativeGramSet on obj's device: the distinct 64-bit keys of every n-gram of `width` elements of obj's rows (a
    NativeResult: ids; a NativeCorpus: bytes), queued on torch's current stream.  Made of a small held-out set and handed
    to gram_hits.  A row shorter than `width` owns no n-gram."""
    import torch
    dev = _device_of(torch, obj)
    return obj.gram_set(width, seed, stream=torch.cuda.current_stream(dev).cuda_stream)


def gram_hits(obj, grams, return_mask: bool = False):
    """-> [S] torch.int64 on obj's device: per row the n-grams (of grams.width elements) whose key is in `grams`; with
    return_mask also [n_elems] torch.uint8, 1 where such an n-gram begins.  Membership is by 64-bit key, so
    probabilistic in the sense of row_hashes; a hit is not verified against the elements."""
    import torch
    dev = _device_of(torch, obj)
    count = torch.empty((obj.num_samples,), dtype=torch.int64, device=dev)
    n_elems = obj.num_tokens if isinstance(obj, _lib.NativeResult) else obj.num_bytes
    mask = torch.empty((n_elems,), dtype=torch.uint8, device=dev) if return_mask else None
    spare = torch.empty(1, dtype=torch.int64, device=dev)  # (no row: the pointer still says that the counts are asked for)
    obj.gram_hits(grams, (count if count.numel() else spare).data_ptr(), mask.data_ptr() if return_mask and n_elems else 0,
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    return (count, mask) if return_mask else count


def clean_rows(obj, grams, max_hits: int = 0):
    """-> torch.int64 indices, ascending, of the rows of obj with at most max_hits n-grams in `grams`: what `select` takes
    to drop the contaminated rows (of a corpus and, with the same indices, of its encoded result)."""
    return (gram_hits(obj, grams) <= int(max_hits)).nonzero().reshape(-1)


# ---- per-row text statistics and the line view: quality filters (csrc/textstat.hip) --------------------------------------

class TextStats:
    """What text_stats returns: `table`, [11, S] torch.int64 on the corpus's device, and a [S] view of it per statistic
    (bytes, chars, newlines, lines, max_line, long_lines, alpha, digit, space, non_ascii, control: include/tgx.h);
    `unit` ("char" or "byte") is what max_line and long_lines are counted in; `line_start` is the [N] uint8 mask of the
    bytes at which a line begins, or None when it was not asked for."""

    def __init__(self, table, unit: str, line_limit: int, line_start=None):
        self.table, self.unit, self.line_limit, self.line_start = table, unit, int(line_limit), line_start
        for k, name in enumerate(_lib.TEXTSTAT_NAMES):
            setattr(self, name, table[k])

    @property
    def units(self):
        """[S]: the rows' lengths in the unit (chars or bytes)."""
        return self.chars if self.unit == "char" else self.bytes

    @property
    def mean_line(self):
        """[S] float64: (units - newlines) / max(lines, 1), the mean length of a row's lines without their '\\n'."""
        import torch
        return (self.units - self.newlines).to(torch.float64) / self.lines.clamp(min=1).to(torch.float64)

    @property
    def alnum_frac(self):
        """[S] float64: (alpha + digit) / max(chars, 1), the ASCII letters' and digits' share of the row's characters."""
        import torch
        return (self.alpha + self.digit).to(torch.float64) / self.chars.clamp(min=1).to(torch.float64)


def text_stats(corpus: "_lib.NativeCorpus", unit: str = "char", line_limit: int = 1000, return_line_start: bool = False) -> TextStats:
    """-> a TextStats of the corpus's rows, computed on its device and queued on torch's current stream: per row the
    bytes, characters, '\\n's, lines, the longest line and the lines longer than line_limit (both in `unit`: "char", a
    byte that is no UTF-8 continuation byte, or "byte"), and the ASCII letters, digits, white space, non-ASCII characters
    and control bytes.  Only '\\n' ends a line, no line crosses a row's end, and a trailing '\\n' opens no empty last line.
    With return_line_start also the [N] uint8 mask of the bytes at which a line begins."""
    import torch
    dev = _device_of(torch, corpus)
    _lib.textstat_flags(unit)  # (raises on an unknown unit before anything is allocated)
    S, N = corpus.num_samples, corpus.num_bytes
    table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device=dev)
    marks = torch.empty((N,), dtype=torch.uint8, device=dev) if return_line_start else None
    spare = torch.empty(1, dtype=torch.int64, device=dev)  # (no row: the pointer still says that the table is asked for)
    corpus.text_stats((table if S else spare).data_ptr(), marks.data_ptr() if return_line_start and N else 0, line_limit, unit,
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    return TextStats(table, unit, line_limit, marks)


def quality_rows(corpus: "_lib.NativeCorpus", max_line: int = 1000, mean_line: float = 100.0, min_alnum: float = 0.25, unit: str = "char"):
    """-> torch.int64 indices, ascending, of the rows that pass the line-length and alphanumeric filters of the Stack /
    StarCoder recipe: what `select` takes to drop the others (of a corpus and, with the same indices, of its encoded
    result).  A row is kept iff its longest line has at most max_line units, units - newlines <= mean_line · lines (its
    mean line length is at most mean_line) and alpha + digit >= min_alnum · chars.  The comparisons are division-free
    float64, so an empty row is kept.  Unlike the BigCode scripts, whose share is Python's Unicode str.isalnum over the
    characters, the letters and digits counted here are ASCII only; text_stats gives `non_ascii` beside them for a caller
    who wants to credit or discount the rest."""
    import torch
    s = text_stats(corpus, unit=unit, line_limit=max_line)
    f64 = torch.float64
    keep = s.max_line <= int(max_line)
    keep &= (s.units - s.newlines).to(f64) <= float(mean_line) * s.lines.to(f64)
    keep &= (s.alpha + s.digit).to(f64) >= float(min_alnum) * s.chars.to(f64)
    return keep.nonzero().reshape(-1)


def line_rows(corpus: "_lib.NativeCorpus"):
    """-> (lines_corpus, line_row): a new resident corpus whose rows are the lines of `corpus`, in order, each with its
    '\\n' if it has one, and [n_lines] torch.int64, the row of `corpus` that each line came from.  first_equal of the lines
    plus torch gives the duplicate-line shares of the Gopher rules."""
    import torch
    dev = _device_of(torch, corpus)
    lines = corpus.lines(stream=torch.cuda.current_stream(dev).cuda_stream)
    counts = text_stats(corpus, unit="byte").lines
    return lines, torch.repeat_interleave(torch.arange(corpus.num_samples, dtype=torch.int64, device=dev), counts)


# ---- per-row word statistics: the Gopher quality filters (csrc/wordstat.hip) ------------------------------------------------

GOPHER_STOP_WORDS = _lib.GOPHER_STOP_WORDS


class WordStats:
    """What word_stats returns: `table`, [14, S] torch.int64 on the corpus's device, and a [S] view of it per statistic
    (words, word_units, max_word, long_words, alpha_words, alpha_wide_words, hash, ellipsis, lines, bullet_lines,
    ellipsis_lines, punct_lines, stop_words, stop_mask: include/tgx_words.h); `unit` ("char" or "byte") is what a word's
    length is counted in; `stop_words`, the table's entries, bit k of stop_mask being entry k; `mask` is the [N] uint8
    tensor of the bytes' marks (bit 0 a word start, bit 1 a word end, bit 2 the end of a stop word, bit 3 the last byte
    of a line-leading bullet), or None when it was not asked for.  The shares are float64 with a denominator of at
    least 1, so a row without a word or a line has 0."""

    def __init__(self, table, unit: str, word_limit: int, stop_words=(), mask=None):
        self.table, self.unit, self.word_limit, self.stop_words, self.mask = table, unit, int(word_limit), tuple(stop_words), mask
        for k, name in enumerate(_lib.WORDSTAT_NAMES):
            setattr(self, name, table[k])

    def _share(self, count, of):
        import torch
        return count.to(torch.float64) / of.clamp(min=1).to(torch.float64)

    @property
    def mean_word(self):
        """[S] float64: word_units / max(words, 1), the mean length of a row's words."""
        return self._share(self.word_units, self.words)

    @property
    def alpha_frac(self):
        """[S] float64: alpha_words / max(words, 1), the share of the words that hold an ASCII letter."""
        return self._share(self.alpha_words, self.words)

    @property
    def alpha_wide_frac(self):
        """[S] float64: alpha_wide_words / max(words, 1): an ASCII letter or any non-ASCII byte."""
        return self._share(self.alpha_wide_words, self.words)

    @property
    def hash_ratio(self):
        """[S] float64: hash / max(words, 1)."""
        return self._share(self.hash, self.words)

    @property
    def ellipsis_ratio(self):
        """[S] float64: ellipsis / max(words, 1)."""
        return self._share(self.ellipsis, self.words)

    @property
    def bullet_frac(self):
        """[S] float64: bullet_lines / max(lines, 1)."""
        return self._share(self.bullet_lines, self.lines)

    @property
    def ellipsis_line_frac(self):
        """[S] float64: ellipsis_lines / max(lines, 1)."""
        return self._share(self.ellipsis_lines, self.lines)

    @property
    def punct_line_frac(self):
        """[S] float64: punct_lines / max(lines, 1), the share of the lines that end in . ! ? or a double quote (C4,
        FineWeb)."""
        return self._share(self.punct_lines, self.lines)

    @property
    def stop_distinct(self):
        """[S] int64: the popcount of stop_mask, how many different stop words the row holds."""
        return _popcount63(self.stop_mask)


def _popcount63(mask):
    """the set bits among bits 0 .. 62 of every entry of an int64 tensor (a stop table has at most 63 entries)"""
    import torch
    bits = torch.arange(63, dtype=torch.int64, device=mask.device).reshape(-1, *([1] * mask.dim()))
    return ((mask.unsqueeze(0) >> bits) & 1).sum(0)


def word_stats(corpus: "_lib.NativeCorpus", word_limit: int = 20, stop_words=GOPHER_STOP_WORDS, unit: str = "char", fold_case: bool = True,
               return_mask: bool = False) -> WordStats:
    """-> a WordStats of the corpus's rows, computed on its device and queued on torch's current stream: per row the
    words, the sum of their lengths, the longest and those longer than word_limit (lengths in `unit`: "char", a byte that
    is no UTF-8 continuation byte, or "byte"), the words that hold a letter, the '#'s and ellipses, the lines and those
    that begin with a bullet, end with an ellipsis or end with terminal punctuation, and the occurrences and the set of
    the stop words (at most 63 words of 1 to 8 bytes, bytes or str; with fold_case the text's A-Z match a-z, and an entry
    must then hold no A-Z).  With return_mask also the [N] uint8 marks of the bytes.

    A word is a maximal run of bytes that are no white space (0x20, 0x09 .. 0x0D: what bytes.split() splits on; non-ASCII
    spaces are ordinary bytes) within a row.  Gopher's words come from a word tokenizer, these from white space: "end."
    is one word here and punctuation counts into its length.  The letter test is ASCII (alpha_words) or ASCII plus any
    non-ASCII byte (alpha_wide_words), not Unicode's classes.  Trailing spaces at a line's end are not trimmed before the
    ellipsis and punctuation tests."""
    import torch
    dev = _device_of(torch, corpus)
    _lib.wordstat_flags(unit, fold_case)  # (raises on an unknown unit before anything is allocated)
    stop_words = tuple(stop_words or ())
    S, N = corpus.num_samples, corpus.num_bytes
    table = torch.empty((_lib.WORDSTAT_N, S), dtype=torch.int64, device=dev)
    marks = torch.empty((N,), dtype=torch.uint8, device=dev) if return_mask else None
    spare = torch.empty(1, dtype=torch.int64, device=dev)  # (no row: the pointer still says that the table is asked for)
    corpus.word_stats((table if S else spare).data_ptr(), marks.data_ptr() if return_mask and N else 0, word_limit, stop_words, unit, fold_case,
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    return WordStats(table, unit, word_limit, stop_words, marks)


def gopher_quality_keep(table, min_words: int = 50, max_words: int = 100_000, mean_word=(3, 10), max_symbol_ratio: float = 0.1,
                        max_bullet_lines: float = 0.9, max_ellipsis_lines: float = 0.3, min_alpha_words: float = 0.8, min_stop_words: int = 2,
                        wide_is_alpha: bool = True):
    """-> [S] torch.bool, the rows that pass Gopher's quality rules, from a [14, S] int64 table of word_stats on any
    device.  A row is kept iff min_words <= words <= max_words, mean_word[0] · words <= word_units <= mean_word[1] · words,
    hash <= max_symbol_ratio · words and ellipsis <= max_symbol_ratio · words, bullet_lines <= max_bullet_lines · lines,
    ellipsis_lines <= max_ellipsis_lines · lines, the words with a letter >= min_alpha_words · words (alpha_wide_words
    with wide_is_alpha, which credits every non-ASCII byte as a letter, else alpha_words), and at least min_stop_words
    different stop words occur.  The comparisons are division-free float64: a row exactly on a threshold is kept, and an
    empty row fails min_words >= 1.  The defaults are Gopher's figures over white-space words, which are not Gopher's
    tokenizer's words: the thresholds are the caller's to tune."""
    import torch
    f64 = torch.float64
    d = dict(zip(_lib.WORDSTAT_NAMES, table))
    words, lines = d["words"].to(f64), d["lines"].to(f64)
    keep = (d["words"] >= int(min_words)) & (d["words"] <= int(max_words))
    keep &= (d["word_units"].to(f64) >= float(mean_word[0]) * words) & (d["word_units"].to(f64) <= float(mean_word[1]) * words)
    keep &= (d["hash"].to(f64) <= float(max_symbol_ratio) * words) & (d["ellipsis"].to(f64) <= float(max_symbol_ratio) * words)
    keep &= d["bullet_lines"].to(f64) <= float(max_bullet_lines) * lines
    keep &= d["ellipsis_lines"].to(f64) <= float(max_ellipsis_lines) * lines
    keep &= d["alpha_wide_words" if wide_is_alpha else "alpha_words"].to(f64) >= float(min_alpha_words) * words
    keep &= _popcount63(d["stop_mask"]) >= int(min_stop_words)
    return keep


def gopher_quality_rows(corpus: "_lib.NativeCorpus", min_words: int = 50, max_words: int = 100_000, mean_word=(3, 10), max_symbol_ratio: float = 0.1,
                        max_bullet_lines: float = 0.9, max_ellipsis_lines: float = 0.3, min_alpha_words: float = 0.8, min_stop_words: int = 2,
                        wide_is_alpha: bool = True, stop_words=GOPHER_STOP_WORDS, unit: str = "char", fold_case: bool = True):
    """-> torch.int64 indices, ascending, of the rows that pass gopher_quality_keep over word_stats of the corpus: what
    `select` takes to drop the others (of a corpus and, with the same indices, of its encoded result).  The words come
    from white space, not from Gopher's word tokenizer, the letter test is ASCII plus (with wide_is_alpha) any non-ASCII
    byte, and the thresholds are the caller's to tune."""
    s = word_stats(corpus, stop_words=stop_words, unit=unit, fold_case=fold_case)
    keep = gopher_quality_keep(s.table, min_words, max_words, mean_word, max_symbol_ratio, max_bullet_lines, max_ellipsis_lines, min_alpha_words,
                               min_stop_words, wide_is_alpha)
    return keep.nonzero().reshape(-1)


# ---- repeated n-grams within a row: the Gopher repetition filters (csrc/repeat.hip) ---------------------------------------

# ---- literal phrase matching: blocklists and keyword filters (csrc/phrase.hip) ---------------------------------------------

AUTOGENERATED = ("auto-generated", "autogenerated", "automatically generated", "generated automatically", "this file is generated")


def phrase_set(phrases, *, kind: str = "bytes", fold_case: bool = False, whole_word: bool = False, device: int = 0):
    """-> a NativePhraseSet on `device`: a trie in device memory over a list of literal phrases, handed to phrase_hits.
    kind "bytes": list[bytes | str] (a str as UTF-8), each of 1 to 255 bytes, for a NativeCorpus; kind "ids":
    list[list[int]], each of 1 to 64 ids, for a NativeResult.  fold_case lowers A-Z in the phrases and in the text (ASCII
    only); whole_word asks that the bytes on either side of an occurrence, inside its row, are no word bytes
    ([A-Za-z0-9_] and every byte >= 0x80); both need kind "bytes".  Phrases equal after folding are one phrase under
    the lowest index.  It carries .size, .distinct, .kind, .max_len, .device and .free()."""
    return _lib.NativePhraseSet(phrases, kind, fold_case, whole_word, int(device))


def phrase_hits(obj, phrases, return_longest: bool = False, return_per_phrase: bool = False):
    """-> [S] torch.int64 on obj's device: per row the occurrences (start, phrase) of the phrases of `phrases` (a
    NativePhraseSet of obj's kind), queued on torch's current stream.  Occurrences may overlap and none crosses a row's
    end.  With return_longest also [n_elems] torch.uint8, the length of the longest occurrence that begins at each
    element (0: none); with return_per_phrase also [P] torch.int64, the occurrences of each phrase over all rows.  The
    extras follow the counts in that order.  Matching is exact, unlike gram_hits' keys."""
    import torch
    dev = _device_of(torch, obj)
    n_elems = obj.num_tokens if isinstance(obj, _lib.NativeResult) else obj.num_bytes
    count = torch.empty((obj.num_samples,), dtype=torch.int64, device=dev)
    longest = torch.empty((n_elems,), dtype=torch.uint8, device=dev) if return_longest else None
    per = torch.empty((phrases.size,), dtype=torch.int64, device=dev) if return_per_phrase else None
    spare = torch.empty(1, dtype=torch.int64, device=dev)  # (no row: the pointer still says that the counts are asked for)
    obj.phrase_hits(phrases, (count if count.numel() else spare).data_ptr(), longest.data_ptr() if return_longest and n_elems else 0,
                    per.data_ptr() if return_per_phrase and per.numel() else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
    out = (count,) + ((longest,) if return_longest else ()) + ((per,) if return_per_phrase else ())
    return out if len(out) > 1 else count


def phrase_rows(obj, phrases, max_hits: int = 0):
    """-> torch.int64 indices, ascending, of the rows of obj with at most max_hits occurrences of the phrases: what `select`
    takes to drop the others (of a corpus and, with the same indices, of its encoded result)."""
    return (phrase_hits(obj, phrases) <= int(max_hits)).nonzero().reshape(-1)


def phrase_cover(longest):
    """Plain torch, on any device: `longest` [N] uint8 of phrase_hits -> [N] bool, True for the elements inside some
    occurrence: cummax(e + longest[e]) > e over the flat array, which is right across rows because no occurrence crosses
    a row's end.  For redaction, or the share of a row's bytes in blocked phrases."""
    import torch
    n = longest.shape[0]
    at = torch.arange(n, dtype=torch.int64, device=longest.device)
    if n == 0:
        return at.to(torch.bool)
    return torch.cummax(at + longest.to(torch.int64), 0).values > at


def head_lines_keep(line_row, line_hits, n_rows: int, head_lines: int = 5):
    """The rule of autogenerated_rows alone, on tensors of any device: line_row [n_lines] int64 (ascending: the row of
    every line), line_hits [n_lines] int64 (the occurrences in every line) -> [n_rows] bool, False for a row with an
    occurrence in one of its first head_lines lines."""
    import torch
    n_lines, n_rows = line_row.shape[0], int(n_rows)
    lines_of = torch.zeros(n_rows, dtype=torch.int64, device=line_row.device).scatter_add_(0, line_row, torch.ones_like(line_row))
    first = torch.cumsum(lines_of, 0) - lines_of
    in_row = torch.arange(n_lines, dtype=torch.int64, device=line_row.device) - first[line_row]
    bad = ((in_row < int(head_lines)) & (line_hits > 0)).to(torch.int64)
    return torch.zeros(n_rows, dtype=torch.int64, device=line_row.device).scatter_add_(0, line_row, bad) == 0


def autogenerated_rows(corpus: "_lib.NativeCorpus", head_lines: int = 5, phrases=AUTOGENERATED):
    """-> torch.int64 indices, ascending, of the rows with none of `phrases` in their first head_lines lines, matched with
    A-Z lowered: what `select` takes to drop the files that say they were generated, as the BigCode (Stack / StarCoder)
    filter does.  The default list is that filter's: "auto-generated", "autogenerated", "automatically generated",
    "generated automatically", "this file is generated".  A composition of line_rows, phrase_hits of the lines and torch,
    no kernel of its own.  Where it differs from the script: a line here ends at '\\n' only (line_rows), where Python's
    splitlines also ends one at '\\r', form feed and the Unicode line separators, and the fold is ASCII, where str.lower
    also lowers other scripts (the keywords are ASCII, so only text such as a Kelvin sign for 'k' could differ)."""
    lines, line_row = line_rows(corpus)
    ps = phrases if isinstance(phrases, _lib.NativePhraseSet) else phrase_set(list(phrases), fold_case=True, device=corpus.device)
    try:
        hits = phrase_hits(lines, ps)
        return head_lines_keep(line_row, hits, corpus.num_samples, head_lines).nonzero().reshape(-1)
    finally:
        lines.free()
        if ps is not phrases:
            ps.free()


GOPHER_TOP = ((2, .20), (3, .18), (4, .16))
GOPHER_DUP = ((5, .15), (6, .14), (7, .13), (8, .12), (9, .11), (10, .10))


class RepeatStats:
    """What repeat_stats returns: `table`, [6, S] torch.int64 on the source's device, and a [S] view of it per statistic
    (grams, repeated, multi, top, covered, covered_all: include/tgx.h); `elems`, [S] torch.int64, the rows' lengths in
    elements (ids or bytes); `width`; `mask`, the [n_elems] uint8 tensor (bit 0: a repeat begins here, bit 1: a member
    of a class of two or more begins here), or None when it was not asked for."""

    def __init__(self, table, elems, width: int, mask=None):
        self.table, self.elems, self.width, self.mask = table, elems, int(width), mask
        for k, name in enumerate(_lib.REPEAT_NAMES):
            setattr(self, name, table[k])

    def _per_elem(self, count):
        import torch
        return count.to(torch.float64) / self.elems.clamp(min=1).to(torch.float64)

    @property
    def repeated_frac(self):
        """[S] float64: repeated / max(grams, 1), the share of the row's n-grams that occurred earlier in the row."""
        import torch
        return self.repeated.to(torch.float64) / self.grams.clamp(min=1).to(torch.float64)

    @property
    def covered_frac(self):
        """[S] float64: covered / max(elems, 1), the share of the row's elements inside a repeated n-gram."""
        return self._per_elem(self.covered)

    @property
    def covered_all_frac(self):
        """[S] float64: covered_all / max(elems, 1), first occurrences of the repeated n-grams included."""
        return self._per_elem(self.covered_all)

    @property
    def top_frac(self):
        """[S] float64: top · width / max(elems, 1) where top >= 2, else 0: the share of the row taken by the
        occurrences of its most frequent n-gram (overlaps counted as often as they occur, as Gopher counts them)."""
        import torch
        frac = self._per_elem(self.top * self.width)
        return torch.where(self.top >= 2, frac, torch.zeros_like(frac))


def _elem_bytes(obj) -> int:
    return 4 if isinstance(obj, _lib.NativeResult) else 1


def _row_elems(obj):
    return row_lengths(obj) if isinstance(obj, _lib.NativeResult) else text_stats(obj, unit="byte").bytes


def repeat_stats(obj, width: int, seed: int = 0, return_mask: bool = False, *, elems=None) -> RepeatStats:
    """-> a RepeatStats of obj's rows (a NativeResult: n-grams of `width` ids; a NativeCorpus: of `width` bytes),
    computed on its device and queued on torch's current stream: per row the n-grams, those that occurred earlier in
    the same row, those that occur twice or more, the occurrences of the most frequent one, and the elements covered
    by repeats.  Equality is by 64-bit key, so probabilistic in the sense of gram_hits.  A row shorter than `width`
    owns no n-gram.  elems: the rows' lengths if the caller has them (else they are computed)."""
    import torch
    dev = _device_of(torch, obj)
    width = _lib.repeat_check_width(width, _elem_bytes(obj))  # (raises before anything is allocated)
    S = obj.num_samples
    n_elems = obj.num_tokens if isinstance(obj, _lib.NativeResult) else obj.num_bytes
    table = torch.empty((_lib.REPEAT_N, S), dtype=torch.int64, device=dev)
    mask = torch.empty((n_elems,), dtype=torch.uint8, device=dev) if return_mask else None
    spare = torch.empty(1, dtype=torch.int64, device=dev)  # (no row: the pointer still says that the table is asked for)
    obj.repeat_stats(width, seed, (table if S else spare).data_ptr(), mask.data_ptr() if return_mask and n_elems else 0,
                     stream=torch.cuda.current_stream(dev).cuda_stream)
    return RepeatStats(table, _row_elems(obj) if elems is None else elems, width, mask)


def repetition_keep(stats, top=GOPHER_TOP, dup=GOPHER_DUP, literal: bool = False):
    """The keep rule of repetition_rows alone, on tensors of any device: stats maps a width to its RepeatStats ->
    [S] bool, False for a row with top_frac > limit for some (w, limit) of `top`, or with covered_frac (literal:
    covered_all_frac) > limit for some (w, limit) of `dup`."""
    keep = None
    for w, limit in top:
        ok = ~(stats[int(w)].top_frac > float(limit))
        keep = ok if keep is None else keep & ok
    for w, limit in dup:
        s = stats[int(w)]
        ok = ~((s.covered_all_frac if literal else s.covered_frac) > float(limit))
        keep = ok if keep is None else keep & ok
    return keep


def repetition_rows(obj, top=GOPHER_TOP, dup=GOPHER_DUP, literal: bool = False, seed: int = 0):
    """-> torch.int64 indices, ascending, of the rows that pass the n-gram repetition rules of Gopher / MassiveText: what
    `select` takes to drop the others (of a result and, with the same indices, of its corpus).  A row is dropped iff
    top_frac > limit for some (w, limit) of `top` (the share taken by its most frequent w-gram), or covered_frac > limit
    for some (w, limit) of `dup` (the share covered by repeated w-grams; with literal=True covered_all_frac, which
    counts the first occurrences too, the paper's literal reading, where the default is what a pipeline that deletes
    the repeats would delete).  One repeat_stats call per distinct width.  The defaults are Gopher's numbers; Gopher
    counts word n-grams and characters where this counts elements of the source (token ids or bytes), so the
    thresholds are the caller's to tune.  A width that the source's element size cannot take raises before anything is
    queued."""
    import torch
    top, dup = tuple(top), tuple(dup)
    widths = sorted({int(w) for w, _ in top + dup})
    for w in widths:
        _lib.repeat_check_width(w, _elem_bytes(obj))
    if not widths:
        return torch.arange(obj.num_samples, dtype=torch.int64, device=_device_of(torch, obj))
    elems = _row_elems(obj)
    stats = {w: repeat_stats(obj, w, seed, elems=elems) for w in widths}
    return repetition_keep(stats, top, dup, literal).nonzero().reshape(-1)


def line_dup_counts(line_row, cls, line_bytes, n_rows: int):
    """The duplicate-line rule alone, on tensors of any device: line_row [n_lines] int64 (ascending: the row of every
    line), cls [n_lines] int64 (first_equal of the lines), line_bytes [n_lines] int64 -> (dup_lines, dup_bytes), both
    [n_rows] int64.  A line is a duplicate iff it is not the first of its row with its content: the lines are sorted
    stably by line_row · n_lines + cls, and a duplicate is one whose predecessor has the same key."""
    import torch
    n_lines = line_row.shape[0]
    key = line_row * n_lines + cls
    skey, order = torch.sort(key, stable=True)
    is_dup = torch.zeros(n_lines, dtype=torch.int64, device=key.device)
    if n_lines > 1:
        is_dup[order[1:]] = (skey[1:] == skey[:-1]).to(torch.int64)
    dup_lines = torch.zeros(int(n_rows), dtype=torch.int64, device=key.device).scatter_add_(0, line_row, is_dup)
    dup_bytes = torch.zeros(int(n_rows), dtype=torch.int64, device=key.device).scatter_add_(0, line_row, is_dup * line_bytes)
    return dup_lines, dup_bytes


def line_dup_keep(dup_lines, dup_bytes, n_lines, n_bytes, max_dup_lines: float, max_dup_bytes: float):
    """[S] bool: dup_lines <= max_dup_lines · lines and dup_bytes <= max_dup_bytes · bytes, division-free in float64."""
    import torch
    f64 = torch.float64
    return (dup_lines.to(f64) <= float(max_dup_lines) * n_lines.to(f64)) & (dup_bytes.to(f64) <= float(max_dup_bytes) * n_bytes.to(f64))


def line_repetition_rows(corpus: "_lib.NativeCorpus", max_dup_lines: float = 0.30, max_dup_bytes: float = 0.20, return_stats: bool = False):
    """-> torch.int64 indices, ascending, of the rows that pass the duplicate-line rules of Gopher / MassiveText: what
    `select` takes to drop the others.  A line (line_rows: '\\n' ends it and belongs to it, no line crosses a row's end)
    is a duplicate iff an earlier line of the same row has exactly its bytes; a row is kept iff its duplicate lines are
    at most max_dup_lines of its lines and their bytes at most max_dup_bytes of its bytes.  The comparisons are
    division-free, so an empty row is kept.  A composition of line_rows, first_equal and torch, no kernel of its own.
    The defaults are Gopher's numbers, where the byte share is a character share.  With return_stats also (dup_lines,
    dup_bytes, lines, bytes), each [S] torch.int64."""
    import torch
    S = corpus.num_samples
    lines, line_row = line_rows(corpus)
    cls = first_equal(lines)
    line_bytes = text_stats(lines, unit="byte").bytes
    dup_lines, dup_bytes = line_dup_counts(line_row, cls, line_bytes, S)
    s = text_stats(corpus, unit="byte")
    rows = line_dup_keep(dup_lines, dup_bytes, s.lines, s.bytes, max_dup_lines, max_dup_bytes).nonzero().reshape(-1)
    return (rows, (dup_lines, dup_bytes, s.lines, s.bytes)) if return_stats else rows


def _window_len(max_length, stride) -> tuple[int, int]:
    if max_length is None:
        raise TypeError("max_length is required for overflow windows")
    L, s = int(max_length), int(stride)
    if L < 1:
        raise _lib.TokenGeeXError("max_length must be at least 1", _lib.ERR_INVALID)
    if s < 0:
        raise _lib.TokenGeeXError("stride must not be negative", _lib.ERR_INVALID)
    return L, s


def window_into(result: "_lib.NativeResult", input_ids, attention_mask=None, lengths=None, window_row=None, window_first=None, *,
                row_len: int, stride: int = 0, pad_id: int, n_windows: int | None = None, bos_id: int | None = None,
                eos_id: int | None = None, padding_side: str = "right", truncation_side: str = "right") -> int:
    """The overflow windows written into tensors the caller owns (input_ids: int32 or int64, at least W·row_len elements;
    attention_mask: uint8, the same count; lengths, window_row, window_first: int32, W), checked as in pad_into.
    n_windows: the W the tensors are sized for (None: result.window_info is asked).  -> W."""
    import torch
    dev = _device_of(torch, result)
    L, s = _window_len(row_len, stride)
    if not isinstance(input_ids, torch.Tensor):
        raise TypeError("input_ids must be a torch.Tensor")
    flags = _lib.layout_flags(padding_side, truncation_side, _np_dtype(torch, input_ids.dtype))
    W = result.window_info(L, s, bos_id=bos_id, eos_id=eos_id, flags=flags) if n_windows is None else int(n_windows)
    p_ids = _check_dest(torch, "input_ids", input_ids, dev, input_ids.dtype, W * L)
    p_mask = 0 if attention_mask is None else _check_dest(torch, "attention_mask", attention_mask, dev, torch.uint8, W * L)
    p_len, p_row, p_first = (0 if t is None else _check_dest(torch, name, t, dev, torch.int32, W)
                             for name, t in (("lengths", lengths), ("window_row", window_row), ("window_first", window_first)))
    stream = torch.cuda.current_stream(dev).cuda_stream
    result.window_pad_device(L, s, pad_id, W, p_ids, mask_ptr=p_mask, lengths_ptr=p_len, window_row_ptr=p_row, window_first_ptr=p_first,
                             bos_id=bos_id, eos_id=eos_id, flags=flags, stream=stream)
    return W


def to_windows(result: "_lib.NativeResult", *, max_length: int, stride: int = 0, pad_id: int, bos_id: int | None = None,
               eos_id: int | None = None, padding_side: str = "right", truncation_side: str = "right", dtype=None,
               return_lengths: bool = False) -> dict:
    """Every token of every row, long rows as overlapping windows -> {"input_ids": [W, L] of dtype (torch.int64 by
    default, or torch.int32), "attention_mask": [W, L] torch.uint8, "overflow_to_sample_mapping": [W] torch.int32, the
    row a window came from, "window_first": [W] torch.int32, the index of its first token in that row [, "lengths": [W]
    torch.int32]} on the result's device.

    L = max_length.  A window is [bos] + up to L - A tokens + [eos]; the next one starts stride tokens before this one
    ends (truncation_side "left": the windows run from the row's end), so stride < L - A.  A row that fits is one
    window, as to_padded gives it; window 0 of any row is its to_padded row."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    flags = _lib.layout_flags(padding_side, truncation_side, _np_dtype(torch, dtype))
    dev = _device_of(torch, result)
    L, s = _window_len(max_length, stride)
    W = result.window_info(L, s, bos_id=bos_id, eos_id=eos_id, flags=flags)
    out = {"input_ids": torch.empty((W, L), dtype=dtype, device=dev),
           "attention_mask": torch.empty((W, L), dtype=torch.uint8, device=dev),
           "overflow_to_sample_mapping": torch.empty((W,), dtype=torch.int32, device=dev),
           "window_first": torch.empty((W,), dtype=torch.int32, device=dev)}
    if return_lengths:
        out["lengths"] = torch.empty((W,), dtype=torch.int32, device=dev)
    window_into(result, out["input_ids"], out["attention_mask"], out.get("lengths"), out["overflow_to_sample_mapping"], out["window_first"],
                row_len=L, stride=s, pad_id=pad_id, n_windows=W, bos_id=bos_id, eos_id=eos_id, padding_side=padding_side,
                truncation_side=truncation_side)
    return out


def decode_padded(model: "_lib.NativeModel", input_ids, *, attention_mask=None, lengths=None, skip_id: int | None = None,
                  special_flat=(), special_offs=(0,), include_special: bool = True) -> "_lib.NativeText":
    """A [S, L] tensor of ids (int32 or int64, contiguous, on the model's device) decoded to UTF-8 text in HBM with the
    kernels of csrc/decode.hip -> NativeText.  attention_mask (uint8 or bool, the same shape), lengths (int32 [S]) and
    skip_id say which elements are there at all (NativeModel.decode_padded).  Everything is checked before anything is
    launched; the kernels are queued on torch.cuda.current_stream(device) and the call returns once that stream has
    reached its end."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.TokenGeeXError("torch sees no GPU although libtgx.so does: two HIP runtimes in one process "
                                  "(TGX_HIP_RUNTIME=system set? then import torch before tokengeex_amd)", _lib.ERR_DEVICE)
    dev = torch.device("cuda", model.device)
    if not isinstance(input_ids, torch.Tensor):
        raise TypeError("input_ids must be a torch.Tensor")
    if input_ids.dim() != 2:
        raise ValueError(f"input_ids must have two dimensions (got {input_ids.dim()})")
    _np_dtype(torch, input_ids.dtype)
    S, L = input_ids.shape
    p_ids = _check_dest(torch, "input_ids", input_ids, dev, input_ids.dtype, S * L)
    p_mask = 0
    if attention_mask is not None:
        if not isinstance(attention_mask, torch.Tensor):
            raise TypeError("attention_mask must be a torch.Tensor")
        if attention_mask.shape != input_ids.shape:
            raise ValueError(f"attention_mask has shape {tuple(attention_mask.shape)}, input_ids {tuple(input_ids.shape)}")
        mask_dtype = torch.bool if attention_mask.dtype == torch.bool else torch.uint8  # a bool is one byte, 0 or 1
        p_mask = _check_dest(torch, "attention_mask", attention_mask, dev, mask_dtype, S * L)
    p_len = 0
    if lengths is not None:
        if isinstance(lengths, torch.Tensor) and lengths.shape != (S,):
            raise ValueError(f"lengths has shape {tuple(lengths.shape)}, expected ({S},)")
        p_len = _check_dest(torch, "lengths", lengths, dev, torch.int32, S)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return model.decode_padded(p_ids, S, L, input_ids.dtype == torch.int64, mask_ptr=p_mask, lengths_ptr=p_len, skip_id=skip_id,
                               special_flat=special_flat, special_offs=special_offs, include_special=include_special, stream=stream)


# ---- token spans: which part of its row's text a token covers (csrc/spans.hip) -----------------------------------------

def _special_arrays(specials):
    """None, a list of special tokens (bytes or str), or their packed form (uint8 flat, uint64 offsets) -> the packed form."""
    import numpy as np
    if specials is None:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    if isinstance(specials, tuple) and len(specials) == 2 and all(isinstance(a, np.ndarray) for a in specials):
        return specials
    return _lib.pack([t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in specials])


def _span_dest(torch, result, model, spans, numel: int):
    if result.device != model.device:
        raise ValueError(f"the result is on device {result.device}, the model on device {model.device}")
    dev = _device_of(torch, result)
    if not isinstance(spans, torch.Tensor):
        raise TypeError("spans must be a torch.Tensor")
    _np_dtype(torch, spans.dtype)
    return dev, _check_dest(torch, "spans", spans, dev, spans.dtype, numel)


def spans_into(result: "_lib.NativeResult", model: "_lib.NativeModel", spans, specials=None, *, unit: str = "byte") -> None:
    """The span of every token in its row's text written into a tensor the caller owns (int32 or int64, contiguous, on the
    result's device, at least num_tokens·2 elements; checked before anything is launched): element (j, 0) is the start
    and (j, 1) the end of token j, in bytes or (unit "char") code points, relative to the token's own row."""
    import torch
    dev, p = _span_dest(torch, result, model, spans, result.num_tokens * 2 if result.num_samples else 0)
    sf, so = _special_arrays(specials)
    flags = _lib.span_flags(unit, _np_dtype(torch, spans.dtype))
    model.result_spans(result, sf, so, p, flags=flags, stream=torch.cuda.current_stream(dev).cuda_stream)


def pad_spans_into(result: "_lib.NativeResult", model: "_lib.NativeModel", spans, specials=None, *, row_len: int, unit: str = "byte",
                   bos_id: int | None = None, eos_id: int | None = None, padding_side: str = "right",
                   truncation_side: str = "right") -> None:
    """spans_into in the padded form: at least S·row_len·2 elements, aligned element for element with pad_into's input_ids
    for the same row_len, bos_id, eos_id and sides; bos, eos and padding get (0, 0)."""
    import torch
    L = int(row_len)
    if L < 1:
        raise _lib.TokenGeeXError("row_len must be at least 1", _lib.ERR_INVALID)
    dev, p = _span_dest(torch, result, model, spans, result.num_samples * L * 2)
    sf, so = _special_arrays(specials)
    flags = _lib.span_flags(unit, _np_dtype(torch, spans.dtype), padding_side, truncation_side)
    model.result_pad_spans(result, sf, so, L, p, bos_id=bos_id, eos_id=eos_id, flags=flags,
                           stream=torch.cuda.current_stream(dev).cuda_stream)


def to_spans(result: "_lib.NativeResult", model: "_lib.NativeModel", specials=None, unit: str = "byte", dtype=None):
    """-> [T, 2] of dtype (torch.int64 by default, or torch.int32) on the result's device: the (start, end) of every token
    in its row's text.  `specials`: the special tokens behind the ids >= model.vocab_size (a list of bytes or str, or
    their packed form), None when the result has none.  torch.int32 raises TokenGeeXError (ERR_UNSUPPORTED) when a row
    has 2^31 units or more."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    _np_dtype(torch, dtype)
    out = torch.empty((result.num_tokens if result.num_samples else 0, 2), dtype=dtype, device=_device_of(torch, result))
    spans_into(result, model, out, specials, unit=unit)
    return out


def to_padded_spans(result: "_lib.NativeResult", model: "_lib.NativeModel", specials=None, unit: str = "byte", dtype=None, *,
                    max_length: int | None = None, bos_id: int | None = None, eos_id: int | None = None,
                    padding_side: str = "right", truncation_side: str = "right"):
    """-> [S, L, 2] of dtype: to_spans laid out as to_padded lays the ids out for the same max_length, bos_id, eos_id and
    sides (max_length=None: the longest row with its bos / eos, at least 1)."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    _np_dtype(torch, dtype)
    if max_length is None:
        L = max(1, result.layout_info(bos_id, eos_id)[0])
    else:
        L = int(max_length)
        if L < 1:
            raise _lib.TokenGeeXError("max_length must be at least 1", _lib.ERR_INVALID)
    out = torch.empty((result.num_samples, L, 2), dtype=dtype, device=_device_of(torch, result))
    pad_spans_into(result, model, out, specials, row_len=L, unit=unit, bos_id=bos_id, eos_id=eos_id, padding_side=padding_side,
                   truncation_side=truncation_side)
    return out


def window_spans_into(result: "_lib.NativeResult", model: "_lib.NativeModel", spans, specials=None, *, row_len: int, stride: int = 0,
                      n_windows: int | None = None, unit: str = "byte", bos_id: int | None = None, eos_id: int | None = None,
                      padding_side: str = "right", truncation_side: str = "right") -> int:
    """spans_into for the overflow windows: at least W·row_len·2 elements, aligned element for element with window_into's
    input_ids for the same row_len, stride, bos_id, eos_id and sides.  A kept token gets its span in its whole row's text,
    whichever window it stands in; bos, eos and padding get (0, 0).  -> W."""
    import torch
    L, s = _window_len(row_len, stride)
    if not isinstance(spans, torch.Tensor):
        raise TypeError("spans must be a torch.Tensor")
    flags = _lib.span_flags(unit, _np_dtype(torch, spans.dtype), padding_side, truncation_side)
    W = result.window_info(L, s, bos_id=bos_id, eos_id=eos_id, flags=flags) if n_windows is None else int(n_windows)
    dev, p = _span_dest(torch, result, model, spans, W * L * 2)
    sf, so = _special_arrays(specials)
    result.window_spans_device(model, sf, so, L, s, W, p, bos_id=bos_id, eos_id=eos_id, flags=flags,
                               stream=torch.cuda.current_stream(dev).cuda_stream)
    return W


def to_window_spans(result: "_lib.NativeResult", model: "_lib.NativeModel", specials=None, unit: str = "byte", dtype=None, *,
                    max_length: int, stride: int = 0, bos_id: int | None = None, eos_id: int | None = None,
                    padding_side: str = "right", truncation_side: str = "right"):
    """-> [W, L, 2] of dtype: to_spans laid out as to_windows lays the ids out for the same max_length, stride, bos_id,
    eos_id and sides.  The pairs index the sample's text, so a window's tokens name the substring they came from."""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    flags = _lib.span_flags(unit, _np_dtype(torch, dtype), padding_side, truncation_side)
    L, s = _window_len(max_length, stride)
    W = result.window_info(L, s, bos_id=bos_id, eos_id=eos_id, flags=flags)
    out = torch.empty((W, L, 2), dtype=dtype, device=_device_of(torch, result))
    window_spans_into(result, model, out, specials, row_len=L, stride=s, n_windows=W, unit=unit, bos_id=bos_id, eos_id=eos_id,
                      padding_side=padding_side, truncation_side=truncation_side)
    return out
