"""Host-side mirror of the reference's `Tokenizer` (src/tokenizer.rs:6-435) and of
its PyO3 surface (bindings/python/src/lib.rs:41-223, tokengeex.pyi:10-255).

Same method names, argument order and error strings as the PyO3 class; the hot
path (Model::encode over a batch) goes through the C ABI to the HIP kernels, the
rest (special-token splitting, processors, decode, JSON) is host glue in Python.
"""
from __future__ import annotations

import base64
import json
import random
import re
import unicodedata

import numpy as np

from . import _lib
from . import _tgxfast as _fast  # csrc/pyfast.c, built by tokengeex_amd/build.py beside libtgx.so
from ._lib import TokenGeeXError

SERIALIZATION_VERSION = "2.0"  # src/tokenizer.rs:347


# ---- processors: src/processor.rs ---------------------------------------------

class CrlfProcessor:
    """src/processor.rs:37-54: plain "\\r\\n" -> "\\n"; postprocess is identity."""

    def preprocess(self, s: str) -> str:
        return s.replace("\r\n", "\n")

    def postprocess(self, s: str) -> str:
        return s

    def to_json(self):
        return {"type": "crlf"}


class UnicodeProcessor:
    """src/processor.rs:124-137.  The reference delegates to the
    unicode-normalization crate; here unicodedata does the same UAX #15 forms
    (parity with the crate's Unicode version is not pinned by any reference test)."""

    FORMS = {"nfc": "NFC", "nfd": "NFD", "nfkc": "NFKC", "nfkd": "NFKD"}

    def __init__(self, form: str):
        if form not in self.FORMS:
            raise TokenGeeXError(f"unknown variant `{form}`, expected one of `nfc`, `nfd`, `nfkc`, `nfkd`",
                                 _lib.ERR_JSON)
        self.form = form

    def preprocess(self, s: str) -> str:
        return unicodedata.normalize(self.FORMS[self.form], s)

    def postprocess(self, s: str) -> str:
        return s

    def to_json(self):
        return {"type": "unicode", "form": self.form}


def _processor_from_json(obj):
    # untagged enum, src/processor.rs:13-18: Crlf is tried first, then Unicode
    if not isinstance(obj, dict):
        raise TokenGeeXError("data did not match any variant of untagged enum ProcessorWrapper", _lib.ERR_JSON)
    if obj.get("type") == "crlf" and "form" not in obj:
        return CrlfProcessor()
    if "form" in obj:
        return UnicodeProcessor(obj["form"])
    raise TokenGeeXError("data did not match any variant of untagged enum ProcessorWrapper", _lib.ERR_JSON)


# ---- special token splitter: src/tokenizer.rs:299-347 ------------------------------

def split_special_tokens(text: str, special_tokens: list[str]) -> list[tuple[str, bool]]:
    """Earliest char position wins; at one position the first special in list order
    wins (not the longest).  A regex alternation has exactly these semantics."""
    if not text:
        return []
    if not special_tokens:
        return [(text, False)]
    pat = re.compile("|".join(re.escape(t) for t in special_tokens))
    out, cursor = [], 0
    for mt in pat.finditer(text):
        if mt.start() > cursor:
            out.append((text[cursor:mt.start()], False))
        out.append((mt.group(0), True))
        cursor = mt.end()
    if cursor < len(text):
        out.append((text[cursor:], False))
    return out


def _split_rows(ids: np.ndarray, offs: np.ndarray) -> list[list[int]]:
    flat = ids.tolist()  # one conversion for the batch, then list slices
    o = offs.tolist()
    return [flat[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def combine_nbest(seg_offs: np.ndarray, seg_special: np.ndarray, base_vocab: int, ids: np.ndarray, id_offs: np.ndarray,
                  scores: np.ndarray, n_found: np.ndarray, nbest: int):
    """Per-segment n-best lists -> per-sample lists (Tokenizer.encode_batch_nbest_flat).  `ids` / `id_offs` / `scores` /
    `n_found` are the device's output over the non-special segments (nbest rows each).  A sample's list is the k-best
    product of its segments' lists, taken left to right: the candidates (C[i].score + Lseg[j].score, i, j), ordered by
    score descending, then i, then j; the top nbest are kept.  Special tokens add nothing to the score; a sample without
    non-special segments has one row of score 0.0.  Samples made of one non-special segment are mapped directly.
    -> (ids u32, offsets u64[S·nbest+1], scores f64[S·nbest], n_found u32[S])."""
    k = int(nbest)
    seg_offs = seg_offs.astype(np.int64)
    n = seg_offs.shape[0] - 1
    ss = np.asarray(seg_special, np.int64)
    id_offs = id_offs.astype(np.int64)
    nseg = np.diff(seg_offs)
    text_idx = np.cumsum(ss < 0) - 1  # segment -> its index among the non-special segments
    first = np.minimum(seg_offs[:-1], max(ss.size - 1, 0))
    simple = (nseg == 1) & (ss[first] < 0) if ss.size else np.zeros(n, bool)
    out_scores = np.full(n * k, -np.inf)
    out_nf = np.zeros(n, np.uint32)
    sp_base = int(ids.shape[0])  # special token t sits at sp_base + t of the pool
    n_sp = int(ss.max()) + 1 if ss.size and ss.max() >= 0 else 0
    pool = np.concatenate([ids.astype(np.uint32), (base_vocab + np.arange(n_sp)).astype(np.uint32)])
    # one non-special segment: its rows are the sample's
    s1 = np.nonzero(simple)[0]
    j1 = text_idx[seg_offs[s1]]
    rows = (s1[:, None] * k + np.arange(k)[None, :]).ravel()
    src = (j1[:, None] * k + np.arange(k)[None, :]).ravel()
    out_scores[rows] = scores[src]
    out_nf[s1] = n_found[j1]
    p_row, p_start, p_len = [rows], [id_offs[src]], [id_offs[src + 1] - id_offs[src]]
    # no segment (an empty sample): one empty row
    s0 = np.nonzero(nseg == 0)[0]
    out_scores[s0 * k] = 0.0
    out_nf[s0] = 1
    # the rest (specials, several segments): the product, sample by sample
    rr, rs, rl = [], [], []
    for s in np.nonzero(~simple & (nseg > 0))[0].tolist():
        cur = [(0.0, [])]
        for g in range(int(seg_offs[s]), int(seg_offs[s + 1])):
            if ss[g] >= 0:
                cur = [(sc, pcs + [(sp_base + int(ss[g]), 1)]) for sc, pcs in cur]
                continue
            j = int(text_idx[g])
            cands = [(cur[i][0] + float(scores[j * k + jj]), i, jj) for i in range(len(cur)) for jj in range(int(n_found[j]))]
            cands.sort(key=lambda t: (-t[0], t[1], t[2]))
            cur = [(sc, cur[i][1] + [(int(id_offs[j * k + jj]), int(id_offs[j * k + jj + 1] - id_offs[j * k + jj]))])
                   for sc, i, jj in cands[:k]]
        out_nf[s] = len(cur)
        for r, (sc, pcs) in enumerate(cur):
            out_scores[s * k + r] = sc
            for st, ln in pcs:
                rr.append(s * k + r)
                rs.append(st)
                rl.append(ln)
    p_row.append(np.asarray(rr, np.int64))
    p_start.append(np.asarray(rs, np.int64))
    p_len.append(np.asarray(rl, np.int64))
    p_row, p_start, p_len = np.concatenate(p_row), np.concatenate(p_start), np.concatenate(p_len)
    o = np.argsort(p_row, kind="stable")
    p_row, p_start, p_len = p_row[o], p_start[o], p_len[o]
    out_offs = np.zeros(n * k + 1, np.uint64)
    out_offs[1:] = np.cumsum(np.bincount(p_row, weights=p_len, minlength=n * k).astype(np.int64))
    total = int(out_offs[-1])
    at = np.cumsum(p_len) - p_len
    idx = np.repeat(p_start - at, p_len) + np.arange(total)
    return pool[idx], out_offs, out_scores, out_nf


def nbest_draw(scores: np.ndarray, n_found: np.ndarray, alpha: float, seed: int) -> np.ndarray:
    """The row each sample draws from its n-best list (scores f64[S, k]): the largest alpha · score_r − log(−log u_r),
    u_r = tgx_sample_u01(seed, i, r, 0), over r < n_found[i]; ties to the lower r."""
    S, k = scores.shape
    i = np.repeat(np.arange(S, dtype=np.uint64), k)
    r = np.tile(np.arange(k, dtype=np.uint64), S)
    u = _lib.sample_u01_array(seed, i, r, np.zeros(S * k, np.uint64)).reshape(S, k)
    valid = np.arange(k)[None, :] < np.asarray(n_found, np.int64)[:, None]
    key = np.where(valid, float(alpha) * np.where(valid, scores, 0.0) - np.log(-np.log(u)), -np.inf)
    return np.argmax(key, axis=1) if S else np.zeros(0, np.int64)


# ---- Tokenizer ---------------------------------------------------------------------

class Tokenizer:
    """tokengeex.Tokenizer (bindings/python/src/lib.rs:11-224)."""

    def __init__(self, vocab: list[tuple[bytes, float, bool]] | None = None, processors=None,
                 special_tokens=None, device: int = 0):
        # Model: src/model.rs:8-12
        self._vocab: list[tuple[bytes, float, bool]] = [(bytes(v), float(s), bool(k)) for v, s, k in (vocab or [])]
        self._token_to_ids: dict[bytes, int] = {}
        for i, (v, _, _) in enumerate(self._vocab):
            self._token_to_ids[v] = i  # later duplicates overwrite, src/model.rs:21
        self._processors = list(processors or [])
        self._special_tokens: list[str] = []
        self._special_tokens_map: dict[str, int] = {}
        self._device = device
        self._native: _lib.NativeModel | None = None
        self.seed: int | None = None  # dropout seed; None = fresh random seed per call
        # the encode_corpus_* methods normalise on the device (csrc/norm.hip) when asked: [UnicodeProcessor] and
        # [CrlfProcessor, UnicodeProcessor] are then taken instead of refused (_corpus_front)
        self.device_unicode = False
        self.add_special_tokens(list(special_tokens or []))

    # -- native model (lazy: building it needs the GPU) --
    def _model(self) -> _lib.NativeModel:
        if self._native is None:
            self._native = _lib.NativeModel([v for v, _, _ in self._vocab],
                                            np.array([s for _, s, _ in self._vocab], dtype=np.float64),
                                            self._device)
        return self._native

    def _seed(self, dropout: float) -> int:
        if dropout <= 0.0:
            return 0
        return self.seed if self.seed is not None else random.getrandbits(64)

    def _preprocess(self, s: str) -> str:
        for p in self._processors:  # src/tokenizer.rs:79-82
            s = p.preprocess(s)
        return s

    # -- encode: src/tokenizer.rs:65-123 --
    def encode(self, text: str, dropout: float) -> list[int]:
        return self.encode_batch([text], dropout)[0]

    def encode_ordinary(self, text: str, dropout: float) -> list[int]:
        return self.encode_ordinary_batch([text], dropout)[0]

    def _native_front(self) -> bool:
        """The packed-buffer front end covers both processors of the reference (src/processor.rs): CRLF (csrc/frontback.cpp)
        and, from round 4, the Unicode normalisation forms (csrc/unicode_norm.cpp; `unicodedata` stays as the checker of the
        tests and in UnicodeProcessor.preprocess for single strings)."""
        return all(isinstance(p, (CrlfProcessor, UnicodeProcessor)) for p in self._processors)

    def _preprocess_flat(self, flat: np.ndarray, offs: np.ndarray):
        """The processors, in order (src/tokenizer.rs:79-82), over a packed batch of segments."""
        for p in self._processors:
            if isinstance(p, CrlfProcessor):
                flat, offs = _lib.pack_segments(flat, np.ascontiguousarray(offs[:-1]), np.ascontiguousarray(offs[1:]), None, True)
            else:
                flat, offs = _lib.normalize_flat(p.form, flat, offs)
        return flat, offs

    def _rows_native(self, texts: list[str], dropout: float, ordinary: bool) -> list[list[int]]:
        """list[str] -> list[list[int]] with both ends in native code (csrc/pyfast.c; bindings/python/src/lib.rs:51-69 builds
        the same shapes in Rust): the samples' UTF-8 packed by host threads straight from the strings, the rows built from
        shared int objects (one per id, made once per tokenizer) — no bytes object per sample, no int object per token."""
        text_b, offs_b = _fast.pack_strs(texts)
        flat = np.frombuffer(text_b, dtype=np.uint8)
        offs = np.frombuffer(offs_b, dtype=np.uint64)
        ids, o = self.encode_batch_flat(flat, offs, dropout, ordinary=ordinary)
        n_ids = self.vocab_size()
        if getattr(self, "_int_cache", None) is None or len(self._int_cache) != n_ids:
            self._int_cache = list(range(n_ids))
        return _fast.rows_from_flat(np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(o, np.uint64), self._int_cache)

    def encode_ordinary_batch(self, texts: list[str], dropout: float) -> list[list[int]]:
        if self._native_front():
            return self._rows_native(texts, dropout, True)
        segs = [self._preprocess(t).encode("utf-8") for t in texts]
        ids, offs = self._encode_segments(segs, dropout)
        return [ids[int(offs[i]):int(offs[i + 1])].tolist() for i in range(len(texts))]

    def encode_batch_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0, ordinary: bool = False):
        """encode_batch / encode_ordinary_batch over a packed batch of UTF-8 samples (uint8 flat, uint64
        offsets[S+1]) -> (ids uint32[T], offsets uint64[S+1]): special-token split, CRLF processor, encode and
        the assembly of the ids all run on packed buffers in native code (src/tokenizer.rs:65-123)."""
        if not self._native_front():
            raise TokenGeeXError("encode_batch_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        only_crlf = all(isinstance(p, CrlfProcessor) for p in self._processors)  # then the packing pass does it on the way
        crlf = only_crlf and len(self._processors) > 0
        n = offs.shape[0] - 1
        if ordinary or not self._special_tokens:
            if n and self._processors:
                flat, offs = self._preprocess_flat(flat, offs)
            return self.encode_ordinary_batch_flat(flat, offs, dropout) if n else (np.zeros(0, np.uint32), np.zeros(1, np.uint64))
        seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, [t.encode("utf-8") for t in self._special_tokens])
        pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
        if not only_crlf and poffs.shape[0] > 1:
            pflat, poffs = self._preprocess_flat(pflat, poffs)
        if poffs.shape[0] > 1:
            ids, id_offs = self.encode_ordinary_batch_flat(pflat, poffs, dropout)
        else:
            ids, id_offs = np.zeros(0, np.uint32), np.zeros(1, np.uint64)
        return _lib.assemble_ids(seg_offs, ss, ids, id_offs, self.base_vocab_size())

    def encode_batch(self, texts: list[str], dropout: float) -> list[list[int]]:
        if not self._special_tokens:
            return self.encode_ordinary_batch(texts, dropout)
        if self._native_front():
            return self._rows_native(texts, dropout, False)
        base = self.base_vocab_size()
        plan, segs = [], []  # per text: list of (special id | -1)
        for t in texts:
            row = []
            for sub, is_special in split_special_tokens(t, self._special_tokens):
                if is_special:
                    row.append(base + self._special_tokens_map[sub])  # src/tokenizer.rs:70-77
                else:
                    row.append(-1)
                    segs.append(self._preprocess(sub).encode("utf-8"))
            plan.append(row)
        ids, offs = self._encode_segments(segs, dropout)
        out, k = [], 0
        for row in plan:
            cur: list[int] = []
            for item in row:
                if item >= 0:
                    cur.append(item)
                else:
                    cur.extend(ids[int(offs[k]):int(offs[k + 1])].tolist())
                    k += 1
            out.append(cur)
        return out

    def _encode_segments(self, segs: list[bytes], dropout: float):
        if not segs:
            return np.zeros(0, np.uint32), np.zeros(1, np.uint64)
        flat, offs = _lib.pack(segs)
        return self.encode_ordinary_batch_flat(flat, offs, dropout)

    def encode_ordinary_batch_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0):
        """Flat-buffer entry point the reference lacks: packed bytes + offsets in,
        (ids uint32[T], offsets uint64[S+1]) out, no per-sample Python objects."""
        res = self._model().encode_batch_flat(flat, offs, dropout, self._seed(dropout))
        try:
            return res.ids(), res.offsets()
        finally:
            res.free()

    # -- encoded ids as device tensors for a model (tokengeex_amd/tensors.py over csrc/layout.hip) --
    def _layout_ids(self, layout: dict) -> dict:
        """pad / bos / eos of a layout request, given as ids or as special-token strings -> pad_id / bos_id / eos_id."""
        out = dict(layout)
        for short in ("pad", "bos", "eos"):
            if short in out:
                if short + "_id" in out:
                    raise TypeError(f"both {short} and {short}_id given")
                out[short + "_id"] = out.pop(short)
            v = out.get(short + "_id")
            if isinstance(v, str):
                k = self.special_token_to_id(v)
                if k is None:
                    raise TokenGeeXError(f"{v!r} is not a special token of this tokenizer", _lib.ERR_INVALID)
                out[short + "_id"] = k
        if out.get("pad_id") is None:
            raise TypeError("pad (or pad_id) is required")
        return out

    @staticmethod
    def _mapping_unit(layout: dict):
        """Takes return_offsets_mapping out of a layout request -> None, "byte" or "char"."""
        unit = layout.pop("return_offsets_mapping", None)
        if unit not in (None, "byte", "char"):
            raise ValueError(f"return_offsets_mapping must be None, 'byte' or 'char' (got {unit!r})")
        return unit

    def _with_offset_mapping(self, res, out: dict, layout: dict, unit) -> dict:
        """Adds "offset_mapping" to a padded layout of `res` (None: a batch without samples) when a unit is asked for."""
        if unit is None:
            return out
        import torch
        from . import tensors
        ids = out["input_ids"]
        if res is None:
            out["offset_mapping"] = torch.empty((0, ids.shape[1], 2), dtype=ids.dtype, device=ids.device)
            return out
        _, _, sf, so = self._vocab_packed()
        out["offset_mapping"] = tensors.to_padded_spans(
            res, self._model(), (sf, so), unit, ids.dtype, max_length=ids.shape[1], bos_id=layout.get("bos_id"), eos_id=layout.get("eos_id"),
            padding_side=layout.get("padding_side", "right"), truncation_side=layout.get("truncation_side", "right"))
        return out

    @staticmethod
    def _window_stride(layout: dict):
        """Takes stride and return_overflowing_tokens out of a layout request -> None, or the stride of the overflow windows."""
        overflow = layout.pop("return_overflowing_tokens", False)
        stride = layout.pop("stride", None)
        if not overflow:
            if stride:
                raise ValueError("stride needs return_overflowing_tokens=True")
            return None
        if layout.get("max_length") is None:
            raise TypeError("return_overflowing_tokens needs max_length")
        return int(stride or 0)

    def _windows(self, res, layout: dict, unit, stride: int) -> dict:
        """The overflow-window form of a padded layout of `res` (None: a batch without samples): tensors.to_windows, and
        tensors.to_window_spans when a unit is asked for."""
        import torch
        from . import tensors
        if res is None:
            out = self._empty_layout(True, None, layout)
            ids = out["input_ids"]
            for key in ("overflow_to_sample_mapping", "window_first"):
                out[key] = torch.empty((0,), dtype=torch.int32, device=ids.device)
            if unit is not None:
                out["offset_mapping"] = torch.empty((0, ids.shape[1], 2), dtype=ids.dtype, device=ids.device)
            return out
        out = tensors.to_windows(res, stride=stride, **layout)
        if unit is not None:
            _, _, sf, so = self._vocab_packed()
            out["offset_mapping"] = tensors.to_window_spans(
                res, self._model(), (sf, so), unit, out["input_ids"].dtype, max_length=layout["max_length"], stride=stride,
                bos_id=layout.get("bos_id"), eos_id=layout.get("eos_id"), padding_side=layout.get("padding_side", "right"),
                truncation_side=layout.get("truncation_side", "right"))
        return out

    # -- fill-in-the-middle on the device (csrc/fim.hip) --
    def _fim_request(self, layout: dict):
        """Takes fim out of a layout request -> None, or the arguments of NativeResult.fim: the sentinels given as ids or
        special-token strings, resolved as _layout_ids resolves pad."""
        fim = layout.pop("fim", None)
        if fim is None:
            return None
        if layout.get("return_offsets_mapping") is not None or layout.get("return_overflowing_tokens"):
            raise ValueError("fim cannot be combined with return_offsets_mapping or return_overflowing_tokens: "
                             "a rearranged row no longer follows its text")
        fim = dict(fim)
        unknown = set(fim) - {"prefix", "suffix", "middle", "rate", "spm_rate", "seed", "first_row"}
        if unknown:
            raise TypeError(f"fim: unknown keys {sorted(unknown)}")
        ids = []
        for key in ("prefix", "suffix", "middle"):
            if fim.get(key) is None:
                raise TypeError(f"fim: {key} is required")
            v = fim[key]
            if isinstance(v, str):
                k = self.special_token_to_id(v)
                if k is None:
                    raise TokenGeeXError(f"{v!r} is not a special token of this tokenizer", _lib.ERR_INVALID)
                v = k
            ids.append(int(v))
        return dict(prefix_id=ids[0], suffix_id=ids[1], middle_id=ids[2], rate=float(fim.get("rate", 1.0)),
                    spm_rate=float(fim.get("spm_rate", 0.5)), seed=self._sample_seed(fim.get("seed")), first_row=int(fim.get("first_row", 0)))

    def fim_result(self, result: "_lib.NativeResult", *, prefix, suffix, middle, rate: float = 1.0, spm_rate: float = 0.5,
                   seed: int | None = None, first_row: int = 0) -> "_lib.NativeResult":
        """The rows of a device result rearranged for fill-in-the-middle training (NativeResult.fim) -> a new NativeResult;
        `result` is only read, and the caller frees both.  A row is rearranged with probability `rate`, into
        PRE prefix SUF suffix MID middle (PSM) or, with probability spm_rate of those, PRE SUF suffix MID prefix middle (SPM),
        at two cuts drawn uniformly per row.  prefix / suffix / middle: the sentinels, ids or special-token strings.
        seed: None takes the tokenizer's seed (a fresh one when that is None too); first_row: the index of the result's
        first row in the batch the draws are made for."""
        req = self._fim_request({"fim": dict(prefix=prefix, suffix=suffix, middle=middle, rate=rate, spm_rate=spm_rate, seed=seed,
                                             first_row=first_row)})
        return result.fim(**req)

    @staticmethod
    def _fim_applied(res, fim):
        """`res` (None: a batch without samples) behind the fim request of a layout call; the intermediate result is freed."""
        if res is None or fim is None:
            return res
        try:
            return res.fim(**fim)
        finally:
            res.free()

    def _ordinary_result(self, flat: np.ndarray, offs: np.ndarray, dropout: float):
        """The ordinary path of encode_batch_flat up to the device result (processors run, text is not split at special
        tokens) -> NativeResult, or None for an empty batch."""
        if not self._native_front():
            raise TokenGeeXError("a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if offs.shape[0] <= 1:
            return None
        if self._processors:
            flat, offs = self._preprocess_flat(flat, offs)
        return self._model().encode_batch_flat(flat, offs, dropout, self._seed(dropout))

    def encode_ordinary_batch_padded_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0, **layout) -> dict:
        """encode_ordinary_batch over a packed batch (uint8 flat, uint64 offsets[S+1]) with the ids laid out on the device
        as torch tensors -> {"input_ids": [S, L], "attention_mask": [S, L] uint8 [, "lengths"]} on the tokenizer's device
        (tensors.to_padded: max_length, padding_side, truncation_side, dtype, return_lengths).  pad (required), bos and eos
        are ids or special-token strings (also spelt pad_id / bos_id / eos_id).  The ids go from the encode kernels to the
        tensors without visiting the host.  return_offsets_mapping="byte" | "char" adds "offset_mapping": [S, L, 2] in the
        dtype of input_ids, the (start, end) of every kept token in its sample's processed text (tensors.to_padded_spans);
        bos, eos and padding get (0, 0).

        return_overflowing_tokens=True with max_length (required then) and stride=s (default 0) keeps every token: a sample
        longer than max_length becomes several rows that each repeat s tokens of the row before (tensors.to_windows),
        the tensors are [W, L], "overflow_to_sample_mapping" and "window_first" ([W] int32) name each row's sample and the
        index of its first token there, and "offset_mapping" is [W, L, 2], still relative to the whole sample's text.

        fim=dict(prefix=, suffix=, middle= [, rate=1.0, spm_rate=0.5, seed=None, first_row=0]) rearranges the samples' ids
        for fill-in-the-middle training on the device before they are laid out (fim_result; the sentinels are ids or
        special-token strings).  It cannot be combined with return_offsets_mapping or return_overflowing_tokens (ValueError):
        those map rows onto their text, which a rearranged row no longer follows.  The packed forms and the encode_batch_* /
        encode_corpus_* forms take the same keyword.

        This is the ORDINARY path: the processors run as in encode_ordinary_batch and the text is not split at special
        tokens — a special token's string inside a text is encoded as ordinary text.  encode_batch_padded_flat is the
        special-aware form: the same layout over encode_batch's ids, put together on the device (encode_batch_result_flat)."""
        from . import tensors
        fim = self._fim_request(layout)
        unit = self._mapping_unit(layout)
        stride = self._window_stride(layout)
        layout = self._layout_ids(layout)
        res = self._fim_applied(self._ordinary_result(flat, offs, dropout), fim)
        if res is None:
            if stride is not None:
                return self._windows(None, layout, unit, stride)
            return self._with_offset_mapping(None, self._empty_layout(True, None, layout), layout, unit)
        try:
            if stride is not None:
                return self._windows(res, layout, unit, stride)
            return self._with_offset_mapping(res, tensors.to_padded(res, **layout), layout, unit)
        finally:
            res.free()

    def encode_ordinary_batch_packed_flat(self, flat: np.ndarray, offs: np.ndarray, block_len: int, dropout: float = 0.0,
                                          **layout) -> dict:
        """As encode_ordinary_batch_padded_flat with the LM-pretraining layout: the samples' sequences [bos] + ids + [eos]
        concatenated and cut into blocks -> {"input_ids": [B, block_len] [, "doc_ids", "positions"]} (tensors.to_packed:
        dtype, return_doc, drop_last).  The ORDINARY path as well; encode_batch_packed_flat is the special-aware form."""
        from . import tensors
        fim = self._fim_request(layout)
        layout = self._layout_ids(layout)
        res = self._fim_applied(self._ordinary_result(flat, offs, dropout), fim)
        if res is None:
            return self._empty_layout(False, block_len, layout)
        try:
            return tensors.to_packed(res, block_len, **layout)
        finally:
            res.free()

    def _empty_layout(self, padded: bool, block_len, layout: dict) -> dict:
        """What the layouts give for a batch without samples: [0, L] tensors (nothing runs on the device)."""
        import torch
        dev = torch.device("cuda", self._device)
        dtype = layout.get("dtype") or torch.int64
        if padded:
            a = (layout.get("bos_id") is not None) + (layout.get("eos_id") is not None)
            L = max(1, a) if layout.get("max_length") is None else int(layout["max_length"])
            out = {"input_ids": torch.empty((0, L), dtype=dtype, device=dev),
                   "attention_mask": torch.empty((0, L), dtype=torch.uint8, device=dev)}
            if layout.get("return_lengths"):
                out["lengths"] = torch.empty((0,), dtype=torch.int32, device=dev)
            return out
        out = {"input_ids": torch.empty((0, int(block_len)), dtype=dtype, device=dev)}
        if layout.get("return_doc"):
            out["doc_ids"] = torch.empty((0, int(block_len)), dtype=torch.int32, device=dev)
            out["positions"] = torch.empty((0, int(block_len)), dtype=torch.int32, device=dev)
        return out

    def encode_ordinary_batch_padded(self, texts: list[str], dropout: float = 0.0, **layout) -> dict:
        """encode_ordinary_batch_padded_flat over a list of strings."""
        text_b, offs_b = _fast.pack_strs(texts)
        return self.encode_ordinary_batch_padded_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64),
                                                      dropout, **layout)

    def encode_ordinary_batch_packed(self, texts: list[str], block_len: int, dropout: float = 0.0, **layout) -> dict:
        """encode_ordinary_batch_packed_flat over a list of strings."""
        text_b, offs_b = _fast.pack_strs(texts)
        return self.encode_ordinary_batch_packed_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64),
                                                      block_len, dropout, **layout)

    # -- the special-aware encode_batch with its ids kept on the device (csrc/assemble.hip) --
    def _split_segments(self, flat: np.ndarray, offs: np.ndarray):
        """The front of encode_batch_flat: the batch split at special tokens, the non-special segments packed and
        processed -> (seg_offs u64[S+1], seg_special i32[K], segments' flat, segments' offsets u64[E+1])."""
        only_crlf = all(isinstance(p, CrlfProcessor) for p in self._processors)  # then the packing pass does it on the way
        crlf = only_crlf and len(self._processors) > 0
        seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, [t.encode("utf-8") for t in self._special_tokens])
        pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
        if not only_crlf and poffs.shape[0] > 1:
            pflat, poffs = self._preprocess_flat(pflat, poffs)
        return seg_offs, ss, pflat, poffs

    def encode_batch_result_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0):
        """encode_batch_flat up to a device result: special-token split, processors and encode as there, then the
        samples' ids — special tokens' included — put together in HBM (NativeModel.assemble) instead of on the host
        -> NativeResult (ids() / offsets() are encode_batch_flat's; tensors.to_padded / to_packed lay it out), or None
        for a batch without samples.  The caller frees it."""
        if not self._native_front():
            raise TokenGeeXError("encode_batch_result_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        if not self._special_tokens:
            return self._ordinary_result(flat, offs, dropout)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if offs.shape[0] <= 1:
            return None
        seg_offs, ss, pflat, poffs = self._split_segments(flat, offs)
        model = self._model()
        segs = model.encode_batch_flat(pflat, poffs, dropout, self._seed(dropout)) if poffs.shape[0] > 1 else None
        try:
            return model.assemble(segs, seg_offs, ss, len(self._special_tokens))
        finally:
            if segs is not None:
                segs.free()

    def encode_batch_sample_result_flat(self, flat: np.ndarray, offs: np.ndarray, alpha: float, seed: int | None = None,
                                        return_logz: bool = False):
        """encode_batch_sample_flat up to a device result, as encode_batch_result_flat -> NativeResult or None
        [, logz f64[S]: a sample's log Z is the sum over its non-special segments, added up on the host]."""
        if not self._native_front():
            raise TokenGeeXError("encode_batch_sample_result_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        seed = self._sample_seed(seed)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        if n <= 0:
            return (None, np.zeros(0, np.float64)) if return_logz else None
        model = self._model()
        if not self._special_tokens:
            if self._processors:
                flat, offs = self._preprocess_flat(flat, offs)
            res, logz = model.encode_batch_sample_flat(flat, offs, alpha, seed, return_logz=True)
            return (res, logz) if return_logz else res
        seg_offs, ss, pflat, poffs = self._split_segments(flat, offs)
        segs, seg_logz = None, np.zeros(0, np.float64)
        if poffs.shape[0] > 1:
            segs, seg_logz = model.encode_batch_sample_flat(pflat, poffs, alpha, seed, return_logz=True)
        try:
            res = model.assemble(segs, seg_offs, ss, len(self._special_tokens))
        finally:
            if segs is not None:
                segs.free()
        if not return_logz:
            return res
        seg_sample = np.repeat(np.arange(n), np.diff(seg_offs.astype(np.int64)))
        return res, np.bincount(seg_sample[ss < 0], weights=seg_logz, minlength=n).astype(np.float64)

    def encode_batch_padded_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0, **layout) -> dict:
        """encode_ordinary_batch_padded_flat for the special-aware encode_batch: the text is split at special tokens, which
        get their own ids, and the ids are put together and laid out on the device (encode_batch_result_flat)."""
        from . import tensors
        fim = self._fim_request(layout)
        unit = self._mapping_unit(layout)
        stride = self._window_stride(layout)
        layout = self._layout_ids(layout)
        res = self._fim_applied(self.encode_batch_result_flat(flat, offs, dropout), fim)
        if res is None:
            if stride is not None:
                return self._windows(None, layout, unit, stride)
            return self._with_offset_mapping(None, self._empty_layout(True, None, layout), layout, unit)
        try:
            if stride is not None:
                return self._windows(res, layout, unit, stride)
            return self._with_offset_mapping(res, tensors.to_padded(res, **layout), layout, unit)
        finally:
            res.free()

    def encode_batch_packed_flat(self, flat: np.ndarray, offs: np.ndarray, block_len: int, dropout: float = 0.0, **layout) -> dict:
        """encode_ordinary_batch_packed_flat for the special-aware encode_batch (encode_batch_result_flat)."""
        from . import tensors
        fim = self._fim_request(layout)
        layout = self._layout_ids(layout)
        res = self._fim_applied(self.encode_batch_result_flat(flat, offs, dropout), fim)
        if res is None:
            return self._empty_layout(False, block_len, layout)
        try:
            return tensors.to_packed(res, block_len, **layout)
        finally:
            res.free()

    def encode_batch_padded(self, texts: list[str], dropout: float = 0.0, **layout) -> dict:
        """encode_batch_padded_flat over a list of strings."""
        text_b, offs_b = _fast.pack_strs(texts)
        return self.encode_batch_padded_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64), dropout, **layout)

    def encode_batch_packed(self, texts: list[str], block_len: int, dropout: float = 0.0, **layout) -> dict:
        """encode_batch_packed_flat over a list of strings."""
        text_b, offs_b = _fast.pack_strs(texts)
        return self.encode_batch_packed_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64), block_len,
                                             dropout, **layout)

    # -- encode_batch over a corpus that is already resident in HBM (csrc/front.hip) --
    def _corpus_front(self, who: str):
        """Which device front end a resident corpus takes -> (crlf, form).  crlf: None (no special tokens and no CRLF pass:
        the rows are encoded as they are) or the CRLF flag of NativeCorpus.split_specials; form: None or the Unicode form of
        NativeCorpus.normalize.  The device front end knows the processor lists [] and [CrlfProcessor] and, with
        device_unicode, [UnicodeProcessor] and [CrlfProcessor, UnicodeProcessor]; anything else (a Unicode form in front of
        CRLF, or a processor twice: "\r\r\n" shows the CRLF pass is not idempotent) stays with the flat route."""
        procs = self._processors
        kinds = [type(p) for p in procs]
        form = None
        if self.device_unicode and kinds in ([UnicodeProcessor], [CrlfProcessor, UnicodeProcessor]):
            form = procs[-1].form
        elif len(procs) > 1 or (procs and not isinstance(procs[0], CrlfProcessor)):
            raise TokenGeeXError(f"{who}: the device front end takes no processor list but [] and one CrlfProcessor; "
                                 "download the text and use encode_batch_result_flat", _lib.ERR_UNSUPPORTED)
        crlf = bool(procs) and isinstance(procs[0], CrlfProcessor)
        if not crlf and not self._special_tokens:
            return None, form
        return crlf, form

    def _split_corpus(self, corpus: "_lib.NativeCorpus", crlf: bool, form: str | None = None):
        """The corpus split at the special tokens, its segments CRLF-normalised if asked and then, as _preprocess_flat orders
        the two, under the Unicode form if one is given -> (the segments' corpus, the plan); the caller frees both.  (A
        window overflow names the segment, not the sample.)"""
        segs, plan = corpus.split_specials([t.encode("utf-8") for t in self._special_tokens], crlf)
        if form is None or not plan.num_encoded:
            return segs, plan
        try:
            return segs.normalize(form), plan
        except BaseException:
            plan.free()
            raise
        finally:
            segs.free()

    def encode_corpus_result(self, corpus: "_lib.NativeCorpus", dropout: float = 0.0) -> "_lib.NativeResult":
        """encode_batch_result_flat over a corpus that is already in HBM (an upload, or decode_result_text(...).to_corpus()):
        the special-token split and the CRLF processor run on the device (NativeCorpus.split_specials) and the plan is
        assembled from where it is (NativeModel.assemble_plan), so neither the text nor the plan visits the host ->
        NativeResult whose ids() / offsets() are encode_batch_flat's over the same samples.  The caller frees it.  (Without
        special tokens a sample is hashed for dropout by its index among the non-empty samples.)  With device_unicode a
        Unicode form behind them runs on the device too (NativeCorpus.normalize); alone and without special tokens it keeps
        every row, so dropout hashes a sample as the flat route does."""
        crlf, form = self._corpus_front("encode_corpus_result")
        model = self._model()
        if crlf is None and form is None:
            return model.encode_corpus(corpus, dropout, self._seed(dropout))
        if crlf is None:  # every row is kept, so a row is hashed for dropout as the flat route hashes it
            rows = corpus.normalize(form)
            try:
                return model.encode_corpus(rows, dropout, self._seed(dropout))
            finally:
                rows.free()
        segs_corpus, plan = self._split_corpus(corpus, crlf, form)
        segs = None
        try:
            if plan.num_encoded:
                segs = model.encode_corpus(segs_corpus, dropout, self._seed(dropout))
            return model.assemble_plan(segs, plan, len(self._special_tokens))
        finally:
            if segs is not None:
                segs.free()
            segs_corpus.free()
            plan.free()

    def encode_corpus_sample_result(self, corpus: "_lib.NativeCorpus", alpha: float, seed: int | None = None, return_logz: bool = False):
        """encode_batch_sample_result_flat over a resident corpus, as encode_corpus_result -> NativeResult [, logz f64[S]: the
        plan is copied to the host only for this sum over a sample's non-special segments]."""
        crlf, form = self._corpus_front("encode_corpus_sample_result")
        seed = self._sample_seed(seed)
        model = self._model()
        if crlf is None and form is None:
            return model.encode_corpus_sample(corpus, alpha, seed, return_logz=return_logz)
        if crlf is None:
            rows = corpus.normalize(form)
            try:
                return model.encode_corpus_sample(rows, alpha, seed, return_logz=return_logz)
            finally:
                rows.free()
        n = corpus.num_samples
        segs_corpus, plan = self._split_corpus(corpus, crlf, form)
        segs, seg_logz = None, np.zeros(0, np.float64)
        try:
            if plan.num_encoded:
                segs, seg_logz = model.encode_corpus_sample(segs_corpus, alpha, seed, return_logz=True)
            res = model.assemble_plan(segs, plan, len(self._special_tokens))
            if not return_logz:
                return res
            seg_offs, ss = plan.seg_offs(), plan.seg_special()
            seg_sample = np.repeat(np.arange(n), np.diff(seg_offs.astype(np.int64)))
            return res, np.bincount(seg_sample[ss < 0], weights=seg_logz, minlength=n).astype(np.float64)
        finally:
            if segs is not None:
                segs.free()
            segs_corpus.free()
            plan.free()

    def encode_corpus_padded(self, corpus: "_lib.NativeCorpus", dropout: float = 0.0, **layout) -> dict:
        """encode_batch_padded_flat over a resident corpus (encode_corpus_result): the same layout requests, offset mapping and
        overflow windows included."""
        from . import tensors
        fim = self._fim_request(layout)
        unit = self._mapping_unit(layout)
        stride = self._window_stride(layout)
        layout = self._layout_ids(layout)
        if corpus.num_samples == 0:
            if stride is not None:
                return self._windows(None, layout, unit, stride)
            return self._with_offset_mapping(None, self._empty_layout(True, None, layout), layout, unit)
        res = self._fim_applied(self.encode_corpus_result(corpus, dropout), fim)
        try:
            if stride is not None:
                return self._windows(res, layout, unit, stride)
            return self._with_offset_mapping(res, tensors.to_padded(res, **layout), layout, unit)
        finally:
            res.free()

    def encode_corpus_packed(self, corpus: "_lib.NativeCorpus", block_len: int, dropout: float = 0.0, **layout) -> dict:
        """encode_batch_packed_flat over a resident corpus (encode_corpus_result)."""
        from . import tensors
        fim = self._fim_request(layout)
        layout = self._layout_ids(layout)
        if corpus.num_samples == 0:
            return self._empty_layout(False, block_len, layout)
        res = self._fim_applied(self.encode_corpus_result(corpus, dropout), fim)
        try:
            return tensors.to_packed(res, block_len, **layout)
        finally:
            res.free()

    # -- subword regularisation: a segmentation drawn from the lattice (csrc/sample.hip) --
    def _sample_seed(self, seed: int | None) -> int:
        if seed is not None:
            return int(seed)
        return self.seed if self.seed is not None else random.getrandbits(64)

    def encode_sample(self, text: str, alpha: float, seed: int | None = None) -> list[int]:
        return self.encode_batch_sample([text], alpha, seed)[0]

    def encode_batch_sample(self, texts: list[str], alpha: float, seed: int | None = None) -> list[list[int]]:
        """encode_batch with every sample's segmentation drawn from P(x | text) ∝ exp(alpha · Σ score) (Kudo 2018)."""
        text_b, offs_b = _fast.pack_strs(texts)
        ids, o = self.encode_batch_sample_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64),
                                               alpha, seed)
        return _split_rows(ids, o)

    def encode_batch_sample_flat(self, flat: np.ndarray, offs: np.ndarray, alpha: float, seed: int | None = None,
                                 ordinary: bool = False, return_logz: bool = False):
        """encode_batch_flat with sampled segmentations -> (ids uint32[T], offsets uint64[S+1]) [, logz f64[S]].  Specials
        keep their ids; a sample's log Z is the sum over its non-special segments.  The draw of a match hashes the index of
        its segment in the packed batch of non-special segments (tgx_sample_u01)."""
        if not self._native_front():
            raise TokenGeeXError("encode_batch_sample_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        seed = self._sample_seed(seed)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        only_crlf = all(isinstance(p, CrlfProcessor) for p in self._processors)
        crlf = only_crlf and len(self._processors) > 0
        n = offs.shape[0] - 1

        def run(pflat, poffs):
            if poffs.shape[0] <= 1:
                return np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.float64)
            res, logz = self._model().encode_batch_sample_flat(pflat, poffs, alpha, seed, return_logz=True)
            try:
                return res.ids(), res.offsets(), logz
            finally:
                res.free()

        if ordinary or not self._special_tokens:
            if n and self._processors:
                flat, offs = self._preprocess_flat(flat, offs)
            ids, id_offs, logz = run(flat, offs)
            if not n:
                logz = np.zeros(0, np.float64)
            return (ids, id_offs, logz) if return_logz else (ids, id_offs)
        seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, [t.encode("utf-8") for t in self._special_tokens])
        pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
        if not only_crlf and poffs.shape[0] > 1:
            pflat, poffs = self._preprocess_flat(pflat, poffs)
        ids, id_offs, seg_logz = run(pflat, poffs)
        out = _lib.assemble_ids(seg_offs, ss, ids, id_offs, self.base_vocab_size())
        if not return_logz:
            return out
        seg_sample = np.repeat(np.arange(n), np.diff(seg_offs.astype(np.int64)))
        logz = np.bincount(seg_sample[ss < 0], weights=seg_logz, minlength=n).astype(np.float64) if n else np.zeros(0)
        return out[0], out[1], logz

    # -- lattice statistics: log Z, expected score and expected tokens per sample (csrc/stats.hip) --
    @staticmethod
    def _sum_segment_stats(seg: "_lib.LatticeStats | None", seg_offs: np.ndarray, ss: np.ndarray, n_bytes: np.ndarray, alpha: float):
        """A sample's values are the sums over its non-special segments, added on the host as encode_corpus_sample_result
        adds logz; every special token is one more expected token.  An unreachable segment (-inf, NaN, NaN) makes its sample
        no_path through the sums themselves."""
        n = seg_offs.shape[0] - 1
        seg_sample = np.repeat(np.arange(n), np.diff(seg_offs.astype(np.int64)))
        enc = seg_sample[ss < 0]
        zero = np.zeros(0, np.float64)
        logz, escore, etokens = (zero, zero, zero) if seg is None else (seg.logz, seg.expected_score, seg.expected_tokens)
        with np.errstate(invalid="ignore"):
            return _lib.LatticeStats(np.bincount(enc, weights=logz, minlength=n).astype(np.float64),
                                     np.bincount(enc, weights=escore, minlength=n).astype(np.float64),
                                     np.bincount(enc, weights=etokens, minlength=n) + np.bincount(seg_sample[ss >= 0], minlength=n),
                                     n_bytes, alpha)

    def lattice_stats(self, texts: list[str], alpha: float = 1.0) -> "_lib.LatticeStats":
        """Per text: log Z, expected score, expected token count (and entropy, bits per byte) of its segmentation
        distribution under temperature alpha — what encode_batch_sample draws from, without drawing."""
        text_b, offs_b = _fast.pack_strs(texts)
        return self.lattice_stats_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64), alpha)

    def lattice_stats_flat(self, flat: np.ndarray, offs: np.ndarray, alpha: float = 1.0) -> "_lib.LatticeStats":
        """lattice_stats over a packed batch: special-token split and processors as encode_batch_flat; n_bytes counts the
        samples as given."""
        if not self._native_front():
            raise TokenGeeXError("lattice_stats_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        n_bytes = np.diff(offs)
        if n <= 0:
            zero = np.zeros(0, np.float64)
            return _lib.LatticeStats(zero, zero, zero, np.zeros(0, np.uint64), alpha)
        model = self._model()
        if not self._special_tokens:
            if self._processors:
                flat, offs = self._preprocess_flat(flat, offs)
            st = model.lattice_stats_flat(flat, offs, alpha)
            return _lib.LatticeStats(st.logz, st.expected_score, st.expected_tokens, n_bytes, alpha, st.n_no_path)
        seg_offs, ss, pflat, poffs = self._split_segments(flat, offs)
        seg = model.lattice_stats_flat(pflat, poffs, alpha) if poffs.shape[0] > 1 else None
        return self._sum_segment_stats(seg, seg_offs, ss, n_bytes, alpha)

    def lattice_stats_corpus(self, corpus: "_lib.NativeCorpus", alpha: float = 1.0) -> "_lib.LatticeStats":
        """lattice_stats_flat over a resident corpus, with the device front end of encode_corpus_result (special-token
        split, CRLF and, with device_unicode, the Unicode form run in HBM)."""
        crlf, form = self._corpus_front("lattice_stats_corpus")
        model = self._model()
        n_bytes = np.diff(corpus.offsets())
        if crlf is None and form is None:
            return model.lattice_stats_corpus(corpus, alpha)
        if crlf is None:
            rows = corpus.normalize(form)
            try:
                st = model.lattice_stats_corpus(rows, alpha)
            finally:
                rows.free()
            return _lib.LatticeStats(st.logz, st.expected_score, st.expected_tokens, n_bytes, alpha, st.n_no_path)
        segs_corpus, plan = self._split_corpus(corpus, crlf, form)
        try:
            seg = model.lattice_stats_corpus(segs_corpus, alpha) if plan.num_encoded else None
            return self._sum_segment_stats(seg, plan.seg_offs(), plan.seg_special(), n_bytes, alpha)
        finally:
            segs_corpus.free()
            plan.free()

    # -- n-best segmentation: the k highest-scoring segmentations per sample (csrc/nbest.hip) --
    def encode_nbest(self, text: str, nbest: int) -> list[list[int]]:
        return self.encode_batch_nbest([text], nbest)[0]

    def encode_batch_nbest(self, texts: list[str], nbest: int) -> list[list[list[int]]]:
        """Per sample, up to nbest segmentations (id lists), best first (SentencePiece's NBestEncode)."""
        text_b, offs_b = _fast.pack_strs(texts)
        ids, o, _, nf = self.encode_batch_nbest_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64),
                                                     nbest)
        rows = _split_rows(ids, o)
        k = int(nbest)
        return [rows[i * k:i * k + int(nf[i])] for i in range(len(texts))]

    def encode_batch_nbest_flat(self, flat: np.ndarray, offs: np.ndarray, nbest: int, ordinary: bool = False):
        """encode_batch_flat with the nbest best segmentations of every sample -> (ids uint32[T], offsets u64[S·nbest+1],
        scores f64[S·nbest], n_found u32[S]); row s·nbest + r is the r-th best of sample s, rows at or beyond n_found are
        empty with score -inf.  Specials keep their ids and add nothing to the score; a sample split by specials gets the
        k-best product of its segments' lists (combine_nbest)."""
        if not self._native_front():
            raise TokenGeeXError("encode_batch_nbest_flat: a processor without a packed-buffer form", _lib.ERR_UNSUPPORTED)
        k = int(nbest)
        if not 1 <= k <= _lib.MAX_NBEST:
            raise TokenGeeXError(f"nbest must be in 1..{_lib.MAX_NBEST} (got {nbest})", _lib.ERR_INVALID)
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        only_crlf = all(isinstance(p, CrlfProcessor) for p in self._processors)
        crlf = only_crlf and len(self._processors) > 0
        n = offs.shape[0] - 1

        def run(pflat, poffs):
            if poffs.shape[0] <= 1:
                return np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.float64), np.zeros(0, np.uint32)
            res, sc, nf = self._model().encode_batch_nbest_flat(pflat, poffs, k)
            try:
                return res.ids(), res.offsets(), sc, nf
            finally:
                res.free()

        if ordinary or not self._special_tokens:
            if n and self._processors:
                flat, offs = self._preprocess_flat(flat, offs)
            return run(flat, offs)
        seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, [t.encode("utf-8") for t in self._special_tokens])
        pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
        if not only_crlf and poffs.shape[0] > 1:
            pflat, poffs = self._preprocess_flat(pflat, poffs)
        ids, id_offs, sc, nf = run(pflat, poffs)
        return combine_nbest(seg_offs, ss, self.base_vocab_size(), ids, id_offs, sc, nf, k)

    def encode_nbest_sample(self, text: str, nbest: int, alpha: float, seed: int | None = None) -> list[int]:
        return self.encode_batch_nbest_sample([text], nbest, alpha, seed)[0]

    def encode_batch_nbest_sample(self, texts: list[str], nbest: int, alpha: float, seed: int | None = None) -> list[list[int]]:
        """One segmentation per sample drawn from its n-best list with P ∝ exp(alpha · score) (SentencePiece's
        SampleEncode with nbest_size > 1): the row with the largest alpha · score_r − log(−log u_r) wins, u_r =
        tgx_sample_u01(seed, i, r, 0) for sample i of the batch, ties to the lower r."""
        if not (alpha >= 0.0 and np.isfinite(alpha)):
            raise TokenGeeXError(f"alpha must be finite and >= 0 (got {alpha})", _lib.ERR_INVALID)
        seed = self._sample_seed(seed)
        text_b, offs_b = _fast.pack_strs(texts)
        ids, o, sc, nf = self.encode_batch_nbest_flat(np.frombuffer(text_b, dtype=np.uint8), np.frombuffer(offs_b, dtype=np.uint64),
                                                      nbest)
        pick = nbest_draw(sc.reshape(len(texts), int(nbest)), nf, alpha, seed)
        rows = np.arange(len(texts)) * int(nbest) + pick
        return [ids[int(o[r]):int(o[r + 1])].tolist() for r in rows.tolist()]

    # -- decode: src/tokenizer.rs:126-187, src/model.rs:146-160 --
    def _model_decode(self, ids) -> str:
        buf = bytearray()
        n = len(self._vocab)
        for i in ids:
            if i >= n:
                raise TokenGeeXError(f"token id {i} is out of bounds", _lib.ERR_TOKEN_ID_OOB)
            buf += self._vocab[i][0]
        return bytes(buf).decode("utf-8", "replace")  # String::from_utf8_lossy

    def _postprocess(self, s: str) -> str:
        for p in reversed(self._processors):
            s = p.postprocess(s)
        return s

    def decode(self, ids: list[int], include_special_tokens: bool) -> str:
        n = len(self._vocab)
        out, run = [], []
        for i in ids:
            if i >= n:
                out.append(self._postprocess(self._model_decode(run)))
                run = []
                k = i - n
                if k >= len(self._special_tokens):
                    raise TokenGeeXError(f"token id {i} is out of bounds", _lib.ERR_TOKEN_ID_OOB)
                if include_special_tokens:
                    out.append(self._special_tokens[k])
            else:
                run.append(i)
        out.append(self._postprocess(self._model_decode(run)))
        return "".join(out)

    def _vocab_packed(self):
        if getattr(self, "_packed", None) is None or self._packed[0] != (len(self._vocab), len(self._special_tokens)):
            vf, vo = _lib.pack([v for v, _, _ in self._vocab])
            sf, so = _lib.pack([t.encode("utf-8") for t in self._special_tokens])
            self._packed = ((len(self._vocab), len(self._special_tokens)), vf, vo, sf, so)
        return self._packed[1:]

    def decode_batch_flat(self, ids: np.ndarray, offs: np.ndarray, include_special_tokens: bool):
        """decode_batch over packed ids (uint32 ids, uint64 offsets[S+1]) -> (utf-8 bytes, offsets[S+1]), in
        native code: src/tokenizer.rs:126-187 incl. String::from_utf8_lossy per run of base ids."""
        vf, vo, sf, so = self._vocab_packed()
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        return _lib.decode_batch_flat(vf, vo, len(self._vocab), sf, so, len(self._special_tokens), ids, offs,
                                      include_special_tokens)

    def decode_batch(self, ids: list[list[int]], include_special_tokens: bool) -> list[str]:
        try:
            flat = np.fromiter((i for row in ids for i in row), dtype=np.uint32, count=sum(len(r) for r in ids))
        except (OverflowError, ValueError):  # negative or > 2^32 - 1: the per-sample path names the id
            return [self.decode(x, include_special_tokens) for x in ids]
        offs = np.zeros(len(ids) + 1, np.uint64)
        if ids:
            np.cumsum(np.fromiter((len(r) for r in ids), dtype=np.uint64, count=len(ids)), out=offs[1:])
        text, to = self.decode_batch_flat(flat, offs, include_special_tokens)
        raw = text.tobytes()
        return [raw[int(to[i]):int(to[i + 1])].decode("utf-8") for i in range(len(ids))]

    # -- decode on the device (NativeModel.decode_result / tensors.decode_padded over csrc/decode.hip) --
    @staticmethod
    def _text_flat(text: "_lib.NativeText"):
        try:
            return text.bytes(), text.offsets()
        finally:
            text.free()

    @staticmethod
    def _text_strs(text: "_lib.NativeText") -> list[str]:
        flat, offs = Tokenizer._text_flat(text)
        raw, o = flat.tobytes(), offs.tolist()
        return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]

    def decode_result_text(self, result: "_lib.NativeResult", include_special_tokens: bool) -> "_lib.NativeText":
        """decode_batch_flat over a device result (of encode_batch_result_flat, encode_corpus, sampling, ...) without its ids
        leaving HBM -> NativeText: UTF-8 bytes and row offsets on the device (to_corpus() re-encodes them under another
        model).  Postprocessors are the identity, as in decode_batch_flat.  The caller frees it; the result is only read."""
        _, _, sf, so = self._vocab_packed()
        return self._model().decode_result(result, sf, so, include_special_tokens)

    def decode_result_flat(self, result: "_lib.NativeResult", include_special_tokens: bool):
        """decode_result_text copied to the host -> (utf-8 bytes, offsets u64[S+1]), what decode_batch_flat returns."""
        return self._text_flat(self.decode_result_text(result, include_special_tokens))

    def decode_result(self, result: "_lib.NativeResult", include_special_tokens: bool) -> list[str]:
        return self._text_strs(self.decode_result_text(result, include_special_tokens))

    # -- token spans on the device (tensors.to_spans over csrc/spans.hip) --
    def result_spans(self, result: "_lib.NativeResult", unit: str = "char", dtype=None):
        """The (start, end) of every token of a device result (of encode_batch_result_flat, encode_corpus, sampling, n-best)
        in its row's text -> torch tensor [T, 2] on the result's device (torch.int64 by default): code points ("char",
        indexes a str) or bytes ("byte") of the PROCESSED text, which is what decode(ids, True) returns; a special token's
        span is its own text.  Neither ids nor text visit the host."""
        from . import tensors
        _, _, sf, so = self._vocab_packed()
        return tensors.to_spans(result, self._model(), (sf, so), unit, dtype)

    def result_spans_flat(self, result: "_lib.NativeResult", unit: str = "char", dtype=None) -> np.ndarray:
        """result_spans copied to the host -> numpy [T, 2]; row i owns [offsets[i], offsets[i+1])."""
        return self.result_spans(result, unit, dtype).cpu().numpy()

    def _skip_id(self, skip) -> int | None:
        if isinstance(skip, str):
            k = self.special_token_to_id(skip)
            if k is None:
                raise TokenGeeXError(f"{skip!r} is not a special token of this tokenizer", _lib.ERR_INVALID)
            return k
        return skip

    def decode_tensor_text(self, input_ids, include_special_tokens: bool, attention_mask=None, lengths=None,
                           skip=None) -> "_lib.NativeText":
        """decode_batch over a [S, L] torch tensor of ids on the model's device (e.g. what a model generated), decoded where
        it lies -> NativeText.  attention_mask / lengths say which elements are there; `skip` (a special-token string or an
        id, typically the pad token) names an id that is dropped wherever it stands."""
        from . import tensors
        _, _, sf, so = self._vocab_packed()
        return tensors.decode_padded(self._model(), input_ids, attention_mask=attention_mask, lengths=lengths, skip_id=self._skip_id(skip),
                                     special_flat=sf, special_offs=so, include_special=include_special_tokens)

    def decode_tensor_flat(self, input_ids, include_special_tokens: bool, attention_mask=None, lengths=None, skip=None):
        """decode_tensor_text copied to the host -> (utf-8 bytes, offsets u64[S+1])."""
        return self._text_flat(self.decode_tensor_text(input_ids, include_special_tokens, attention_mask, lengths, skip))

    def decode_tensor(self, input_ids, include_special_tokens: bool, attention_mask=None, lengths=None, skip=None) -> list[str]:
        return self._text_strs(self.decode_tensor_text(input_ids, include_special_tokens, attention_mask, lengths, skip))

    # -- id / token queries: src/tokenizer.rs:189-259 --
    def token_to_id(self, token: bytes) -> int | None:
        r = self.base_token_to_id(token)
        if r is not None:
            return r
        try:
            return self.special_token_to_id(bytes(token).decode("utf-8"))
        except UnicodeDecodeError:
            return None

    def base_token_to_id(self, token: bytes) -> int | None:
        return self._token_to_ids.get(bytes(token))

    def special_token_to_id(self, token: str) -> int | None:
        k = self._special_tokens_map.get(token)
        return None if k is None else k + len(self._vocab)

    def id_to_token(self, id: int) -> bytes | None:
        s = self.id_to_special_token(id)
        if s is not None:
            return s.encode("utf-8")
        b = self.id_to_base_token(id)
        return None if b is None else b[0]

    def id_to_base_token(self, id: int) -> tuple[bytes, float] | None:
        if 0 <= id < len(self._vocab):
            return self._vocab[id][0], self._vocab[id][1]
        return None

    def id_to_special_token(self, id: int) -> str | None:
        k = id - len(self._vocab)
        if 0 <= k < len(self._special_tokens):
            return self._special_tokens[k]
        return None

    def is_special(self, id: int) -> bool:
        return self.id_to_special_token(id) is not None

    def is_base(self, id: int) -> bool:
        return id < len(self._vocab)

    def add_special_tokens(self, tokens: list[str]) -> None:
        for t in tokens:  # src/tokenizer.rs:39-53: existing specials are ignored
            if t == "":
                raise ValueError("empty special token (the reference's splitter would never advance)")
            if t in self._special_tokens_map:
                continue
            self._special_tokens_map[t] = len(self._special_tokens)
            self._special_tokens.append(t)

    def add_base_tokens(self, tokens: list[tuple[bytes, float, bool]]) -> None:
        """Tokenizer::add_base_tokens -> Model::add_tokens, src/model.rs:184-194."""
        for v, s, k in tokens:
            self._token_to_ids[bytes(v)] = len(self._vocab)
            self._vocab.append((bytes(v), float(s), bool(k)))
        if self._native is not None:  # mutation = build a new device handle
            self._native.free()
            self._native = None

    def special_tokens(self) -> list[str]:
        return list(self._special_tokens)

    def vocab_size(self) -> int:
        return len(self._vocab) + len(self._special_tokens)

    def base_vocab_size(self) -> int:
        return len(self._vocab)

    def special_vocab_size(self) -> int:
        return len(self._special_tokens)

    def common_prefix_search(self, text: str) -> list[int]:
        return [i for i, _ in self._model().common_prefix_search(text.encode("utf-8"))]

    # -- serialisation: src/tokenizer.rs:261-297, 349-435, src/lib.rs:109-204 --
    def to_string(self) -> str:
        vocab = []
        for v, s, k in self._vocab:
            try:
                e = {"value": v.decode("utf-8"), "score": s}
            except UnicodeDecodeError:
                e = {"value": base64.b64encode(v).decode("ascii").rstrip("="), "score": s, "encoded": True}
            if k:
                e["keep"] = True
            vocab.append(e)
        return json.dumps({"version": SERIALIZATION_VERSION, "special_tokens": self._special_tokens,
                           "processors": [p.to_json() for p in self._processors], "vocab": vocab},
                          ensure_ascii=False, separators=(",", ":"))

    def save(self, filename: str) -> None:
        with open(filename, "w", encoding="utf-8") as f:
            f.write(self.to_string())

    @staticmethod
    def from_str(data: str, device: int = 0) -> "Tokenizer":
        try:
            obj = json.loads(data)
        except json.JSONDecodeError as e:
            raise TokenGeeXError(str(e), _lib.ERR_JSON) from None
        if not isinstance(obj, dict):
            raise TokenGeeXError("invalid type: expected struct Tokenizer", _lib.ERR_JSON)
        allowed = ("version", "special_tokens", "processors", "vocab")
        for key in obj:
            if key not in allowed:  # src/tokenizer.rs:414-419
                raise TokenGeeXError(f"unknown field `{key}`, expected one of `version`, `special_tokens`, "
                                     "`processors`, `vocab`", _lib.ERR_JSON)
        if "version" not in obj:
            raise TokenGeeXError("missing field `version`", _lib.ERR_JSON)
        if obj["version"] != SERIALIZATION_VERSION:  # src/tokenizer.rs:423-429
            raise TokenGeeXError(f"unsupported version: {obj['version']}", _lib.ERR_JSON)
        vocab = []
        for e in obj.get("vocab", []):
            for key in e:
                if key not in ("value", "score", "encoded", "keep"):  # src/lib.rs:173-175
                    raise TokenGeeXError(f"unknown field `{key}`, expected one of `value`, `score`, "
                                         "`encoded`, `keep`", _lib.ERR_JSON)
            if "value" not in e:
                raise TokenGeeXError("missing field `token`", _lib.ERR_JSON)  # sic, src/lib.rs:189
            if "score" not in e:
                raise TokenGeeXError("missing field `score`", _lib.ERR_JSON)
            if e.get("encoded", False):
                v = e["value"]
                raw = base64.b64decode(v + "=" * (-len(v) % 4))  # STANDARD_NO_PAD, src/lib.rs:8
            else:
                raw = e["value"].encode("utf-8")
            vocab.append((raw, float(e["score"]), bool(e.get("keep", False))))
        procs = [_processor_from_json(p) for p in obj.get("processors", [])]
        return Tokenizer(vocab, procs, obj.get("special_tokens", []), device=device)

    @staticmethod
    def from_file(filepath: str, device: int = 0) -> "Tokenizer":
        try:
            with open(filepath, encoding="utf-8") as f:
                data = f.read()
        except OSError as e:
            raise TokenGeeXError(str(e), _lib.ERR_IO) from None
        return Tokenizer.from_str(data, device=device)

    def __getstate__(self):
        return self.to_string().encode("utf-8")

    def __setstate__(self, state):
        other = Tokenizer.from_str(bytes(state).decode("utf-8"))
        self.__dict__.update(other.__dict__)

    # -- access for the training-loop entry points --
    def vocab(self) -> list[tuple[bytes, float, bool]]:
        return list(self._vocab)

    def native_model(self) -> _lib.NativeModel:
        return self._model()
