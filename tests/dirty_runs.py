"""A registry of device calls, one or a few per ABI function of include/tgx.h that queues device work, for the tests
that run the library on hostile memory (tests/test_pool_fill_gpu.py: every pooled buffer filled with a byte before its
owner sees it) and in hostile orders (tests/test_pass_sequences_gpu.py).  tests/test_dirty_runs_cpu.py holds the
registry to the header: every function is in some entry's `covers` or in EXCLUDED, never in both.

An entry is a named call:
    covers         the ABI functions it reaches
    env            the knobs it runs under (the test sets them with monkeypatch.setenv; read per call by the library)
    run(ctx)       -> dict name -> numpy array: everything the call gave.  Every handle is made inside run, so that all of
                   the library's memory of the call comes from the pool while the fill is on.  A key that begins with
                   "_" is for check alone (kernel names, counters, messages) and is not compared between runs.
    check(out)     the outputs against the reference the subsystem already has: the CPU oracle for ids, counts and pairs,
                   the *_checker.py modules and the *_host twins for the transforms, sample_checker / nbest_checker for
                   sampling and n-best, util.assert_estep_truth and the 80-bit truth for the E-step and the lattice
                   statistics.  No tolerance is new: every float comparison is the gate its call already has
                   (test_estep_pairs_gpu.py, test_stats_gpu.py, test_sample_gpu.py); everything else is ==.
    deterministic  the outputs are the same bits on every run.  False only where counts are summed with atomics in an
                   order the hardware chooses: the E-step's expected counts and log Z sum (SUMMED; such an entry's other
                   outputs are still compared bit for bit).

Inputs are the smallest that each subsystem's case modules define for its edges (past_cap.edge_*, *_cases.py, the tiny
vocabularies of test_top_table_gpu.py); the past-the-cap batch of a subsystem is here only where its kernels carry state
between a block's tiles (the consecutive-run kernels, textstat's carried line, repeat_cover_kernel's window).  References
are computed once per process and never changed."""
from __future__ import annotations

import functools
import math

import numpy as np

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, synth

ENTRIES: dict = {}


SUMMED = ("expected", "logz")   # the outputs of an entry that is not deterministic which atomics sum; its others are exact


class Entry:
    def __init__(self, name, covers, run, check, env, deterministic):
        self.name, self.covers, self.run, self.check, self.env, self.deterministic = name, tuple(covers), run, check, dict(env), deterministic
        self.summed = () if deterministic else SUMMED


def _add(name, covers, run, check, env=None, deterministic=True):
    assert name not in ENTRIES, name
    ENTRIES[name] = Entry(name, covers, run, check, env or {}, deterministic)


# ABI functions that queue no device work of their own, each with the reason it is on this side.  A function that launches
# a kernel, copies on a stream or takes a pooled buffer does not belong here.
_GETTER = "getter of a handle's or the thread's host-side state"
_FREE = "frees a handle (buffers go back to the pool, nothing is queued)"
_TWIN = "host twin: pure host code"
_HOST = "pure host code"
_TIMES = "*_last_times: reads the thread's recorded stage times"
EXCLUDED = {
    "tgx_last_error": _GETTER, "tgx_last_error_detail": _GETTER, "tgx_abi_version": _GETTER, "tgx_device_count": _GETTER,
    "tgx_model_destroy": _FREE, "tgx_model_vocab_size": _GETTER, "tgx_model_max_token_len": _GETTER, "tgx_model_trie_bytes": _GETTER,
    "tgx_model_device": _GETTER, "tgx_common_prefix_search": _HOST, "tgx_split_specials": _HOST, "tgx_pack_segments": _HOST,
    "tgx_normalize_segments": _HOST, "tgx_unidata_version": _GETTER, "tgx_assemble_ids": _HOST, "tgx_decode_batch": _HOST,
    "tgx_utf8_lossy": _HOST, "tgx_generate_u01": _HOST, "tgx_flat_trie_build": _HOST, "tgx_flat_trie_free": _FREE,
    "tgx_flat_trie_search": _HOST, "tgx_flat_trie_stats": _GETTER, "tgx_flat_trie_search8": _HOST, "tgx_flat_trie_copy": _HOST,
    "tgx_tok_hash_selftest": _HOST, "tgx_dropout_u01_host": _HOST, "tgx_dropout_u01": _HOST,
    "tgx_result_num_samples": _GETTER, "tgx_result_num_tokens": _GETTER,
    "tgx_result_ids_device": _GETTER, "tgx_result_offsets_device": _GETTER,
    "tgx_result_free": _FREE, "tgx_result_device": _GETTER, "tgx_result_vocab_size": _GETTER,
    "tgx_layout_pad_host": _TWIN, "tgx_layout_pack_host": _TWIN, "tgx_layout_windows_host": _TWIN, "tgx_window_spans_host": _TWIN,
    "tgx_assemble_host": _TWIN, "tgx_fim_last_times": _TIMES, "tgx_fim_u01": _HOST, "tgx_fim_host": _TWIN,
    "tgx_select_last_times": _TIMES, "tgx_shuffle_key": _HOST, "tgx_shuffled_rows_host": _TWIN, "tgx_select_host": _TWIN,
    "tgx_select_text_host": _TWIN, "tgx_row_hash": _HOST, "tgx_first_equal_host": _TWIN, "tgx_dedup_last_times": _TIMES,
    "tgx_dedup_last_rounds": _GETTER, "tgx_minhash_value": _HOST, "tgx_minhash_host": _TWIN, "tgx_minhash_bands_host": _TWIN,
    "tgx_minhash_near_first_host": _TWIN, "tgx_minhash_last_times": _TIMES, "tgx_gram_key": _HOST, "tgx_gramset_size": _GETTER,
    "tgx_gramset_info": _GETTER, "tgx_gramset_free": _FREE, "tgx_gram_keys_host": _TWIN,
    "tgx_gram_hits_host": _TWIN, "tgx_gram_contains_host": _TWIN, "tgx_gram_last_times": _TIMES, "tgx_text_stats_host": _TWIN,
    "tgx_lines_host": _TWIN, "tgx_textstat_last_times": _TIMES, "tgx_repeat_stats_host": _TWIN, "tgx_repeat_last_times": _TIMES,
    "tgx_plan_num_samples": _GETTER, "tgx_plan_num_segments": _GETTER, "tgx_plan_num_encoded": _GETTER, "tgx_plan_device": _GETTER,
    "tgx_plan_free": _FREE, "tgx_front_last_times": _TIMES,
    "tgx_front_host": _TWIN, "tgx_normalize_host": _TWIN, "tgx_norm_last_times": _TIMES,
    "tgx_text_num_rows": _GETTER, "tgx_text_num_bytes": _GETTER, "tgx_text_num_replaced": _GETTER, "tgx_text_device": _GETTER,
    "tgx_text_bytes_device": _GETTER, "tgx_text_offsets_device": _GETTER,
    "tgx_text_free": _FREE, "tgx_decode_rows_host": _TWIN, "tgx_spans_host": _TWIN, "tgx_corpus_free": _FREE,
    "tgx_corpus_num_samples": _GETTER, "tgx_corpus_num_bytes": _GETTER, "tgx_sample_u01": _HOST, "tgx_lattice_stats_host": _TWIN,
    "tgx_free": _FREE, "tgx_pool_trim": "hipFree of pooled buffers, nothing is queued", "tgx_pool_filled_bytes": _GETTER,
    "tgx_host_alloc": "page-locked host memory, no device work", "tgx_host_free": _FREE, "tgx_digamma": _HOST,
    "tgx_prune_m_step": _HOST, "tgx_prune_alternatives": _HOST, "tgx_model_prune_alternatives": _HOST, "tgx_prune_select": _HOST,
    "tgx_last_kernel_times": _TIMES, "tgx_last_algorithmic_bytes": _GETTER, "tgx_last_encode_waves_per_cu": _GETTER,
    "tgx_last_encode_redo_samples": _GETTER, "tgx_last_encode_long_samples": _GETTER, "tgx_last_estep_pieces": _GETTER,
    "tgx_last_estep_redo": _GETTER, "tgx_last_encode_corun_cus": _GETTER, "tgx_encode_corun_timeouts": _GETTER,
    "tgx_model_score_values": _GETTER, "tgx_last_encode_hot_values": _GETTER, "tgx_last_encode_lean_items": _GETTER,
    "tgx_last_encode_ids_in_place": _GETTER, "tgx_last_encode_top_table": _GETTER,
}


class Ctx:
    """what a run takes from its test: torch's device tensors (over a sentinel: torch's allocator is not the library's
    pool, so the fill does not reach them) and the caller's stream"""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", 0)

    def full(self, shape, dtype, fill):
        return self.torch.full(shape, fill, dtype=getattr(self.torch, dtype), device=self.device)

    def dev(self, a):
        a = np.array(a, order="C")
        return self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device)

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy()


_REF: dict = {}


def _ref(key, compute):
    """a reference, computed once per process (check runs once per fill byte) and never changed"""
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), what


def _rows(ids, offs):
    return [ids[int(offs[i]):int(offs[i + 1])].tolist() for i in range(offs.size - 1)]


def _take_result(res, out, key=""):
    out[key + "ids"], out[key + "offs"] = res.ids(), res.offsets()
    res.free()


def _take_text(text, out, key=""):
    out[key + "bytes"], out[key + "offs"], out[key + "replaced"] = text.bytes(), text.offsets(), np.array([text.num_replaced], np.uint64)
    text.free()


# ======================================================================================================================
# model passes: three vocabularies over one corpus (tests/test_pass_sequences_gpu.py runs them on shared handles)
# ======================================================================================================================
LONG_THRESHOLD = 4096   # TGX_LONG_THRESHOLD of the entries that want encode6_kernel: two samples of the corpus lie above
NO_TOKEN = b"\x01"      # a byte of one sample that model C has no token for


@functools.lru_cache(maxsize=None)
def pass_texts():
    """About a hundred samples: empty ones; 1 and 2 bytes; 47 / 48 / 49 and 63 / 64 / 65 bytes, the trips of three and four
    positions per lane; a few of 300 to 3 000 bytes; two above LONG_THRESHOLD; one with the byte that model C lacks."""
    flat, offs = synth.make_corpus(192 << 10, "mixed", max_len=3000, seed_offset=41)
    o = offs.astype(np.int64)
    rows = [bytes(flat[o[i]:o[i + 1]]) for i in range(o.size - 1)]
    raw = bytes(flat)
    trips = [raw[7 * n:8 * n] for n in (0, 1, 2, 47, 48, 49, 63, 64, 65)]
    small = [r for r in rows if len(r) < 300][:76]
    mid = [r for r in rows if 300 <= len(r) <= 3000][:8]
    assert len(small) == 76 and len(mid) == 8, (len(small), len(mid))
    texts = [b"", b""] + trips + small[:30] + [b""] + mid[:4] + [raw[2000:7000]] + small[30:] + mid[4:] + [raw[20000:26500], b"",
                                                                                                         b"plain " + NO_TOKEN + b" text", raw[:65]]
    n = [len(t) for t in texts]
    assert 95 <= len(texts) <= 110 and sum(x >= LONG_THRESHOLD for x in n) == 2 and n.count(0) >= 4
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def pass_batch():
    flat, offs = tgx.pack(list(pass_texts()))
    flat.setflags(write=False)
    offs.setflags(write=False)
    return flat, offs


@functools.lru_cache(maxsize=None)
def vocab(name):
    """A: a few thousand tokens of at most 16 bytes, every byte among them.  B: tokens of 17 .. 32 bytes too (rows2, the
    LONG build).  C: A without the token NO_TOKEN and with other scores: one sample has no path under it."""
    text = bytes(pass_batch()[0][: 96 << 10])
    rng = np.random.default_rng({"A": 21, "B": 22, "C": 23}[name])
    if name == "B":
        toks, scores = synth.random_vocab(rng, text, 1500, 32, tie_fraction=0.0)
        assert 17 <= max(map(len, toks)) <= 32
        return list(toks), np.asarray(scores, np.float64)
    toks, scores = synth.random_vocab(np.random.default_rng(21), text, 2500, 16, tie_fraction=0.2)
    toks, scores = list(toks), np.asarray(scores, np.float64)
    if name == "C":
        keep = [i for i, t in enumerate(toks) if NO_TOKEN not in t]
        assert len(keep) < len(toks)
        return [toks[i] for i in keep], -(rng.random(len(keep)) * 6.0 + 1.0)
    assert max(map(len, toks)) <= 16
    return toks, scores


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    return orc.OracleModel(*vocab(name))


def native_of(name, for_estep=False):
    return tgx.NativeModel(*vocab(name), for_estep=for_estep)


def native_plain(name):
    """a model through tgx_model_create, the entry point without flags (NativeModel() goes through tgx_model_create_ex)"""
    return tgx.NativeModel.create_plain(*vocab(name))


@functools.lru_cache(maxsize=None)
def oracle_encode(name, dropout=0.0, seed=0):
    """the oracle's (ids, offs) of the corpus, or its NoPath"""
    try:
        return oracle_of(name).encode_batch_flat(*pass_batch(), dropout, seed, threads=4)
    except orc.NoPath as e:
        return e


def run_encode(nat, source, dropout=0.0, seed=0, how="corpus"):
    """-> outputs of an encode of the corpus (source: a NativeCorpus for how="corpus", else unused); a refusal is an output"""
    out = {}
    try:
        if how == "corpus":
            res = nat.encode_corpus(source, dropout, seed)
        elif how == "batch":
            res = nat.encode_batch_flat(*pass_batch(), dropout, seed)
        elif how == "host":
            out["ids"], out["offs"] = nat.encode_batch_host(*pass_batch(), dropout, seed)
            out["ids"] = out["ids"].copy()
            res = None
        else:
            out["ids"], out["offs"] = tgx.NativeModel.encode_batch_multi([nat], *pass_batch(), dropout, seed)
            out["ids"] = out["ids"].copy()
            res = None
        if res is not None:
            _take_result(res, out)
    except tgx.TokenGeeXError as e:
        out["error"] = np.array([e.status, -1 if e.sample is None else e.sample], np.int64)
        out["_message"] = str(e)
    out["_kernels"] = sorted(nat.last_kernel_times())
    out["_flags"] = dict(top=nat.last_encode_top_table(), in_place=nat.last_encode_ids_in_place(), long=nat.last_encode_long_samples(),
                         hot=nat.last_encode_hot_values(), values=nat.score_values(), redo=nat.last_encode_redo_samples())
    return out


def check_encode(out, name, dropout=0.0, seed=0):
    want = oracle_encode(name, dropout, seed)
    if isinstance(want, orc.NoPath):
        assert "error" in out and out["error"].tolist() == [_lib.ERR_NO_PATH, want.sample] and out["_message"] == str(want), (out.get("_message"), str(want))
        return
    assert "error" not in out, out.get("_message")
    _eq(out["offs"], want[1], "offsets")
    _eq(out["ids"], want[0], "ids")


def _encode_entry(name, vocab_name, env, kernels=(), flags=None, dropout=0.0, seed=0, how="corpus", covers=("tgx_encode_corpus",)):
    def run(ctx):
        nat = native_plain(vocab_name) if how == "batch" else native_of(vocab_name)
        corpus = tgx.NativeCorpus(*pass_batch()) if how == "corpus" else None
        try:
            return run_encode(nat, corpus, dropout, seed, how)
        finally:
            if corpus is not None:
                corpus.free()
            nat.free()

    def check(out):
        check_encode(out, vocab_name, dropout, seed)
        for k in kernels:
            assert k in out["_kernels"], (k, out["_kernels"])
        for k, v in (flags or {}).items():
            got = out["_flags"][k]
            assert (got < out["_flags"]["values"]) if v == "below_values" else got == v, (k, got, v)

    _add(name, covers + (("tgx_model_create_ex", "tgx_corpus_upload") if how == "corpus" else ()), run, check, env)


_LT = {"TGX_LONG_THRESHOLD": str(LONG_THRESHOLD)}
_encode_entry("encode_fused", "A", {"TGX_PATH": "fused"}, ("encode_kernel",))
_encode_entry("encode_rows4", "A", {"TGX_PATH": "rows4"}, ("compact_kernel",), {"in_place": False})
_encode_entry("encode_rows4l", "B", {"TGX_PATH": "rows4l"})
_encode_entry("encode_rows2", "B", {"TGX_PATH": "rows2"}, ("encode2_kernel",))
_encode_entry("encode_rows5_long_build", "B", {"TGX_PATH": "rows5"}, ("encode5_kernel",))
_encode_entry("encode_rows5_top", "A", {"TGX_PATH": "rows5", "TGX_E5_TOP": "1", "TGX_LONG_THRESHOLD": "0"}, ("encode5_kernel",), {"top": True, "in_place": True})
_encode_entry("encode_rows5_no_top", "A", {"TGX_PATH": "rows5", "TGX_E5_TOP": "0", "TGX_LONG_THRESHOLD": "0"}, ("encode5_kernel",), {"top": False})
_encode_entry("encode_rows5_through_tmp", "A", {"TGX_PATH": "rows5", "TGX_IDS_IN_PLACE": "0", "TGX_LONG_THRESHOLD": "0"}, ("encode5_kernel", "compact_kernel"),
              {"in_place": False})
_encode_entry("encode_rows5_dropout", "A", {"TGX_PATH": "rows5"}, ("encode5_kernel",), dropout=0.2, seed=7)
_encode_entry("encode_rows5_cold", "A", {"TGX_PATH": "rows5", "TGX_E5_HOT": "100"}, ("encode5_kernel",), {"hot": "below_values"})
_encode_entry("encode_rows5_long_samples", "A", {"TGX_PATH": "rows5", **_LT}, ("encode5_kernel", "encode6_kernel"), {"long": 2})
# (the re-rank's count array is pooled and pre-set; the ABI has no getter for the ranks, and any rank order encodes the same ids:
# the entry sees a count array that breaks the remap of the records, not one that merely orders the values badly)
_encode_entry("encode_value_rank_counts", "A", {"TGX_VALUE_RANK": "counts"}, ("encode5_kernel",))
_encode_entry("encode_no_path", "C", {}, ())
_encode_entry("encode_batch", "A", {}, how="batch", covers=("tgx_encode_batch", "tgx_model_create"))
_encode_entry("encode_batch_host", "A", {"TGX_E2E_CHUNK_MB": "1"}, how="host", covers=("tgx_encode_batch_host",))
_encode_entry("encode_batch_multi", "A", {}, how="multi", covers=("tgx_encode_batch_multi",))


# ---- a derived model through encode and E-step --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def derived_vocab():
    toks, _ = vocab("A")
    rng = np.random.default_rng(31)
    keep = np.array([i for i, t in enumerate(toks) if len(t) == 1 or rng.random() < 0.6], np.uint32)
    return keep, -(rng.random(keep.size) * 7.0 + 1.0)


@functools.lru_cache(maxsize=None)
def derived_oracle():
    toks, _ = vocab("A")
    keep, sc = derived_vocab()
    return orc.OracleModel([toks[int(i)] for i in keep], sc)


def _estep_out(nat, corpus, snippet_len, dropout, seed):
    got, gz = nat.estep(corpus, snippet_len, dropout, seed)
    return {"expected": got, "logz": np.array([gz]), "_kernels": dict(nat.last_kernel_times()),
            "_flags": dict(redo=nat.last_estep_redo(), pieces=nat.last_estep_pieces())}


def check_estep(out, ora, snippet_len, dropout, seed, kernels=()):
    """the gate of test_estep_pairs_gpu.py: against the f64 oracle at util.rtol_for, and through util.assert_estep_truth"""
    from util import assert_estep_truth, rtol_for
    flat, offs = estep_batch()
    st, want, wz, _ = ora.estep_flat(flat, offs, snippet_len, dropout, seed, threads=4)
    assert st == orc.OK
    longest = int(np.diff(offs.astype(np.int64)).max())
    got, gz = out["expected"], float(out["logz"][0])
    np.testing.assert_allclose(got, want, rtol=rtol_for(min(snippet_len, longest)), atol=1e-12)
    assert np.array_equal(got != 0, want != 0) and abs(gz - wz) <= 1e-12 * abs(wz) + 1e-9
    assert_estep_truth(got, gz, out["_kernels"], ora, flat, offs, snippet_len, dropout, seed, want, wz)
    for k in kernels:
        assert k in out["_kernels"], (k, sorted(out["_kernels"]))


def estep_batch():
    """the whole corpus: A, B and the derived model have a token for every byte, so every snippet has a normal z"""
    return pass_batch()


def _run_derived(ctx):
    parent = native_of("A")
    keep, sc = derived_vocab()
    child = parent.derive(keep, sc, for_estep=True)
    corpus = tgx.NativeCorpus(*pass_batch())
    try:
        out = run_encode(child, corpus)
        e = _estep_out(child, corpus, 81920, 0.0, 0)
        out.update({"expected": e["expected"], "logz": e["logz"], "_estep_kernels": e["_kernels"]})
        return out
    finally:
        corpus.free()
        child.free()
        parent.free()


def _check_derived(out):
    want = derived_oracle().encode_batch_flat(*pass_batch(), threads=4)
    _eq(out["offs"], want[1], "offsets")
    _eq(out["ids"], want[0], "ids")
    check_estep({"expected": out["expected"], "logz": out["logz"], "_kernels": out["_estep_kernels"]}, derived_oracle(), 81920, 0.0, 0)


_add("derived_model_encode_and_estep", ("tgx_model_create_derived", "tgx_encode_corpus", "tgx_estep"), _run_derived, _check_derived, deterministic=False)


# ---- the E-step -----------------------------------------------------------------------------------------------------------
def _estep_entry(name, vocab_name, env, kernels=(), snippet_len=81920, dropout=0.0, seed=0, flags=None):
    def run(ctx):
        nat = native_of(vocab_name, for_estep=True)
        corpus = tgx.NativeCorpus(*estep_batch())
        try:
            return _estep_out(nat, corpus, snippet_len, dropout, seed)
        finally:
            corpus.free()
            nat.free()

    def check(out):
        check_estep(out, oracle_of(vocab_name), snippet_len, dropout, seed, kernels)
        for k, low in (flags or {}).items():
            assert out["_flags"][k] >= low, (k, out["_flags"])

    _add(name, ("tgx_estep",), run, check, env, deterministic=False)


_estep_entry("estep7", "A", {}, ("estep7_kernel",))
_estep_entry("estep7_redo", "A", {"TGX_E7_OVF_AT": "40", "TGX_E7_HOT": "20"}, ("estep7_kernel", "estep7_redo_kernel"), flags={"redo": 1})
_estep_entry("estep7_dropout_short_snippets", "A", {}, ("estep7_kernel",), snippet_len=700, dropout=0.2, seed=9)
_estep_entry("estep_log", "A", {"TGX_ESTEP": "log"}, ("estep4_fwd_kernel", "estep4_bwd_kernel"))
_estep_entry("estep_chain", "A", {"TGX_ESTEP": "chain"}, ("estep4l_bwd_kernel",))
_estep_entry("estep_chain_pieces", "A", {"TGX_ESTEP": "chain", "TGX_ESTEP_PIECES": "1", "TGX_ESTEP_WINDOW": "256"}, ("estep4l_bwd_kernel", "cut_windows_kernel"),
             flags={"pieces": 100})
_estep_entry("estep_chain_dropout", "A", {"TGX_ESTEP": "chain"}, ("estep4l_bwd_kernel",), dropout=0.1, seed=5)
_estep_entry("estep_fused", "A", {"TGX_PATH": "fused"}, ("estep_kernel",))
_estep_entry("estep_long_tokens", "B", {}, ())


# ---- counting passes ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_reference(name):
    import scan_cases
    flat, offs = estep_batch()
    return scan_cases.reference_of(oracle_of(name), flat, offs, len(vocab(name)[0]))


def run_counts(nat, corpus, top_k):
    out = {"freq": nat.count_tokens(corpus)}
    out["_after_tokens"] = sorted(nat.last_kernel_times())
    out["keys"], out["counts"] = nat.count_pairs(corpus)
    out["top_keys"], out["top_counts"], total = nat.count_pairs_top(corpus, top_k)
    out["total"] = np.array([total], np.uint64)
    return out


def check_counts(out, name, top_k):
    ref = count_reference(name)
    for key in ("freq", "keys", "counts"):
        _eq(out[key], ref[key], key)
    _eq(out["top_keys"], ref["top_keys"][:top_k], "top keys")
    _eq(out["top_counts"], ref["top_counts"][:top_k], "top counts")
    assert int(out["total"][0]) == ref["keys"].size


def _counts_entry(name, env, kernel, top_k=50):
    def run(ctx):
        nat, corpus = native_of("A"), tgx.NativeCorpus(*estep_batch())
        try:
            return run_counts(nat, corpus, top_k)
        finally:
            corpus.free()
            nat.free()

    def check(out):
        check_counts(out, "A", top_k)
        assert kernel in out["_after_tokens"], out["_after_tokens"]

    _add(name, ("tgx_count_tokens", "tgx_count_pairs", "tgx_count_pairs_top"), run, check, env)


_counts_entry("counts_histogram", {}, "ids_histogram_kernel")
_counts_entry("counts_sort", {"TGX_FREQ_SORT": "1"}, "ids_sort+rle")


# ---- sampling, n-best, lattice statistics -----------------------------------------------------------------------------------
SAMPLE_ALPHA, SAMPLE_SEED, NBEST_K = 0.5, 0x5EED5A3B1E, 4


def lattice_texts():
    """the whole corpus: under A every sample has a path (the checkers walk its ~29 KB in Python, once)"""
    return pass_texts()


def lattice_batch():
    return pass_batch()


@functools.lru_cache(maxsize=None)
def _incoming(name):
    import sample_checker as sc
    ml = max(map(len, vocab(name)[0]))
    return [sc.incoming(oracle_of(name), t, ml) for t in lattice_texts()]


@functools.lru_cache(maxsize=None)
def sample_reference(name):
    import sample_checker as sc
    scores = vocab(name)[1]
    return [sc.check_sample(inc, scores, len(t), SAMPLE_ALPHA, SAMPLE_SEED, i) for i, (inc, t) in enumerate(zip(_incoming(name), lattice_texts()))]


@functools.lru_cache(maxsize=None)
def logz_truth(name, alpha):
    om = orc.OracleModel(vocab(name)[0], alpha * vocab(name)[1])
    return np.array([om.marginal_ext(t)[1] for t in lattice_texts()])


def check_sample(out, name):
    """the gates of test_sample_gpu.py::test_ids_match_the_checker"""
    want = sample_reference(name)
    rows, logz = _rows(out["ids"], out["offs"]), out["logz"]
    truth = logz_truth(name, SAMPLE_ALPHA)
    lens = np.array([len(t) for t in lattice_texts()], np.float64)
    if "sample_rows_kernel" in out["_kernels"]:
        bound = 1e-13 * np.maximum(1.0, np.abs(truth))
    else:
        assert "sample_kernel" in out["_kernels"], out["_kernels"]
        bound = 64.0 * np.sqrt(np.maximum(lens, 1.0)) * 2.0 ** -52 * np.abs(truth) + 1e-13
    assert np.all(np.abs(logz - truth) <= bound)
    close = 0
    for i, w in enumerate(want):
        assert abs(logz[i] - w["logz"]) <= 1e-9 * max(1.0, abs(w["logz"])), (i, logz[i], w["logz"])
        if rows[i] != w["ids"]:
            assert w["gap"] < 1e-6, (i, w["gap"])
            close += 1
    assert close < 0.01 * len(want), close


def run_sample(nat, corpus):
    """corpus: a NativeCorpus, or None for the batch form"""
    if corpus is None:
        res, logz = nat.encode_batch_sample_flat(*lattice_batch(), SAMPLE_ALPHA, SAMPLE_SEED, return_logz=True)
    else:
        res, logz = nat.encode_corpus_sample(corpus, SAMPLE_ALPHA, SAMPLE_SEED, return_logz=True)
    out = {"logz": np.array(logz)}
    _take_result(res, out)
    out["_kernels"] = sorted(nat.last_kernel_times())
    return out


def _sample_entry(path, kernel):
    def run(ctx):
        nat, corpus = native_of("A"), tgx.NativeCorpus(*lattice_batch())
        try:
            a, b = run_sample(nat, corpus), run_sample(nat, None)
            a.update({"batch_" + k: v for k, v in b.items() if not k.startswith("_")})
            return a
        finally:
            corpus.free()
            nat.free()

    def check(out):
        other = {"sample_rows_kernel": "sample_kernel", "sample_kernel": "sample_rows_kernel"}[kernel]
        assert kernel in out["_kernels"] and other not in out["_kernels"], out["_kernels"]
        check_sample(out, "A")
        for k in ("ids", "offs", "logz"):
            _eq(out["batch_" + k], out[k], "the batch form is the corpus form: " + k)

    _add("sample_" + path, ("tgx_encode_corpus_sample", "tgx_encode_batch_sample"), run, check, {"TGX_SAMPLE_PATH": path})


_sample_entry("rows", "sample_rows_kernel")
_sample_entry("generic", "sample_kernel")


@functools.lru_cache(maxsize=None)
def nbest_reference(name, k):
    import nbest_checker as nc
    scores = vocab(name)[1]
    return [nc.nbest(inc, scores, len(t), k) for inc, t in zip(_incoming(name), lattice_texts())]


def check_nbest(out, name, k):
    """test_nbest_gpu.py::test_against_the_checker: rows and scores ==, -inf and empty rows past n_found"""
    rows, scores, nf = _rows(out["ids"], out["offs"]), out["scores"], out["n_found"]
    want = nbest_reference(name, k)
    assert len(rows) == k * len(want)
    for i, (wr, ws) in enumerate(want):
        assert nf[i] == min(k, len(wr)), i
        for r in range(k):
            if r < nf[i]:
                assert rows[i * k + r] == wr[r] and scores[i * k + r] == ws[r], (i, r)
            else:
                assert rows[i * k + r] == [] and scores[i * k + r] == -math.inf, (i, r)


def timed_launches(nat):
    """the names of tgx_last_kernel_times in launch order, repeats kept: a chunked pass times every chunk's kernels"""
    import ctypes as C
    names, ms = (C.c_char_p * 8)(), (C.c_float * 8)()
    return [names[i].decode() for i in range(_lib.lib.tgx_last_kernel_times(nat._h, names, ms, 8))]


def run_nbest(nat, corpus, k=NBEST_K):
    res, scores, nf = nat.encode_batch_nbest_flat(*lattice_batch(), k) if corpus is None else nat.encode_corpus_nbest(corpus, k)
    out = {"scores": np.array(scores), "n_found": np.array(nf)}
    _take_result(res, out)
    out["_kernels"] = sorted(nat.last_kernel_times())
    out["_launches"] = timed_launches(nat)
    return out


def _run_nbest_corpus(ctx):
    nat, corpus = native_of("A"), tgx.NativeCorpus(*lattice_batch())
    try:
        return run_nbest(nat, corpus)
    finally:
        corpus.free()
        nat.free()


def _run_nbest_batch(ctx):
    nat = native_of("A")
    try:
        return run_nbest(nat, None, 8)
    finally:
        nat.free()


def _check_nbest(out):
    assert out["_launches"].count("nbest_kernel") == 1, out["_launches"]
    check_nbest(out, "A", NBEST_K)


def _check_nbest_batch(out):
    # TGX_NBEST_CHUNK_MB=1, the knob's smallest value: at k = 8 the batch does not fit one chunk's scratch
    assert out["_launches"].count("nbest_kernel") == 2, out["_launches"]
    check_nbest(out, "A", 8)


_add("nbest_corpus", ("tgx_encode_corpus_nbest",), _run_nbest_corpus, _check_nbest)
_add("nbest_batch_two_chunks", ("tgx_encode_batch_nbest",), _run_nbest_batch, _check_nbest_batch, {"TGX_NBEST_CHUNK_MB": "1"})


STATS_ALPHA = 1.0


@functools.lru_cache(maxsize=None)
def stats_truth(name, alpha):
    """test_stats_gpu.py::_truth_of: log Z, expected score and expected tokens per sample in 80-bit arithmetic"""
    toks, scores = vocab(name)
    om = orc.OracleModel(toks, alpha * scores)
    res = [om.marginal_ext(t) for t in lattice_texts()]
    return (np.array([z for _, z in res]), np.array([float(np.dot(e, scores)) for e, _ in res]), np.array([float(e.sum()) for e, _ in res]),
            np.array([len(t) for t in lattice_texts()], np.float64))


def check_stats(out, name, alpha, rows):
    """test_stats_gpu.py::_assert_truth off the shared case list: rows 1e-10 max(1, |truth|), generic stats_cases.twin_bound"""
    import stats_cases as sx
    z, es, et, n = stats_truth(name, alpha)
    zb = sx.logz_bound(rows, n, z)
    if rows:
        eb, tb = sx.ROWS_RTOL * np.maximum(1.0, np.abs(es)), sx.ROWS_RTOL * np.maximum(1.0, np.abs(et))
    else:
        eb, tb = sx.twin_bound(n, z, es), sx.twin_bound(n, z, et)
    assert int(out["no_path"][0]) == 0
    assert np.all(np.abs(out["logz"] - z) <= zb) and np.all(np.abs(out["escore"] - es) <= eb) and np.all(np.abs(out["etokens"] - et) <= tb)


def run_stats(nat, corpus, alpha=STATS_ALPHA):
    st = nat.lattice_stats_flat(*lattice_batch(), alpha) if corpus is None else nat.lattice_stats_corpus(corpus, alpha)
    return {"logz": st.logz, "escore": st.expected_score, "etokens": st.expected_tokens, "no_path": np.array([st.n_no_path], np.uint64),
            "_kernels": sorted(nat.last_kernel_times())}


def _stats_entry(path, kernel):
    def run(ctx):
        nat, corpus = native_of("A"), tgx.NativeCorpus(*lattice_batch())
        try:
            a, b = run_stats(nat, corpus), run_stats(nat, None)
            a.update({"batch_" + k: v for k, v in b.items() if not k.startswith("_")})
            return a
        finally:
            corpus.free()
            nat.free()

    def check(out):
        other = {"stats_rows_kernel": "stats_kernel", "stats_kernel": "stats_rows_kernel"}[kernel]
        assert kernel in out["_kernels"] and other not in out["_kernels"], out["_kernels"]
        check_stats(out, "A", STATS_ALPHA, path == "rows")
        for k in ("logz", "escore", "etokens"):
            assert np.array_equal(out["batch_" + k].view(np.uint64), out[k].view(np.uint64)), k

    _add("lattice_stats_" + path, ("tgx_lattice_stats_corpus", "tgx_lattice_stats_batch"), run, check, {"TGX_STATS_PATH": path})


_stats_entry("rows", "stats_rows_kernel")
_stats_entry("generic", "stats_kernel")


# ---- the tiny vocabularies of test_top_table_gpu.py ---------------------------------------------------------------------------
def _tiny_entry(top):
    from test_top_table_gpu import TINY_TEXTS, TINY_VOCABS

    def run(ctx):
        out = {}
        for name in sorted(TINY_VOCABS):
            nat = tgx.NativeModel(*TINY_VOCABS[name])
            for k, texts in enumerate(TINY_TEXTS[name]):
                f, o = tgx.pack(texts)
                try:
                    _take_result(nat.encode_batch_flat(f, o), out, f"{name}/{k}/")
                except tgx.TokenGeeXError as e:
                    out[f"{name}/{k}/error"] = np.array([e.status, e.sample], np.int64)
                    out[f"_{name}/{k}/message"] = str(e)
            out[f"_{name}/top"] = nat.last_encode_top_table()
            nat.free()
        return out

    def check(out):
        for name in sorted(TINY_VOCABS):
            ora = orc.OracleModel(*TINY_VOCABS[name])
            for k, texts in enumerate(TINY_TEXTS[name]):
                f, o = tgx.pack(texts)
                try:
                    ids, offs = ora.encode_batch_flat(f, o)
                except orc.NoPath as want:
                    assert out[f"{name}/{k}/error"].tolist() == [_lib.ERR_NO_PATH, want.sample] and out[f"_{name}/{k}/message"] == str(want)
                    continue
                _eq(out[f"{name}/{k}/offs"], offs, (name, k))
                _eq(out[f"{name}/{k}/ids"], ids, (name, k))
            assert out[f"_{name}/top"] == (top == "1")

    _add("encode_tiny_vocabularies_top" + top, ("tgx_encode_batch",), run, check, {"TGX_PATH": "rows5", "TGX_E5_TOP": top})


_tiny_entry("1")
_tiny_entry("0")


# ---- the document-frequency pass (csrc/generate.hip: an allocator of its own) ---------------------------------------------------
def _df_entry():
    import generate_cases as gc
    names, mtl = ("utf8", "gaps", "one_part_over_three_blocks", "last_part_ends_at_513"), 7

    def table(c, pos, ln, df):
        text = c["text"]
        got = {text[int(p):int(p) + int(l)]: int(d) for p, l, d in zip(pos, ln, df)}
        assert len(got) == pos.size
        return got

    def run(ctx):
        out = {}
        for name in names:
            c = gc.case(name)
            flat, pb, pe, ps, po = gc.arrays(c)
            for prob, seed in ((1.0, 0), (0.3, 9)):
                pos, ln, df, n_windows = _lib.substring_df(flat, pb, pe, ps, mtl, prob, seed, part_origin=po)
                t = table(c, pos, ln, df)
                keys = sorted(t)
                out[f"{name}/{prob}/strings"] = np.frombuffer(b"\x00".join(keys), np.uint8).copy()
                out[f"{name}/{prob}/df"] = np.array([t[k] for k in keys] + [n_windows], np.int64)
                out[f"_{name}/{prob}"] = (t, n_windows)
            want, _ = gc.brute_force(c["text"], c["parts"], c["origin"], mtl)
            for kind, k in gc.top_ks(want).items():
                pos, ln, df, n_windows, n_distinct, cutoff = _lib.substring_df_top(flat, pb, pe, ps, mtl, k, part_origin=po)
                out[f"{name}/top/{kind}"] = np.array(df.tolist() + [n_windows, n_distinct, cutoff], np.int64)
                out[f"_{name}/top/{kind}"] = table(c, pos, ln, df)
        return out

    def check(out):
        for name in names:
            c = gc.case(name)
            for prob, seed in ((1.0, 0), (0.3, 9)):
                assert out[f"_{name}/{prob}"] == gc.brute_force(c["text"], c["parts"], c["origin"], mtl, prob, seed), (name, prob)
            want, want_windows = gc.brute_force(c["text"], c["parts"], c["origin"], mtl)
            for kind, k in gc.top_ks(want).items():
                got = out[f"{name}/top/{kind}"]
                df, (n_windows, n_distinct, cutoff) = got[:-3].tolist(), got[-3:].tolist()
                top, cut = gc.top_expectation(want, k)
                assert (n_distinct, n_windows, cutoff) == (len(want), want_windows, cut), (name, kind)
                assert sorted(df, reverse=True) == top and (k >= len(want) or df == top), (name, kind)
                assert all(want.get(sub) == d for sub, d in out[f"_{name}/top/{kind}"].items()), (name, kind)

    _add("substring_df", ("tgx_substring_df", "tgx_substring_df_top"), run, check)


_df_entry()


# ======================================================================================================================
# calls on a caller's stream: results, texts, corpora
# ======================================================================================================================
PAD, POISON = 7, -77
SEED = 0xC0FFEE1234567890


def _pattern_ids(n_out, V=1000):
    """rows of tests/past_cap.py's pattern that sum to n_out ids"""
    import past_cap
    offs = past_cap.edge_offsets(n_out)
    return (np.arange(n_out, dtype=np.uint64) * 7 % V).astype(np.uint32), offs


ID_SIZES = (0, 1, 5, 1023, 1025)   # of past_cap.edge_sizes(4, 1024): none, one, a slot and one over, a tile less one and one over


def _run_layouts(ctx):
    """pad, pack and windows of pattern rows at the edges of a slot and a tile; from_ids and lengths on the way"""
    out = {}
    for n in ID_SIZES:
        ids, offs = _pattern_ids(n)
        S = offs.size - 1
        res = _lib.NativeResult.from_ids(ids, offs, 1000)
        lens = ctx.full((S,), "int64", POISON)
        res.lengths_device(lens.data_ptr(), stream=ctx.stream)
        out[f"{n}/lengths"] = _np(lens)
        mx, n_stream = res.layout_info(1, 2)
        out[f"{n}/info"] = np.array([mx, n_stream], np.uint64)
        L = 5
        ids_t, mask, ln = ctx.full((S, L), "int32", POISON), ctx.full((S, L), "uint8", 9), ctx.full((S,), "int32", POISON)
        nt = res.pad_device(L, PAD, ids_t.data_ptr(), mask_ptr=mask.data_ptr(), lengths_ptr=ln.data_ptr(), bos_id=1, eos_id=2, stream=ctx.stream)
        out[f"{n}/pad"], out[f"{n}/pad_mask"], out[f"{n}/pad_len"], out[f"{n}/pad_nt"] = _np(ids_t), _np(mask), _np(ln), np.array([nt])
        B = n_stream   # blocks of one element: B·L is the stream's length
        if B:
            p_ids, doc, pos = (ctx.full((B, 1), "int32", POISON) for _ in range(3))
            assert res.pack_device(1, PAD, p_ids.data_ptr(), doc_ptr=doc.data_ptr(), pos_ptr=pos.data_ptr(), bos_id=1, eos_id=2, stream=ctx.stream) == B
            out[f"{n}/pack"], out[f"{n}/pack_doc"], out[f"{n}/pack_pos"] = _np(p_ids), _np(doc), _np(pos)
        W = res.window_info(4, 1, bos_id=1)
        out[f"{n}/W"] = np.array([W], np.uint64)
        if W:
            w_ids, w_mask = ctx.full((W, 4), "int32", POISON), ctx.full((W, 4), "uint8", 9)
            i32 = [ctx.full((W,), "int32", POISON) for _ in range(3)]
            res.window_pad_device(4, 1, PAD, W, w_ids.data_ptr(), mask_ptr=w_mask.data_ptr(), lengths_ptr=i32[0].data_ptr(), window_row_ptr=i32[1].data_ptr(),
                                  window_first_ptr=i32[2].data_ptr(), bos_id=1, stream=ctx.stream)
            for k, t in zip(("win", "win_mask", "win_len", "win_row", "win_first"), [w_ids, w_mask] + i32):
                out[f"{n}/{k}"] = _np(t)
        import ctypes as C
        T = res.num_tokens   # the accessors that copy into the handle's own host arrays, then the ones that copy into the caller's
        out[f"{n}/own_ids"] = np.ctypeslib.as_array(C.cast(_lib.lib.tgx_result_ids(res._h), C.POINTER(C.c_uint32)), shape=(max(T, 1),))[:T].copy()
        out[f"{n}/own_offs"] = np.ctypeslib.as_array(C.cast(_lib.lib.tgx_result_offsets(res._h), C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
        _take_result(res, out, f"{n}/src_")
    return out


def _check_layouts(out):
    import layout_checker as lc
    import windows_checker as wc
    for n in ID_SIZES:
        ids, offs = _pattern_ids(n)
        S = offs.size - 1
        _eq(out[f"{n}/src_ids"], ids, "from_ids round-trips")
        _eq(out[f"{n}/src_offs"], offs, "from_ids round-trips")
        _eq(out[f"{n}/own_ids"], ids, "tgx_result_ids")
        _eq(out[f"{n}/own_offs"], offs, "tgx_result_offsets")
        _eq(out[f"{n}/lengths"], np.diff(offs.astype(np.int64)), "lengths")
        lens = np.diff(offs.astype(np.int64))
        assert out[f"{n}/info"].tolist() == [(int(lens.max()) if S else 0) + 2, n + 2 * S]
        w_out, w_mask, w_len, w_nt = lc.padded(ids, offs, 5, PAD, 1, 2)
        _eq(out[f"{n}/pad"], w_out, "pad")
        _eq(out[f"{n}/pad_mask"], w_mask, "pad mask")
        _eq(out[f"{n}/pad_len"], w_len, "pad lengths")
        assert int(out[f"{n}/pad_nt"][0]) == w_nt
        if n + 2 * S:
            for got, want in zip(("pack", "pack_doc", "pack_pos"), lc.packed(ids, offs, 1, PAD, 1, 2)):
                _eq(out[f"{n}/{got}"], want, got)
        assert int(out[f"{n}/W"][0]) == wc.n_windows(offs, 4, 1, 1, None)
        if int(out[f"{n}/W"][0]):
            for got, want in zip(("win", "win_mask", "win_len", "win_row", "win_first"), wc.windows(ids, offs, 4, 1, PAD, 1, None)):
                _eq(out[f"{n}/{got}"], want, got)


_add("layouts_pad_pack_windows", ("tgx_result_from_ids", "tgx_result_lengths_device", "tgx_result_layout_info", "tgx_result_pad_device",
                                  "tgx_result_pack_device", "tgx_result_window_info", "tgx_result_window_pad_device", "tgx_result_ids", "tgx_result_offsets",
                                  "tgx_result_copy_ids", "tgx_result_copy_offsets"), _run_layouts, _check_layouts)


# ---- spans, decode, assemble over one-byte tokens and a few special tokens ------------------------------------------------------
BYTE_TOKENS = [bytes([b]) for b in range(256)]
SPECIALS = [b"<s>", b"", b"\xff<bad\x80>", "<|é|>".encode()]


def _byte_model():
    return tgx.NativeModel(BYTE_TOKENS, np.full(256, -1.0))


def _special_ids(n):
    """pattern rows over byte ids with every fifth id a special token"""
    ids, offs = _pattern_ids(n, 256)
    ids = ids.copy()
    ids[::5] = 256 + (np.arange(ids[::5].size) % len(SPECIALS)).astype(np.uint32)
    return ids, offs


def _run_spans_decode(ctx):
    out = {}
    nat = _byte_model()
    sf, so = _lib.pack(SPECIALS)
    for n in ID_SIZES:
        ids, offs = _special_ids(n)
        S = offs.size - 1
        res = _lib.NativeResult.from_ids(ids, offs, 256 + len(SPECIALS))
        for unit in ("byte", "char"):
            spans = ctx.full((max(n, 1), 2), "int32", POISON)
            nat.result_spans(res, sf, so, spans.data_ptr(), flags=_lib.span_flags(unit, np.int32), stream=ctx.stream)
            out[f"{n}/{unit}/spans"] = _np(spans)[:n]
            L = 5
            padded = ctx.full((S, L, 2), "int32", POISON)
            nat.result_pad_spans(res, sf, so, L, padded.data_ptr(), bos_id=1, flags=_lib.span_flags(unit, np.int32), stream=ctx.stream)
            out[f"{n}/{unit}/pad_spans"] = _np(padded)
        W = res.window_info(4, 1, bos_id=1)
        if W:
            ws = ctx.full((W, 4, 2), "int32", POISON)
            res.window_spans_device(nat, sf, so, 4, 1, W, ws.data_ptr(), bos_id=1, flags=_lib.span_flags("char", np.int32), stream=ctx.stream)
            out[f"{n}/win_spans"] = _np(ws)
        for inc in (False, True):
            _take_text(nat.decode_result(res, sf, so, inc, stream=ctx.stream), out, f"{n}/{int(inc)}/text_")
        # the padded form: what pad_device gives, decoded with the mask and with the lengths
        L = 5
        ids_t, mask, ln = ctx.full((S, L), "int32", POISON), ctx.full((S, L), "uint8", 9), ctx.full((S,), "int32", POISON)
        res.pad_device(L, PAD, ids_t.data_ptr(), mask_ptr=mask.data_ptr(), lengths_ptr=ln.data_ptr(), stream=ctx.stream)
        out[f"_{n}/padded"] = (_np(ids_t), _np(mask), _np(ln))
        _take_text(nat.decode_padded(ids_t.data_ptr(), S, L, False, mask_ptr=mask.data_ptr(), special_flat=sf, special_offs=so, stream=ctx.stream), out,
                   f"{n}/masked_")
        _take_text(nat.decode_padded(ids_t.data_ptr(), S, L, False, lengths_ptr=ln.data_ptr(), special_flat=sf, special_offs=so, stream=ctx.stream), out,
                   f"{n}/lengths_")
        res.free()
    nat.free()
    return out


def _same_text(out, key, want, what):
    """a NativeText's outputs against decode_checker's (bytes, offsets, n_replaced)"""
    _eq(out[key + "offs"], want[1], what)
    _eq(out[key + "bytes"], want[0], what)
    assert int(out[key + "replaced"][0]) == want[2], what


def _check_spans_decode(out):
    import decode_checker as dc
    import spans_checker as sc
    import windows_checker as wc
    lookup = sc.vocab_lookup(BYTE_TOKENS, SPECIALS)
    for n in ID_SIZES:
        ids, offs = _special_ids(n)
        rows = _rows(ids, offs)
        for unit in ("byte", "char"):
            flat = sc.flat(ids, offs, lookup, unit, np.int32)
            _eq(out[f"{n}/{unit}/spans"], flat, (n, unit, "spans"))
            _eq(out[f"{n}/{unit}/pad_spans"], sc.padded(ids, offs, lookup, unit, 5, 1, None, dtype=np.int32, flat_spans=flat), (n, unit, "padded spans"))
        if f"{n}/win_spans" in out:
            _eq(out[f"{n}/win_spans"], wc.window_spans(offs, sc.flat(ids, offs, lookup, "char", np.int64), 4, 1, 1, None, dtype=np.int32), (n, "window spans"))
        for inc in (False, True):
            _same_text(out, f"{n}/{int(inc)}/text_", dc.decode_rows(rows, BYTE_TOKENS, SPECIALS, inc), (n, inc))
        p_ids, p_mask, p_len = out[f"_{n}/padded"]
        for key, kw in (("masked_", dict(mask=p_mask)), ("lengths_", dict(lengths=p_len))):
            _same_text(out, f"{n}/{key}", dc.decode_padded(p_ids, BYTE_TOKENS, SPECIALS, True, **kw), (n, key))


_add("spans_and_decode", ("tgx_result_spans_device", "tgx_result_pad_spans_device", "tgx_result_window_spans_device", "tgx_decode_result",
                          "tgx_decode_padded", "tgx_text_copy_bytes", "tgx_text_copy_offsets"), _run_spans_decode, _check_spans_decode)


def _assemble_case(n):
    """test_assemble_gpu.py::_pattern_rows_against_the_twin: a pattern row is a segment, every third one-id row a special token"""
    import past_cap
    lens = past_cap.edge_lengths(n)
    ones = np.flatnonzero(lens == 1)
    ss = np.full(lens.size, -1, np.int32)
    ss[ones[::3]] = np.arange(ones[::3].size) % len(SPECIALS)
    enc = lens[ss < 0]
    oo = np.concatenate([np.zeros(1, np.uint64), np.cumsum(enc, dtype=np.uint64)])
    ids = (np.arange(int(oo[-1]), dtype=np.uint64) * 7 % 256).astype(np.uint32)
    seg_offs = np.unique(np.append(np.arange(0, lens.size, 5), lens.size)).astype(np.uint64)
    return seg_offs, ss, ids, oo


def _run_assemble(ctx):
    out = {}
    nat = _byte_model()
    for n in ID_SIZES:
        seg_offs, ss, ids, oo = _assemble_case(n)
        segs = _lib.NativeResult.from_ids(ids, oo, 256)
        _take_result(nat.assemble(segs, seg_offs, ss, len(SPECIALS)), out, f"{n}/")
        segs.free()
    nat.free()
    return out


def _check_assemble(out):
    import assemble_checker as ac
    for n in ID_SIZES:
        seg_offs, ss, ids, oo = _assemble_case(n)
        want_ids, want_offs = ac.assemble(ids, oo, seg_offs, ss, 256)
        _eq(out[f"{n}/offs"], want_offs, (n, "offsets"))
        _eq(out[f"{n}/ids"], want_ids, (n, "ids"))


_add("assemble_result", ("tgx_assemble_result",), _run_assemble, _check_assemble)


# ---- the front end of a resident corpus: split at special tokens, the plan assembled from HBM, normalisation --------------------
def _front_cases():
    """the first case of each of front_cases' groups (a group's cases differ in a length by one)"""
    import front_cases as fc
    seen, out = set(), []
    for name, samples, specials in fc.fixed_cases():
        group = name.rstrip("0123456789").rstrip("_")
        if group not in seen and sum(map(len, samples)) < 64 << 10:
            seen.add(group)
            out.append((name, samples, specials))
    return out


def _run_front(ctx):
    out = {}
    nat = _byte_model()
    for name, samples, specials in _front_cases():
        for crlf in (False, True):
            key = f"{name}/{int(crlf)}/"
            corpus = tgx.NativeCorpus(*tgx.pack(list(samples)))
            segs, plan = corpus.split_specials(list(specials), crlf)
            out[key + "seg_offs"], out[key + "seg_special"] = plan.seg_offs(), plan.seg_special()
            out[key + "bytes"], out[key + "offs"] = segs.bytes(), segs.offsets()
            enc = nat.encode_corpus(segs) if plan.num_encoded else None
            _take_result(nat.assemble_plan(enc, plan, len(specials)), out, key + "assembled_")
            for h in (enc, segs, plan, corpus):
                if h is not None:
                    h.free()
    nat.free()
    return out


def _check_front(out):
    import assemble_checker as ac
    import front_cases as fc
    for name, samples, specials in _front_cases():
        for crlf in (False, True):
            key = f"{name}/{int(crlf)}/"
            flat, offs = tgx.pack(list(samples))
            seg_offs, ss, pflat, poffs = fc.truth_flat(flat, offs, list(specials), crlf)
            for k, want in (("seg_offs", seg_offs), ("seg_special", ss), ("bytes", pflat), ("offs", poffs)):
                _eq(out[key + k], want, (name, crlf, k))
            want_ids, want_offs = ac.assemble(pflat.astype(np.uint32), poffs, seg_offs, ss, 256)   # (one-byte tokens: a segment's ids are its bytes)
            _eq(out[key + "assembled_offs"], want_offs, (name, crlf))
            _eq(out[key + "assembled_ids"], want_ids, (name, crlf))


_add("split_specials_and_plan", ("tgx_corpus_split_specials", "tgx_assemble_result_plan", "tgx_encode_corpus", "tgx_plan_copy", "tgx_corpus_copy_text",
                                 "tgx_corpus_copy_offsets"), _run_front, _check_front)


def _norm_rows():
    import norm_cases as nc
    return list(nc.edge_batch()) + list(nc.INVALID) + list(nc.mixed_rows())


def _run_normalize(ctx):
    import norm_cases as nc
    out = {}
    flat, offs = tgx.pack(_norm_rows())
    for form in nc.FORMS:
        corpus = tgx.NativeCorpus(flat, offs)
        got = corpus.normalize(form)
        out[form + "/bytes"], out[form + "/offs"], out[form + "/pieces"] = got.bytes(), got.offsets(), np.array([got.n_pieces], np.uint64)
        got.free()
        corpus.free()
    # a corpus without pieces is a device-to-device copy
    plain = tgx.NativeCorpus(*tgx.pack([b"plain", b"", b"ascii rows"]))
    got = plain.normalize("nfc")
    out["plain/bytes"], out["plain/offs"], out["plain/pieces"] = got.bytes(), got.offsets(), np.array([got.n_pieces], np.uint64)
    got.free()
    plain.free()
    return out


def _check_normalize(out):
    import norm_cases as nc
    rows = _norm_rows()
    flat, offs = tgx.pack(rows)
    for form in nc.FORMS:
        want_f, want_o = nc.truth(form, rows)
        _eq(out[form + "/offs"], want_o, form)
        _eq(out[form + "/bytes"], want_f, form)
        twin_f, twin_o, twin_k = _lib.normalize_host_twin(form, flat, offs)
        _eq(out[form + "/bytes"], twin_f, form)
        assert int(out[form + "/pieces"][0]) == twin_k > 20
    pf, po = tgx.pack([b"plain", b"", b"ascii rows"])
    _eq(out["plain/bytes"], pf, "copy")
    _eq(out["plain/offs"], po, "copy")
    assert int(out["plain/pieces"][0]) == 0


_add("corpus_normalize", ("tgx_corpus_normalize",), _run_normalize, _check_normalize)


# ---- fill-in-the-middle, select, shuffled rows ---------------------------------------------------------------------------------
FIM_BATCHES = (0, 4, 8, 13)   # of fim_cases: rates 0 / .5 / 1 and T' at a tile's edge, one less, one over


def _run_fim(ctx):
    import fim_cases
    out = {}
    for k in FIM_BATCHES:
        case = fim_cases.batch(k)
        src = _lib.NativeResult.from_ids(case["ids"], case["offs"], case["vocab_size"])
        res, mode, cuts = src.fim(case["pre"], case["suf"], case["mid"], return_info=True, stream=ctx.stream, **fim_cases.args(case))
        out[f"{k}/vocab"], out[f"{k}/mode"], out[f"{k}/cuts"] = np.array([res.vocab_size], np.uint64), mode, cuts
        _take_result(res, out, f"{k}/")
        src.free()
    return out


def _check_fim(out):
    import fim_cases
    import fim_checker as fc
    for k in FIM_BATCHES:
        case = fim_cases.batch(k)
        want = fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case))
        for got, w, name in zip((out[f"{k}/ids"], out[f"{k}/offs"], int(out[f"{k}/vocab"][0]), out[f"{k}/mode"], out[f"{k}/cuts"]), want,
                                ("ids", "offsets", "vocab_size", "mode", "cuts")):
            assert np.array_equal(got, w), (k, name)
        assert int(out[f"{k}/offs"][-1]) == case["want_total"]


_add("result_fim", ("tgx_result_fim",), _run_fim, _check_fim)

SELECT_BATCHES = tuple(range(6))   # one of each index pattern


def _select_entry(kind, device_rows):
    import select_cases

    def make(case):
        return _lib.NativeResult.from_ids(case["data"], case["offs"], case["vocab_size"]) if kind == "ids" else tgx.NativeCorpus(case["data"], case["offs"])

    def run(ctx):
        out = {}
        for k in SELECT_BATCHES:
            case = select_cases.batch(k, kind)
            src = make(case)
            rows = ctx.dev(case["rows"]) if device_rows else case["rows"]
            got = src.select(rows, stream=ctx.stream)
            out[f"{k}/data"], out[f"{k}/offs"] = (got.ids() if kind == "ids" else got.bytes()), got.offsets()
            got.free()
            src.free()
        return out

    def check(out):
        import select_checker
        for k in SELECT_BATCHES:
            case = select_cases.batch(k, kind)
            want_d, want_o = select_checker.select(case["data"], case["offs"], case["rows"])
            _eq(out[f"{k}/offs"], want_o, (k, "offsets"))
            _eq(out[f"{k}/data"], want_d, (k, "data"))
            assert int(want_o[-1]) == case["want_total"]

    _add(f"select_{kind}_{'device' if device_rows else 'host'}_rows", ("tgx_result_select" if kind == "ids" else "tgx_corpus_select",), run, check)


for _kind in ("ids", "bytes"):
    for _dev_rows in (False, True):
        _select_entry(_kind, _dev_rows)


def _run_shuffled(ctx):
    out = {}
    for n in (1, 255, 256, 257, 70_000):
        rows = ctx.full((n,), "int64", POISON)
        _lib.shuffled_rows_device(0, n, SEED, rows.data_ptr(), stream=ctx.stream)
        out[str(n)] = _np(rows)
    return out


def _check_shuffled(out):
    import select_checker
    for n in (1, 255, 256, 257, 70_000):
        _eq(out[str(n)], select_checker.shuffled_rows(n, SEED), n)


_add("shuffled_rows", ("tgx_shuffled_rows_device",), _run_shuffled, _check_shuffled)


# ---- exact and near duplicates, shared and repeated n-grams, text statistics ------------------------------------------------------
def make_source(kind, data, offs, V=1000):
    return _lib.NativeResult.from_ids(data, offs, V) if kind == "ids" else tgx.NativeCorpus(data, offs)


DEDUP_CASES = ("lengths", "tile_edges", "alignments", "pairs")


def _dedup_case(name, kind):
    import dedup_cases
    return dedup_cases.past_cap_case(kind) if name == "past_cap" else dedup_cases.case(name, kind)


def _dedup_entry(kind, names, env, suffix=""):
    def run(ctx):
        out = {}
        for name in names:
            c = _dedup_case(name, kind)
            src = make_source(kind, c["data"], c["offs"], c.get("vocab_size", 1000))
            S = src.num_samples
            first = ctx.full((S,), "int64", -5)
            out[f"{name}/unique"] = np.array([src.first_equal(first.data_ptr(), stream=ctx.stream)], np.uint64)
            out[f"{name}/first"] = _np(first)
            hashes = ctx.full((S,), "int64", -5)
            src.row_hashes(hashes.data_ptr(), SEED, stream=ctx.stream)
            out[f"{name}/hashes"] = _np(hashes).view(np.uint64)
            src.free()
        return out

    def check(out):
        import dedup_checker as dc
        for name in names:
            c = _dedup_case(name, kind)
            want_first, want_unique = _ref(("dedup", kind, name), lambda: dc.first_equal(c["data"], c["offs"]))
            _eq(out[f"{name}/first"], want_first, (name, "first"))
            assert int(out[f"{name}/unique"][0]) == want_unique
            _eq(out[f"{name}/hashes"], _ref(("hashes", kind, name), lambda: dc.row_hashes(c["data"], c["offs"], SEED)), (name, "hashes"))

    fn = "result" if kind == "ids" else "corpus"
    _add(f"dedup_{kind}{suffix}", (f"tgx_{fn}_first_equal_device", f"tgx_{fn}_row_hashes_device"), run, check, env)


for _kind in ("ids", "bytes"):
    _dedup_entry(_kind, DEDUP_CASES, {})
    _dedup_entry(_kind, ("pairs", "lengths"), {"TGX_DEDUP_HASH_BITS": "4"}, "_colliding_keys")   # the rounds go on: compare, resolve, the lists
    _dedup_entry(_kind, ("past_cap",), {}, "_past_cap")   # dedup_hash_kernel carries sums between a block's tiles


def _minhash_entry(kind, names, suffix=""):
    import minhash_cases

    def case(name):
        return minhash_cases.past_cap_case(kind) if name == "past_cap" else minhash_cases.case(name, kind)

    def run(ctx):
        out = {}
        for name in names:
            c = case(name)
            src = make_source(kind, c["data"], c["offs"], c.get("vocab_size", 1000))
            S, K = src.num_samples, c["n_perm"]
            sig = ctx.full((S, K), "int32", POISON)
            src.minhash(sig.data_ptr(), c["width"], K, SEED, stream=ctx.stream)
            out[f"{name}/sig"] = _np(sig).view(np.uint32)
            if name != "past_cap":
                bands = c["bands"][0]
                keys, heads, first = ctx.full((S, bands), "int64", -5), ctx.full((S, bands), "int64", -5), ctx.full((S,), "int64", -5)
                _lib.minhash_bands(0, sig.data_ptr(), S, K, bands, 3, keys.data_ptr(), heads.data_ptr(), stream=ctx.stream)
                n_clusters = _lib.minhash_near_first(0, sig.data_ptr(), S, K, heads.data_ptr(), bands, (K + 1) // 2, first.data_ptr(), stream=ctx.stream)
                out[f"{name}/keys"], out[f"{name}/heads"], out[f"{name}/first"] = _np(keys).view(np.uint64), _np(heads), _np(first)
                out[f"{name}/clusters"] = np.array([n_clusters], np.uint64)
            src.free()
        return out

    def check(out):
        import minhash_checker as mc
        for name in names:
            c = case(name)
            K = c["n_perm"]
            want_sig = _ref(("minhash", kind, name), lambda: mc.signatures(c["data"], c["offs"], c["width"], K, SEED))
            _eq(out[f"{name}/sig"], want_sig, (name, "signatures"))
            if name != "past_cap":
                bands = c["bands"][0]
                want_keys = mc.band_keys(want_sig, bands, 3)
                want_heads = mc.heads_of(want_keys)
                want_first, want_clusters, _ = mc.near_first(want_sig, want_heads, (K + 1) // 2)
                _eq(out[f"{name}/keys"], want_keys, (name, "band keys"))
                _eq(out[f"{name}/heads"], want_heads, (name, "heads"))
                _eq(out[f"{name}/first"], want_first, (name, "near first"))
                assert int(out[f"{name}/clusters"][0]) == want_clusters

    fn = "result" if kind == "ids" else "corpus"
    covers = (f"tgx_{fn}_minhash_device",) + (("tgx_minhash_bands_device", "tgx_minhash_near_first_device") if names != ("past_cap",) else ())
    _add(f"minhash_{kind}{suffix}", covers, run, check)


MINHASH_CASES = ("short_w5", "edges_chunk", "edges_tile", "edges_four_tiles")
for _kind in ("ids", "bytes"):
    _minhash_entry(_kind, MINHASH_CASES)
    _minhash_entry(_kind, ("past_cap",), "_past_cap")   # minhash_sig_kernel keeps running minima between a block's tiles

GRAM_CASES = ("short_w5", "edges_chunk", "edges_tile", "edges_two_tiles")


def _gram_entry(kind, with_mask, names=GRAM_CASES, suffix=""):
    import gram_cases

    def case(name):
        return _ref(("gram case", kind, name), lambda: gram_cases.past_cap_case(kind) if name == "past_cap" else gram_cases.case(name, kind))

    def run(ctx):
        out = {}
        for name in names:
            c = case(name)
            w = c["width"]
            src, ev = make_source(kind, c["data"], c["offs"], gram_cases.V), make_source(kind, c["eval_data"], c["eval_offs"], gram_cases.V)
            gs = ev.gram_set(w, SEED, stream=ctx.stream)
            out[f"{name}/keys"] = gs.keys()
            again = _lib.NativeGramSet.from_keys(np.concatenate([out[f"{name}/keys"][::-1], out[f"{name}/keys"][:3]]), w, kind, SEED)
            out[f"{name}/keys_again"] = again.keys()
            S, N = len(c["offs"]) - 1, c["data"].size
            count, mask = ctx.full((S,), "int64", -7), ctx.full((max(N, 1),), "uint8", 7)
            src.gram_hits(again, count.data_ptr(), mask.data_ptr() if with_mask and N else 0, stream=ctx.stream)
            out[f"{name}/count"], out[f"{name}/mask"] = _np(count), _np(mask)[:N]
            for h in (gs, again, src, ev):
                h.free()
        return out

    def check(out):
        import gram_checker as gc
        for name in names:
            c = case(name)
            w = c["width"]
            keys = _ref(("gram keys", kind, name), lambda: gc.keys_of(c["eval_data"], c["eval_offs"], w, SEED))
            _eq(out[f"{name}/keys"], keys, (name, "keys"))
            _eq(out[f"{name}/keys_again"], keys, (name, "from_keys sorts and drops duplicates"))
            want_count, want_mask = _ref(("gram hits", kind, name), lambda: gc.hits(c["data"], c["offs"], w, SEED, keys))
            _eq(out[f"{name}/count"], want_count, (name, "count"))
            if with_mask:
                _eq(out[f"{name}/mask"], want_mask, (name, "mask"))
            else:
                assert (out[f"{name}/mask"] == 7).all()

    fn = "result" if kind == "ids" else "corpus"
    _add(f"gram_{kind}_{'with' if with_mask else 'without'}_mask{suffix}", (f"tgx_{fn}_gramset_create", "tgx_gramset_create_from_keys", f"tgx_{fn}_gram_hits_device", "tgx_gramset_keys"),
         run, check)


for _kind in ("ids", "bytes"):
    for _mask in (True, False):
        _gram_entry(_kind, _mask)
    _gram_entry(_kind, True, ("past_cap",), "_past_cap")   # gram_walk gallops from the owners of the tile before; two blocks add to one count


def _repeat_entry(kind, with_mask, names, suffix=""):
    """with_mask: the caller's mask is the flag array; without one the flags are pooled scratch (launch_repeat_preset's memset)"""
    import repeat_cases
    w = 5

    def case(name):
        return repeat_cases.past_cap_case(kind, w) if name == "past_cap" else repeat_cases.case(name, kind, w)

    def run(ctx):
        out = {}
        for name in names:
            c = case(name)
            src = make_source(kind, c["data"], c["offs"])
            S, N = len(c["offs"]) - 1, c["data"].size
            stats, mask = ctx.full((6, S), "int64", -7), ctx.full((max(N, 1),), "uint8", 7)
            src.repeat_stats(w, SEED, stats.data_ptr(), mask.data_ptr() if with_mask and N else 0, stream=ctx.stream)
            out[f"{name}/stats"], out[f"{name}/mask"] = _np(stats), _np(mask)[:N]
            src.free()
        return out

    def check(out):
        import repeat_checker as rc
        for name in names:
            c = case(name)
            want_stats, want_mask = _ref(("repeat", kind, name), lambda: rc.stats(c["data"], c["offs"], w))
            _eq(out[f"{name}/stats"], want_stats, (name, "stats"))
            if with_mask:
                _eq(out[f"{name}/mask"], want_mask, (name, "mask"))
            else:
                assert (out[f"{name}/mask"] == 7).all()

    fn = "result" if kind == "ids" else "corpus"
    _add(f"repeat_stats_{kind}_{'with' if with_mask else 'without'}_mask{suffix}", (f"tgx_{fn}_repeat_stats_device",), run, check)


REPEAT_CASES = ("short", "period3", "reach", "row_end", "edges_chunk", "edges_tile", "edges_two_tiles")
for _kind in ("ids", "bytes"):
    for _mask in (True, False):
        _repeat_entry(_kind, _mask, REPEAT_CASES)
_repeat_entry("bytes", False, ("past_cap",), "_past_cap")   # repeat_cover_kernel's window reaches a chunk back, across a block's tiles

TEXTSTAT_CASES = ("short_rows", "nl_at_chunk_edges", "limit_lines", "edges_chunk", "edges_tile", "edges_two_tiles", "empty_rows")


def _textstat_entry(with_marks, names, suffix=""):
    import textstat_cases

    def case(name):
        return textstat_cases.past_cap_case() if name == "past_cap" else textstat_cases.case(name)

    def run(ctx):
        out = {}
        for name in names:
            c = case(name)
            corpus = tgx.NativeCorpus(c["text"], c["offs"])
            S, N = len(c["offs"]) - 1, c["text"].size
            table, marks = ctx.full((11, S), "int64", -7), ctx.full((max(N, 1),), "uint8", 7)
            corpus.text_stats(table.data_ptr(), marks.data_ptr() if with_marks and N else 0, 5, "char", stream=ctx.stream)
            out[f"{name}/table"], out[f"{name}/marks"] = _np(table), _np(marks)[:N]
            lines = corpus.lines(stream=ctx.stream)
            out[f"{name}/line_offs"], out[f"{name}/line_bytes"] = lines.offsets(), lines.bytes()
            lines.free()
            corpus.free()
        return out

    def check(out):
        import textstat_checker as tc
        for name in names:
            c = case(name)
            want, want_marks = _ref(("textstat", name), lambda: tc.stats_of(c["text"], c["offs"], 5, "char"))
            _eq(out[f"{name}/table"], want, (name, "table"))
            if with_marks:
                _eq(out[f"{name}/marks"], want_marks, (name, "line starts"))
            else:
                assert (out[f"{name}/marks"] == 7).all()
            _eq(out[f"{name}/line_offs"], _ref(("lines", name), lambda: tc.lines_of(c["text"], c["offs"])[0]), (name, "lines"))
            _eq(out[f"{name}/line_bytes"], c["text"], (name, "the lines' bytes"))

    _add(f"text_stats_{'with' if with_marks else 'without'}_line_starts{suffix}", ("tgx_corpus_text_stats_device", "tgx_corpus_lines"), run, check)


_textstat_entry(True, TEXTSTAT_CASES)
_textstat_entry(False, TEXTSTAT_CASES)
_textstat_entry(True, ("past_cap",), "_past_cap")   # textstat_kernel carries a line across a block's tiles


# ---- a decoded text as a corpus ------------------------------------------------------------------------------------------------
def _run_from_text(ctx):
    out = {}
    nat = _byte_model()
    sf, so = _lib.pack(SPECIALS)
    ids, offs = _special_ids(1025)
    res = _lib.NativeResult.from_ids(ids, offs, 256 + len(SPECIALS))
    text = nat.decode_result(res, sf, so, True, stream=ctx.stream)
    corpus = text.to_corpus()
    out["bytes"], out["offs"] = corpus.bytes(), corpus.offsets()
    _take_result(nat.encode_corpus(corpus), out, "encoded_")   # and the corpus is one: an encode reads its padded text
    _take_text(text, out, "text_")
    corpus.free()
    res.free()
    nat.free()
    return out


def _check_from_text(out):
    import decode_checker as dc
    ids, offs = _special_ids(1025)
    want = dc.decode_rows(_rows(ids, offs), BYTE_TOKENS, SPECIALS, True)
    flat, o = want[0], want[1]
    _same_text(out, "text_", want, "the text")
    _eq(out["bytes"], flat, "the corpus's bytes")
    _eq(out["offs"], o, "the corpus's offsets")
    _eq(out["encoded_ids"], flat.astype(np.uint32), "one-byte tokens: the ids are the bytes")
    _eq(out["encoded_offs"], o, "encoded offsets")


_add("corpus_from_text", ("tgx_corpus_from_text", "tgx_decode_result", "tgx_encode_corpus"), _run_from_text, _check_from_text)
