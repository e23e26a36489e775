"""The integer counting passes at their edges: the token histogram (tgx_count_tokens: ids_histogram_kernel, or sort +
run-length encode above 36 864 ids), the pair scan (tgx_count_pairs: pair_keys_kernel, radix sort over 2 shift + 1 bits,
run-length encode, pair_expand_kernel) and its head (tgx_count_pairs_top) on the cases of tests/scan_cases.py.  Every
comparison is == on integers; every expected value is the CPU oracle's ids reduced with numpy (scan_cases.reference), never
device output.  tests/test_scan_cases_cpu.py shows that each case sits on the edge it is named for."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc

import hostile_cases as hc
import scan_cases as sc


@functools.lru_cache(maxsize=None)
def _nat(name: str):
    return tgx.NativeModel(*sc.vocab(name))


def _corpus(name, kind, tail):
    flat, offs, _, _ = sc.corpus(name, kind, tail)
    return tgx.NativeCorpus(flat, offs)


def _same(got, want, what):
    assert got.dtype == want.dtype == np.uint64, what
    np.testing.assert_array_equal(got, want, err_msg=what)


def check_passes(nat, corpus, ref, what, after=lambda nat, pass_name: None):
    """count_tokens, count_pairs and every k of count_pairs_top against the reference; after(nat, pass) runs after each."""
    _same(nat.count_tokens(corpus), ref["freq"], f"{what}: count_tokens")
    after(nat, "tokens")
    keys, counts = nat.count_pairs(corpus)
    after(nat, "pairs")
    _same(keys, ref["keys"], f"{what}: count_pairs keys")
    _same(counts, ref["counts"], f"{what}: count_pairs counts")
    total = int(ref["keys"].size)
    for kind, k in sc.top_ks(ref["top_counts"]).items():
        tk, tc, n_total = nat.count_pairs_top(corpus, k)
        after(nat, "top")
        assert n_total == total, (what, kind, k, n_total, total)
        _same(tk, ref["top_keys"][:k], f"{what}: count_pairs_top({k}) [{kind}] keys")
        _same(tc, ref["top_counts"][:k], f"{what}: count_pairs_top({k}) [{kind}] counts")


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_counts_equal_the_reference(case):
    name, kind, tail = case
    corpus = _corpus(name, kind, tail)
    check_passes(_nat(name), corpus, sc.reference(name, kind, tail), sc.case_id(case))
    corpus.free()


# ---- the histogram / sort crossover -------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.SIZES)
def test_crossover_of_the_frequency_pass(monkeypatch, V):
    """ids_histogram_kernel up to 36 864 ids, sort + run-length encode from 36 865; with TGX_FREQ_SORT=1 the sort path
    gives the same vector below the limit too."""
    name = str(V)
    nat = _nat(name)
    monkeypatch.delenv("TGX_FREQ_SORT", raising=False)
    for kind, tail in (("edges", 1), ("bulk", 3)):
        corpus, ref = _corpus(name, kind, tail), sc.reference(name, kind, tail)
        _same(nat.count_tokens(corpus), ref["freq"], f"V={V} {kind}")
        times = nat.last_kernel_times()
        hist = V <= sc.HIST_MAX_VOCAB
        assert ("ids_histogram_kernel" in times) == hist and ("ids_sort+rle" in times) == (not hist), (V, sorted(times))
        if hist:
            monkeypatch.setenv("TGX_FREQ_SORT", "1")
            _same(nat.count_tokens(corpus), ref["freq"], f"V={V} {kind} TGX_FREQ_SORT=1")
            times = nat.last_kernel_times()
            assert "ids_sort+rle" in times and "ids_histogram_kernel" not in times, sorted(times)
            monkeypatch.delenv("TGX_FREQ_SORT")
        corpus.free()


@pytest.mark.parametrize("V", [36864, 36865])
def test_count_tokens_adds_to_the_callers_vector(V):
    name = str(V)
    nat = _nat(name)
    for kind, tail in (("edges", 3), ("bulk", 1)):
        corpus, ref = _corpus(name, kind, tail), sc.reference(name, kind, tail)
        freq = np.full(V, 1 << 40, np.uint64)
        out = nat.count_tokens(corpus, freq)
        assert out is freq
        _same(freq, ref["freq"] + np.uint64(1 << 40), f"V={V} {kind}")
        corpus.free()


# ---- who wrote the ids that the passes read ---------------------------------------------------------------------------------
MID = "32769"


@pytest.mark.parametrize("switch", ["0", "1"])
def test_ids_written_in_place_or_compacted(monkeypatch, switch):
    """The same counts whether trace_kernel wrote the ids in place (TGX_IDS_IN_PLACE=1: no compact_kernel) or they went
    through the scratch and compact_kernel (=0), and the pass that should have run in place did."""
    monkeypatch.setenv("TGX_LONG_THRESHOLD", "0")  # (a lone long sample of a small batch would go to encode6_kernel: not in place)
    monkeypatch.setenv("TGX_IDS_IN_PLACE", switch)
    nat = _nat(MID)

    def after(nat, pass_name):
        times = nat.last_kernel_times()
        assert nat.last_encode_ids_in_place() == (switch == "1"), (pass_name, sorted(times))
        assert "encode5_kernel" in times and "trace_kernel" in times and ("compact_kernel" in times) == (switch == "0"), (pass_name, sorted(times))

    for kind, tail in (("edges", 1), ("bulk", 2)):
        corpus = _corpus(MID, kind, tail)
        check_passes(nat, corpus, sc.reference(MID, kind, tail), f"V={MID} {kind} TGX_IDS_IN_PLACE={switch}", after)
        corpus.free()


@pytest.mark.parametrize("name,kernels", [("4096+24", ("encode5_kernel", "trace32_kernel", "compact_kernel")), ("4096+40", ("encode_kernel",))])
def test_ids_of_the_long_token_and_the_generic_kernels(name, kernels):
    """grid(4096) and one token of 24 bytes (the LONG build of encode5_kernel, trace32_kernel) or of 40 bytes (the generic
    kernel), which is the largest id and occurs hundreds of times."""
    nat = _nat(name)

    def after(nat, pass_name):
        times = nat.last_kernel_times()
        assert not nat.last_encode_ids_in_place() and all(k in times for k in kernels), (pass_name, sorted(times))

    for tail in (1, 2):
        corpus = _corpus(name, "edges", tail)
        ref = sc.reference(name, "edges", tail)
        assert ref["freq"][4096] > 300
        check_passes(nat, corpus, ref, f"{name} edges tail {tail}", after)
        corpus.free()


# ---- degenerate inputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["513", "36865"])
def test_degenerate_inputs(name):
    nat = _nat(name)
    toks, _ = sc.vocab(name)
    V = len(toks)
    one = toks[V - 1]
    for texts in ([], [b""], [b""] * 5, [one], [one] * 67, [b"", one, b"", b"", one, b""]):  # S = 0; all empty; one token each
        flat, offs = tgx.pack(texts)
        assert offs.size == len(texts) + 1
        ref = sc.reference_of(sc.oracle_model(name), flat, offs, V)
        assert ref["keys"].size == 0 and int(ref["freq"].sum()) == sum(1 for t in texts if t) == int(ref["freq"][V - 1])
        corpus = tgx.NativeCorpus(flat, offs)
        check_passes(nat, corpus, ref, f"V={name} {len(texts)} samples")
        corpus.free()


# ---- refusal ----------------------------------------------------------------------------------------------------------------
def test_a_sample_without_a_path_is_refused_and_nothing_is_counted():
    """A vocabulary without the byte 'q' and one sample that holds it: every pass raises the no-path error with the oracle's
    sample, the caller's frequency vector keeps every byte, and no table comes back."""
    toks, scores = hc.bytes_heavy(-6.0, without=(ord("q"),))
    nat, om = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    flat, offs = tgx.pack([b"sampling the lattice", b"", b"range q fallback", b"lattice" * 30])
    with pytest.raises(orc.NoPath) as want:
        om.encode_batch_flat(flat, offs)
    assert want.value.sample == 2
    corpus = tgx.NativeCorpus(flat, offs)
    freq = np.arange(len(toks), dtype=np.uint64) * np.uint64(0x0101010101) + np.uint64(1 << 40)
    before = freq.tobytes()
    with pytest.raises(tgx.TokenGeeXError) as e:
        nat.count_tokens(corpus, freq)
    assert e.value.status == 4 and e.value.sample == 2 and freq.tobytes() == before
    for call in (lambda: nat.count_pairs(corpus), lambda: nat.count_pairs_top(corpus, 1), lambda: nat.count_pairs_top(corpus, 1000)):
        out = None
        with pytest.raises(tgx.TokenGeeXError) as e:
            out = call()
        assert e.value.status == 4 and e.value.sample == 2 and out is None
    # the same model and corpus object still count a batch that has a path
    good_flat, good_offs = tgx.pack([b"sampling the lattice", b"", b"range fallback", b"lattice" * 30])
    good = tgx.NativeCorpus(good_flat, good_offs)
    check_passes(nat, good, sc.reference_of(om, good_flat, good_offs, len(toks)), "after the refusal")
    good.free()
    corpus.free()
    nat.free()
