"""Word ids on the GPU (tgx_corpus_words; csrc/words.hip) against the host twin and the definition, on the case table of
tests/test_words_cpu.py with and without the fold, and two passes over the result end to end: the repeat statistics and
the gram hits, which then count words.  Everything is compared exactly: this is integer work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from test_words_cpu import NAMES, SEED, case

STAGES = ["words_summary_kernel", "words_scan", "words_kernel", "words_offsets_kernel"]


@pytest.mark.parametrize("fold", (False, True))
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_twin_and_definition(name, fold):
    text, offs, want_ids, want_offs = case(name, fold)
    twin_ids, twin_offs = _lib.words_host(text, offs, fold, SEED)
    corpus = _lib.NativeCorpus(text, offs)
    try:
        res = tgx.word_rows(corpus, fold_case=fold, seed=SEED)
        assert res.vocab_size == 2**31 and res.num_samples == offs.size - 1 and res.num_tokens == want_ids.size
        assert list(_lib.words_last_times()) == STAGES
        ids, out_offs = res.ids(), res.offsets()
        assert np.array_equal(out_offs, want_offs) and np.array_equal(out_offs, twin_offs)
        assert np.array_equal(ids, want_ids) and np.array_equal(ids, twin_ids)
        assert np.array_equal(corpus.bytes(), text) and np.array_equal(corpus.offsets(), offs), "the corpus is only read"
        res.free()
        with pytest.raises(tgx.TokenGeeXError) as e:
            corpus.words(2, SEED)
        assert e.value.status == _lib.ERR_INVALID
    finally:
        corpus.free()


def test_repeat_stats_count_words():
    """a b a b a b x: the 2-grams of words are (a b) three times, (b a) twice and (b x); aa bb aa bb: (aa bb) twice, (bb aa)"""
    corpus = _lib.NativeCorpus(*_lib.pack([b"a b a b a b x", b"", b"aa  bb\taa bb"]))
    try:
        s = tgx.repeat_stats(tgx.word_rows(corpus), 2)
        assert s.top.tolist() == [3, 0, 2] and s.grams.tolist() == [6, 0, 3] and s.elems.tolist() == [7, 0, 4]
    finally:
        corpus.free()


def test_gram_hits_flag_the_row_that_shares_three_words():
    """the three consecutive words of the held-out row, spaced otherwise and, under the fold, cased otherwise"""
    held = _lib.NativeCorpus(*_lib.pack([b"the quick brown fox"]))
    rows = [b"a quick brown dog and the fox", b"see\tThe   QUICK\n\nbrown  cat", b"thequick brown fox.", b"", b"quick brown"]
    corpus = _lib.NativeCorpus(*_lib.pack(rows))
    try:
        for fold, want in ((True, [0, 1, 0, 0, 0]), (False, [0, 0, 0, 0, 0])):
            grams = tgx.gram_set(tgx.word_rows(held, fold_case=fold), 3)
            assert tgx.gram_hits(tgx.word_rows(corpus, fold_case=fold), grams).tolist() == want
    finally:
        held.free()
        corpus.free()
