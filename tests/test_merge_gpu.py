"""End-to-end `merge` (src/merge.rs:33-134) on the GPU path against the same loop over the oracle's pair scan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tokengeex_amd.merge import ModelVocabularyMerger

from util import AllowByHand, corpus_and_vocab
from test_merge_cpu import ALLOW


def oracle_select(vocab, pairs, budget, rx, scale_factor, max_token_length, ignore):
    """One round's selection (src/merge.rs:84-126) over `pairs` in table order -> the new tokens."""
    new = []
    for k, _ in pairs:
        if len(new) == budget:
            break
        a, b = k >> 32, k & 0xFFFFFFFF
        value = vocab[a][0] + vocab[b][0]
        if len(value) > max_token_length or not rx.search(value.decode("utf-8", errors="replace")):
            ignore.add(k)
            continue
        new.append((value, (vocab[a][1] + vocab[b][1]) * scale_factor, False))
    return new


def oracle_merge(vocab, flat, offs, allow, num_merges, step, scale_factor, max_token_length, head=None, heads=None):
    """The reference loop restated over oracle functions only (checker); ties: ascending (a, b).  The allow
    pattern is evaluated by hand (util.AllowByHand), not through the product's pattern translation.
    head, heads: per round, (merges that the first `head` pairs of the table yield, the round's budget, the table's size)
    is appended to `heads`."""
    assert allow == ALLOW
    rx = AllowByHand()
    vocab, start, ignore = list(vocab), len(vocab), set()
    while len(vocab) < start + num_merges:
        m = orc.OracleModel([t[0] for t in vocab], [t[1] for t in vocab])
        keys, counts = m.count_pairs_flat(flat, offs, threads=8)
        pairs = sorted(zip(keys.tolist(), counts.tolist()), key=lambda kc: (-kc[1], kc[0]))
        budget = min(step, num_merges - (len(vocab) - start))
        if heads is not None:
            heads.append((len(oracle_select(vocab, pairs[:head], budget, rx, scale_factor, max_token_length, set())), budget, len(pairs)))
        new = oracle_select(vocab, pairs, budget, rx, scale_factor, max_token_length, ignore)
        vocab.extend(new)
        merges = budget - len(new)
        if merges == step or merges == budget:
            break
    return vocab


def test_merge_end_to_end_matches_oracle_loop():
    flat, offs, toks, scores = corpus_and_vocab(2 << 20, "mixed", 3000, 12, max_len=16384)
    vocab = [(t, float(s), len(t) == 1) for t, s in zip(toks, scores)]
    merger = ModelVocabularyMerger(ALLOW, num_merges=150, step=40, scale_factor=0.9, max_token_length=20)
    got = merger.merge(vocab, flat, offs)
    want = oracle_merge(vocab, flat, offs, ALLOW, 150, 40, 0.9, 20)
    assert len(got) == len(vocab) + 150 and len(merger.rounds) == 4
    assert got == want                      # same tokens, same order, bit-identical scores
    assert max(len(t[0]) for t in got) > 12  # merged tokens outgrow the 12-byte start; past 16 bytes the model
    # moves from the four-samples-per-wave kernels to the one-sample-per-wave kernel, both are exercised


def test_merge_fetches_the_whole_table_when_the_head_runs_dry():
    """head_pairs = 16 and tokens of at most 6 bytes: the 16 most frequent pairs yield fewer merges than a round may take
    (established on the CPU, by the oracle loop's own selection over the head of the oracle's table), so the merger must
    fetch the whole table (tgx_count_pairs) — the result is the oracle loop's, and the rounds whose head ran dry looked
    at the whole table, the others at the head alone."""
    flat, offs, toks, scores = corpus_and_vocab(512 << 10, "mixed", 2000, 10, max_len=4096)
    vocab = [(t, float(s), len(t) == 1) for t, s in zip(toks, scores)]
    heads = []
    want = oracle_merge(vocab, flat, offs, ALLOW, 30, 12, 0.9, 6, head=16, heads=heads)
    assert len(want) == len(vocab) + 30 and len(heads) == 3
    assert heads[0][0] < heads[0][1] == 12 and all(total > 16 for _, _, total in heads)   # the precondition: round 1 runs dry
    merger = ModelVocabularyMerger(ALLOW, num_merges=30, step=12, scale_factor=0.9, max_token_length=6)
    merger.head_pairs = 16
    got = merger.merge(vocab, flat, offs)
    assert got == want
    assert [r["merged"] for r in merger.rounds] == [12, 12, 6]
    for r, (from_head, budget, total) in zip(merger.rounds, heads):
        assert r["pairs"] == (total if from_head < budget else 16), (r, from_head, budget, total)
    assert any(r["pairs"] > merger.head_pairs for r in merger.rounds)
