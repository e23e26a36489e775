"""The allow filter inside the document-frequency pass on the device (tgx_substring_df_allow: csrc/allow.hip) against the
brute force of tests/generate_cases.py filtered by a plain walk of the automaton (tests/allow_cases.py), and against the
parent pass filtered on the host, row for row.  Exact comparisons."""
import re

import numpy as np
import pytest

from tokengeex_amd import _lib
from tokengeex_amd.generate import VocabularyGenerator

import allow_cases as ac
import generate_cases as gc

pytestmark = pytest.mark.gpu


def _allow(c, which, mtl, top_k=0, prob=1.0, seed=0, **kw):
    flat, pb, pe, ps, po = gc.arrays(c)
    return _lib.substring_df_allow(flat, pb, pe, ps, mtl, top_k, ac.automaton(which), prob, seed, part_origin=po, **kw)


def _table(c, pos, ln, df):
    out = {c["text"][int(p):int(p) + int(l)]: int(d) for p, l, d in zip(pos, ln, df)}
    assert len(out) == len(pos), "a substring came back twice"
    return out


def _rows(pos, ln, df, keep=None):
    rows = sorted(zip(pos.tolist(), ln.tolist(), df.tolist()))
    return rows if keep is None else [r for r in rows if keep(r)]


def _check(c, which, mtl, prob=1.0, seed=0):
    """the table and the window count against the filtered brute force; (pos, len, df) against the parent's rows, filtered"""
    _, want, want_windows = ac.reference(c, which, mtl, prob, seed)
    pos, ln, df, n_windows, n_distinct, cutoff = _allow(c, which, mtl, 0, prob, seed)
    assert _table(c, pos, ln, df) == want and n_windows == want_windows and n_distinct == len(want) and cutoff == 0, (c["name"], mtl)
    flat, pb, pe, ps, po = gc.arrays(c)
    parent = _lib.substring_df(flat, pb, pe, ps, mtl, prob, seed, part_origin=po)
    pat = ac.automaton(which)
    assert _rows(pos, ln, df) == _rows(*parent[:3], keep=lambda r: ac.allows(pat, c["text"][r[0]:r[0] + r[1]])), (c["name"], mtl)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", gc.GEOMETRY_NAMES)
def test_geometry(name, which):
    for mtl in gc.MTLS:
        _check(gc.case(name), which, mtl)


@pytest.mark.parametrize("which", ["A", "B"])
def test_chunk_edges(which):
    for c in ac.chunk_cases():
        _check(c, which, 32)


@pytest.mark.parametrize("which", ["A", "B"])
def test_insert_probability_with_origins(which):
    for lead, gap in ((0, 0), (33, 7), (300, 1)):
        _check(gc.place((0, 1, 2, 3, 4, 5), lead, gap), which, gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED)


@pytest.mark.parametrize("name,mtl,which", [("utf8", 7, "A"), ("sample_ids", 32, "B")])
def test_top_k_is_over_allowed_substrings_only(name, mtl, which):
    c = gc.case(name)
    _, want, want_windows = ac.reference(c, which, mtl)
    for kind, k in gc.top_ks(want).items():
        pos, ln, df, n_windows, n_distinct, cutoff = _allow(c, which, mtl, k)
        top, cut = gc.top_expectation(want, k)
        assert n_distinct == len(want) and n_windows == want_windows and cutoff == cut, (kind, k)
        assert sorted(df.tolist(), reverse=True) == top and (k >= len(want) or df.tolist() == top), (kind, k)
        assert all(want.get(sub) == d for sub, d in _table(c, pos, ln, df).items()), (kind, k)


def test_forced_collisions_give_the_same_counts(monkeypatch):
    monkeypatch.setenv("TGX_KNOBS", "1")
    monkeypatch.setenv("TGX_GENERATE_COLLIDE", "8")
    for name, mtl, which in (("one_part_over_three_blocks", 7, "A"), ("utf8", 5, "B")):
        c = gc.case(name)
        _, want, want_windows = ac.reference(c, which, mtl)
        pos, ln, df, n_windows, _, _, collisions = _allow(c, which, mtl, with_collisions=True)
        assert _table(c, pos, ln, df) == want and n_windows == want_windows and collisions > 0
    monkeypatch.delenv("TGX_GENERATE_COLLIDE")
    pos, ln, df, n_windows, _, _, collisions = _allow(c, which, mtl, with_collisions=True)
    assert _table(c, pos, ln, df) == want and collisions == 0


def test_vocabulary_generator_filters_on_the_device():
    words = ["return", "Return", "x += 1", "if (a != b)", "中文 text", "don't", "  indent", "é", "foo()", "a->b"]
    samples = [" ".join(words[(i + j) % len(words)] for j in range(1 + i % 4)) for i in range(40)]
    exact = re.compile(ac.exact_source())

    def generator(allow, top_k=None):
        gen = VocabularyGenerator(12, 1.0, allow=allow, top_k=top_k)
        gen.feed(samples[:25])
        gen.feed(samples[25:])
        return gen

    parent = {tok: d for tok, d in generator(None).frequencies.items() if exact.fullmatch(tok.encode())}
    assert generator(ac.automaton("B")).frequencies == parent and len(parent) > 30
    cut_parent, cut_device = generator(None, 20), generator(ac.automaton("B"), 20)
    assert cut_parent.frequencies and set(cut_device.frequencies) <= set(parent)  # (reading the frequencies runs the pending pass)
    assert 0 < cut_device._bound_total <= cut_parent._bound_total
