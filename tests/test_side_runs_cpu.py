"""The registry of tests/side_runs.py against the side headers (every include/tgx_*.h): each function they declare and
include/tgx.h does not is either reached by some entry (its `covers`) or listed in EXCLUDED with the reason it queues
no device work, never both, and the functions that queue device work are on the covers side by name.  Then the entries'
checks themselves, without a device: every entry's twin() gives its output dictionary through the host twins; check
passes it, and fails once one element of any output is changed.  A check that compares nothing does not pass here."""
import glob
import os
import re

import numpy as np
import pytest

from tokengeex_amd import _lib

import side_runs
from test_dirty_runs_cpu import ROOT, header_functions

SIDE_TABLES = ("WORD_SYMBOLS", "WORDS_SYMBOLS", "PHRASE_SYMBOLS", "PATTERN_SYMBOLS", "PATTERN64_SYMBOLS", "REDACT_SYMBOLS", "SHAPE_SYMBOLS",
               "HASHED_SYMBOLS", "FIND_SYMBOLS", "ALLOW_SYMBOLS", "DUPSPAN_SYMBOLS")
# the functions of the side headers that queue device work: moving one of them into EXCLUDED does not pass
DEVICE_CALLS = {
    "tgx_corpus_word_stats_device", "tgx_corpus_words", "tgx_phraseset_create", "tgx_corpus_phrase_hits_device", "tgx_result_phrase_hits_device",
    "tgx_corpus_dfa_hits_device", "tgx_corpus_dfa64_hits_device", "tgx_corpus_dfa_cover_device", "tgx_corpus_redact", "tgx_corpus_shape_hits_device",
    "tgx_corpus_shape_cover_device", "tgx_corpus_hashed_counts_device", "tgx_result_hashed_counts_device", "tgx_corpus_hashed_scores_device",
    "tgx_result_hashed_scores_device", "tgx_corpus_find_device", "tgx_corpus_mine_device", "tgx_substring_df_allow", "tgx_corpus_dup_spans_device",
    "tgx_result_dup_spans_device",
}


def side_header_functions():
    """the functions the side headers declare or define and include/tgx.h does not, comments taken out first"""
    paths = sorted(glob.glob(os.path.join(ROOT, "include", "tgx_*.h")))
    assert len(paths) == len(SIDE_TABLES), paths
    names = set()
    for path in paths:
        with open(path, encoding="utf-8") as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        names |= set(re.findall(r"\b(tgx_[a-z0-9_]+)\s*\(", text))
    return names - header_functions()


def covered():
    return {fn for e in side_runs.ENTRIES.values() for fn in e.covers}


def test_the_parser_sees_what_the_binding_declares():
    tables = set().union(*(getattr(_lib, t) for t in SIDE_TABLES))
    assert side_header_functions() == tables and not tables & set(_lib.SYMBOLS)


def test_every_function_is_covered_or_excluded_and_none_is_both():
    names = side_header_functions()
    missing = sorted(names - covered() - set(side_runs.EXCLUDED))
    assert not missing, f"neither in an entry's covers nor in EXCLUDED: {missing}"
    both = sorted(covered() & set(side_runs.EXCLUDED))
    assert not both, both


def test_no_entry_names_a_function_that_no_side_header_declares():
    names = side_header_functions()
    assert not sorted(covered() - names), sorted(covered() - names)
    assert not sorted(set(side_runs.EXCLUDED) - names), sorted(set(side_runs.EXCLUDED) - names)


def test_the_calls_that_queue_device_work_are_covered():
    assert DEVICE_CALLS <= side_header_functions()
    assert not sorted(DEVICE_CALLS - covered()), sorted(DEVICE_CALLS - covered())
    assert not sorted(DEVICE_CALLS & set(side_runs.EXCLUDED))


def test_every_exclusion_has_a_reason_and_every_entry_its_parts():
    assert all(isinstance(r, str) and r.strip() for r in side_runs.EXCLUDED.values())
    for name, e in side_runs.ENTRIES.items():
        assert e.name == name and e.covers and callable(e.run) and callable(e.check) and callable(e.twin), name
        assert e.deterministic is True and e.env == {} and e.summed == (), name


def _changed(a):
    """a copy with one element changed: the first that is not zero, where there is one"""
    b = np.array(a, copy=True)
    flat = b.reshape(-1)
    nz = np.flatnonzero(flat)
    k = int(nz[0]) if nz.size else 0
    flat[k] = flat[k] ^ flat.dtype.type(1)
    return b


@pytest.mark.parametrize("name", sorted(side_runs.ENTRIES))
def test_check_passes_the_twin_and_fails_at_one_changed_element(name):
    e = side_runs.ENTRIES[name]
    out = e.twin()
    keys = [k for k in out if not k.startswith("_")]
    assert keys and all(isinstance(out[k], np.ndarray) and out[k].size for k in keys), "an output without an element checks nothing"
    assert all(out[k].dtype in (np.int64, np.uint8, np.uint32, np.uint64) for k in keys), "integer work throughout"
    e.check(out)
    for k in keys:
        bad = dict(out)
        bad[k] = _changed(out[k])
        assert not np.array_equal(bad[k], out[k])
        with pytest.raises(AssertionError):
            e.check(bad)
