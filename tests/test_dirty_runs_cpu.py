"""The registry of tests/dirty_runs.py against include/tgx.h: every function of the ABI is either reached by some entry
(its `covers`) or listed in EXCLUDED with the reason it queues no device work, and never both.  A function added to the
header fails this test until somebody decides which side it is on.  Needs no device: nothing here calls an entry."""
import os
import re

import dirty_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    """the names of the functions include/tgx.h declares or defines, comments taken out first"""
    with open(os.path.join(ROOT, "include", "tgx.h"), encoding="utf-8") as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = set(re.findall(r"\b(tgx_[a-z0-9_]+)\s*\(", text))
    assert len(names) > 150, len(names)
    return names


def covered():
    return {fn for e in dirty_runs.ENTRIES.values() for fn in e.covers}


def test_the_parser_sees_the_abi_the_binding_declares():
    """the ctypes binding lists every exported symbol and checks each at import: the header's functions are those, and
    tgx_dropout_u01, the header's one inline function"""
    from tokengeex_amd import _lib
    assert header_functions() == set(_lib.SYMBOLS) | {"tgx_dropout_u01"}


def test_every_function_is_covered_or_excluded():
    names = header_functions()
    missing = sorted(names - covered() - set(dirty_runs.EXCLUDED))
    assert not missing, f"neither in an entry's covers nor in EXCLUDED: {missing}"


def test_no_function_is_on_both_sides():
    both = sorted(covered() & set(dirty_runs.EXCLUDED))
    assert not both, both


def test_no_entry_names_a_function_the_header_lacks():
    names = header_functions()
    assert not sorted(covered() - names), sorted(covered() - names)
    assert not sorted(set(dirty_runs.EXCLUDED) - names), sorted(set(dirty_runs.EXCLUDED) - names)


def test_every_exclusion_has_a_reason_and_every_entry_its_parts():
    assert all(isinstance(r, str) and r.strip() for r in dirty_runs.EXCLUDED.values())
    for name, e in dirty_runs.ENTRIES.items():
        assert e.name == name and e.covers and callable(e.run) and callable(e.check) and isinstance(e.deterministic, bool), name
        assert all(k.startswith("TGX_") and isinstance(v, str) for k, v in e.env.items()) and "TGX_POOL_FILL" not in e.env, name
