"""The table derivation of tgx_model_create_derived (csrc/trie_build.cpp: derive_flat_trie, gather_derived_vocab) under
AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.

The derivation and everything built over a derived table on the host (build_trie8, build_trie8t, build_tok_hash, the
prune alternatives) call no HIP function, so tests/native/derive_main.cpp builds host-only with csrc/trie_build.cpp and
csrc/prune_host.cpp.  The cases are those of tests/derived_cases.py, written to a file this test hands the program: on
every suffix of every text the derived table, the 8-byte and the ranked records built over it, and a table built from
the child's vocabulary give the matches of a brute-force search; chains derive from derived tables.  The program runs
as a child process: nothing is loaded into python, and no device is opened."""
import os
import shutil
import subprocess

import pytest

import derived_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tokengeex_amd", "csrc")
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
NAMES = dc.STRUCTURAL + ("byte_dropped", "keep_one", "keep_none", "scores_past_300", "scores_minus_inf")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_derivation_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    exe = tmp_path / "derive"
    sources = [os.path.join(CSRC, "trie_build.cpp"), os.path.join(CSRC, "prune_host.cpp"), os.path.join(ROOT, "tests", "native", "derive_main.cpp")]
    built = subprocess.run([hipcc] + FLAGS + sources + ["-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    fixture = tmp_path / "cases.bin"
    dc.write_fixture(str(fixture), NAMES)
    n_links = sum(len(dc.case(n)["links"]) for n in NAMES)
    ran = subprocess.run([str(exe), str(fixture)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-4000:])
    assert f"derive: ok ({len(NAMES)} cases, {n_links} derivations)" in ran.stdout
