"""encode5_kernel's top table (csrc/top_table.h) and LDS layout (csrc/encode5_layout.h) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a program of its own.

Both headers are host code without a HIP call, so tests/native/top_table_main.cpp builds host-only with
csrc/trie_build.cpp: for small vocabularies (missing single bytes, 1-byte tokens without children, 0x00 and 0xFF in either
place, duplicates, random ones) it compares all 65 536 entries with a brute-force reading of the vocabulary, checks that
remapping both halves of an entry's ranks equals rebuilding the table, and that encode5_max_hot's answer fits while its
answer + 1 does not, for every (waves, positions per lane).  The program runs as a child process: nothing is loaded
into python, and no device is opened."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tokengeex_amd", "csrc")
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_top_table_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    exe = tmp_path / "top_table"
    sources = [os.path.join(CSRC, "trie_build.cpp"), os.path.join(ROOT, "tests", "native", "top_table_main.cpp")]
    built = subprocess.run([hipcc] + FLAGS + sources + ["-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-4000:])
    assert "top table: ok" in ran.stdout
