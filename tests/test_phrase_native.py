"""The phrase twin (tgx_phrase_hits_host of include/tgx_phrases.h) under AddressSanitizer and UndefinedBehaviorSanitizer,
as a program of its own.

csrc/host_twins.cpp calls no HIP function, so it builds host-only with tests/native/phrase_main.cpp, which hands the
twin heap blocks of exactly the documented sizes (rows of 0 .. 6 elements, rows that end one to three elements on either
side of a chunk, of a tile and of two tiles, runs of empty rows, a row of about five tiles, no rows; phrases of 1, 2, 3,
9 and the greatest number of elements with duplicates, under every flag combination and every combination of outputs)
and checks every answer against the definition written out plainly.  The program runs as a child process: nothing is
loaded into python, and no device is opened."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tokengeex_amd", "csrc")
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_phrase_twin_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    exe = tmp_path / "phrase"
    sources = [os.path.join(CSRC, "host_twins.cpp"), os.path.join(ROOT, "tests", "native", "phrase_main.cpp")]
    built = subprocess.run([hipcc] + FLAGS + sources + ["-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-4000:])
    assert "phrase twin: ok" in ran.stdout
