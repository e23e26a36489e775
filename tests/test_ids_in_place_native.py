"""The host side of "ids in place" (csrc/ids_in_place.h) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a program of its own.

The header is host code without a HIP call, so tests/native/ids_in_place_main.cpp builds host-only: it checks every term
of the decision, the edge of the 24-bit count field (samples of 2^24 - 1 and 2^24 bytes), and one relaxation step's
packed-count arithmetic against a direct count along random winner sequences.  The program runs as a child process:
nothing is loaded into python, and no device is opened."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_ids_in_place_decision_and_count_arithmetic_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    exe = tmp_path / "ids_in_place"
    built = subprocess.run([hipcc] + FLAGS + [os.path.join(ROOT, "tests", "native", "ids_in_place_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-4000:])
    assert "ids in place: ok" in ran.stdout
