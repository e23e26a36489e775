"""The duplicate-span twin (tgx_dup_spans_host) under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its
own: csrc/host_twins.cpp calls no HIP function, so it builds host-only with tests/native/dupspan_main.cpp and runs as a
child process on heap blocks of exactly the documented sizes.  Nothing is loaded into python, no device is opened."""
import os
import subprocess

import pytest

from test_repeat_native import CSRC, FLAGS, ROOT, _hipcc


def test_dupspan_twin_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    sources = [os.path.join(CSRC, "host_twins.cpp"), os.path.join(ROOT, "tests", "native", "dupspan_main.cpp")]
    built = subprocess.run([hipcc] + FLAGS + sources + ["-o", str(tmp_path / "dupspan")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([str(tmp_path / "dupspan")], capture_output=True, text=True)
    assert ran.returncode == 0 and "dupspan twin: ok" in ran.stdout, (ran.stdout[-1000:], ran.stderr[-4000:])
