"""The encode pass's long-sample split (csrc/encode_split.h; encode_pass.cpp: split_long_samples) under AddressSanitizer
and UndefinedBehaviorSanitizer, as a program of its own.

The header is host code without a HIP call, so tests/native/encode_split_main.cpp builds host-only.  It checks the
properties that follow from the function's code (n_long within the batch; a co-run only of a split batch, on fewer CUs than
the device has, with two blocks of encode6_kernel per CU; the forced thresholds and shares; no co-run by estimate after a
timeout or when the values do not fit; an empty batch and a single sample inside their arrays), and it prints its decision
for its built-in batches and the three synth batches at 256 CUs.  Those are compared with RECORDED: what the block of run_encode_kernel that the header
was lifted from (tgx_api.cpp:558-629 at 1d11215) printed for the same batches, copied verbatim into a program outside the
repository — profiles/encode_split/README.md says how.  The program runs as a child process: nothing is loaded into
python, and no device is opened.

The three synth batches are the sample lengths of synth.make_corpus(M << 20, "mixed", seed_offset=1000) for M = 64, 256 and
512, the corpora of tests/test_configs_gpu.py::test_default_decisions_by_batch_size_on_the_spec_vocabulary.  Generating
them takes 1.3 + 3.3 + 6.6 s, so their lengths are committed as tests/golden/encode_split_synth_lengths.npz, made by

    python -c "import numpy as np; from tokengeex_amd import synth; np.savez_compressed('tests/golden/encode_split_synth_lengths.npz', **{'mib%d' % M: np.diff(synth.make_corpus(M << 20, 'mixed', seed_offset=1000)[1].astype(np.int64)).astype(np.uint32) for M in (64, 256, 512)})"
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# (n_long, corun_cus) for (cold6, fit) = (0, 1), (0, 0), (1, 1), (1, 0): cold6 — encode6_kernel's LDS copy does not hold
# every value; fit — every value fits encode5_kernel's LDS at 8 waves x 4 positions per lane
RECORDED = {
    "empty": [(0, 0)] * 4,
    "one_1023": [(0, 0)] * 4,
    "one_1024": [(1, 0)] * 4,
    "one_65536": [(1, 0)] * 4,
    "one_1048576": [(1, 0)] * 4,
    "short_100000x140": [(0, 0)] * 4,
    "short_plus_65536": [(1, 0)] * 4,
    "short_plus_8192_8191": [(2, 0)] * 4,
    "long_64x49152": [(64, 0)] * 4,
    "ladder_1KiB_1MiB_x4": [(44, 0)] * 4,
    # the spec vocabulary of test_configs_gpu.py is the (1, 1) column: 9 652 values, of which encode6_kernel's LDS holds
    # ~4 500 and encode5_kernel's, at 8 waves, all.  There the device test asserts what is recorded here:
    "mib64": [(4229, 0)] * 4,                                      # long samples, no co-run
    "mib256": [(16825, 0), (16825, 0), (1945, 128), (16825, 0)],   # co-run
    "mib512": [(0, 0)] * 4,                                        # encode6_kernel not used
}
VARIANTS = [(0, 1), (0, 0), (1, 1), (1, 0)]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_encode_split_properties_and_recorded_decisions_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([hipcc] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + linked.stderr[-300:])
    exe = tmp_path / "encode_split"
    built = subprocess.run([hipcc] + FLAGS + [os.path.join(ROOT, "tests", "native", "encode_split_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    # the synth batches as files of offsets (raw little-endian u64), named as in RECORDED
    lengths = np.load(os.path.join(ROOT, "tests", "golden", "encode_split_synth_lengths.npz"))
    files = []
    for name in ("mib64", "mib256", "mib512"):
        offs = np.zeros(lengths[name].size + 1, dtype="<u8")
        np.cumsum(lengths[name], dtype=np.uint64, out=offs[1:])
        assert abs(int(offs[-1]) - (int(name[3:]) << 20)) < 70_000
        offs.tofile(tmp_path / name)
        files.append(str(tmp_path / name))
    ran = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-4000:])
    assert "encode split: ok" in ran.stdout
    got = {}
    for line in ran.stdout.splitlines():
        if line.startswith("split "):
            _, name, cold6, fit, n_long, corun = line.split()
            key = (int(cold6.split("=")[1]), int(fit.split("=")[1]))
            got.setdefault(name, {})[key] = (int(n_long.split("=")[1]), int(corun.split("=")[1]))
    assert sorted(got) == sorted(RECORDED)
    for name, want in RECORDED.items():
        assert [got[name][v] for v in VARIANTS] == want, name
