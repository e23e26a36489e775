"""Randomised differential run of sampling, n-best and the lattice statistics on the GPU against their checkers (not part
of the pytest suite: run it on the GPU box, `python tests/measure/fuzz_lattice_gpu.py [cases] [seed]`).  Every case
(tests/lattice_fuzz_cases.make_case) draws a vocabulary family (random with and without byte cover, with duplicates, the
hostile families; a derived model in a quarter of the cases), texts (empty batches, lengths around the 16/32/64 block
boundaries, now and then a sample above 64 KiB, samples without a path, a poison sample that trips the range flag), alpha, k,
the three switches TGX_SAMPLE_PATH / TGX_STATS_PATH / TGX_NBEST_CHUNK_MB, and the form and order of the three passes; the
comparison is tests/test_lattice_fuzz_gpu.run_case.  The run stops at the first mismatch with the case's tag and prints the
largest error-to-bound ratio per kernel and quantity at the end.  tests/measure/fuzz_gpu.py is the run of the encode ids and
the E-step counts."""
import os, sys, time
os.environ["TGX_KNOBS"] = "1"  # the library honours its kernel switches only in processes that opt in
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lattice_fuzz_cases as lf
from test_lattice_fuzz_gpu import run_case

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 2
t0 = time.time()
ratios, ran = {}, {}
for case in range(cases):
    c = lf.make_case(seed0, case)
    if c["seed"] is None:  # no case is skipped: the generator is at fault, and the run ends
        print("NO SAMPLING SEED within 8 tries:", lf.tag(c), flush=True)
        sys.exit(1)
    c.update(lf.references(c))
    try:
        run_case(c, ratios)
    except AssertionError as ex:
        print("MISMATCH", ex.args[0] if ex.args else "", flush=True)
        print("  case:", lf.tag(c), flush=True)
        sys.exit(1)
    for p in ("sample", "stats"):
        ran[(p, c["expect"][p])] = ran.get((p, c["expect"][p]), 0) + 1
    if case % 10 == 9:
        print(f"{case + 1} cases ok, {time.time() - t0:.0f} s", flush=True)
print("all", cases, f"cases of seed {seed0} ok: 0 kernel failures, {time.time() - t0:.0f} s")
print("  paths:", {f"{p}:{k}": v for (p, k), v in sorted(ran.items())})
for key, v in sorted(ratios.items()):
    print(f"  {key:28s} largest error / bound {v:.3g}")
