"""Re-runs one case of tests/measure/fuzz_gpu.py (seed, case) and prints the E-step's expected count of a token under
several kernel choices next to the oracle's and the truth's (orc_estep_ext).  usage: fuzz_case.py SEED CASE TOKEN_ID"""
import os, sys
os.environ["TGX_KNOBS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import tokengeex_amd as tgx
from oracle import oracle as orc

from fuzz_cases import make_case
seed0, case, tok = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
c = make_case(seed0, case)
toks, scores, flat, offs, sd = c["toks"], c["scores"], c["flat"], c["offs"], c["seed"]
d = c["estep_dropout"]
ora = orc.OracleModel(toks, scores)
corpus = tgx.NativeCorpus(flat, offs)
print("token", tok, toks[tok], scores[tok], "dropout", d, "samples", len(c["texts"]), "longest", max(c["lens"]))
for snip in (81920, 4096):
    st, want, wz, _ = ora.estep_flat(flat, offs, snip, d, sd, threads=8)
    _, truth, tz, _ = ora.estep_ext_flat(flat, offs, snip, d, sd, threads=8)
    print(f"snip={snip} oracle           {want[tok]:.12f}  logz {wz:.6f}")
    print(f"snip={snip} truth (80-bit)   {truth[tok]:.12f}  logz {tz:.6f}")
    for env in ({}, {"TGX_ESTEP_PIECES": "1", "TGX_ESTEP_WINDOW": "512"}, {"TGX_ESTEP_PIECES": "0"}, {"TGX_ESTEP": "log"}, {"TGX_PATH": "fused"}):
        for k in ("TGX_ESTEP_PIECES", "TGX_ESTEP_WINDOW", "TGX_ESTEP", "TGX_PATH"):
            os.environ.pop(k, None)
        os.environ.update(env)
        nat = tgx.NativeModel(toks, scores, for_estep=True)
        got, gz = nat.estep(corpus, snip, d, sd)
        bad = np.nonzero(~np.isclose(got, want, rtol=1.2e-8, atol=1e-12))[0]
        tbad = np.nonzero(~np.isclose(got, truth, rtol=1e-10, atol=1e-13))[0]
        print(f"snip={snip} {str(env):52s} {got[tok]:.12f}  logz {gz:.6f}  kernels {sorted(nat.last_kernel_times())}  "
              f"tokens beyond rtol 1.2e-8 of the oracle: {bad.size}, beyond 1e-10 of the truth: {tbad.size}")
