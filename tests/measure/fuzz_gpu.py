"""Randomised differential run of the GPU paths against the CPU oracle (not part of the pytest suite: run it
on the GPU box, `python tests/measure/fuzz_gpu.py [cases] [seed]`).  Every case (tests/fuzz_cases.make_case) draws a
vocabulary shape (max token length 1..40, with or without full byte cover, duplicate and tied scores), a batch shape
(empty and 1-byte samples, lengths around the 16/32/64 block boundaries, a few long ones), dropout, and the kernel
variant knobs (positions per lane); encode ids must be bit-identical.  The E-step is gated two-sided against the truth
(orc_estep_ext, 80-bit): a case fails when a kernel misses it (util.estep_gate: 1e-10 for the linear-domain kernels,
rtol_for for the log-domain ones); the f64 oracle's own distance from the truth is printed and summarised, not treated
as a kernel failure.  The passes covered are encode and the E-step; sampling, n-best and the lattice statistics are run
by tests/measure/fuzz_lattice_gpu.py over tests/lattice_fuzz_cases.make_case."""
import os, sys, time
os.environ["TGX_KNOBS"] = "1"  # the library honours its kernel switches only in processes that opt in
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import tokengeex_amd as tgx
from oracle import oracle as orc

from fuzz_cases import SWITCHES, make_case
from util import estep_gate, rtol_for

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t0 = time.time()
worst = {}        # (family, snippet length) -> [largest kernel-to-truth, largest oracle-to-truth]
oracle_beyond = 0  # E-step passes where the f64 oracle itself is beyond rtol_for from the truth
for case in range(cases):
    c = make_case(seed0, case)
    toks, scores, texts, lens, flat, offs, dropout, sd = (c[k] for k in ("toks", "scores", "texts", "lens", "flat", "offs", "dropout", "seed"))
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(c["env"])
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    e = c["env"]
    tag = (f"case {case} max_len={c['max_len']} all_bytes={c['all_bytes']} V={len(toks)} S={len(texts)} N={flat.size} dropout={dropout} "
           f"env={e.get('TGX_PPL')}/{e.get('TGX_EPPL')}/{e.get('TGX_PATH')}/{e.get('TGX_LONG_THRESHOLD')}/{e.get('TGX_E5_HOT')}/{e.get('TGX_E6_POOL')}/"
           f"{e.get('TGX_ESTEP_PIECES')}/{e.get('TGX_ESTEP_WINDOW')}/{e.get('TGX_CORUN')} r4={e.get('TGX_TRACE_CARRY')}/{e.get('TGX_E7_HOT')}/"
           f"{e.get('TGX_E7_WAVES')}/{e.get('TGX_E7_RANK')}/{e.get('TGX_E7_OVF_AT')}/{e.get('TGX_ESTEP')}")
    try:
        want_ids, want_offs = ora.encode_batch_flat(flat, offs, dropout, sd, threads=8)
        want_err = None
    except orc.NoPath as ex:
        want_err = ex
    try:
        res = nat.encode_batch_flat(flat, offs, dropout, sd)
        got_ids, got_offs = res.ids(), res.offsets(); res.free()
        got_err = None
    except tgx.TokenGeeXError as ex:
        got_err = ex
    if (want_err is None) != (got_err is None):
        print("MISMATCH (error)", tag, want_err, got_err); sys.exit(1)
    if want_err is None and not (np.array_equal(got_ids, want_ids) and np.array_equal(got_offs, want_offs)):
        print("MISMATCH (ids)", tag, nat.last_kernel_times()); sys.exit(1)
    if want_err is None and dropout == 0.0 and case % 4 == 0:  # the host-to-host entry point, in small chunks
        os.environ["TGX_E2E_CHUNK_MB"] = "1"
        hi, ho = nat.encode_batch_host(flat, offs)
        if not (np.array_equal(hi, want_ids) and np.array_equal(ho, want_offs)):
            print("MISMATCH (host-to-host)", tag); sys.exit(1)
    # E-step on the same batch (every byte must be coverable for z to be normal: skip otherwise)
    if c["all_bytes"] and flat.size:
        snip, d = c["snip"], c["estep_dropout"]
        corpus = tgx.NativeCorpus(flat, offs)
        got, gz = nat.estep(corpus, snip, d, sd)
        kernels = nat.last_kernel_times()
        st, want, wz, _ = ora.estep_flat(flat, offs, snip, d, sd, threads=8)
        tst, truth, tz, _ = ora.estep_ext_flat(flat, offs, snip, d, sd, threads=8)
        longest = min(snip, max(lens))
        fam, ok, dist = estep_gate(got, gz, kernels, truth, tz, longest)
        big = truth > 1e-9
        odist = float((np.abs(want - truth)[big] / truth[big]).max()) if big.any() else 0.0
        ok = ok and st == tst == orc.OK and np.array_equal(got != 0, truth != 0)
        w = worst.setdefault((fam, snip), [0.0, 0.0])
        w[0], w[1] = max(w[0], dist), max(w[1], odist)
        if odist > rtol_for(longest):
            oracle_beyond += 1
            print(f"note: the f64 oracle is {odist:.3g} from the truth (rtol_for {rtol_for(longest):.3g}) — its own rounding", tag, "snip", snip, flush=True)
        if not ok:
            bad = np.nonzero(~np.isclose(got, truth, rtol=1e-10, atol=1e-13))[0][:5]
            print("MISMATCH (estep vs truth)", tag, "snip", snip, fam, sorted(kernels), bad, got[bad], truth[bad], want[bad], gz, tz, wz); sys.exit(1)
        corpus.free()
    if case % 10 == 9:
        print(f"{case + 1} cases ok, {time.time() - t0:.0f} s", flush=True)
print("all", cases, "cases ok: 0 kernel failures")
for (fam, snip), (kd, od) in sorted(worst.items()):
    print(f"  {fam:6s} snippet {snip:6d}: largest kernel-to-truth {kd:.3g}, oracle-to-truth {od:.3g}")
print(f"  f64 oracle beyond rtol_for from the truth in {oracle_beyond} passes")
