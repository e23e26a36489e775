"""SHA-256 digests of what sampling, n-best and the lattice statistics write, over the raw bytes of every output array (not
part of the pytest suite: run it on the GPU box).  It is the bit-for-bit comparison of two builds of the library: run it
once per build and compare the lines,

    python tests/measure/lattice_digest.py [--root TREE] [--size-mb 8] [--cases 160]

where TREE is the checkout whose tokengeex_amd is loaded (this one by default; the cases and the corpus always come from this
one's tests/ and synth).  One line per workload and array, `<workload> <array> <sha256>`:

  * fuzz: the cases of tests/lattice_fuzz_cases.make_case(2, i), each with its own switches, forms and order of the three
    passes as tests/test_lattice_fuzz_gpu.run_case runs them; an array's digest runs over all cases in order, and a call
    that raises contributes its message;
  * corpus: --size-mb MiB of synth's mixed corpus (samples of up to 64 KiB) with the 32 000-token spec vocabulary, through
    sampling and the statistics with the path forced to `rows` and then to `generic`, and through n-best at k = 1, 4, 16.

The arrays: sampling's ids, offsets and log Z; n-best's ids, offsets, scores and n_found; the statistics' log Z, expected
score and expected tokens."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--size-mb", type=int, default=8)
ap.add_argument("--cases", type=int, default=160)
args = ap.parse_args()
os.environ["TGX_KNOBS"] = "1"  # the library honours its kernel switches only in processes that opt in
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.root))  # tokengeex_amd (and its libtgx.so) from TREE

import numpy as np  # noqa: E402

import tokengeex_amd as tgx  # noqa: E402
from tokengeex_amd import synth  # noqa: E402

sys.path.insert(0, HERE)  # everything else, the CPU checkers that draw the cases among it, from this checkout
import lattice_fuzz_cases as lf  # noqa: E402

digests = {}


def add(workload, name, value):
    h = digests.setdefault((workload, name), hashlib.sha256())
    h.update(value.encode() if isinstance(value, str) else np.ascontiguousarray(value).tobytes())


def add_result(workload, prefix, res):
    add(workload, prefix + ".ids", res.ids())
    add(workload, prefix + ".offsets", res.offsets())
    res.free()


def sample(workload, model, c, corpus):
    try:
        if corpus is not None:
            res, z = model.encode_corpus_sample(corpus, c["alpha"], c["seed"], return_logz=True)
        else:
            res, z = model.encode_batch_sample_flat(c["flat"], c["offs"], c["alpha"], c["seed"], return_logz=True)
    except tgx.TokenGeeXError as ex:
        add(workload, "sample.ids", str(ex))
        return
    add_result(workload, "sample", res)
    add(workload, "sample.logz", np.asarray(z))


def nbest(workload, model, c, corpus):
    try:
        res, scores, nf = model.encode_corpus_nbest(corpus, c["k"]) if corpus is not None else model.encode_batch_nbest_flat(c["flat"], c["offs"], c["k"])
    except tgx.TokenGeeXError as ex:
        add(workload, "nbest.ids", str(ex))
        return
    add_result(workload, "nbest", res)
    add(workload, "nbest.scores", np.asarray(scores))
    add(workload, "nbest.n_found", np.asarray(nf))


def stats(workload, model, c, corpus):
    st = model.lattice_stats_corpus(corpus, c["alpha"]) if corpus is not None else model.lattice_stats_flat(c["flat"], c["offs"], c["alpha"])
    add(workload, "stats.logz", np.asarray(st.logz))
    add(workload, "stats.expected_score", np.asarray(st.expected_score))
    add(workload, "stats.expected_tokens", np.asarray(st.expected_tokens))


PASSES = {"sample": sample, "nbest": nbest, "stats": stats}


def switches(env):
    for name in lf.SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(env)


def fuzz_model(c):
    if c["parent"] is None:
        return tgx.NativeModel(c["toks"], c["scores"])
    parent = tgx.NativeModel(c["parent"]["toks"], c["parent"]["scores"])
    child = parent.derive(c["parent"]["keep"], c["scores"])
    parent.free()
    return child


print("tokengeex_amd from", os.path.dirname(os.path.abspath(tgx.__file__)), file=sys.stderr, flush=True)  # (stdout is for diff)
if tgx.device_count() < 1:
    raise SystemExit("lattice_digest needs a GPU: no usable HIP device")

for i in range(args.cases):
    c = lf.make_case(2, i)
    switches(c["env"])
    model = fuzz_model(c)
    for p in c["order"]:
        PASSES[p]("fuzz", model, c, tgx.NativeCorpus(c["flat"], c["offs"]) if c["forms"][p] else None)
    model.free()

toks, scores, _ = synth.load_spec_vocab(32000)
flat, offs = synth.make_corpus(args.size_mb << 20, "mixed", max_len=65536, seed_offset=1000)
corpus = tgx.NativeCorpus(flat, offs)
model = tgx.NativeModel(toks, scores)
for path in ("rows", "generic"):
    switches({"TGX_SAMPLE_PATH": path, "TGX_STATS_PATH": path})
    sample("corpus " + path, model, {"alpha": 1.0, "seed": 7}, corpus)
    stats("corpus " + path, model, {"alpha": 1.0}, corpus)
switches({})
for k in (1, 4, 16):
    nbest(f"corpus k={k}", model, {"k": k}, corpus)

for (workload, name), h in digests.items():
    print(workload, name, h.hexdigest(), flush=True)
