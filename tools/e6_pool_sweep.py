import os, sys
os.environ["TGX_KNOBS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import tokengeex_amd as tgx
from tokengeex_amd import synth
import small_batch_sweep as sb
toks, scores, _ = synth.load_spec_vocab(32000)
models = {"spec32k": tgx.NativeModel(toks, scores), "distinct32k": tgx.NativeModel(toks, scores + np.random.default_rng(5).uniform(-0.4, 0.4, len(toks)))}
cfgs = [dict(TGX_E6_POOL=str(p)) for p in (0, 16, 32, 64, 96, 128, 192, 256)]
for mib in (64, 256):
    flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)
    corpus = tgx.NativeCorpus(flat, offs)
    for name, m in models.items():
        print(f"== {mib} MiB {name}", flush=True)
        sb.run(m, corpus, cfgs)
    corpus.free()
