"""tgx_encode_corpus_nbest on bench.py's mixed corpus (samples of up to 64 KiB, seed offset 1000) resident as a
tgx_corpus, synth.load_spec_vocab(32000).  Prints one JSON line per measurement: GB/s of input and the per-kernel times
of the n-best pass for k in {1, 2, 4, 8, 16}, and of encode as the reference point.

    python tools/nbest_bench.py [--size-mb 256] [--steps 3] [--warmup 1] [--ks 1,2,4,8,16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tokengeex_amd as tgx  # noqa: E402
from tokengeex_amd import synth  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    best = None
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ks", default="1,2,4,8,16")
    args = ap.parse_args()
    toks, scores, _ = synth.load_spec_vocab(32000)
    flat, offs = synth.make_corpus(args.size_mb << 20, "mixed", max_len=65536, seed_offset=1000)
    corpus = tgx.NativeCorpus(flat, offs)
    model = tgx.NativeModel(toks, scores)
    n = flat.size

    def report(what, dt, **kw):
        print(json.dumps({"what": what, "bytes": int(n), "samples": int(offs.size - 1), "best_ms": round(dt * 1e3, 3),
                          "GBps": round(n / dt / 1e9, 3), "kernels_ms": {k: round(v, 3) for k, v in model.last_kernel_times().items()},
                          **kw}), flush=True)

    report("encode", timed(lambda: model.encode_corpus(corpus).free(), args.steps, args.warmup))
    for k in (int(x) for x in args.ks.split(",") if x):
        report("nbest", timed(lambda: model.encode_corpus_nbest(corpus, k)[0].free(), args.steps, args.warmup), k=k)


if __name__ == "__main__":
    main()
