"""tgx_encode_corpus_sample on bench.py's default workload: the 1 GiB mixed corpus (samples of up to 64 KiB, seed offset
1000) resident as a tgx_corpus, synth.load_spec_vocab(32000).  Prints one JSON line per measurement: GB/s and the
per-kernel times of sampling at alpha 0.1 and 1.0 (both kernels), and of encode and the E-step as the reference points.

    python tools/sample_bench.py [--size-mb 1024] [--steps 5] [--warmup 2]"""
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
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated subset of: encode,estep,sample")
    args = ap.parse_args()
    os.environ["TGX_KNOBS"] = "1"  # (read once per process: TGX_SAMPLE_PATH below picks the kernel)
    only = set(filter(None, args.only.split(",")))
    toks, scores, _ = synth.load_spec_vocab(32000)
    flat, offs = synth.make_corpus(args.size_mb << 20, "mixed", max_len=65536, seed_offset=1000)
    corpus = tgx.NativeCorpus(flat, offs)
    model = tgx.NativeModel(toks, scores)
    n = flat.size

    def report(what, dt, **kw):
        print(json.dumps({"what": what, "bytes": int(n), "samples": int(offs.size - 1), "best_ms": round(dt * 1e3, 3),
                          "GBps": round(n / dt / 1e9, 2), "kernels_ms": {k: round(v, 3) for k, v in model.last_kernel_times().items()},
                          **kw}), flush=True)

    if not only or "encode" in only:
        report("encode", timed(lambda: model.encode_corpus(corpus).free(), args.steps, args.warmup))
    if not only or "estep" in only:
        report("estep", timed(lambda: model.estep(corpus), args.steps, args.warmup))
    if not only or "sample" in only:
        for path in ("rows", "generic"):
            os.environ["TGX_SAMPLE_PATH"] = path
            for alpha in (0.1, 1.0):
                steps, warmup = (args.steps, args.warmup) if path == "rows" else (1, 0)  # the generic kernel is the anchor, not fast
                report("sample", timed(lambda: model.encode_corpus_sample(corpus, alpha, 7).free(), steps, warmup),
                       alpha=alpha, path=path)


if __name__ == "__main__":
    main()
