"""tgx_lattice_stats_corpus on bench.py's default workload: the 1 GiB mixed corpus (samples of up to 64 KiB, seed offset
1000) resident as a tgx_corpus, synth.load_spec_vocab(32000).  Prints one JSON line per measurement: the median and the best
of the timed calls (a host clock around a call that ends in a stream synchronise), GB/s of the median and the per-kernel
times of the last call, for the statistics pass at alpha 0.1 and 1.0 on the rows kernel, once on the generic kernel, and for
the sampling pass it replaces (alpha 1.0, rows) as the reference point in the same process.

    python tools/stats_bench.py [--size-mb 1024] [--steps 7] [--warmup 2] [--only stats,sample]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tokengeex_amd as tgx  # noqa: E402
from tokengeex_amd import synth  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated subset of: stats,sample,generic")
    args = ap.parse_args()
    os.environ["TGX_KNOBS"] = "1"  # (read once per process: TGX_STATS_PATH below picks the kernel)
    only = set(filter(None, args.only.split(",")))
    if tgx.device_count() < 1:
        raise SystemExit("stats_bench needs a GPU: no usable HIP device")
    toks, scores, _ = synth.load_spec_vocab(32000)
    flat, offs = synth.make_corpus(args.size_mb << 20, "mixed", max_len=65536, seed_offset=1000)
    corpus = tgx.NativeCorpus(flat, offs)
    model = tgx.NativeModel(toks, scores)
    n = flat.size

    def report(what, times, **kw):
        med = statistics.median(times)
        print(json.dumps({"what": what, "bytes": int(n), "samples": int(offs.size - 1), "median_ms": round(med * 1e3, 3),
                          "best_ms": round(min(times) * 1e3, 3), "steps": len(times), "GBps": round(n / med / 1e9, 2),
                          "kernels_ms": {k: round(v, 3) for k, v in model.last_kernel_times().items()}, **kw}), flush=True)

    if not only or "stats" in only:
        os.environ["TGX_STATS_PATH"] = "rows"
        for alpha in (0.1, 1.0):
            st = model.lattice_stats_corpus(corpus, alpha)
            report("stats", timed(lambda: model.lattice_stats_corpus(corpus, alpha), args.steps, args.warmup), alpha=alpha, path="rows",
                   n_no_path=st.n_no_path, mean_bits_per_byte=round(float(-st.logz.sum() / (n * 0.6931471805599453)), 6),
                   mean_tokens=round(float(st.expected_tokens.mean()), 3), mean_entropy=round(float(st.entropy.mean()), 3))
    if not only or "sample" in only:
        os.environ["TGX_SAMPLE_PATH"] = "rows"
        report("sample", timed(lambda: model.encode_corpus_sample(corpus, 1.0, 7).free(), args.steps, args.warmup), alpha=1.0, path="rows")
    if not only or "generic" in only:
        os.environ["TGX_STATS_PATH"] = "generic"  # the anchor, not fast: one call
        report("stats", timed(lambda: model.lattice_stats_corpus(corpus, 1.0), 1, 0), alpha=1.0, path="generic")


if __name__ == "__main__":
    main()
