"""The device decode (csrc/decode.hip) on a resident encode of bench.py's mixed corpus with the spec 32 000 vocabulary: time
of NativeModel.decode_result beside two yardsticks measured in the same run:

  (a) hipMemcpyAsync device-to-device of the same number of output bytes: the floor of a kernel that only writes;
  (b) the route a caller had before: NativeResult.ids() + offsets() to the host, then the host decode (tgx_decode_batch).

Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup; (b) is a host clock, one call.  The kernels' shares of the call come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/decode_bench.py --no-host` (the kernels run on the
caller's stream, so tgx_last_kernel_times does not see them).
One JSON line per corpus size.   usage: decode_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--no-host]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from layout_bench import _hip, d2d, rate, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip yardstick (b)")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("decode_bench.py needs a GPU")
    hip = _hip()
    toks, scores, _ = synth.load_spec_vocab(32000)
    toks = list(toks)
    model = tgx.NativeModel(toks, np.asarray(scores, np.float64))
    vf, vo = _lib.pack(toks)
    sf, so = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T = res.num_samples, res.num_tokens
        stream = torch.cuda.current_stream().cuda_stream
        text = model.decode_result(res, sf, so, True, stream)
        out_bytes, replaced = text.num_bytes, text.num_replaced
        same = bool(np.array_equal(text.bytes(), flat)) and bool(np.array_equal(text.offsets(), offs))
        text.free()

        def call():
            model.decode_result(res, sf, so, True, stream).free()
        t = timed(call, args.steps, args.warmup)
        c = d2d(hip, out_bytes, args.steps, args.warmup)
        # what the call moves: ids read twice (classes, fill), the scanned starts and special counts written and read, the meta
        # words written and read twice, a 16-byte slot per token, the text written once and read once, the flag and code words
        moved = T * (4 + 4 + 4 + 2 * 4 + 2 * 8 + 2 * 8 + 16) + out_bytes * 2 + out_bytes // 16 * (4 + 4 + 4) + 8 * (S + 1) * 2
        rec = {"corpus_mib": mib, "bytes": int(flat.size), "samples": S, "tokens": T, "bytes_per_token": round(flat.size / T, 2),
               "out_bytes": out_bytes, "replaced": replaced, "round_trip_exact": same, "steps": args.steps,
               "encode_ms": round(sum(model.last_kernel_times().values()), 3), "decode": {**t, "out_gb_s": rate(out_bytes, t["ms"])},
               "moved_bytes": moved, "moved_gb_s": rate(moved, t["ms"]),
               "d2d": {**c, "gb_s": rate(out_bytes, c["ms"])}, "x_d2d": round(t["ms"] / c["ms"], 2)}
        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, oo = res.ids(), res.offsets()
            t1 = time.perf_counter()
            h_text, h_offs = _lib.decode_batch_flat(vf, vo, len(toks), sf, so, 0, ids, oo, True)
            t2 = time.perf_counter()
            rec["host_route"] = {"ms": round((t2 - t0) * 1e3, 1), "ms_ids_to_host": round((t1 - t0) * 1e3, 1), "ms_decode_batch": round((t2 - t1) * 1e3, 1),
                                 "threads": len(os.sched_getaffinity(0))}
            rec["x_host_route"] = round((t2 - t0) * 1e3 / t["ms"], 1)
            del ids, oo, h_text, h_offs
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
