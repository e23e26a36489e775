"""Fill-in-the-middle on the device (csrc/fim.hip) on a resident encode of bench.py's mixed corpus with the spec 32 000
vocabulary: time of NativeResult.fim at rate 0.5 and 1.0 — the whole call, and fim_fill_kernel alone (tgx_fim_last_times) —
beside two things measured in the same run over the same result:

  (a) layout_pack_kernel, i32 ids alone, block length 4096: the same bytes through the same per-tile row search;
  (b) hipMemcpyAsync device-to-device of 4·T' bytes: the floor of a kernel that reads and writes that much.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup.  One JSON line per corpus size.
usage: fim_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

from layout_bench import _hip, d2d, rate, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("fim_bench.py needs a GPU")
    hip = _hip()
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    V = model.vocab_size
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T = res.num_samples, res.num_tokens
        rec = {"corpus_mib": mib, "bytes": int(flat.size), "samples": S, "tokens": T, "mean_row": round(T / S, 1), "steps": args.steps, "runs": []}
        for r in (0.5, 1.0):
            fill, scan = [], []

            def call():
                out = res.fim(V, V + 1, V + 2, rate=r, spm_rate=0.5, seed=1, stream=stream)
                t = _lib.fim_last_times()
                fill.append(t["fim_fill_kernel"])
                scan.append(t["fim_offsets_scan"])
                n = out.num_tokens
                out.free()
                return n
            T2 = call()
            whole = timed(call, args.steps, args.warmup)
            moved = 4 * (T + T2) + 16 * (S + 1)   # ids read and written, both offset arrays read
            k_ms = statistics.median(fill[-args.steps:])
            c = d2d(hip, 4 * T2, args.steps, args.warmup)
            rec["runs"].append({"what": "fim", "rate": r, "out_tokens": T2, "applied": (T2 - T) // 3, "call_ms": whole["ms"], "call_ms_min": whole["ms_min"],
                                "fill_kernel_ms": round(k_ms, 4), "fill_kernel_ms_min": round(min(fill[-args.steps:]), 4),
                                "offsets_scan_ms": round(statistics.median(scan[-args.steps:]), 4), "moved_bytes": moved,
                                "fill_gb_s": rate(moved, k_ms), "d2d_bytes": 4 * T2, "d2d_ms": c["ms"], "d2d_gb_s": rate(8 * T2, c["ms"])})
        # (a) the packed layout of the same result: i32 ids alone
        L = 4096
        B = -(-T // L)
        ids = torch.empty((B, L), dtype=torch.int32, device="cuda")
        t = timed(lambda: tensors.pack_into(res, ids, None, None, block_len=L, pad_id=0), args.steps, args.warmup)
        moved = 4 * T + 4 * B * L + 8 * (S + 1)
        rec["runs"].append({"what": "layout_pack_kernel i32 (call)", "L": L, "call_ms": t["ms"], "call_ms_min": t["ms_min"], "moved_bytes": moved,
                            "gb_s": rate(moved, t["ms"])})
        c = d2d(hip, 4 * T, args.steps, args.warmup)
        rec["runs"].append({"what": "d2d", "bytes": 4 * T, "ms": c["ms"], "gb_s": rate(8 * T, c["ms"])})
        for run in rec["runs"][:2]:
            run["fill_x_pack_call"] = round(run["fill_kernel_ms"] / t["ms"], 2)
            run["fill_x_d2d"] = round(run["fill_kernel_ms"] / run["d2d_ms"], 2)
        print(json.dumps(rec), flush=True)
        del ids
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
