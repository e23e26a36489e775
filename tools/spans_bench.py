"""Token spans on the device (csrc/spans.hip) on a resident encode of bench.py's mixed corpus with the spec 32 000 vocabulary:
times of tensors.spans_into (byte and char unit) and tensors.pad_spans_into at L = 4096 beside two yardsticks measured in
the same run:

  (a) hipMemcpyAsync device-to-device of the output's size: the floor of a kernel that only writes;
  (b) the route a caller had before: NativeResult.ids() + offsets() to the host, a numpy gather of the tokens' lengths and a
      per-row cumulative sum, then the upload of the [T, 2] spans (byte unit).

Times are device events on torch's current stream around the whole call (which returns once the stream has reached its
end), the median of --steps calls after --warmup; (b) is a host clock, one call.  The kernels' shares of a call come from
a separate run under `rocprofv3 --kernel-trace --stats -- python tools/spans_bench.py --no-host` (the kernels run on the
caller's stream, so tgx_last_kernel_times does not see them).
One JSON line per corpus size.   usage: spans_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--dtype int32] [--no-host]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import synth, tensors

from layout_bench import _hip, d2d, rate, timed

ROW_LEN = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="int32", choices=["int32", "int64"])
    ap.add_argument("--no-host", action="store_true", help="skip yardstick (b)")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("spans_bench.py needs a GPU")
    hip = _hip()
    dtype = torch.int32 if args.dtype == "int32" else torch.int64
    el = 4 if args.dtype == "int32" else 8
    toks, scores, _ = synth.load_spec_vocab(32000)
    toks = list(toks)
    model = tgx.NativeModel(toks, np.asarray(scores, np.float64))
    tok_len = np.array([len(t) for t in toks], np.int64)
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T = res.num_samples, res.num_tokens
        out = torch.empty((T, 2), dtype=dtype, device="cuda")
        pout = torch.empty((S, ROW_LEN, 2), dtype=dtype, device="cuda")
        rec = {"corpus_mib": mib, "bytes": int(flat.size), "samples": S, "tokens": T, "mean_row": round(T / S, 1), "dtype": args.dtype,
               "steps": args.steps, "encode_ms": round(sum(model.last_kernel_times().values()), 3)}
        # what a flat call moves per token: the id and its table word in, the value word out and in (the scan; the writer
        # reads it again in the char unit), the 64-bit sum out and in, the pair out; the int32 check reads two sums per row
        flat_moved = {"byte": T * (4 + 2 + 4 + 4 + 8 + 8 + 2 * el), "char": T * (4 + 2 + 4 + 4 + 4 + 8 + 8 + 2 * el)}
        for unit in ("byte", "char"):
            t = timed(lambda: tensors.spans_into(res, model, out, unit=unit), args.steps, args.warmup)
            c = d2d(hip, out.numel() * el, args.steps, args.warmup)
            rec[f"flat_{unit}"] = {**t, "out_bytes": out.numel() * el, "out_gb_s": rate(out.numel() * el, t["ms"]),
                                   "moved_bytes": flat_moved[unit], "moved_gb_s": rate(flat_moved[unit], t["ms"]),
                                   "d2d": {**c, "gb_s": rate(out.numel() * el, c["ms"])}, "x_d2d": round(t["ms"] / c["ms"], 2)}
        t = timed(lambda: tensors.pad_spans_into(res, model, pout, row_len=ROW_LEN, unit="byte"), args.steps, args.warmup)
        c = d2d(hip, pout.numel() * el, args.steps, args.warmup)
        pad_moved = T * (4 + 2 + 4 + 4 + 8) + S * ROW_LEN * 2 * el   # + 8 B of sums per kept token
        rec["padded_byte"] = {**t, "row_len": ROW_LEN, "out_bytes": pout.numel() * el, "out_gb_s": rate(pout.numel() * el, t["ms"]),
                              "moved_bytes_at_least": pad_moved, "d2d": {**c, "gb_s": rate(pout.numel() * el, c["ms"])},
                              "x_d2d": round(t["ms"] / c["ms"], 2)}
        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, oo = res.ids(), res.offsets()
            t1 = time.perf_counter()
            ends = np.cumsum(tok_len[ids])
            row_of = np.repeat(np.arange(S), np.diff(oo.astype(np.int64)))
            base = np.concatenate([[0], ends])[oo[:-1].astype(np.int64)][row_of]
            h = np.empty((T, 2), np.int32 if args.dtype == "int32" else np.int64)
            h[:, 1] = ends - base
            h[:, 0] = h[:, 1] - tok_len[ids]
            t2 = time.perf_counter()
            up = torch.from_numpy(h).to("cuda")
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            tensors.spans_into(res, model, out, unit="byte")
            rec["host_route"] = {"ms": round((t3 - t0) * 1e3, 1), "ms_ids_to_host": round((t1 - t0) * 1e3, 1), "ms_numpy": round((t2 - t1) * 1e3, 1),
                                 "ms_upload": round((t3 - t2) * 1e3, 1), "equal": bool(torch.equal(up, out))}
            rec["x_host_route"] = round((t3 - t0) * 1e3 / rec["flat_byte"]["ms"], 1)
            del ids, oo, ends, row_of, base, h, up
        print(json.dumps(rec), flush=True)
        del out, pout
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
