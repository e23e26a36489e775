"""Overflow windows on the device (csrc/layout.hip: layout_window_kernel) on a resident encode of bench.py's mixed corpus
with the spec 32 000 vocabulary, at L = 512 and stride = 64 with bos and eos, beside two yardsticks measured in the same run:

  (a) tensors.pad_into (layout_pad_kernel, which this change does not touch) on the same result at the row length that
      gives about the same number of output elements: the same stores without the search for a window's row;
  (b) the route a caller had before: NativeResult.ids() + offsets() to the host, tgx_layout_windows_host there, and the
      upload of ids, mask and the window-to-sample mapping.

A window call is the count kernel, the scan over the S rows, the read-back of W and the fill kernel; `window_info` alone
is all of that but the fill, so `fill_ms` = call - info is the fill kernel's time as the caller sees it.  The kernels' own
times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/windows_bench.py --no-host`.
Times are device events on torch's current stream around the whole call (which returns once the stream has reached its
end), the median of --steps calls after --warmup; (b) is a host clock, one call.
One JSON line per corpus size.   usage: windows_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--dtype int32] [--no-host]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

from layout_bench import rate, timed

PAD, BOS, EOS = 0, 1, 2
ROW_LEN, STRIDE = 512, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="int32", choices=["int32", "int64"])
    ap.add_argument("--no-host", action="store_true", help="skip yardstick (b)")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("windows_bench.py needs a GPU")
    dtype, np_dtype = (torch.int32, np.int32) if args.dtype == "int32" else (torch.int64, np.int64)
    el = 4 if args.dtype == "int32" else 8
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    kw = dict(pad_id=PAD, bos_id=BOS, eos_id=EOS)
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T = res.num_samples, res.num_tokens
        W = res.window_info(ROW_LEN, STRIDE, bos_id=BOS, eos_id=EOS)
        rec = {"corpus_mib": mib, "bytes": int(flat.size), "samples": S, "tokens": T, "mean_row": round(T / S, 1), "dtype": args.dtype,
               "steps": args.steps, "row_len": ROW_LEN, "stride": STRIDE, "windows": W}
        # the window call: ids + mask + lengths + the two per-window outputs
        ids = torch.empty((W, ROW_LEN), dtype=dtype, device="cuda")
        mask = torch.empty((W, ROW_LEN), dtype=torch.uint8, device="cuda")
        lengths, row, first = (torch.empty((W,), dtype=torch.int32, device="cuda") for _ in range(3))
        out_bytes = W * ROW_LEN * (el + 1) + 12 * W
        call = timed(lambda: tensors.window_into(res, ids, mask, lengths, row, first, row_len=ROW_LEN, stride=STRIDE, n_windows=W, **kw),
                     args.steps, args.warmup)
        info = timed(lambda: res.window_info(ROW_LEN, STRIDE, bos_id=BOS, eos_id=EOS), args.steps, args.warmup)
        fill_ms = round(call["ms"] - info["ms"], 4)
        rec["windows_call"] = {**call, "out_bytes": out_bytes, "out_gb_s": rate(out_bytes, call["ms"]), "info_ms": info["ms"], "fill_ms": fill_ms,
                               "fill_gb_s": rate(out_bytes, fill_ms), "fill": round(int(lengths.sum()) / (W * ROW_LEN), 4)}
        # (a) the padded layout of the same result at about the same element count
        L = max(1, round(W * ROW_LEN / S))
        pids = torch.empty((S, L), dtype=dtype, device="cuda")
        pmask = torch.empty((S, L), dtype=torch.uint8, device="cuda")
        plen = torch.empty((S,), dtype=torch.int32, device="cuda")
        pad_bytes = S * L * (el + 1) + 4 * S
        pad = timed(lambda: tensors.pad_into(res, pids, pmask, plen, row_len=L, **kw), args.steps, args.warmup)
        rec["pad_call"] = {**pad, "row_len": L, "out_bytes": pad_bytes, "out_gb_s": rate(pad_bytes, pad["ms"]),
                           "fill": round(int(plen.sum()) / (S * L), 4)}
        rec["fill_rate_vs_pad"] = round(rec["windows_call"]["fill_gb_s"] / rec["pad_call"]["out_gb_s"], 3)
        del pids, pmask, plen
        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_ids, h_offs = res.ids(), res.offsets()
            t1 = time.perf_counter()
            h = _lib.layout_windows_host(h_ids, h_offs, ROW_LEN, STRIDE, PAD, bos_id=BOS, eos_id=EOS, dtype=np_dtype)
            t2 = time.perf_counter()
            up = [torch.from_numpy(h[k]).to("cuda") for k in ("input_ids", "attention_mask", "overflow_to_sample_mapping")]
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            rec["host_route"] = {"ms": round((t3 - t0) * 1e3, 1), "ms_ids_to_host": round((t1 - t0) * 1e3, 1), "ms_host_twin": round((t2 - t1) * 1e3, 1),
                                 "ms_upload": round((t3 - t2) * 1e3, 1),
                                 "equal": bool(torch.equal(up[0], ids) and torch.equal(up[1], mask) and torch.equal(up[2], row))}
            rec["x_host_route"] = round((t3 - t0) * 1e3 / call["ms"], 1)
            del h_ids, h_offs, h, up
        print(json.dumps(rec), flush=True)
        del ids, mask, lengths, row, first
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
