"""The padded and packed layouts (csrc/layout.hip) on a resident encode of bench.py's mixed corpus with the spec 32 000
vocabulary: time of each layout call at L = 512 and L = 4096, i32 and i64, beside two baselines measured in the same run:

  (a) hipMemcpyAsync device-to-device of the same number of output bytes: the floor of a kernel that only writes;
  (b) the host round trip a caller had before: NativeResult.ids() -> pad_host / pack_host (i64) -> torch.from_numpy().cuda().

Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup; (b) is a host clock around work that ends in a synchronise, one call.
One JSON line per corpus size.   usage: layout_bench.py [--sizes 256,1024] [--steps 10] [--warmup 3] [--no-host]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import synth, tensors

PAD, BOS, EOS = 0, 1, 2


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            lib = ctypes.CDLL(name)
            lib.hipMemcpyAsync.restype = ctypes.c_int
            lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
            return lib
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found: baseline (a) needs hipMemcpyAsync")


def timed(fn, steps, warmup):
    """median / min ms of fn() between two events on the current stream"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}


def d2d(hip, nbytes, steps, warmup):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream)  # hipMemcpyDeviceToDevice
        assert rc == 0, rc
        torch.cuda.current_stream().synchronize()   # as the layout calls do
    return timed(fn, steps, warmup)


def rate(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)   # GB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip baseline (b)")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("layout_bench.py needs a GPU")
    hip = _hip()
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T = res.num_samples, res.num_tokens
        max_row, n_stream = res.layout_info(BOS, EOS)
        rec = {"corpus_mib": mib, "bytes": int(flat.size), "samples": S, "tokens": T, "mean_row": round(T / S, 1), "max_row_len": max_row,
               "n_stream": n_stream, "steps": args.steps, "encode_ms": round(sum(model.last_kernel_times().values()), 3), "layouts": []}
        for L in (512, 4096):
            for dt in (torch.int32, torch.int64):
                esz = 4 if dt == torch.int32 else 8
                # padded: ids + mask (+ lengths), rows cut to L
                ids = torch.empty((S, L), dtype=dt, device="cuda")
                mask = torch.empty((S, L), dtype=torch.uint8, device="cuda")
                lengths = torch.empty((S,), dtype=torch.int32, device="cuda")
                nt = tensors.pad_into(res, ids, mask, lengths, row_len=L, pad_id=PAD, bos_id=BOS, eos_id=EOS)
                filled = int(lengths.sum())
                for what, m in (("padded ids+mask", mask), ("padded ids", None)):
                    out_bytes = S * L * (esz + (1 if m is not None else 0)) + 4 * S
                    t = timed(lambda: tensors.pad_into(res, ids, m, lengths, row_len=L, pad_id=PAD, bos_id=BOS, eos_id=EOS), args.steps, args.warmup)
                    c = d2d(hip, out_bytes, args.steps, args.warmup)
                    rec["layouts"].append({"layout": what, "L": L, "dtype": str(dt).split(".")[1], "out_bytes": out_bytes,
                                           "read_bytes": 4 * (filled - 2 * S) + 8 * (S + 1), "truncated_rows": nt,
                                           "fill": round(filled / (S * L), 4), **t, "out_gb_s": rate(out_bytes, t["ms"]),
                                           "d2d_ms": c["ms"], "d2d_gb_s": rate(out_bytes, c["ms"]), "x_d2d": round(t["ms"] / c["ms"], 2)})
                del ids, mask, lengths
                # packed: ids alone, and with doc + pos
                B = -(-n_stream // L)
                ids = torch.empty((B, L), dtype=dt, device="cuda")
                doc = torch.empty((B, L), dtype=torch.int32, device="cuda")
                pos = torch.empty((B, L), dtype=torch.int32, device="cuda")
                for what, d, p in (("packed ids", None, None), ("packed ids+doc+pos", doc, pos)):
                    out_bytes = B * L * (esz + (8 if d is not None else 0))
                    t = timed(lambda: tensors.pack_into(res, ids, d, p, block_len=L, pad_id=PAD, bos_id=BOS, eos_id=EOS), args.steps, args.warmup)
                    c = d2d(hip, out_bytes, args.steps, args.warmup)
                    rec["layouts"].append({"layout": what, "L": L, "dtype": str(dt).split(".")[1], "out_bytes": out_bytes,
                                           "read_bytes": 4 * T + 8 * (S + 1), **t, "out_gb_s": rate(out_bytes, t["ms"]),
                                           "d2d_ms": c["ms"], "d2d_gb_s": rate(out_bytes, c["ms"]), "x_d2d": round(t["ms"] / c["ms"], 2)})
                del ids, doc, pos
        if not args.no_host:
            # (b): what a caller did before — ids to the host, numpy layout (the host twins), tensor back to the device
            for L in (512, 4096):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = res.pad_host(L, PAD, bos_id=BOS, eos_id=EOS, dtype=np.int64)
                t1 = time.perf_counter()
                a, b = torch.from_numpy(h["input_ids"]).cuda(), torch.from_numpy(h["attention_mask"]).cuda()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                rec["layouts"].append({"layout": "host round trip: padded ids+mask", "L": L, "dtype": "int64", "ms": round((t2 - t0) * 1e3, 1),
                                       "ms_ids_and_pad_host": round((t1 - t0) * 1e3, 1), "ms_to_device": round((t2 - t1) * 1e3, 1)})
                del a, b, h
                t0 = time.perf_counter()
                h = res.pack_host(L, PAD, bos_id=BOS, eos_id=EOS, dtype=np.int64)
                t1 = time.perf_counter()
                a = torch.from_numpy(h["input_ids"]).cuda()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                rec["layouts"].append({"layout": "host round trip: packed ids", "L": L, "dtype": "int64", "ms": round((t2 - t0) * 1e3, 1),
                                       "ms_ids_and_pack_host": round((t1 - t0) * 1e3, 1), "ms_to_device": round((t2 - t1) * 1e3, 1)})
                del a, h
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
