"""Hashed n-gram features on the device (csrc/hashed.hip) on bench.py's mixed corpus resident in HBM and on its encode under
the spec 32 000 vocabulary: hashed_counts and hashed_scores (K = 1 and 8) under widths (1, 2) over the ids and (3,) over
the text, at B = 10 000 and with B on either side of the LDS threshold of each K.  Beside them, in the same process and on
the same object:

  (a) gram_hits against a set of 2^10 random keys at the widest width: the same walk and hash, two gathers per gram in
      place of the LDS read;
  (b) torch.bincount and index_add_ over buckets and owners materialised beforehand (by torch, from the same hash): what
      a user would write without the kernels.  The bincount is also compared with hashed_counts, bucket by bucket.

A constant source of the same shape (every id 7, every byte 'a': each width's grams land in one bucket) is timed beside
the mixed one: the ratio shows what the hot-bucket measure leaves of the same-address adds.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end) and
the stages of tgx_hashed_last_times, the median of --steps calls after --warmup with the smallest and the largest beside
it.  One JSON line per corpus size.
usage: hashed_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from select_bench import spread, timed

M64 = (1 << 64) - 1


def _i64(x):
    """a 64-bit pattern as the int64 torch computes with (its multiply wraps as the u64's does)"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _mix(x):
    def shr(v, s):  # a logical shift of the u64 pattern
        return (v >> s) & ((1 << (64 - s)) - 1)
    x = x ^ shr(x, 30)
    x = x * _i64(0xBF58476D1CE4E5B9)
    x = x ^ shr(x, 27)
    x = x * _i64(0x94D049BB133111EB)
    return x ^ shr(x, 31)


def torch_buckets(data, width, buckets, seed):
    """The bucket of the gram of `width` elements at every element but the last width - 1 of data (a uint8 or int32 torch
    tensor, at most 8 bytes a gram), as int64: csrc/dedup.h's hash of one word and csrc/hashed.h's bucket, in torch."""
    eb = data.element_size()
    n_bytes = width * eb
    assert n_bytes <= 8
    n = data.numel() - width + 1
    word = torch.zeros(n, dtype=torch.int64, device=data.device)
    for t in range(width):
        part = data[t:t + n].to(torch.int64) & ((1 << (8 * eb)) - 1)
        word |= part << (8 * eb * t)
    def mix_int(v):  # the same rounds on a Python integer
        v &= M64
        v ^= v >> 30
        v = v * 0xBF58476D1CE4E5B9 & M64
        v ^= v >> 27
        v = v * 0x94D049BB133111EB & M64
        return v ^ v >> 31
    hs = mix_int((seed ^ 0xD6E8FEB86659FD93) ^ 0xA0761D6478BD642F)
    term = _mix(word ^ _i64(0x9E3779B97F4A7C15 ^ hs))
    key = _mix(term ^ _i64((n_bytes * 0xC2B2AE3D27D4EB4F) ^ hs))
    hi, lo = (key >> 32) & 0xFFFFFFFF, key & 0xFFFFFFFF
    return (hi * buckets + ((lo * buckets) >> 32)) >> 32


def put(out, name, s):
    out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]


def staged(call, stage, args):
    """call() timed, with the named stage of tgx_hashed_last_times of the timed calls -> (call's spread, stage's spread)"""
    seen = []

    def fn():
        call()
        seen.append(_lib.hashed_last_times()[stage])
    t_call = timed(fn, args.steps, args.warmup)
    return t_call, spread(seen[-args.steps:])


def hashed_run(obj, flat_obj, what, widths, elem_bytes, data, offs, args, stream):
    """obj (mixed) and flat_obj (constant, same shape) timed -> the record.  data, offs: obj's elements and offsets on the device"""
    S = obj.num_samples
    n_elems = obj.num_tokens if elem_bytes == 4 else obj.num_bytes
    out = {"what": what, "rows": S, "elems": n_elems, "widths": list(widths), "counts": [], "scores": []}
    lds1 = _lib.hashed_info(1)["lds_max_buckets"]
    for B in (10000, lds1, lds1 + 1):
        d_counts = torch.empty(B, dtype=torch.int64, device="cuda")
        rec = {"buckets": B, "lds": B <= lds1}
        for label, o in (("mixed", obj), ("constant", flat_obj)):
            t_call, t_k = staged(lambda: _lib.hashed_counts_device(o, widths, B, 0, d_counts.data_ptr(), stream=stream), "hashed_counts_kernel", args)
            put(rec, label + "_call", t_call)
            put(rec, label + "_kernel", t_k)
        rec["constant_x_mixed"] = round(rec["constant_kernel_ms"] / rec["mixed_kernel_ms"], 2)
        out["counts"].append(rec)
    for K in (1, 8):
        lds = _lib.hashed_info(K)["lds_max_buckets"]
        for B in sorted({10000, lds, lds + 1}):
            q = torch.randint(-2**31, 2**31, (K, B), dtype=torch.int64, device="cuda").to(torch.int32)
            d_scores = torch.empty((S, K), dtype=torch.int64, device="cuda")
            rec = {"vectors": K, "buckets": B, "lds": B <= lds}
            t_call, t_k = staged(lambda: _lib.hashed_scores_device(obj, widths, B, K, 0, q.data_ptr(), d_scores.data_ptr(), stream=stream),
                                 "hashed_scores_kernel", args)
            put(rec, "call", t_call)
            put(rec, "kernel", t_k)
            rec["gelems_s"] = round(n_elems / t_k["ms"] / 1e6, 2)
            out["scores"].append(rec)
    # (a) the same walk and hash with two gathers per gram: a set of 2^10 random keys at the widest width
    count = torch.empty(S, dtype=torch.int64, device="cuda")
    mask = torch.empty(n_elems, dtype=torch.uint8, device="cuda")
    gs = _lib.NativeGramSet.from_keys(np.random.default_rng(1).integers(0, 1 << 64, 1 << 10, dtype=np.uint64), widths[-1], "ids" if elem_bytes == 4 else "bytes")
    for label, m_ptr in (("gram_hits_count_only", 0), ("gram_hits_count_and_mask", mask.data_ptr())):
        ms = []

        def fn():
            obj.gram_hits(gs, count.data_ptr(), m_ptr, stream=stream)
            ms.append(_lib.gram_last_times()["gram_hits_kernel"])
        put(out, label + "_call", timed(fn, args.steps, args.warmup))
        put(out, label + "_kernel", spread(ms[-args.steps:]))
    gs.free()
    del mask
    # (b) torch over materialised buckets and owners (rows cut a gram: those positions are dropped beforehand, too)
    B = 10000
    lens = offs[1:] - offs[:-1]
    owner = torch.repeat_interleave(torch.arange(S, device="cuda"), lens)
    buckets, owners = [], []
    for w in widths:
        b = torch_buckets(data, w, B, 0)
        ok = torch.arange(b.numel(), device="cuda") + w <= offs[1:][owner[:b.numel()]]
        buckets.append(b[ok])
        owners.append(owner[:b.numel()][ok])
    buckets, owners = torch.cat(buckets), torch.cat(owners)
    put(out, "torch_bincount", timed(lambda: torch.bincount(buckets, minlength=B), args.steps, args.warmup))
    q = torch.randint(-2**31, 2**31, (1, B), dtype=torch.int64, device="cuda").to(torch.int32)
    dst = torch.zeros(S, dtype=torch.int64, device="cuda")
    put(out, "torch_index_add", timed(lambda: dst.zero_().index_add_(0, owners, q[0].to(torch.int64)[buckets]), args.steps, args.warmup))
    out["grams"] = int(buckets.numel())
    out["counts_equal_bincount"] = bool(torch.equal(tgx.hashed_counts(obj, B, widths, 0), torch.bincount(buckets, minlength=B)))
    want = torch.zeros(S, dtype=torch.int64, device="cuda").index_add_(0, owners, q[0].to(torch.int64)[buckets])
    out["scores_equal_index_add"] = bool(torch.equal(tgx.hashed_scores(obj, q, widths, 0, raw=True)[:, 0], want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("hashed_bench.py needs a GPU")
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        ids, id_offs = res.ids(), res.offsets()
        flat_corpus = tgx.NativeCorpus(np.full(flat.size, ord("a"), np.uint8), offs)
        flat_res = _lib.NativeResult.from_ids(np.full(ids.size, 7, np.uint32), id_offs, 32000)
        rec = {"corpus_mib": mib, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "tokens": res.num_tokens, "steps": args.steps, "runs": []}
        d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
        rec["runs"].append(hashed_run(res, flat_res, "result_hashed", (1, 2), 4, d_ids, torch.from_numpy(id_offs.astype(np.int64)).cuda(), args, stream))
        del d_ids
        torch.cuda.empty_cache()
        d_text = torch.from_numpy(np.asarray(flat)).cuda()
        rec["runs"].append(hashed_run(corpus, flat_corpus, "corpus_hashed", (3,), 1, d_text, torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda(), args, stream))
        del d_text
        print(json.dumps(rec), flush=True)
        for o in (res, corpus, flat_res, flat_corpus):
            o.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
