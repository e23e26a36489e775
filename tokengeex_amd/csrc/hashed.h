// Hashed n-gram features (include/tgx_hashed.h: tgx_*_hashed_counts_device, tgx_*_hashed_scores_device, tgx_hashed_bucket):
// what a feature and its bucket are, the keys of all widths from one window, the limits, the LDS budget and the bound on
// a narrow bin.  The kernels of hashed.hip and the host twins in host_twins.cpp (tgx_hashed_counts_host,
// tgx_hashed_scores_host) both go through these functions; gram.h has the validity rule, the chunk and the store / add
// rule that they share with the gram kernels.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) (u8 text bytes or u32 ids).  Under 1 to 4 distinct
// ascending widths w_j the feature of the valid gram (gram_valid) of width w_j at element e is the bucket of its key
// (tgx_gram_key of its w_j·eb bytes under the seed): floor(key · B / 2^64).  The elements of all rows are laid end to
// end and a wave takes a chunk of 64 consecutive elements (kGramChunk), a lane an element, as the gram kernels do; here a
// wave walks a run of consecutive chunks of its own, and the sixteen waves of a block share one table in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "api_internal.h"
#include "gram.h"

namespace tgx {

constexpr uint32_t kHashedMaxWidths = 4;
constexpr uint32_t kHashedMaxVectors = 16;          // K
constexpr uint64_t kHashedMaxEntries = 1ull << 24;  // K·B
constexpr uint32_t kHashedWaves = 16;               // waves of a block: one table serves them all
constexpr uint32_t kHashedBlock = kHashedWaves * kGramChunk;
// The table's budget: 16 384 words of 32 bits, 64 KiB of a CU's 160 KiB.  Two blocks fit a CU by LDS; a block is a full
// complement of waves by itself where the kernel needs more than 64 VGPRs (profiles/hashed/kernel_resources.txt).
constexpr uint32_t kHashedLdsEntries = 16384;
constexpr int kHashedStages = 2;

// the widths of a call, as the kernels take them
struct HashedWidths {
    uint32_t n;
    uint32_t w[kHashedMaxWidths];
};

// floor(key · B / 2^64): the high half of the 128-bit product, below B for every key
__host__ __device__ inline uint64_t hashed_bucket(uint64_t key, uint64_t buckets) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __umul64hi(key, buckets);
#else
    return (uint64_t)(((unsigned __int128)key * buckets) >> 64);
#endif
}

// How many of the widths own a valid gram at element e of a row that ends at row_end.  The widths ascend, so the valid
// ones are the first n_valid of them, and the window of the last of those holds the windows of the others.
__host__ __device__ inline uint32_t hashed_valid_widths(const HashedWidths& ws, uint64_t e, uint64_t row_end) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < kHashedMaxWidths; j++)
        if (j < ws.n && gram_valid(e, ws.w[j], row_end)) n = j + 1;
    return n;
}
__host__ __device__ inline uint32_t hashed_window(const HashedWidths& ws, uint32_t n_valid) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < kHashedMaxWidths; j++)
        if (j < n_valid) w = ws.w[j];
    return w;
}

// The keys of the first n_valid widths from the words of the longest window (minhash_hash_words' layout: words[q] = its
// bytes [8q, 8q + 8) little-endian; what lies past that window is never looked at).  A key is the hash of the summed
// terms of its words: a width's whole words are a prefix of the longer widths' whole words, so their terms are computed
// once and summed as a prefix, and a width adds the term of its own last, partial word.  hs as for minhash_hash_words.
__host__ __device__ inline void hashed_keys(const uint64_t (&words)[8], const HashedWidths& ws, uint32_t elem_bytes, uint32_t n_valid, uint64_t hs,
                                            uint64_t (&keys)[kHashedMaxWidths]) {
    const uint32_t whole = hashed_window(ws, n_valid) * elem_bytes / 8;  // whole words of the longest window
    const uint32_t whole_max = hashed_window(ws, ws.n) * elem_bytes / 8;  // and of any lane's: a branch the whole wave takes
    uint64_t pre[9];                                                    // pre[q]: the terms of words 0 .. q - 1
    pre[0] = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        pre[q + 1] = pre[q];
        if (q < whole_max) pre[q + 1] += q < whole ? dedup_term(words[q], q, hs) : 0;
    }
#pragma unroll
    for (uint32_t j = 0; j < kHashedMaxWidths; j++) {
        keys[j] = 0;
        if (j >= n_valid) continue;
        const uint32_t n_bytes = ws.w[j] * elem_bytes, q = n_bytes / 8, rest = n_bytes & 7u;
        uint64_t acc = 0, last = 0;
#pragma unroll
        for (uint32_t t = 0; t < 8; t++) {  // (selects, not indexing: the arrays stay in registers)
            if (t == q) {
                acc = pre[t];
                last = words[t];
            }
        }
        if (q == 8) acc = pre[8];
        if (rest) acc += dedup_term(last & ((1ull << (8 * rest)) - 1), q, hs);
        keys[j] = dedup_finish(acc, n_bytes, hs);
    }
}

// K padded to a power of two: one feature's weights are KP consecutive i32 in the table, one wide read
__host__ __device__ inline uint32_t hashed_padded(uint32_t n_vectors) {
    uint32_t kp = 1;
    while (kp < n_vectors) kp *= 2;
    return kp;
}
// the most buckets whose K weights each (K = 1: the bins of the counts) fit the LDS budget
__host__ __device__ inline uint64_t hashed_lds_buckets(uint32_t n_vectors) { return kHashedLdsEntries / hashed_padded(n_vectors); }

// The counts' LDS bins are 32 bits wide and are flushed once, at the end of the block's run.  A bin receives at most one
// add per element of the run and width, so the bins are used only where that product stays below 2^32.
__host__ __device__ inline uint64_t hashed_run_chunks(uint64_t n_elems, uint64_t n_blocks) {
    const uint64_t n_chunks = (n_elems + kGramChunk - 1) / kGramChunk, n_waves = n_blocks * kHashedWaves;
    return (n_chunks + n_waves - 1) / n_waves;  // of one wave
}
__host__ __device__ inline bool hashed_bins_hold(uint64_t n_elems, uint64_t n_blocks, uint32_t n_widths) {
    return hashed_run_chunks(n_elems, n_blocks) <= (0xFFFFFFFFull / ((uint64_t)kHashedBlock * n_widths));
}

// The arguments' check that the device calls and the twins share; n_vectors = 1 for the counts.
inline tgx_status hashed_check(const char* who, const uint32_t* widths, uint32_t n_widths, uint32_t elem_bytes, uint64_t buckets, uint32_t n_vectors,
                               HashedWidths* ws) {
    using host::fail;
    if (elem_bytes != 1 && elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, elem_bytes);
    if (n_widths < 1 || n_widths > kHashedMaxWidths) return fail(TGX_ERR_INVALID, "%s: n_widths %u is not in 1 .. %u", who, n_widths, kHashedMaxWidths);
    if (!widths) return fail(TGX_ERR_INVALID, "%s: widths is NULL", who);
    ws->n = n_widths;
    for (uint32_t j = 0; j < kHashedMaxWidths; j++) ws->w[j] = j < n_widths ? widths[j] : 0;
    for (uint32_t j = 0; j < n_widths; j++) {
        if (widths[j] == 0 || (uint64_t)widths[j] * elem_bytes > kMinhashMaxBytes)
            return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, widths[j], elem_bytes, kMinhashMaxBytes / elem_bytes);
        if (j && widths[j] <= widths[j - 1]) return fail(TGX_ERR_INVALID, "%s: width %u after width %u: the widths must ascend", who, widths[j], widths[j - 1]);
    }
    if (n_vectors < 1 || n_vectors > kHashedMaxVectors) return fail(TGX_ERR_INVALID, "%s: n_vectors %u is not in 1 .. %u", who, n_vectors, kHashedMaxVectors);
    if (buckets < 1 || buckets > kHashedMaxEntries / n_vectors)
        return fail(TGX_ERR_INVALID, "%s: buckets %llu is not in 1 .. %llu for %u vectors", who, (unsigned long long)buckets,
                    (unsigned long long)(kHashedMaxEntries / n_vectors), n_vectors);
    return TGX_OK;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// hashed.hip.  All pointers are device memory; the launchers pre-set what they add to.
// counts i64[B] of the rows' features; *used_lds (may be NULL): the LDS histogram ran
hipError_t launch_hashed_counts(const DedupRows& rows, const HashedWidths& ws, uint64_t buckets, uint64_t seed, int64_t* counts, bool* used_lds,
                                hipStream_t stream);
// table i32[B][KP] (scratch) from q i32[K][B]; scores i64[S][K] of the rows
hipError_t launch_hashed_scores(const DedupRows& rows, const HashedWidths& ws, uint64_t buckets, uint32_t n_vectors, uint64_t seed, const int32_t* q,
                                int32_t* table, int64_t* scores, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
