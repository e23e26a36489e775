// Near-duplicate rows (include/tgx.h: tgx_result_minhash_device, tgx_corpus_minhash_device, tgx_minhash_bands_device,
// tgx_minhash_near_first_device): the pinned arithmetic of a signature, the tiling of the shingle positions, the flush
// rule, the band key and the rules of the clustering.  The kernels of minhash.hip and the host twins in host_twins.cpp
// (tgx_minhash_host, tgx_minhash_bands_host, tgx_minhash_near_first_host) both go through these functions.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) (u8 text bytes or u32 ids).  Row i owns
// m_i = max(1, n_i - w + 1) shingle positions; sh_offs is their exclusive scan, and position p of row i is shingle
// t = p - sh_offs[i], the elements [t, t + min(w, n_i)) of the row.  Every row owns at least one position, so sh_offs
// ascends strictly and the owner of a position is unique.  A wave takes a chunk of 64 consecutive positions, a block of
// four waves a tile of 256, and a block a run of consecutive tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dedup.h"

namespace tgx {

constexpr uint64_t kMinhashSalt = 0xD6E8FEB86659FD93ULL;  // TGX_MINHASH_SALT
constexpr uint64_t kMinhashGolden = 0x9E3779B97F4A7C15ULL;  // G
constexpr uint32_t kMinhashChunk = 64;                    // shingle positions of a wave's step
constexpr uint32_t kMinhashTile = 256;                    // shingle positions of a block's step: four chunks
constexpr uint32_t kMinhashMaxPerm = 1024;                // K <= 1024: at most 16 permutations per lane
constexpr uint32_t kMinhashMaxBytes = 64;                 // w·eb <= 64: a shingle is at most 8 words
constexpr uint32_t kMinhashNoSig = 0xFFFFFFFFu;           // what the signatures are pre-set to: the neutral element of min
constexpr int kMinhashStages = 6;

// shingle positions of a row of n elements under width w
__host__ __device__ inline uint64_t minhash_shingles(uint64_t n, uint32_t w) { return n >= w ? n - w + 1 : 1; }
// elements of every shingle of that row
__host__ __device__ inline uint32_t minhash_shingle_len(uint64_t n, uint32_t w) { return n < w ? (uint32_t)n : w; }
// positions of row k; entry S (which the scan turns into the total) is 0 and reads nothing
__host__ __device__ inline uint64_t minhash_row_positions(const uint64_t* offs, uint64_t n_rows, uint32_t w, uint64_t k) {
    return k < n_rows ? minhash_shingles(offs[k + 1] - offs[k], w) : 0;
}

// the seed of the shingle hash and the seed s of the permutations
__host__ __device__ inline uint64_t minhash_hash_seed(uint64_t seed) { return seed ^ kMinhashSalt; }
__host__ __device__ inline uint64_t minhash_perm_seed(uint64_t seed) { return dedup_mix(seed ^ kMinhashSalt); }
// (a_k, b_k) of permutation k under s
__host__ __device__ inline void minhash_perm(uint64_t s, uint32_t k, uint64_t& a, uint64_t& b) {
    a = dedup_mix(s ^ ((2ull * k + 1) * kMinhashGolden)) | 1;
    b = dedup_mix(s ^ ((2ull * k + 2) * kMinhashGolden));
}
// v_k(h) = (uint32_t)((a·h + b) >> 32) wrapping at 2^64.  Only the top word of the low 64 bits is wanted: a_lo·h_lo + b
// in full (one 32 x 32 + 64 multiply-add) and the low words of the two cross products; a_hi·h_hi lies above bit 63.
__host__ __device__ inline uint32_t minhash_value(uint64_t a, uint64_t b, uint64_t h) {
    const uint32_t a_lo = (uint32_t)a, a_hi = (uint32_t)(a >> 32), h_lo = (uint32_t)h, h_hi = (uint32_t)(h >> 32);
    const uint64_t t = (uint64_t)a_lo * h_lo + b;
    return (uint32_t)(t >> 32) + a_lo * h_hi + a_hi * h_lo;
}

// tgx_row_hash of a shingle from its words: n_bytes <= 64, words[j] = its bytes [8j, 8j + 8) little-endian, bytes past
// n_bytes zero.  hs = dedup_seed(minhash_hash_seed(seed))
__host__ __device__ inline uint64_t minhash_hash_words(const uint64_t* words, uint32_t n_bytes, uint64_t hs) {
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMinhashMaxBytes / 8; j++)
        if (8 * j < n_bytes) acc += dedup_term(words[j], j, hs);
    return dedup_finish(acc, n_bytes, hs);
}

// The flush rule.  A wave that leaves row `row` in the chunk that starts at position c0 stores the row's minima plainly
// when every position of the row lies in that chunk (no other wave has any of them), and otherwise takes the minimum
// with what is there, atomically: every chunk of such a row does, and the signatures were pre-set to kMinhashNoSig.
__host__ __device__ inline bool minhash_row_inside(const uint64_t* sh_offs, uint64_t row, uint64_t c0) {
    return sh_offs[row] >= c0 && sh_offs[row + 1] <= c0 + kMinhashChunk;
}

// The band key: tgx_row_hash of the 4r little-endian bytes of sig_row[b·r .. (b+1)·r) under the seed
// (seed ^ TGX_MINHASH_SALT) + b + 1.  Word j is values 2j and 2j + 1; an odd r leaves the last word's top half zero.
__host__ __device__ inline uint64_t minhash_band_key(const uint32_t* sig_row, uint32_t r, uint32_t b, uint64_t seed) {
    const uint32_t* v = sig_row + (uint64_t)b * r;
    const uint64_t s = dedup_seed(minhash_hash_seed(seed) + b + 1);
    uint64_t acc = 0;
    for (uint32_t j = 0; 2 * j < r; j++) {
        const uint64_t w = (uint64_t)v[2 * j] | (2 * j + 1 < r ? (uint64_t)v[2 * j + 1] << 32 : 0);
        acc += dedup_term(w, j, s);
    }
    return dedup_finish(acc, 4ull * r, s);
}

// The star rule of the clustering.  Row i looks at the head of its bucket in band b only when that head is an earlier
// row than the best it has so far (a head that is no row, or not before i, is never read), and takes it when at least
// min_agree of the K signature values agree.
__host__ __device__ inline bool minhash_looks_at(int64_t head, uint64_t best) { return head >= 0 && (uint64_t)head < best; }
__host__ __device__ inline bool minhash_takes(uint32_t agree, uint32_t min_agree) { return agree >= min_agree; }
// one round of pointer doubling: first[i] through first of the round before
__host__ __device__ inline int64_t minhash_hop(const int64_t* first, uint64_t i) { return first[first[i]]; }

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// minhash.hip.  All pointers are device memory.
hipError_t minhash_scan_bytes(uint64_t n_rows, size_t* scan_bytes);
// sig u32[S, K] of the rows; sh_offs u64[S + 1] and scan_tmp are scratch
hipError_t launch_minhash_sig(const DedupRows& rows, uint32_t width, uint32_t n_perm, uint64_t seed, uint64_t* sh_offs, void* scan_tmp,
                              size_t scan_bytes, uint32_t* sig, hipStream_t stream);
// keys of every (row, band): row-major into keys (u64[S, B], may be NULL) and band-major into keys_t (u64[B, S], may be NULL)
hipError_t launch_minhash_band_keys(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed, uint64_t* keys,
                                    uint64_t* keys_t, hipStream_t stream);
hipError_t launch_minhash_iota(uint32_t* rows, uint64_t n_rows, hipStream_t stream);
// heads[rows[i]·B + b] = rows[the head of sorted position i's run]
hipError_t launch_minhash_heads(const uint64_t* sorted_keys, const uint32_t* sorted_rows, uint64_t n_rows, uint32_t bands, uint32_t b, int64_t* heads,
                                hipStream_t stream);
// first0 of every row
hipError_t launch_minhash_verify(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, const int64_t* heads, uint32_t bands, uint32_t min_agree,
                                 int64_t* first0, hipStream_t stream);
// out[i] = in[in[i]]; *changed += 1 when any out[i] != in[i].  changed is zeroed by the launcher
hipError_t launch_minhash_hop(const int64_t* in, int64_t* out, uint64_t n_rows, unsigned long long* changed, hipStream_t stream);
// *count = #{ i : first[i] == i }.  count is zeroed by the launcher
hipError_t launch_minhash_count(const int64_t* first, uint64_t n_rows, unsigned long long* count, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
