// Shared n-grams (include/tgx.h: tgx_*_gramset_create, tgx_gramset_create_from_keys, tgx_*_gram_hits_device): what a gram
// and its key are, the gram set's bucket directory, the membership test, the tiling of the elements and the rule by
// which a row's hits reach its count.  The kernels of gram.hip and the host twins in host_twins.cpp (tgx_gram_keys_host,
// tgx_gram_hits_host, tgx_gram_contains_host) both go through these functions.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) (u8 text bytes or u32 ids).  The gram at element
// e (a global element index) of row i is the w elements from e on, and it is valid iff e + w <= offs[i+1]: a row shorter
// than w owns no gram (MinHash gives such a row one short shingle; here an empty row of an eval set must not flag every
// empty training row).  Its key is MinHash's hash of a full shingle: minhash_hash_words of its w·eb bytes under
// dedup_seed(minhash_hash_seed(seed)).  The elements of all rows are laid end to end: a wave takes a chunk of 64
// consecutive elements, a block of four waves a tile of 256, and a block a run of consecutive tiles.  offs itself is
// the array of starts, so the owner search steps over empty rows and they are never visited.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minhash.h"

namespace tgx {

constexpr uint32_t kGramChunk = 64;     // elements of a wave's step
constexpr uint32_t kGramTile = 256;     // elements of a block's step: four chunks
constexpr uint32_t kGramMaxBits = 28;   // the directory has at most 2^28 + 1 entries
constexpr uint64_t kGramMaxKeys = 0xFFFFFFFEull;  // dir entries are u32 and 2^32 - 1 keys are refused
constexpr int kGramStages = 4;

// valid grams of a row of n elements under width w
__host__ __device__ inline uint64_t gram_count(uint64_t n, uint32_t w) { return n >= w ? n - w + 1 : 0; }
// the same of row k; entry S (which the scan turns into the total) is 0 and reads nothing
__host__ __device__ inline uint64_t gram_row_count(const uint64_t* offs, uint64_t n_rows, uint32_t w, uint64_t k) {
    return k < n_rows ? gram_count(offs[k + 1] - offs[k], w) : 0;
}
// is the gram at element e valid in a row that ends at row_end?
__host__ __device__ inline bool gram_valid(uint64_t e, uint32_t w, uint64_t row_end) { return e + w <= row_end; }

// bits of the directory of a set of n_keys keys: a bucket holds about one key, and at most 2^28 buckets
__host__ __device__ inline uint32_t gram_dir_bits(uint64_t n_keys) {
    if (n_keys <= 1) return 0;
    uint32_t bits = 0;
    while (bits < kGramMaxBits && (1ull << bits) < n_keys) bits++;
    return bits;
}
// dir[b], b in 0 .. 2^bits: the lower bound of the first key whose bucket is >= b (dir[2^bits] = n_keys).  keys ascend.
__host__ __device__ inline uint32_t gram_dir_entry(const uint64_t* keys, uint64_t n_keys, uint32_t bits, uint64_t b) {
    uint64_t lo = 0, hi = n_keys;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (dedup_key(keys[mid], bits) < b)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (uint32_t)lo;
}
// Membership: the bucket of k from the directory (two adjacent entries), then a binary search inside the bucket, so a
// bucket that an adversary filled costs its logarithm.  An empty bucket reads no key.
__host__ __device__ inline bool gram_contains(const uint64_t* keys, const uint32_t* dir, uint32_t bits, uint64_t k) {
    const uint64_t b = dedup_key(k, bits);
    uint32_t lo = dir[b];
    const uint32_t end = dir[b + 1];
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && keys[lo] == k;
}

// The count rule.  A wave that has the hits of a stretch of row `row` in the chunk that starts at element c0 stores
// them plainly when every element of the row lies in that chunk (no other wave has any), and otherwise adds them to
// the row's count, which was pre-set to 0; a stretch without a hit adds nothing.
__host__ __device__ inline bool gram_row_inside(const uint64_t* offs, uint64_t row, uint64_t c0) {
    return offs[row] >= c0 && offs[row + 1] <= c0 + kGramChunk;
}
__host__ __device__ inline bool gram_adds(uint64_t n_hits) { return n_hits != 0; }

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// gram.hip.  All pointers are device memory.
// the room that the scan of the rows' gram counts needs, and that the sort and the unique of n keys need
hipError_t gram_scan_bytes(uint64_t n_rows, size_t* scan_bytes);
hipError_t gram_sort_bytes(uint64_t n, size_t* sort_bytes, size_t* unique_bytes);
// g_offs u64[S + 1] = the exclusive scan of the rows' gram counts (entry S: the total)
hipError_t launch_gram_offsets(const DedupRows& rows, uint32_t width, uint64_t* g_offs, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// keys_out[g_offs[i] + t] = the key of gram t of row i
hipError_t launch_gram_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, hipStream_t stream);
// keys_in[0 .. n) sorted into sorted (scratch, u64[n]), its distinct keys into unique_out (u64[n]) and their number into *d_count
hipError_t launch_gram_sort_unique(const uint64_t* keys_in, uint64_t* sorted, uint64_t* unique_out, unsigned long long* d_count, uint64_t n,
                                   void* sort_tmp, size_t sort_bytes, void* unique_tmp, size_t unique_bytes, hipStream_t stream);
// dir u32[2^bits + 1] over the ascending keys
hipError_t launch_gram_dir(const uint64_t* keys, uint64_t n_keys, uint32_t bits, uint32_t* dir, hipStream_t stream);
// count i64[S] (may be NULL) and mask u8[n_elems] (may be NULL) of the rows against the set (keys, dir, bits)
hipError_t launch_gram_hits(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* keys, const uint32_t* dir, uint32_t bits,
                            int64_t* count, uint8_t* mask, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
