// Exact row deduplication (include/tgx.h: tgx_corpus_first_equal_device, tgx_result_first_equal_device, tgx_row_hash):
// the hash, the key of `bits` bits, the tiling of the hash, the run rule and the compare and resolve rules.  The kernels
// of dedup.hip and the host twin in host_twins.cpp (tgx_first_equal_host) both go through these functions, so a machine
// without a GPU checks the rounds, the collision path included.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) (u8 text bytes or u32 ids; a row of ids is hashed
// as its 4·n_i little-endian bytes).  A round works on a list of L unresolved rows, ascending by row index (NULL: every
// row).  The hash tiles the PADDED bytes of the listed rows: row k of the list owns 8·W_k positions, W_k = ceil(n_k / 8)
// its 8-byte words, so a 16-byte slot is always two whole words, each of one row, and an empty row owns nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_fill.h"

namespace tgx {

constexpr uint64_t kDedupSalt = 0xA0761D6478BD642FULL;  // TGX_DEDUP_SALT
constexpr uint32_t kDedupTile = 4096;                   // padded bytes per tile of the hash: 256 threads x 16 bytes
constexpr uint32_t kDedupGroup = 16;                    // padded bytes of a thread slot: two words
constexpr uint32_t kDedupCmpByteTile = 4096;            // the compare over text: bytes per tile, a slot of 16
constexpr uint32_t kDedupCmpByteGroup = 16;
constexpr uint32_t kDedupCmpTile = 1024;                // the compare over ids: ids per tile, a slot of 4
constexpr uint32_t kDedupCmpGroup = 4;
constexpr int kDedupStages = 4;

// R: the three xor-shift / multiply rounds of tgx_dropout_u01
__host__ __device__ inline uint64_t dedup_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}
// tgx_row_hash in its parts: s of a seed, the term of word j, the hash of the summed terms of a row of n_bytes
__host__ __device__ inline uint64_t dedup_seed(uint64_t seed) { return dedup_mix(seed ^ kDedupSalt); }
__host__ __device__ inline uint64_t dedup_term(uint64_t w, uint64_t j, uint64_t s) { return dedup_mix(w ^ ((j + 1) * 0x9E3779B97F4A7C15ULL) ^ s); }
__host__ __device__ inline uint64_t dedup_finish(uint64_t acc, uint64_t n_bytes, uint64_t s) {
    return dedup_mix(acc ^ (n_bytes * 0xC2B2AE3D27D4EB4FULL) ^ s);
}
// the sort key: the hash's top `bits` bits (0: every row collides)
__host__ __device__ inline uint64_t dedup_key(uint64_t hash, uint32_t bits) { return bits ? hash >> (64 - bits) : 0; }

// word j < W of a row of n_bytes in host memory: little-endian, bytes past the row read as 0
inline uint64_t dedup_word_host(const uint8_t* row, uint64_t n_bytes, uint64_t j) {
    uint64_t w = 0;
    for (uint32_t b = 0; b < 8 && 8 * j + b < n_bytes; b++) w |= (uint64_t)row[8 * j + b] << (8 * b);
    return w;
}
inline uint64_t dedup_row_hash_host(const uint8_t* row, uint64_t n_bytes, uint64_t seed) {
    const uint64_t s = dedup_seed(seed), W = (n_bytes + 7) / 8;
    uint64_t acc = 0;
    for (uint64_t j = 0; j < W; j++) acc += dedup_term(dedup_word_host(row, n_bytes, j), j, s);
    return dedup_finish(acc, n_bytes, s);
}

// listed row k -> its row index
__host__ __device__ inline uint64_t dedup_listed(const uint32_t* list, uint64_t k) { return list ? list[k] : k; }
// padded bytes of listed row k; entry L (which the scan turns into the total) is 0 and reads nothing
__host__ __device__ inline uint64_t dedup_pad_len(const uint64_t* offs, uint32_t elem_bytes, const uint32_t* list, uint64_t n_list, uint64_t k) {
    if (k >= n_list) return 0;
    const uint64_t r = dedup_listed(list, k);
    return ((offs[r + 1] - offs[r]) * elem_bytes + 7) & ~7ull;
}

// The owner of position j when a row at or before it is known: the LARGEST i in [start, last] with offs[i] <= j, as
// pack_find_row finds it, by galloping up from `start` (offs[start] <= j).  The hash walks its tiles in ascending order, and
// the owner of a tile's edge is seldom far behind the owner of the edge before it: a few dependent loads where the
// search over all the rows takes log2(L) of them, which was what a tile waited for.
__host__ __device__ inline uint64_t dedup_find_from(const uint64_t* offs, uint64_t start, uint64_t last, uint64_t j) {
    uint64_t lo = start, step = 1;
    while (lo + step <= last && offs[lo + step] <= j) {
        lo += step;
        step *= 2;
    }
    return pack_find_row(offs, 0, lo, lo + step - 1 < last ? lo + step - 1 : last, j);
}

// The one or two words of the slot of n_in = 8 or 16 padded positions from e0 on: word q is word j[q] of listed row
// k[q].  lo / hi: the owners of the first and last position of the slot's tile.
struct DedupSlot {
    uint64_t k[2], j[2];
    uint32_t n;
};
__host__ __device__ inline void dedup_slot(const uint64_t* pad_offs, uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in, DedupSlot& s) {
    s.n = n_in / 8;
    s.k[0] = pack_find_row(pad_offs, 0, lo, hi, e0);
    s.j[0] = (e0 - pad_offs[s.k[0]]) / 8;
    s.k[1] = s.k[0];
    s.j[1] = s.j[0] + 1;
    if (s.n == 2 && e0 + 8 >= pad_offs[s.k[0] + 1]) {  // the second word begins the next row that owns anything
        s.k[1] = pack_find_row(pad_offs, 0, s.k[0] + 1, hi, e0 + 8);
        s.j[1] = (e0 + 8 - pad_offs[s.k[1]]) / 8;
    }
}

// The run rule.  keys[0 .. L) are sorted ascending, stably, from a list ascending by row: the head of position i's run is
// the first position with its key, and holds the run's smallest row.
__host__ __device__ inline uint64_t dedup_run_head(const uint64_t* keys, uint64_t i) {
    const uint64_t key = keys[i];
    uint64_t lo = 0, hi = i;  // the smallest p in [0, i] with keys[p] == key
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// The compare rules.  A candidate (a row r that is not its run's head row h) of another length than its head is flagged
// at once; one of the same length owns that many positions of the compare, and a head or a flagged row owns none.
__host__ __device__ inline bool dedup_len_differs(const uint64_t* offs, uint64_t r, uint64_t h) { return offs[r + 1] - offs[r] != offs[h + 1] - offs[h]; }
__host__ __device__ inline uint64_t dedup_cmp_len(const uint64_t* offs, const uint32_t* rows, const uint32_t* head_row, const uint8_t* flag,
                                                  uint64_t n_list, uint64_t i) {
    if (i >= n_list) return 0;
    const uint64_t r = rows[i];
    return (head_row[i] == r || flag[i]) ? 0 : offs[r + 1] - offs[r];
}

// A walk over ascending positions of the compare that all lie between the positions owned by sorted positions lo and hi
// (a tile's first and last), as SelectCursor's.
struct DedupCursor {
    uint64_t i = 0, next = 0;       // the current sorted position and cmp_offs[i + 1]
    uint64_t start = 0;             // cmp_offs[i]
    uint64_t a = 0, b = 0;          // offs of the candidate's row and of its head's
    bool have = false;
};
__host__ __device__ inline void dedup_enter(DedupCursor& cur, const uint64_t* offs, const uint32_t* rows, const uint32_t* head_row,
                                            const uint64_t* cmp_offs, uint64_t lo, uint64_t hi, uint64_t j) {
    if (!cur.have || j >= cur.next) {
        cur.i = pack_find_row(cmp_offs, 0, cur.have ? cur.i + 1 : lo, hi, j);
        cur.start = cmp_offs[cur.i];
        cur.next = cmp_offs[cur.i + 1];
        cur.a = offs[rows[cur.i]];
        cur.b = offs[head_row[cur.i]];
        cur.have = true;
    }
}
// the slot of n_in positions from e0 on, element by element: every candidate with a difference inside it is flagged
template <class T>
__host__ __device__ inline void dedup_compare_walk(DedupCursor& cur, const T* data, const uint64_t* offs, const uint32_t* rows, const uint32_t* head_row,
                                                   const uint64_t* cmp_offs, uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in, uint8_t* flag) {
    for (uint32_t q = 0; q < n_in; q++) {
        dedup_enter(cur, offs, rows, head_row, cmp_offs, lo, hi, e0 + q);
        const uint64_t t = e0 + q - cur.start;
        if (data[cur.a + t] != data[cur.b + t]) flag[cur.i] = 1;
    }
}
// does the whole slot lie inside the candidate the cursor stands on (entered for e0)?
__host__ __device__ inline bool dedup_slot_inside(const DedupCursor& cur, uint64_t e0, uint32_t n_in, uint32_t group) {
    return n_in == group && e0 + group <= cur.next;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// dedup.hip.  All pointers are device memory.  The scratch of a call, sized for S rows and used by every round:
struct DedupScratch {
    uint64_t *keys_a, *keys_b;  // u64[S]: the rows' sums, then their keys; the sorted keys
    uint32_t *rows_a, *rows_b;  // u32[S]: the listed rows beside keys_a; the sorted rows
    uint64_t* offs_tmp;         // u64[S+1]: the padded offsets of the hash, then the offsets of the compare
    uint32_t* head_row;         // u32[S]: per sorted position, its run's head row
    uint8_t *flag, *mark;       // u8[S]: per sorted position, the candidate differs; per ROW, it goes to the next round
    uint32_t* list[2];          // u32[S] each: the next rounds' lists
    unsigned long long* words;  // [2]: rows left for the next round; heads so far
    void *scan_tmp, *sort_tmp, *select_tmp;
    size_t scan_bytes, sort_bytes, select_bytes;
};
struct DedupRows {
    const void* data;      // u8[N] (a corpus's text: 256 bytes of slack on either side) or u32[T]
    const uint64_t* offs;  // u64[S+1]
    uint64_t n_rows;       // S
    uint64_t n_elems;      // N or T
    uint32_t elem_bytes;   // 1 or 4
};
hipError_t dedup_temp_bytes(uint64_t n_rows, size_t* scan_bytes, size_t* sort_bytes, size_t* select_bytes);
// sums[k] (scratch, u64[L]) and out[k] = tgx_row_hash(listed row k, seed) >> (64 - bits); rows_out[k] = the row (may be NULL).
// out may be sums.  list == NULL: every row
hipError_t launch_dedup_hash(const DedupRows& rows, const uint32_t* list, uint64_t n_list, uint64_t seed, uint32_t bits, uint64_t* pad_offs,
                             void* scan_tmp, size_t scan_bytes, uint64_t* sums, uint64_t* out, uint32_t* rows_out, hipStream_t stream);
// (keys_a, rows_a) sorted stably by the keys' low `bits` bits into (keys_b, rows_b)
hipError_t launch_dedup_sort(const DedupScratch& s, uint64_t n_list, uint32_t bits, hipStream_t stream);
// head_row and flag of every sorted position
hipError_t launch_dedup_compare(const DedupRows& rows, const DedupScratch& s, uint64_t n_list, hipStream_t stream);
// first[] of the heads and of the unflagged candidates; the flagged rows, ascending, into list_out; words[0] = their number
hipError_t launch_dedup_resolve(const DedupScratch& s, const uint32_t* list, uint64_t n_list, uint32_t* list_out, int64_t* first,
                                hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
