// Index arithmetic of row selection (include/tgx.h: tgx_result_select, tgx_corpus_select) and the key of the seeded
// permutation (tgx_shuffle_key).  The kernels of select.hip and the host twins in host_twins.cpp (tgx_select_host,
// tgx_select_text_host, tgx_shuffled_rows_host) both go through these functions, so a machine without a GPU checks the
// kernels' index arithmetic.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) (u32 ids or u8 text bytes).  Output row k < M is
// source row rows[k]; out_offs = the exclusive prefix sums of the selected rows' lengths.  An index outside [0, S)
// contributes length 0 (and is reported by the callers), so it owns no output position and never becomes an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace tgx {

constexpr uint64_t kShuffleSalt = 0xD6E8FEB86659FD93ULL;  // TGX_SHUFFLE_SALT
constexpr uint32_t kSelectGroup = 4;                      // ids of a thread slot: one 16-byte store
constexpr uint32_t kSelectTile = kPackTile;               // ids per tile: the kernel's block of 256 threads x 4 ids
constexpr uint32_t kSelectByteGroup = 16;                 // text bytes of a thread slot: one 16-byte store
constexpr uint32_t kSelectByteTile = 4096;                // bytes per tile: 256 threads x 16 bytes
constexpr uint64_t kSelectNoBad = ~0ull;                  // the bad-index word when every index is in range

// tgx_shuffle_key: the rounds of fim_u01, all 64 bits kept
__host__ __device__ inline uint64_t shuffle_key(uint64_t seed, uint64_t g) {
    uint64_t x = seed ^ kShuffleSalt ^ (g * 0x9E3779B97F4A7C15ULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}

// is rows[k] a row of the source?  (a negative index is a large unsigned one)
__host__ __device__ inline bool select_in_range(int64_t row, uint64_t n_src) { return (uint64_t)row < n_src; }

// elements of output row k: the bounds rule
__host__ __device__ inline uint64_t select_out_len(const uint64_t* offs, uint64_t n_src, const int64_t* rows, uint64_t k) {
    const int64_t r = rows[k];
    return select_in_range(r, n_src) ? offs[r + 1] - offs[r] : 0;
}

// A walk over ascending output positions that all lie between the positions owned by output rows lo and hi (a tile's
// first and last), as FimCursor's: the first position searches [lo, hi], a later one stays on its row until the next
// row's start and then searches from the row after it.
struct SelectCursor {
    uint64_t k = 0, next = 0;     // the current output row and out_offs[k + 1]
    uint64_t start = 0, src = 0;  // out_offs[k] and offs[rows[k]]
    bool have = false;
};

// the cursor on the row that owns output position j < T'
__host__ __device__ inline void select_enter(SelectCursor& cur, const uint64_t* offs, const int64_t* rows, const uint64_t* out_offs, uint64_t lo,
                                             uint64_t hi, uint64_t j) {
    if (!cur.have || j >= cur.next) {
        cur.k = pack_find_row(out_offs, 0, cur.have ? cur.k + 1 : lo, hi, j);
        cur.start = out_offs[cur.k];
        cur.next = out_offs[cur.k + 1];
        cur.src = offs[rows[cur.k]];  // (a row that owns a position has an index in range)
        cur.have = true;
    }
}

// v[q] = the element at output position e0 + q for q < n_in <= W, the cursor going on from where it stands
template <uint32_t W, class T>
__host__ __device__ inline void select_walk(SelectCursor& cur, const T* data, const uint64_t* offs, const int64_t* rows, const uint64_t* out_offs,
                                            uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in, T (&v)[W]) {
#pragma unroll
    for (uint32_t q = 0; q < W; q++)
        if (q < n_in) {
            select_enter(cur, offs, rows, out_offs, lo, hi, e0 + q);
            v[q] = data[cur.src + (e0 + q - cur.start)];
        }
}

// A thread slot's walk.  lo / hi: the owners of the first and last position of the slot's tile.
template <uint32_t W, class T>
__host__ __device__ inline void select_group(const T* data, const uint64_t* offs, const int64_t* rows, const uint64_t* out_offs, uint64_t lo,
                                             uint64_t hi, uint64_t e0, uint32_t n_in, T (&v)[W]) {
    SelectCursor cur;
    select_walk<W, T>(cur, data, offs, rows, out_offs, lo, hi, e0, n_in, v);
}

// Text: does the whole slot of 16 bytes from e0 on lie inside the row the cursor stands on (entered for e0)?  Then its
// source bytes are consecutive, from select_slot_source on.
__host__ __device__ inline bool select_slot_inside(const SelectCursor& cur, uint64_t e0, uint32_t n_in) {
    return n_in == kSelectByteGroup && e0 + kSelectByteGroup <= cur.next;
}
__host__ __device__ inline uint64_t select_slot_source(const SelectCursor& cur, uint64_t e0) { return cur.src + (e0 - cur.start); }

// The 16 bytes that start r = 0 .. 3 bytes into d[0], as four little-endian dwords: d[0 .. 4] are the aligned dwords that
// cover them (d[4] is not used when r = 0).
__host__ __device__ inline void select_shift16(const uint32_t (&d)[5], uint32_t r, uint32_t (&w)[4]) {
    const uint32_t sh = 8 * r;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) w[q] = sh ? (d[q] >> sh) | (d[q + 1] << (32 - sh)) : d[q];
}

}  // namespace tgx
