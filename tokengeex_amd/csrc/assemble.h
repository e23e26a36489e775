// Index arithmetic of the assembly of a sample-level result from the result over the non-special segments and the split
// plan (include/tgx.h: tgx_assemble_result).  The kernels of assemble.hip and the host twin in host_twins.cpp
// (tgx_assemble_host) both go through these functions, so a machine without a GPU checks the kernels' index arithmetic.
//
// Segment k of K is special (seg_special[k] >= 0: one id, V + seg_special[k]) or the next encoded segment.  rank[k] =
// r_k = encoded segments before k (rank[K] = E), so k - rank[k] specials lie before k.  offs = o[0..E] are the offsets
// of the segment-level result.  Segment k starts at output position D_k = o[r_k] + (k - r_k); D_K = T'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kAssembleGroup = 4;    // consecutive positions of a thread slot: one 16-byte store
constexpr uint32_t kAssembleTile = 1024;  // positions per tile: the kernel's block of 256 threads x 4 positions

// D_k, k <= K
__host__ __device__ inline uint64_t assemble_seg_start(const uint64_t* offs, const uint64_t* rank, uint64_t k) {
    const uint64_t r = rank[k];
    return offs[r] + (k - r);
}

// The segment that owns position j is the LARGEST k with D_k <= j (pack_find_row of tile_fill.h over D with A = 0), so a run
// of segments with equal D (encoded segments without ids) is stepped over.
// A walk over ascending positions that all lie between the positions owned by segments lo and hi (a tile's first and
// last): the first position searches [lo, hi], a later one stays on its segment until the next one's start and then
// searches from the segment after it.  What does not change inside a segment is read once per segment.
struct AssembleCursor {
    uint64_t k = 0, next = 0;  // the current segment and D_{k+1}
    uint64_t shift = 0;        // k - r_k: position j of an encoded segment k is ids[j - shift] (= ids[o[r_k] + (j - D_k)])
    int32_t special = -1;      // seg_special[k]
    bool have = false;
};

// the id at position j < T'
__host__ __device__ inline uint32_t assemble_at(AssembleCursor& cur, const uint32_t* ids, const uint64_t* D, const uint64_t* rank,
                                                const int32_t* seg_special, uint32_t vocab_size, uint64_t lo, uint64_t hi, uint64_t j) {
    if (!cur.have || j >= cur.next) {
        cur.k = pack_find_row(D, 0, cur.have ? cur.k + 1 : lo, hi, j);
        cur.next = D[cur.k + 1];
        cur.special = seg_special[cur.k];
        cur.shift = cur.special < 0 ? cur.k - rank[cur.k] : 0;
        cur.have = true;
    }
    return cur.special >= 0 ? vocab_size + (uint32_t)cur.special : ids[j - cur.shift];
}

// A thread slot's walk: v[q] = the id at position e0 + q for q < n_in <= kAssembleGroup.  lo / hi: the owners of the
// first and last position of the slot's tile.
__host__ __device__ inline void assemble_group(const uint32_t* ids, const uint64_t* D, const uint64_t* rank, const int32_t* seg_special,
                                               uint32_t vocab_size, uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in,
                                               uint32_t (&v)[kAssembleGroup]) {
    AssembleCursor cur;
#pragma unroll
    for (uint32_t q = 0; q < kAssembleGroup; q++)
        if (q < n_in) v[q] = assemble_at(cur, ids, D, rank, seg_special, vocab_size, lo, hi, e0 + q);
}

}  // namespace tgx
