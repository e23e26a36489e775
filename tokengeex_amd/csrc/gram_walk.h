// The walk over the elements of all rows laid end to end that the gram kernels (gram.hip) and the repetition kernels
// (repeat.hip) share: GramLane and gram_walk, moved here from gram.hip as shingle_load.h took the loaders.  gram.h has
// the tiling and the validity rule.  For translation units with kernels only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram.h"
#include "shingle_load.h"

namespace tgx {

// What a lane knows of its element: `in`, the element exists (the last chunk may be short); row, its owner; valid and
// key, of the gram that begins there.  An invalid position loads nothing.
struct GramLane {
    uint64_t pos, key;
    uint32_t row;
    bool in, valid;
};

// The walk the kernels share.  A wave takes the chunk of 64 elements that is its part of the block's tile; the owners
// of the chunk's ends are wave-uniform and found by galloping from the chunk before, and a lane's owner by a search
// between them.  body(c0, n_in, lane_state) runs with the whole wave converged, n_in being the chunk's elements.
// kKeys = false (repeat_cover_kernel) leaves the key 0 and never reads data_: the owners and the validity alone.
template <bool kText, bool kKeys = true, class Body>
__device__ inline void gram_walk(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t width, uint64_t hs,
                                 Body body) {
    const uint64_t M = offs[n_rows];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_tiles = (M + kGramTile - 1) / kGramTile, per_block = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per_block, tile_end = tile_begin + per_block < n_tiles ? tile_begin + per_block : n_tiles;
    uint64_t hi = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t c0 = tile * kGramTile + (uint64_t)wave * kGramChunk;
        if (c0 >= M) break;  // (the last tile: the chunks after this one are empty too)
        const uint64_t c_last = tile_last(c0, kGramChunk, M);
        const uint64_t lo = tile == tile_begin ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(offs, lo, n_rows - 1, c_last);
        GramLane g = {c0 + lane, 0, (uint32_t)lo, false, false};
        g.in = g.pos <= c_last;
        if (g.in) {
            const uint64_t i = pack_find_row(offs, 0, lo, hi, g.pos);
            g.row = (uint32_t)i;
            g.valid = gram_valid(g.pos, width, offs[i + 1]);
            if constexpr (kKeys) {
                if (g.valid) {
                    uint64_t w[8];
                    if constexpr (kText)
                        minhash_load_text(static_cast<const uint8_t*>(data_), g.pos, width, w);
                    else
                        minhash_load_ids(static_cast<const uint32_t*>(data_), g.pos, width, w);
                    g.key = minhash_hash_words(w, width * (kText ? 1u : 4u), hs);
                }
            }
        }
        body(c0, (uint32_t)(c_last - c0) + 1, g);
    }
}

}  // namespace tgx
