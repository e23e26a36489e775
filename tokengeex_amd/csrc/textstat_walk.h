// The walk over the bytes of all rows laid end to end that the kernels of textstat.hip and wordstat.hip share (textstat.h
// has the tiling; DESIGN.md, sections L.13 and L.15): device code only, for a translation unit with kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_helpers.h"
#include "textstat.h"

namespace tgx {

constexpr uint32_t kTextstatBlock = 256;
static_assert(kTextstatBlock == kTextstatTile && kTextstatTile == 4 * kTextstatChunk && kTextstatChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kTextstatMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

// What a lane knows of its byte: `in`, the byte exists (the last chunk may be short); row, its owner, which begins at
// row_begin and ends before row_end; b, the byte.  A lane that is not in loads nothing.
struct TextLane {
    uint64_t pos, row_begin, row_end;
    uint32_t row;
    uint8_t b;
    bool in;
};

// The walk both kernels share, in gram_walk's shape.  A wave takes the chunk of 64 bytes that is its part of the
// block's tile; the owners of the chunk's ends are wave-uniform and found by galloping from the chunk before, and a
// lane's owner by a search between them.  body(c0, n_in, starts, lane_state) runs with the whole wave converged: n_in
// the chunk's bytes, starts the mask of its line starts.
template <class Body>
__device__ inline void textstat_walk(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows, Body body) {
    const uint64_t M = offs[n_rows];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_tiles = (M + kTextstatTile - 1) / kTextstatTile, per_block = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per_block, tile_end = tile_begin + per_block < n_tiles ? tile_begin + per_block : n_tiles;
    uint64_t hi = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t c0 = tile * kTextstatTile + (uint64_t)wave * kTextstatChunk;
        if (c0 >= M) break;  // (the last tile: the chunks after this one are empty too)
        const uint64_t c_last = tile_last(c0, kTextstatChunk, M);
        const uint64_t lo = tile == tile_begin ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(offs, lo, n_rows - 1, c_last);
        TextLane t = {c0 + lane, 0, 0, (uint32_t)lo, 0, false};
        t.in = t.pos <= c_last;
        if (t.in) {
            const uint64_t i = pack_find_row(offs, 0, lo, hi, t.pos);
            t.row = (uint32_t)i;
            t.row_begin = offs[i];
            t.row_end = offs[i + 1];
            t.b = text[t.pos];
        }
        // a line start: its row's first byte, or the byte after a '\n' of its row (which, not being the row's first
        // byte, has its row's byte before it).  The byte before the chunk is wave-uniform.
        const bool nl_before = c0 > 0 && text[c0 - 1] == '\n';
        const uint64_t after_nl = (__ballot(t.in && t.b == '\n') << 1) | (nl_before ? 1ull : 0ull);
        const uint64_t starts = __ballot(t.in && (t.pos == t.row_begin || ((after_nl >> lane) & 1ull)));
        body(c0, (uint32_t)(c_last - c0) + 1, starts, t);
    }
}

}  // namespace tgx
