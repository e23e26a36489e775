// The output-centric tiled fill that the transforms of a resident result or corpus share (assemble.hip, fim.hip,
// select.hip, layout.hip, spans.hip, decode.hip, and their twins in host_twins.cpp).  The output is
// n_out consecutive positions, each owned by one row of an ascending array of starts.  A tile of TILE positions goes to a
// block, a slot of GROUP consecutive positions to a thread; the owners of the tile's first and last position are searched
// once per tile and bound every search inside it.  A transform supplies the owners (a search over its array), the walk
// of a slot between those two owners, and the store.  The kernels and the host twins go through the same functions, so
// a machine without a GPU checks the loop's arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

// row i of an array of starts with A extra positions per row starts at P_i = offs[i] + i·A
__host__ __device__ inline uint64_t pack_row_start(const uint64_t* offs, uint64_t A, uint64_t i) { return offs[i] + i * A; }

// The row that owns position j: the LARGEST i in [lo, hi] with P_i <= j, so a run of rows with equal P (rows that
// contribute nothing) is stepped over and its last row, the one with P_{i+1} > j, is found.  Needs P_lo <= j and the
// owner to be <= hi.
__host__ __device__ inline uint64_t pack_find_row(const uint64_t* offs, uint64_t A, uint64_t lo, uint64_t hi, uint64_t j) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (pack_row_start(offs, A, mid) <= j)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the last position of the tile of `tile` positions that starts at t0 (t0 < n)
__host__ __device__ inline uint64_t tile_last(uint64_t t0, uint64_t tile, uint64_t n) { return t0 + tile - 1 < n ? t0 + tile - 1 : n - 1; }
// the first position whose owner a tile's slots ask for: `back` positions before the tile belong to it
__host__ __device__ inline uint64_t tile_first(uint64_t t0, uint64_t back) { return t0 >= back ? t0 - back : 0; }

// The host loop.  Positions below n_search <= n_out have owners (a fill may run on over padding); owner(j) is the owner of
// position j < n_search; body(lo, hi, e0, n_in) fills the slot of n_in <= group positions from e0 on, lo / hi being the
// owners of tile_first and tile_last of its tile, and returns false to stop.  -> false when a body stopped the loop
template <class Owner, class Body>
inline bool tiled_fill_host(uint64_t n_out, uint64_t n_search, uint32_t tile, uint32_t group, uint32_t back, Owner owner, Body body) {
    uint64_t lo = 0, hi = 0;
    for (uint64_t t0 = 0; t0 < n_out; t0 += tile) {
        if (t0 < n_search) {
            lo = owner(tile_first(t0, back));
            hi = owner(tile_last(t0, tile, n_search));
        }
        for (uint64_t e0 = t0; e0 < n_out && e0 < t0 + tile; e0 += group) {
            const uint32_t n_in = n_out - e0 < group ? (uint32_t)(n_out - e0) : group;
            if (!body(lo, hi, e0, n_in)) return false;
        }
    }
    return true;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// The device loop of a block of TILE / GROUP threads on a capped grid that strides over the tiles: the twin of
// tiled_fill_host, two threads searching the owners into LDS.  (n_search differs from n_out only in the pack fill, whose
// kernel keeps its loop written out, so today every kernel passes n_out twice and only the host twin of pack uses it.)
template <uint32_t TILE, uint32_t GROUP, uint32_t BACK = 0, class Owner, class Body>
__device__ inline void tiled_fill(uint64_t n_out, uint64_t n_search, Owner owner, Body body) {
    __shared__ uint64_t s_own[2];
    const uint64_t n_tiles = (n_out + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * TILE;
        if (threadIdx.x < 2 && t0 < n_search) s_own[threadIdx.x] = owner(threadIdx.x ? tile_last(t0, TILE, n_search) : tile_first(t0, BACK));
        __syncthreads();  // s_own is written
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * GROUP;
        if (e0 < n_out) {
            const uint32_t n_in = n_out - e0 < GROUP ? (uint32_t)(n_out - e0) : GROUP;
            body(s_own[0], s_own[1], e0, n_in);
        }
        __syncthreads();  // s_own is rewritten for the next tile
    }
}

// A slot's four ids or sixteen bytes: one 16-byte store when the slot is full (out is 16-byte aligned, checked by the
// launchers, and e0 a multiple of the slot), else the tail of the last tile, element by element.
__device__ inline void store_ids4(uint32_t* __restrict__ out, uint64_t e0, const uint32_t (&v)[4], uint32_t n_in) {
    if (n_in == 4) {
        *reinterpret_cast<uint4*>(out + e0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (uint32_t q = 0; q < n_in; q++) out[e0 + q] = v[q];
    }
}
__device__ inline void store_bytes16(uint8_t* __restrict__ out, uint64_t e0, const uint8_t (&v)[16], uint32_t n_in) {
    if (n_in == 16) {
        uint32_t w[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            w[q] = (uint32_t)v[4 * q] | ((uint32_t)v[4 * q + 1] << 8) | ((uint32_t)v[4 * q + 2] << 16) | ((uint32_t)v[4 * q + 3] << 24);
        *reinterpret_cast<uint4*>(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 16; q++)
            if (q < n_in) out[e0 + q] = v[q];
    }
}

// launch geometry: a memory-bound kernel takes a capped grid and strides over the rest
inline uint32_t capped_grid(uint64_t blocks, uint64_t cap) { return (uint32_t)(blocks < cap ? (blocks ? blocks : 1) : cap); }
inline uint32_t grid_for(uint64_t items, uint64_t block, uint64_t cap) { return capped_grid((items + block - 1) / block, cap); }

#endif  // TGX_HOST_ONLY

}  // namespace tgx
