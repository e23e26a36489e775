// Near-duplicate rows on the device (include/tgx.h: tgx_result_minhash_device, tgx_corpus_minhash_device,
// tgx_minhash_bands_device, tgx_minhash_near_first_device; minhash.h has the arithmetic, the tiling and the rules;
// DESIGN.md, section L.11).  The signature kernel is the compute-bound one: rows x shingles x permutations multiply-adds.
// A row is 0 to 10^8 elements, so no unit of work is a row: the rows' shingle positions are laid end to end, a wave takes
// 64 consecutive positions, and a minimum may be taken in any order and in any number of parts to the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minhash.h"
#include "scan_helpers.h"
#include "shingle_load.h"

namespace tgx {

namespace {

constexpr uint32_t kMinhashBlock = 256;
static_assert(kMinhashBlock == kMinhashTile && kMinhashTile == 4 * kMinhashChunk && kMinhashChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kMinhashMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

struct MinhashPositions {
    const uint64_t* offs;
    uint64_t n_rows;
    uint32_t width;
    __host__ __device__ uint64_t operator()(uint64_t k) const { return minhash_row_positions(offs, n_rows, width, k); }
};

// sig[i][k] = the minimum of v_k over the shingles of row i.  A wave takes the chunk of 64 positions that is its part
// of the block's tile.  First lane = shingle: the owner row of the position (a search between the owners of the chunk's
// ends, which are wave-uniform and found by galloping from the chunk before) and the shingle's hash.  Then lane =
// permutation: the wave walks its 64 shingles, the hash of each broadcast to every lane, and each lane keeps the running
// minima of its P = ceil(K / 64) permutations in registers: no reduction across lanes anywhere.  When the owner
// changes, and at the chunk's end, the minima go to the row: a plain store when the row lies inside the chunk, else a
// 32-bit atomicMin (sig was pre-set to 0xFFFFFFFF by the launcher).
template <bool kText, int P>
__global__ __launch_bounds__(kMinhashBlock) void minhash_sig_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                    const uint64_t* __restrict__ sh_offs, uint32_t width, uint32_t K, uint64_t hs,
                                                                    uint64_t ps, uint32_t* sig) {
    const uint64_t M = sh_offs[n_rows];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t a_lo[P], a_hi[P], mn[P];
    uint64_t bb[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        uint64_t a;
        minhash_perm(ps, lane + 64u * p, a, bb[p]);
        a_lo[p] = (uint32_t)a;
        a_hi[p] = (uint32_t)(a >> 32);
        mn[p] = kMinhashNoSig;
    }
    const uint64_t n_tiles = (M + kMinhashTile - 1) / kMinhashTile, per_block = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per_block, tile_end = tile_begin + per_block < n_tiles ? tile_begin + per_block : n_tiles;
    uint64_t hi = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t c0 = tile * kMinhashTile + (uint64_t)wave * kMinhashChunk;
        if (c0 >= M) break;  // (the last tile: the chunks after this one are empty too)
        const uint64_t c_last = tile_last(c0, kMinhashChunk, M);
        const uint64_t lo = tile == tile_begin ? pack_find_row(sh_offs, 0, 0, n_rows - 1, c0) : dedup_find_from(sh_offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(sh_offs, lo, n_rows - 1, c_last);
        // lane = shingle
        const uint64_t pos = c0 + lane;
        uint64_t h = 0;
        uint32_t row = (uint32_t)lo;
        if (pos <= c_last) {
            const uint64_t i = pack_find_row(sh_offs, 0, lo, hi, pos);
            const uint64_t t = pos - sh_offs[i], b0 = offs[i];
            const uint32_t len = minhash_shingle_len(offs[i + 1] - b0, width);
            uint64_t w[8];
            if constexpr (kText)
                minhash_load_text(static_cast<const uint8_t*>(data_), b0 + t, len, w);
            else
                minhash_load_ids(static_cast<const uint32_t*>(data_), b0 + t, len, w);
            h = minhash_hash_words(w, len * (kText ? 1u : 4u), hs);
            row = (uint32_t)i;
        }
        const uint32_t h_lo = (uint32_t)h, h_hi = (uint32_t)(h >> 32);
        // lane = permutation.  The positions at which a new row begins, as a wave-uniform mask: the walk is then a loop
        // over stretches of one row, with nothing but the two broadcasts and the arithmetic inside a stretch
        const uint32_t n_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(c_last - c0) + 1));
        const uint32_t row_before = (uint32_t)__shfl_up((int)row, 1, 64);
        uint64_t begins = __ballot(lane > 0 && pos <= c_last && row != row_before);
        auto flush = [&](uint32_t r) {
            const bool inside = minhash_row_inside(sh_offs, r, c0);
            uint32_t* out = sig + (uint64_t)r * K;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const uint32_t k = lane + 64u * p;
                if (k < K) {
                    if (inside)
                        out[k] = mn[p];
                    else
                        atomicMin(&out[k], mn[p]);
                }
                mn[p] = kMinhashNoSig;
            }
        };
        for (uint32_t t = 0; t < n_in;) {
            const uint32_t t_end = begins ? (uint32_t)__builtin_ctzll(begins) : n_in;  // (every bit left is above t)
            begins &= begins - 1;
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)row, (int)t);
            for (; t < t_end; t++) {
                const uint32_t x_lo = (uint32_t)__builtin_amdgcn_readlane((int)h_lo, (int)t), x_hi = (uint32_t)__builtin_amdgcn_readlane((int)h_hi, (int)t);
                const uint64_t x = (uint64_t)x_lo | ((uint64_t)x_hi << 32);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const uint32_t v = minhash_value((uint64_t)a_lo[p] | ((uint64_t)a_hi[p] << 32), bb[p], x);
                    mn[p] = v < mn[p] ? v : mn[p];
                }
            }
            flush(r);
        }
    }
}

// the keys of every (row, band): one thread each, the threads of a row side by side
__global__ __launch_bounds__(kMinhashBlock) void minhash_band_keys_kernel(const uint32_t* __restrict__ sig, uint64_t n_rows, uint32_t K, uint32_t B,
                                                                          uint64_t seed, uint64_t* __restrict__ keys, uint64_t* __restrict__ keys_t) {
    const uint64_t n = n_rows * B;
    const uint32_t r = K / B;
    for (uint64_t x = (uint64_t)blockIdx.x * kMinhashBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kMinhashBlock) {
        const uint64_t i = x / B;
        const uint32_t b = (uint32_t)(x - i * B);
        const uint64_t key = minhash_band_key(sig + i * K, r, b, seed);
        if (keys) keys[x] = key;
        if (keys_t) keys_t[(uint64_t)b * n_rows + i] = key;
    }
}

__global__ __launch_bounds__(kMinhashBlock) void minhash_iota_kernel(uint32_t* __restrict__ rows, uint64_t n_rows) {
    for (uint64_t i = (uint64_t)blockIdx.x * kMinhashBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kMinhashBlock) rows[i] = (uint32_t)i;
}

// the run rule of dedup.h on one band's sorted (key, row): one thread per sorted position
__global__ __launch_bounds__(kMinhashBlock) void minhash_heads_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rows, uint64_t n_rows,
                                                                      uint32_t B, uint32_t b, int64_t* __restrict__ heads) {
    for (uint64_t i = (uint64_t)blockIdx.x * kMinhashBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kMinhashBlock)
        heads[(uint64_t)rows[i] * B + b] = (int64_t)rows[dedup_run_head(keys, i)];
}

// first0 of every row: a wave per row, the lanes over the K values of the two signatures, the bands one after another
__global__ __launch_bounds__(kMinhashBlock) void minhash_verify_kernel(const uint32_t* __restrict__ sig, uint64_t n_rows, uint32_t K,
                                                                       const int64_t* __restrict__ heads, uint32_t B, uint32_t min_agree,
                                                                       int64_t* __restrict__ first0) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + wave; i < n_rows; i += (uint64_t)gridDim.x * 4) {
        uint64_t best = i;
        const uint32_t* mine = sig + i * K;
        for (uint32_t b = 0; b < B; b++) {
            const int64_t head = heads[i * B + b];
            if (!minhash_looks_at(head, best)) continue;
            const uint32_t* theirs = sig + (uint64_t)head * K;
            uint32_t agree = 0;
            for (uint32_t k0 = 0; k0 < K; k0 += 64) {  // (every lane takes every step: the ballot counts the whole wave)
                const uint32_t k = k0 + lane;
                const bool eq = k < K && mine[k] == theirs[k];
                agree += (uint32_t)__popcll(__ballot(eq));
            }
            if (minhash_takes(agree, min_agree)) best = (uint64_t)head;
        }
        if (lane == 0) first0[i] = (int64_t)best;
    }
}

__global__ __launch_bounds__(kMinhashBlock) void minhash_hop_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out, uint64_t n_rows,
                                                                    unsigned long long* changed) {
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kMinhashBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kMinhashBlock) {
        const int64_t f = minhash_hop(in, i);
        out[i] = f;
        any = any || f != in[i];
    }
    if (__ballot(any) && (threadIdx.x & 63u) == 0) atomicAdd(changed, 1ull);
}

__global__ __launch_bounds__(kMinhashBlock) void minhash_count_kernel(const int64_t* __restrict__ first, uint64_t n_rows, unsigned long long* count) {
    unsigned long long mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kMinhashBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kMinhashBlock) mine += first[i] == (int64_t)i;
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(count, mine);
}

inline uint32_t row_grid(uint64_t n) { return grid_for(n, kMinhashBlock, kMinhashMaxBlocks); }

template <bool kText>
hipError_t launch_sig(int P, dim3 grid, hipStream_t stream, const DedupRows& rows, const uint64_t* sh_offs, uint32_t width, uint32_t K, uint64_t hs,
                      uint64_t ps, uint32_t* sig) {
    const dim3 block(kMinhashBlock);
#define TGX_MINHASH_LAUNCH(PP) \
    hipLaunchKernelGGL((minhash_sig_kernel<kText, PP>), grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, sh_offs, width, K, hs, ps, sig)
    if (P <= 1)
        TGX_MINHASH_LAUNCH(1);
    else if (P <= 2)
        TGX_MINHASH_LAUNCH(2);
    else if (P <= 4)
        TGX_MINHASH_LAUNCH(4);
    else if (P <= 8)
        TGX_MINHASH_LAUNCH(8);
    else
        TGX_MINHASH_LAUNCH(16);
#undef TGX_MINHASH_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t minhash_scan_bytes(uint64_t n_rows, size_t* scan_bytes) {
    *scan_bytes = 0;
    uint64_t* out = nullptr;
    return scan_of(MinhashPositions{}, n_rows + 1, out, nullptr, *scan_bytes, nullptr);
}

hipError_t launch_minhash_sig(const DedupRows& rows, uint32_t width, uint32_t n_perm, uint64_t seed, uint64_t* sh_offs, void* scan_tmp, size_t scan_bytes,
                              uint32_t* sig, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    hipError_t e = scan_of(MinhashPositions{rows.offs, rows.n_rows, width}, rows.n_rows + 1, sh_offs, scan_tmp, scan_bytes, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sig, 0xFF, (size_t)rows.n_rows * n_perm * 4, stream)) != hipSuccess) return e;
    // (the positions' total stays on the device: the grid comes from its bound, a position per element and one more per row)
    const dim3 grid(grid_for(rows.n_elems + rows.n_rows, kMinhashTile, kMinhashMaxBlocks));
    const int P = (int)((n_perm + 63) / 64);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed)), ps = minhash_perm_seed(seed);
    return rows.elem_bytes == 1 ? launch_sig<true>(P, grid, stream, rows, sh_offs, width, n_perm, hs, ps, sig)
                                : launch_sig<false>(P, grid, stream, rows, sh_offs, width, n_perm, hs, ps, sig);
}

hipError_t launch_minhash_band_keys(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed, uint64_t* keys, uint64_t* keys_t,
                                    hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(minhash_band_keys_kernel, dim3(row_grid(n_rows * bands)), dim3(kMinhashBlock), 0, stream, sig, n_rows, n_perm, bands, seed, keys,
                       keys_t);
    return hipGetLastError();
}

hipError_t launch_minhash_iota(uint32_t* rows, uint64_t n_rows, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(minhash_iota_kernel, dim3(row_grid(n_rows)), dim3(kMinhashBlock), 0, stream, rows, n_rows);
    return hipGetLastError();
}

hipError_t launch_minhash_heads(const uint64_t* sorted_keys, const uint32_t* sorted_rows, uint64_t n_rows, uint32_t bands, uint32_t b, int64_t* heads,
                                hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(minhash_heads_kernel, dim3(row_grid(n_rows)), dim3(kMinhashBlock), 0, stream, sorted_keys, sorted_rows, n_rows, bands, b, heads);
    return hipGetLastError();
}

hipError_t launch_minhash_verify(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, const int64_t* heads, uint32_t bands, uint32_t min_agree,
                                 int64_t* first0, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(minhash_verify_kernel, dim3(grid_for(n_rows, 4, 8 * kMinhashMaxBlocks)), dim3(kMinhashBlock), 0, stream, sig, n_rows, n_perm, heads,
                       bands, min_agree, first0);
    return hipGetLastError();
}

hipError_t launch_minhash_hop(const int64_t* in, int64_t* out, uint64_t n_rows, unsigned long long* changed, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(changed, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(minhash_hop_kernel, dim3(row_grid(n_rows)), dim3(kMinhashBlock), 0, stream, in, out, n_rows, changed);
    return hipGetLastError();
}

hipError_t launch_minhash_count(const int64_t* first, uint64_t n_rows, unsigned long long* count, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || n_rows == 0) return e;
    hipLaunchKernelGGL(minhash_count_kernel, dim3(row_grid(n_rows)), dim3(kMinhashBlock), 0, stream, first, n_rows, count);
    return hipGetLastError();
}

}  // namespace tgx
