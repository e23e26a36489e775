// The device front end: a resident corpus split at special tokens and the segments between them packed with the CRLF
// pass applied, in HBM (include/tgx.h: tgx_corpus_split_specials; front.h has the index arithmetic and the data flow).
// The byte kernels (mark, keep, pack) take tiles of 4096 consecutive bytes on a capped striding grid, 16 bytes per thread
// with one 16-byte load; the kernels between them take one candidate, sample or segment per thread.  Every order comes
// from a scan (rocPRIM, as assemble.hip's and spans.hip's), none from an atomic, so the result does not depend on timing.
// The text is read twice (mark, pack) and written once; between the two go 3 bits per byte of masks (three 16-bit masks per slot).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "front.h"
#include "kernels.h"
#include "scan_helpers.h"

namespace tgx {

namespace {

constexpr uint32_t kFrontBlock = 256;
static_assert(kFrontBlock * kFrontGroup == kFrontTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kFrontMaxBlocks = 4096;  // memory-bound: a capped grid that strides over the rest

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

__global__ __launch_bounds__(kFrontBlock) void front_mark_kernel(FrontParams p) {
    __shared__ uint32_t s_mask[8];
    __shared__ uint64_t s_row[2];
    __shared__ uint32_t s_part[kFrontBlock / 64];
    if (threadIdx.x < 8) s_mask[threadIdx.x] = p.tab.first_mask[threadIdx.x];
    FrontTables tab = p.tab;
    tab.first_mask = s_mask;
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFrontTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.offs, 0, 0, p.n_samples - 1, threadIdx.x ? tile_last(t0, kFrontTile, n) : t0);
        __syncthreads();
        const uint64_t p0 = t0 + (uint64_t)threadIdx.x * kFrontGroup;
        uint32_t hits = 0;
        if (p0 < n) {
            const uint32_t n_in = n - p0 < kFrontGroup ? (uint32_t)(n - p0) : kFrontGroup;
            uint8_t v[kFrontGroup];
            load_slot(p.text, p0, v);
            const uint8_t next = p0 + kFrontGroup < n ? p.text[p0 + kFrontGroup] : 0;
            uint32_t cr = 0;
            hits = front_mark_slot(tab, p.text, p.offs, s_row[0], s_row[1], p0, n_in, v, next, &cr);
            p.hit_mask[p0 / kFrontGroup] = (uint16_t)hits;
            p.crlf_mask[p0 / kFrontGroup] = (uint16_t)cr;
        }
        uint32_t total;
        block_exclusive_sum<kFrontBlock>(front_popc(hits), s_part, &total);  // (its barriers also keep s_row for the whole tile)
        if (threadIdx.x == 0) p.tile_count[tile] = total;
    }
}

__global__ __launch_bounds__(kFrontBlock) void front_candidates_kernel(FrontParams p) {
    __shared__ uint32_t s_mask[8];
    __shared__ uint64_t s_row[2];
    __shared__ uint32_t s_part[kFrontBlock / 64];
    if (threadIdx.x < 8) s_mask[threadIdx.x] = p.tab.first_mask[threadIdx.x];
    FrontTables tab = p.tab;
    tab.first_mask = s_mask;
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = p.tile_base[tile];
        if (p.tile_base[tile + 1] == base) continue;  // (the whole block takes the same way)
        const uint64_t t0 = tile * kFrontTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.offs, 0, 0, p.n_samples - 1, threadIdx.x ? tile_last(t0, kFrontTile, n) : t0);
        __syncthreads();
        const uint64_t p0 = t0 + (uint64_t)threadIdx.x * kFrontGroup;
        const uint32_t hits = p0 < n ? p.hit_mask[p0 / kFrontGroup] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive_sum<kFrontBlock>(front_popc(hits), s_part, &total);
        if (hits)
            front_write_slot(tab, p.text, p.offs, s_row[0], s_row[1], p0, hits, base + before, p.cand_pos, p.cand_end, p.cand_special, p.cand_sample);
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

__global__ __launch_bounds__(kFrontBlock) void front_resolve_kernel(FrontParams p) {
    for (uint64_t c = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; c < p.n_cand; c += (uint64_t)gridDim.x * kFrontBlock)
        if (front_is_head(p.cand_pos, p.pm, c)) front_resolve_run(p.cand_pos, p.cand_end, p.pm, p.n_cand, c, p.acc_end);
}

// cand_segs[0..C] (entry C is 0 and belongs to the scan) and first[0..S]
__global__ __launch_bounds__(kFrontBlock) void front_cand_segs_kernel(FrontParams p) {
    const uint64_t n = p.n_cand > p.n_samples ? p.n_cand + 1 : p.n_samples + 1;
    for (uint64_t x = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kFrontBlock) {
        if (x <= p.n_cand) p.cand_segs[x] = x < p.n_cand ? front_cand_segs(p.cand_pos, p.acc_end, p.la, p.cand_sample, p.offs, x) : 0u;
        if (x <= p.n_samples) p.first[x] = front_first_cand(p.cand_pos, p.n_cand, p.offs[x]);
    }
}

// sample_segs[0..S] (entry S is 0 and belongs to the scan)
__global__ __launch_bounds__(kFrontBlock) void front_sample_segs_kernel(FrontParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; i <= p.n_samples; i += (uint64_t)gridDim.x * kFrontBlock) {
        uint64_t tail;
        p.sample_segs[i] = i < p.n_samples ? front_sample_segs(p.offs, p.first, p.seg_sum, p.la, i, &tail) : 0u;
    }
}

// the segments of the accepted candidates and the samples' tails
__global__ __launch_bounds__(kFrontBlock) void front_segments_kernel(FrontParams p) {
    const uint64_t n = p.n_cand > p.n_samples ? p.n_cand : p.n_samples;
    for (uint64_t x = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kFrontBlock) {
        if (x < p.n_cand && p.acc_end[x]) {
            const uint64_t i = p.cand_sample[x];
            uint64_t k = p.seg_offs[i] + (p.seg_sum[x] - p.seg_sum[p.first[i]]);
            if (p.cand_segs[x] == 2) {
                p.seg_begin[k] = front_cursor_before(p.la, x, p.offs[i]);
                p.seg_end[k] = p.cand_pos[x];
                p.seg_special[k] = -1;
                k++;
            }
            p.seg_begin[k] = p.cand_pos[x];
            p.seg_end[k] = p.cand_end[x];
            p.seg_special[k] = (int32_t)p.cand_special[x];
        }
        if (x < p.n_samples) {
            uint64_t tail;
            front_sample_segs(p.offs, p.first, p.seg_sum, p.la, x, &tail);
            if (tail < p.offs[x + 1]) {
                const uint64_t k = p.seg_offs[x + 1] - 1;
                p.seg_begin[k] = tail;
                p.seg_end[k] = p.offs[x + 1];
                p.seg_special[k] = -1;
            }
        }
    }
}

__global__ __launch_bounds__(kFrontBlock) void front_encoded_kernel(FrontParams p) {
    for (uint64_t k = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; k < p.n_segs; k += (uint64_t)gridDim.x * kFrontBlock)
        if (p.seg_special[k] < 0) {
            p.enc_begin[p.rank[k]] = p.seg_begin[k];
            p.enc_end[p.rank[k]] = p.seg_end[k];
        }
}

__global__ __launch_bounds__(kFrontBlock) void front_keep_kernel(FrontParams p) {
    __shared__ uint64_t s_enc[2];
    __shared__ uint32_t s_part[kFrontBlock / 64];
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFrontTile;
        if (threadIdx.x < 2) s_enc[threadIdx.x] = front_first_enc(p.enc_end, 0, p.n_enc, threadIdx.x ? tile_last(t0, kFrontTile, n) : t0);
        __syncthreads();
        const uint64_t p0 = t0 + (uint64_t)threadIdx.x * kFrontGroup;
        uint32_t keep = 0, begins = 0;
        uint64_t first_begin = 0;
        if (p0 < n) {
            const uint32_t n_in = n - p0 < kFrontGroup ? (uint32_t)(n - p0) : kFrontGroup;
            keep = front_keep_slot(p.enc_begin, p.enc_end, p.n_enc, s_enc[0], s_enc[1], p0, n_in, p.crlf_mask[p0 / kFrontGroup], p.crlf != 0, &begins, &first_begin);
            p.keep_mask[p0 / kFrontGroup] = (uint16_t)keep;
        }
        uint32_t total;
        const uint32_t before = block_exclusive_sum<kFrontBlock>(front_popc(keep), s_part, &total);  // (its barriers also keep s_enc for the whole tile)
        if (begins) front_slot_begins(keep, begins, first_begin, before, p.enc_local);
        if (threadIdx.x == 0) p.tile_count[tile] = total;
    }
}

// out_offs[0..E]
__global__ __launch_bounds__(kFrontBlock) void front_offsets_kernel(FrontParams p) {
    const uint64_t n_tiles = (p.n_bytes + kFrontTile - 1) / kFrontTile;
    for (uint64_t e = (uint64_t)blockIdx.x * kFrontBlock + threadIdx.x; e <= p.n_enc; e += (uint64_t)gridDim.x * kFrontBlock)
        p.out_offs[e] = e < p.n_enc ? p.tile_base[p.enc_begin[e] / kFrontTile] + p.enc_local[e] : p.tile_base[n_tiles];
}

__global__ __launch_bounds__(kFrontBlock) void front_pack_kernel(FrontParams p) {
    __shared__ uint32_t s_part[kFrontBlock / 64];
    uint8_t* __restrict__ out = p.out;
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = p.tile_base[tile];
        if (p.tile_base[tile + 1] == base) continue;  // (the whole block takes the same way)
        const uint64_t p0 = tile * kFrontTile + (uint64_t)threadIdx.x * kFrontGroup;
        const uint32_t keep = p0 < n ? p.keep_mask[p0 / kFrontGroup] : 0u;
        uint32_t total;
        uint64_t at = base + block_exclusive_sum<kFrontBlock>(front_popc(keep), s_part, &total);
        if (!keep) continue;  // (after the block's barriers)
        uint8_t v[kFrontGroup];
        load_slot(p.text, p0, v);
#pragma unroll
        for (uint32_t q = 0; q < kFrontGroup; q++)
            if ((keep >> q) & 1u) out[at++] = v[q];
    }
}

uint64_t tiles_of(uint64_t n) { return (n + kFrontTile - 1) / kFrontTile; }

hipError_t max_scan(const uint64_t* in, uint64_t* out, uint64_t n, void* temp, size_t& temp_bytes, hipStream_t stream) {
    return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n, rocprim::maximum<uint64_t>(), stream);
}
hipError_t wide_scan(const uint32_t* in, uint64_t* out, uint64_t n, void* temp, size_t& temp_bytes, hipStream_t stream) {
    auto it = rocprim::make_transform_iterator(in, Widen());
    return rocprim::exclusive_scan(temp, temp_bytes, it, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), stream);
}

#define FRONT_TRY(expr)                    \
    do {                                   \
        const hipError_t _e = (expr);      \
        if (_e != hipSuccess) return _e;   \
    } while (0)

}  // namespace

// room for every scan of the launchers below over up to n elements (n at least the larger of tiles, C, S and K, plus 1)
hipError_t front_scan_temp_bytes(uint64_t n, size_t* bytes) {
    size_t a = 0, b = 0, c = 0, d = 0;
    FRONT_TRY(sum_scan(nullptr, nullptr, n, nullptr, a, nullptr));
    FRONT_TRY(max_scan(nullptr, nullptr, n, nullptr, b, nullptr));
    FRONT_TRY(wide_scan(nullptr, nullptr, n, nullptr, c, nullptr));
    FRONT_TRY(assemble_scan_temp_bytes(n, &d));
    *bytes = a > b ? a : b;
    if (c > *bytes) *bytes = c;
    if (d > *bytes) *bytes = d;
    return hipSuccess;
}

// hit_mask, crlf_mask and tile_base[0..tiles]: tile_base[tiles] = C.  Needs N >= 1 and S >= 1.
hipError_t launch_front_mark(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_bytes == 0 || p.n_samples == 0 || (reinterpret_cast<uintptr_t>(p.text) & 15u)) return hipErrorInvalidValue;
    const uint64_t tiles = tiles_of(p.n_bytes);
    FRONT_TRY(hipMemsetAsync(p.tile_count + tiles, 0, 8, stream));
    hipLaunchKernelGGL(front_mark_kernel, dim3(capped_grid(tiles, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    FRONT_TRY(hipGetLastError());
    return sum_scan(p.tile_count, p.tile_base, tiles + 1, temp, temp_bytes, stream);
}

// the C = n_cand candidates, which of them are accepted, and seg_offs[0..S]: seg_offs[S] = K
hipError_t launch_front_candidates(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    const uint64_t C = p.n_cand, S = p.n_samples;
    if (C) {
        hipLaunchKernelGGL(front_candidates_kernel, dim3(capped_grid(tiles_of(p.n_bytes), kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
        FRONT_TRY(hipGetLastError());
        FRONT_TRY(max_scan(p.cand_end, p.pm, C, temp, temp_bytes, stream));
        hipLaunchKernelGGL(front_resolve_kernel, dim3(grid_for(C, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
        FRONT_TRY(hipGetLastError());
        FRONT_TRY(max_scan(p.acc_end, p.la, C, temp, temp_bytes, stream));
    }
    hipLaunchKernelGGL(front_cand_segs_kernel, dim3(grid_for((C > S ? C : S) + 1, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    FRONT_TRY(hipGetLastError());
    FRONT_TRY(wide_scan(p.cand_segs, p.seg_sum, C + 1, temp, temp_bytes, stream));
    hipLaunchKernelGGL(front_sample_segs_kernel, dim3(grid_for(S + 1, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    FRONT_TRY(hipGetLastError());
    return sum_scan(p.sample_segs, p.seg_offs, S + 1, temp, temp_bytes, stream);
}

// seg_begin, seg_end, seg_special[0..K) and rank[0..K]: rank[K] = E.  seg_special has room for K + 1 entries.
hipError_t launch_front_segments(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_segs) {
        hipLaunchKernelGGL(front_segments_kernel, dim3(grid_for(p.n_cand > p.n_samples ? p.n_cand : p.n_samples, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
        FRONT_TRY(hipGetLastError());
    }
    return launch_assemble_ranks(p.seg_special, p.rank, p.n_segs, temp, temp_bytes, stream);
}

// the E = n_enc encoded segments' ends, keep_mask and out_offs[0..E].  Needs E >= 1.
hipError_t launch_front_keep(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_enc == 0) return hipErrorInvalidValue;
    const uint64_t tiles = tiles_of(p.n_bytes);
    hipLaunchKernelGGL(front_encoded_kernel, dim3(grid_for(p.n_segs, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    FRONT_TRY(hipGetLastError());
    FRONT_TRY(hipMemsetAsync(p.tile_count + tiles, 0, 8, stream));
    hipLaunchKernelGGL(front_keep_kernel, dim3(capped_grid(tiles, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    FRONT_TRY(hipGetLastError());
    FRONT_TRY(sum_scan(p.tile_count, p.tile_base, tiles + 1, temp, temp_bytes, stream));
    hipLaunchKernelGGL(front_offsets_kernel, dim3(grid_for(p.n_enc + 1, kFrontBlock, kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    return hipGetLastError();
}

// the kept bytes to out[0 .. out_offs[E])
hipError_t launch_front_pack(const FrontParams& p, hipStream_t stream) {
    if (p.n_enc == 0 || !p.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(front_pack_kernel, dim3(capped_grid(tiles_of(p.n_bytes), kFrontMaxBlocks)), dim3(kFrontBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tgx
