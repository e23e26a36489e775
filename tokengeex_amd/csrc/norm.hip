// Unicode normalisation of a resident corpus in HBM (include/tgx.h: tgx_corpus_normalize; norm.h has the decoder, the
// stream machine, the index arithmetic and the data flow).  The byte kernels (mark, places, copy) take front.hip's tiles
// of 4096 consecutive bytes on a capped striding grid, 16 bytes per thread with one 16-byte load; the piece kernels take
// one piece per thread, 64 to a block, with the block's stream windows interleaved in LDS.  Every order comes from a scan
// (rocPRIM), none from an atomic append; the one atomic is a minimum, so the result does not depend on timing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "norm.h"
#include "scan_helpers.h"

namespace tgx {

namespace {

constexpr uint32_t kNormBlock = 256;
static_assert(kNormBlock * kFrontGroup == kFrontTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kNormMaxBlocks = 4096;  // memory-bound: a capped grid that strides over the rest
constexpr uint32_t kPieceBlock = 64;       // one wave: 64 windows of kNormWindow x 5 bytes of LDS

__device__ inline NormPlaces places_of(const NormParams& p) { return {p.mask, p.slot_pre, p.tile_base, p.piece_sum, p.tile_place}; }

__global__ __launch_bounds__(kNormBlock) void norm_mark_kernel(NormParams p) {
    __shared__ uint64_t s_row[2];
    __shared__ uint32_t s_part[kNormBlock / 64];
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFrontTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.offs, 0, 0, p.n_rows - 1, threadIdx.x ? tile_last(t0, kFrontTile, n) : t0);
        __syncthreads();
        const uint64_t p0 = t0 + (uint64_t)threadIdx.x * kFrontGroup;
        uint32_t m = 0;
        if (p0 < n) {
            const uint32_t n_in = n - p0 < kFrontGroup ? (uint32_t)(n - p0) : kFrontGroup;
            uint8_t v[kFrontGroup];
            load_slot(p.text, p0, v);
            const uint8_t next = p0 + kFrontGroup < n ? p.text[p0 + kFrontGroup] : 0;
            m = norm_mark_slot(p.tab, p.form, p.text, p.offs, s_row[0], s_row[1], p0, n_in, v, next);
            p.mask[p0 / kFrontGroup] = m;
        }
        uint32_t total;
        block_exclusive_sum<kNormBlock>(front_popc(m >> 16), s_part, &total);  // (its barriers also keep s_row for the whole tile)
        if (threadIdx.x == 0) p.tile_count[tile] = total;
    }
}

__global__ __launch_bounds__(kNormBlock) void norm_pieces_kernel(NormParams p) {
    __shared__ uint64_t s_row[2];
    __shared__ uint32_t s_part[kNormBlock / 64];
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = p.tile_base[tile];
        if (p.tile_base[tile + 1] == base) continue;  // (the whole block takes the same way)
        const uint64_t t0 = tile * kFrontTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.offs, 0, 0, p.n_rows - 1, threadIdx.x ? tile_last(t0, kFrontTile, n) : t0);
        __syncthreads();
        const uint64_t p0 = t0 + (uint64_t)threadIdx.x * kFrontGroup;
        const uint32_t heads = p0 < n ? p.mask[p0 / kFrontGroup] >> 16 : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive_sum<kNormBlock>(front_popc(heads), s_part, &total);
        if (heads) norm_write_pieces(p.offs, s_row[0], s_row[1], p0, heads, base + before, p.piece_begin, p.piece_row);
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

// piece_len[0..P] (entry P is 0 and belongs to the scan) and the lowest row whose window overflows
__global__ __launch_bounds__(kPieceBlock) void norm_length_kernel(NormParams p) {
    __shared__ uint32_t s_cp[kNormWindow * kPieceBlock];
    __shared__ uint8_t s_cc[kNormWindow * kPieceBlock];
    for (uint64_t k = (uint64_t)blockIdx.x * kPieceBlock + threadIdx.x; k <= p.n_pieces; k += (uint64_t)gridDim.x * kPieceBlock) {
        if (k == p.n_pieces) {
            p.piece_len[k] = 0;
            continue;
        }
        NormStream s = {s_cp + threadIdx.x, s_cc + threadIdx.x, kPieceBlock, nullptr};
        const uint64_t row = p.piece_row[k];
        norm_run_piece(p.tab, p.form, p.text, p.piece_begin[k], p.offs[row + 1], s);
        p.piece_len[k] = s.produced;
        if (s.overflow) atomicMin(reinterpret_cast<unsigned long long*>(p.overflow_row), (unsigned long long)row);
    }
}

// slot_pre, and what every tile turns into
__global__ __launch_bounds__(kNormBlock) void norm_places_kernel(NormParams p) {
    __shared__ uint32_t s_part[kNormBlock / 64];
    const uint64_t n = p.n_bytes, n_tiles = (n + kFrontTile - 1) / kFrontTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t p0 = tile * kFrontTile + (uint64_t)threadIdx.x * kFrontGroup;
        uint32_t m = 0, n_in = 0;
        if (p0 < n) {
            n_in = n - p0 < kFrontGroup ? (uint32_t)(n - p0) : kFrontGroup;
            m = p.mask[p0 / kFrontGroup];
        }
        uint32_t copied, heads;
        const uint32_t copied_before = block_exclusive_sum<kNormBlock>(front_popc(norm_verbatim(m, n_in)), s_part, &copied);
        const uint32_t heads_before = block_exclusive_sum<kNormBlock>(front_popc(m >> 16), s_part, &heads);
        if (p0 < n) p.slot_pre[p0 / kFrontGroup] = copied_before | heads_before << 16;
        if (threadIdx.x == 0) p.tile_bytes[tile] = norm_tile_bytes(p.tile_base, p.piece_sum, tile, copied);
    }
}

// out_offs[0..S]: the place of every row's first byte
__global__ __launch_bounds__(kNormBlock) void norm_offsets_kernel(NormParams p) {
    const NormPlaces pl = places_of(p);
    const uint64_t n_tiles = (p.n_bytes + kFrontTile - 1) / kFrontTile;
    for (uint64_t r = (uint64_t)blockIdx.x * kNormBlock + threadIdx.x; r <= p.n_rows; r += (uint64_t)gridDim.x * kNormBlock) {
        const uint64_t b = p.offs[r];
        p.out_offs[r] = b < p.n_bytes ? norm_place(pl, b) : p.tile_place[n_tiles];
    }
}

__global__ __launch_bounds__(kNormBlock) void norm_copy_kernel(NormParams p) {
    const NormPlaces pl = places_of(p);
    uint8_t* __restrict__ out = p.out;
    const uint64_t n = p.n_bytes, slots = (n + kFrontGroup - 1) / kFrontGroup;
    for (uint64_t s = (uint64_t)blockIdx.x * kNormBlock + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * kNormBlock) {
        const uint64_t p0 = s * kFrontGroup;
        const uint32_t n_in = n - p0 < kFrontGroup ? (uint32_t)(n - p0) : kFrontGroup;
        uint8_t v[kFrontGroup];
        load_slot(p.text, p0, v);
        norm_copy_slot(pl, p0, n_in, v, out);
    }
}

__global__ __launch_bounds__(kPieceBlock) void norm_write_kernel(NormParams p) {
    __shared__ uint32_t s_cp[kNormWindow * kPieceBlock];
    __shared__ uint8_t s_cc[kNormWindow * kPieceBlock];
    const NormPlaces pl = places_of(p);
    for (uint64_t k = (uint64_t)blockIdx.x * kPieceBlock + threadIdx.x; k < p.n_pieces; k += (uint64_t)gridDim.x * kPieceBlock) {
        const uint64_t begin = p.piece_begin[k];
        NormStream s = {s_cp + threadIdx.x, s_cc + threadIdx.x, kPieceBlock, p.out + norm_place(pl, begin)};
        norm_run_piece(p.tab, p.form, p.text, begin, p.offs[p.piece_row[k] + 1], s);
    }
}

uint64_t tiles_of(uint64_t n) { return (n + kFrontTile - 1) / kFrontTile; }

#define NORM_TRY(expr)                   \
    do {                                 \
        const hipError_t _e = (expr);    \
        if (_e != hipSuccess) return _e; \
    } while (0)

}  // namespace

// room for every scan of the launchers below over up to n elements (n at least the larger of tiles and P, plus 1)
hipError_t norm_scan_temp_bytes(uint64_t n, size_t* bytes) {
    *bytes = 0;
    return sum_scan(nullptr, nullptr, n, nullptr, *bytes, nullptr);
}

// mask and tile_base[0..tiles]: tile_base[tiles] = P.  Needs N >= 1 and S >= 1.
hipError_t launch_norm_mark(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_bytes == 0 || p.n_rows == 0 || p.form > 3 || (reinterpret_cast<uintptr_t>(p.text) & 15u)) return hipErrorInvalidValue;
    const uint64_t tiles = tiles_of(p.n_bytes);
    NORM_TRY(hipMemsetAsync(p.tile_count + tiles, 0, 8, stream));
    hipLaunchKernelGGL(norm_mark_kernel, dim3(capped_grid(tiles, kNormMaxBlocks)), dim3(kNormBlock), 0, stream, p);
    NORM_TRY(hipGetLastError());
    return sum_scan(p.tile_count, p.tile_base, tiles + 1, temp, temp_bytes, stream);
}

// piece_begin and piece_row of the P = n_pieces >= 1 pieces
hipError_t launch_norm_pieces(const NormParams& p, hipStream_t stream) {
    if (p.n_pieces == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(norm_pieces_kernel, dim3(capped_grid(tiles_of(p.n_bytes), kNormMaxBlocks)), dim3(kNormBlock), 0, stream, p);
    return hipGetLastError();
}

// piece_len, piece_sum[0..P] and overflow_row
hipError_t launch_norm_length(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_pieces == 0) return hipErrorInvalidValue;
    NORM_TRY(hipMemsetAsync(p.overflow_row, 0xFF, 8, stream));
    hipLaunchKernelGGL(norm_length_kernel, dim3(grid_for(p.n_pieces + 1, kPieceBlock, kNormMaxBlocks)), dim3(kPieceBlock), 0, stream, p);
    NORM_TRY(hipGetLastError());
    return sum_scan(p.piece_len, p.piece_sum, p.n_pieces + 1, temp, temp_bytes, stream);
}

// slot_pre, tile_place[0..tiles] (tile_place[tiles]: the output's bytes) and out_offs[0..S]
hipError_t launch_norm_places(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n_pieces == 0) return hipErrorInvalidValue;
    const uint64_t tiles = tiles_of(p.n_bytes);
    NORM_TRY(hipMemsetAsync(p.tile_bytes + tiles, 0, 8, stream));
    hipLaunchKernelGGL(norm_places_kernel, dim3(capped_grid(tiles, kNormMaxBlocks)), dim3(kNormBlock), 0, stream, p);
    NORM_TRY(hipGetLastError());
    NORM_TRY(sum_scan(p.tile_bytes, p.tile_place, tiles + 1, temp, temp_bytes, stream));
    hipLaunchKernelGGL(norm_offsets_kernel, dim3(grid_for(p.n_rows + 1, kNormBlock, kNormMaxBlocks)), dim3(kNormBlock), 0, stream, p);
    return hipGetLastError();
}

// the copied bytes and the pieces to out[0 .. tile_place[tiles])
hipError_t launch_norm_write(const NormParams& p, hipStream_t stream) {
    if (p.n_pieces == 0 || !p.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(norm_copy_kernel, dim3(grid_for((p.n_bytes + kFrontGroup - 1) / kFrontGroup, kNormBlock, kNormMaxBlocks)), dim3(kNormBlock), 0, stream, p);
    NORM_TRY(hipGetLastError());
    hipLaunchKernelGGL(norm_write_kernel, dim3(grid_for(p.n_pieces, kPieceBlock, kNormMaxBlocks)), dim3(kPieceBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tgx
