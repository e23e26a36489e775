// Fill-in-the-middle on the device: the rows of a result rearranged behind the three sentinels (include/tgx.h:
// tgx_result_fim; fim.h has the index arithmetic).  Two steps: the new offsets (a device-wide exclusive scan of the rows'
// output lengths, rocPRIM, over an iterator that computes a length from the old offsets: no length array is written) and
// the fill.  The fill is output-centric like assemble_fill_kernel and layout_pack_kernel: a tile of 1024 consecutive
// output positions per block, the owners of the tile's ends found by two threads over the new offsets, every thread
// then walking its four positions between those two and writing them with one 16-byte store.  A row is 0 to 10^5
// tokens, so no unit of work is a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "fim.h"
#include "kernels.h"

namespace tgx {

namespace {

constexpr uint32_t kFimBlock = 256;
static_assert(kFimBlock * kFimGroup == kFimTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kFimMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

// row i -> its output length; entry S (which the scan turns into T') is 0 and reads nothing
struct FimOutLen {
    const uint64_t* offs;
    uint64_t n_rows, seed, first_row;
    double rate;
    __host__ __device__ uint64_t operator()(uint64_t i) const {
        if (i >= n_rows) return 0;
        return fim_out_len(seed, first_row + i, offs[i + 1] - offs[i], rate);
    }
};

FimOutLen out_len_of(const FimParams& p) { return FimOutLen{p.offs, p.n_rows, p.f.seed, p.f.first_row, p.f.rate}; }

__global__ __launch_bounds__(kFimBlock) void fim_fill_kernel(FimParams p) {
    __shared__ uint64_t s_row[2];
    const uint64_t n_out = p.n_out;
    uint32_t* __restrict__ out = p.out_ids;
    const uint64_t n_tiles = (n_out + kFimTile - 1) / kFimTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kFimTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.out_offs, 0, 0, p.n_rows - 1, threadIdx.x ? fim_tile_last(t0, n_out) : t0);
        __syncthreads();
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kFimGroup;
        if (e0 < n_out) {
            const uint32_t n_in = n_out - e0 < kFimGroup ? (uint32_t)(n_out - e0) : kFimGroup;
            uint32_t v[kFimGroup] = {0, 0, 0, 0};
            fim_group(p.f, p.ids, p.offs, p.out_offs, s_row[0], s_row[1], e0, n_in, v);
            if (n_in == kFimGroup) {  // out is 16-byte aligned (checked by the launcher) and e0 a multiple of 4
                *reinterpret_cast<uint4*>(out + e0) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {  // the tail of the last tile
                for (uint32_t q = 0; q < n_in; q++) out[e0 + q] = v[q];
            }
        }
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

// mode[i] and cuts[2i], cuts[2i + 1]: one thread per row
__global__ __launch_bounds__(kFimBlock) void fim_info_kernel(FimParams p, uint8_t* mode, uint64_t* cuts) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFimBlock + threadIdx.x; i < p.n_rows; i += (uint64_t)gridDim.x * kFimBlock) {
        const FimRow r = fim_row(p.f.seed, p.f.first_row + i, p.offs[i + 1] - p.offs[i], p.f.rate, p.f.spm_rate);
        if (mode) mode[i] = (uint8_t)r.mode;
        if (cuts) {
            cuts[2 * i] = r.a;
            cuts[2 * i + 1] = r.b;
        }
    }
}

uint32_t capped_grid(uint64_t blocks) { return (uint32_t)(blocks < kFimMaxBlocks ? (blocks ? blocks : 1) : kFimMaxBlocks); }

}  // namespace

hipError_t fim_scan_temp_bytes(uint64_t n_rows, size_t* bytes) {
    *bytes = 0;
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), FimOutLen{nullptr, 0, 0, 0, 0.0});
    return rocprim::exclusive_scan(nullptr, *bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n_rows + 1), rocprim::plus<uint64_t>());
}

// out_offs[0 .. S]: the exclusive prefix sums of the rows' output lengths, so out_offs[S] = T'
hipError_t launch_fim_offsets(const FimParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), out_len_of(p));
    return rocprim::exclusive_scan(temp, temp_bytes, in, p.out_offs, (uint64_t)0, (size_t)(p.n_rows + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_fim_fill(const FimParams& p, hipStream_t stream) {
    if (p.n_out == 0) return hipSuccess;
    if (p.n_rows == 0 || (reinterpret_cast<uintptr_t>(p.out_ids) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fim_fill_kernel, dim3(capped_grid((p.n_out + kFimTile - 1) / kFimTile)), dim3(kFimBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_fim_info(const FimParams& p, uint8_t* mode, uint64_t* cuts, hipStream_t stream) {
    if (p.n_rows == 0 || (!mode && !cuts)) return hipSuccess;
    hipLaunchKernelGGL(fim_info_kernel, dim3(capped_grid((p.n_rows + kFimBlock - 1) / kFimBlock)), dim3(kFimBlock), 0, stream, p, mode, cuts);
    return hipGetLastError();
}

}  // namespace tgx
