// A sample-level result put together on the device from the result over the non-special segments and the split plan
// (include/tgx.h: tgx_assemble_result; assemble.h has the index arithmetic).  Three steps: the ranks r_k of the segments
// (a device-wide exclusive scan of "segment k is encoded", rocPRIM, as the scan of the encode pass's token counts), the
// segment starts D_k with the samples' offsets, and the fill.  The fill is the tiled fill of DESIGN.md, section L.9, in a copy of its own (tile_fill.h's template measured slower here): a tile of
// 1024 consecutive output positions per block, the owners of the tile's ends found by two threads over all of D, every
// thread then walking its four positions between those two and writing them with one 16-byte store.  A special segment
// is one position and a long sample's segment thousands, so no unit of work is a segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "assemble.h"
#include "kernels.h"

namespace tgx {

namespace {

constexpr uint32_t kAssembleBlock = 256;
static_assert(kAssembleBlock * kAssembleGroup == kAssembleTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kAssembleMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

struct IsEncoded {
    __host__ __device__ uint64_t operator()(int32_t special) const { return special < 0 ? 1u : 0u; }
};

// D[0..K] and out_offs[0..S]: one thread per element
__global__ __launch_bounds__(kAssembleBlock) void assemble_starts_kernel(AssembleParams p) {
    const uint64_t n = p.n_segs > p.n_samples ? p.n_segs + 1 : p.n_samples + 1;
    for (uint64_t x = (uint64_t)blockIdx.x * kAssembleBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kAssembleBlock) {
        if (x <= p.n_segs) p.starts[x] = assemble_seg_start(p.offs, p.rank, x);
        if (x <= p.n_samples) p.out_offs[x] = assemble_seg_start(p.offs, p.rank, p.seg_offs[x]);
    }
}

// (tile_fill.h's loop, written out: profiles/tile_fill)
__global__ __launch_bounds__(kAssembleBlock) void assemble_fill_kernel(AssembleParams p) {
    __shared__ uint64_t s_seg[2];
    const uint64_t n_out = p.n_out;
    uint32_t* __restrict__ out = p.out_ids;
    const uint64_t n_tiles = (n_out + kAssembleTile - 1) / kAssembleTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kAssembleTile;
        if (threadIdx.x < 2) s_seg[threadIdx.x] = pack_find_row(p.starts, 0, 0, p.n_segs - 1, threadIdx.x ? tile_last(t0, kAssembleTile, n_out) : t0);
        __syncthreads();
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kAssembleGroup;
        if (e0 < n_out) {
            const uint32_t n_in = n_out - e0 < kAssembleGroup ? (uint32_t)(n_out - e0) : kAssembleGroup;
            uint32_t v[kAssembleGroup] = {0, 0, 0, 0};
            assemble_group(p.ids, p.starts, p.rank, p.seg_special, p.vocab_size, s_seg[0], s_seg[1], e0, n_in, v);
            if (n_in == kAssembleGroup) {  // out is 16-byte aligned (checked by the launcher) and e0 a multiple of 4
                *reinterpret_cast<uint4*>(out + e0) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {  // the tail of the last tile
                for (uint32_t q = 0; q < n_in; q++) out[e0 + q] = v[q];
            }
        }
        __syncthreads();  // s_seg is rewritten for the next tile
    }
}

}  // namespace

// seg_special must have room for n_segs + 1 entries: entry n_segs is set to 0 (not encoded) and scanned, so that
// rank[n_segs] is the number of encoded segments
hipError_t assemble_scan_temp_bytes(uint64_t n_segs, size_t* bytes) {
    *bytes = 0;
    auto in = rocprim::make_transform_iterator((const int32_t*)nullptr, IsEncoded());
    return rocprim::exclusive_scan(nullptr, *bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n_segs + 1), rocprim::plus<uint64_t>());
}

hipError_t launch_assemble_ranks(int32_t* seg_special, uint64_t* rank, uint64_t n_segs, void* temp, size_t temp_bytes, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(seg_special + n_segs, 0, 4, stream);
    if (e != hipSuccess) return e;
    auto in = rocprim::make_transform_iterator((const int32_t*)seg_special, IsEncoded());
    return rocprim::exclusive_scan(temp, temp_bytes, in, rank, (uint64_t)0, (size_t)(n_segs + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_assemble_starts(const AssembleParams& p, hipStream_t stream) {
    const uint64_t n = (p.n_segs > p.n_samples ? p.n_segs : p.n_samples) + 1;
    hipLaunchKernelGGL(assemble_starts_kernel, dim3(grid_for(n, kAssembleBlock, kAssembleMaxBlocks)), dim3(kAssembleBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_assemble_fill(const AssembleParams& p, hipStream_t stream) {
    if (p.n_out == 0) return hipSuccess;
    if (p.n_segs == 0 || (reinterpret_cast<uintptr_t>(p.out_ids) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assemble_fill_kernel, dim3(grid_for(p.n_out, kAssembleTile, kAssembleMaxBlocks)), dim3(kAssembleBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tgx
