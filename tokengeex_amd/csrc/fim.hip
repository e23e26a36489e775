// Fill-in-the-middle on the device: the rows of a result rearranged behind the three sentinels (include/tgx.h:
// tgx_result_fim; fim.h has the index arithmetic).  Two steps: the new offsets (a device-wide exclusive scan of the rows'
// output lengths, rocPRIM, over an iterator that computes a length from the old offsets: no length array is written) and
// the fill.  The fill is the tiled fill of tile_fill.h: a tile of 1024 consecutive
// output positions per block, the owners of the tile's ends found by two threads over the new offsets, every thread
// then walking its four positions between those two and writing them with one 16-byte store.  A row is 0 to 10^5
// tokens, so no unit of work is a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fim.h"
#include "kernels.h"
#include "scan_helpers.h"

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

__global__ __launch_bounds__(kFimBlock) void fim_fill_kernel(FimParams p) {
    tiled_fill<kFimTile, kFimGroup>(
        p.n_out, p.n_out, [p](uint64_t j) { return pack_find_row(p.out_offs, 0, 0, p.n_rows - 1, j); },
        [p](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint32_t v[kFimGroup] = {0, 0, 0, 0};
            fim_group(p.f, p.ids, p.offs, p.out_offs, lo, hi, e0, n_in, v);
            store_ids4(p.out_ids, e0, v, n_in);
        });
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

// out_offs[0 .. S]: the exclusive prefix sums of the rows' output lengths, so out_offs[S] = T'.  temp == NULL: the size query
hipError_t offsets_scan(const FimParams& p, void* temp, size_t& temp_bytes, hipStream_t stream) {
    return scan_of(FimOutLen{p.offs, p.n_rows, p.f.seed, p.f.first_row, p.f.rate}, p.n_rows + 1, p.out_offs, temp, temp_bytes, stream);
}

}  // namespace

hipError_t fim_scan_temp_bytes(uint64_t n_rows, size_t* bytes) {
    FimParams p = {};
    p.n_rows = n_rows;
    *bytes = 0;
    return offsets_scan(p, nullptr, *bytes, nullptr);
}

hipError_t launch_fim_offsets(const FimParams& p, void* temp, size_t temp_bytes, hipStream_t stream) { return offsets_scan(p, temp, temp_bytes, stream); }

hipError_t launch_fim_fill(const FimParams& p, hipStream_t stream) {
    if (p.n_out == 0) return hipSuccess;
    if (p.n_rows == 0 || (reinterpret_cast<uintptr_t>(p.out_ids) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fim_fill_kernel, dim3(grid_for(p.n_out, kFimTile, kFimMaxBlocks)), dim3(kFimBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_fim_info(const FimParams& p, uint8_t* mode, uint64_t* cuts, hipStream_t stream) {
    if (p.n_rows == 0 || (!mode && !cuts)) return hipSuccess;
    hipLaunchKernelGGL(fim_info_kernel, dim3(grid_for(p.n_rows, kFimBlock, kFimMaxBlocks)), dim3(kFimBlock), 0, stream, p, mode, cuts);
    return hipGetLastError();
}

}  // namespace tgx
