// Ids in HBM decoded to UTF-8 text in HBM (include/tgx.h: tgx_decode_result, tgx_decode_padded; decode.h has the index
// arithmetic).  The meta kernel gives every element its raw length and class and takes the out-of-bounds atomicMin; two
// device-wide exclusive scans (rocPRIM, as the scan of the assembly's ranks) turn them into byte starts B and special
// counts X.  The fill is the tiled fill of tile_fill.h: a tile of 4096 consecutive raw bytes per block, the
// owners of the tile's ends found by two threads over all of B, every thread then walking the few elements that cover its
// 16 bytes and writing them with one 16-byte store.  A token of up to 16 bytes is one 16-byte load from its slot, so no
// unit of work is a token (4-byte tokens would make 4-byte unaligned stores).  The UTF-8 kernel applies from_utf8_lossy
// as a rule local to a byte's run; only when something was replaced are the bytes written a second time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "decode.h"
#include "kernels.h"

namespace tgx {

namespace {

constexpr uint32_t kDecodeBlock = 256;
static_assert(kDecodeBlock * kDecodeGroup == kDecodeTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kDecodeMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

struct MetaLen {
    __host__ __device__ uint64_t operator()(uint32_t m) const { return m & ~kDecodeSpecial; }
};
struct MetaSpecial {
    __host__ __device__ uint64_t operator()(uint32_t m) const { return m >> 31; }
};
struct CodeBytes {
    __host__ __device__ uint64_t operator()(uint32_t code) const { return decode_code_bytes(code, kDecodeGroup); }
};

// meta[0..N): one element per thread slot; the number of live specials; the lowest stream position of an element that is neither a token nor a special
__global__ __launch_bounds__(kDecodeBlock) void decode_meta_kernel(DecodeParams p) {
    __shared__ unsigned long long part[kDecodeBlock / 64];
    unsigned long long bad = ~0ull, specials = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; j < p.src.n; j += (uint64_t)gridDim.x * kDecodeBlock) {
        const int64_t x = decode_elem(p.src, j);
        uint32_t m = 0;
        if (decode_live(p.src, j, x)) {
            bool oob;
            m = decode_meta(p.tab, x, &oob);
            if (oob && j < bad) bad = j;
        }
        p.meta[j] = m;
        specials += m >> 31;
    }
    if (bad != ~0ull) atomicMin(p.bad_pos, bad);  // (a thread's positions ascend: at most one atomic per thread, none in a good call)
    // the live specials, one atomic per block that met one: a stream without any needs no X
    for (int d = 32; d > 0; d >>= 1) specials += __shfl_down(specials, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = specials;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kDecodeBlock / 64; k++) specials += part[k];
        if (specials) atomicAdd(p.n_specials_live, specials);
    }
}

__global__ __launch_bounds__(kDecodeBlock) void decode_fill_kernel(DecodeParams p) {
    tiled_fill<kDecodeTile, kDecodeGroup, kDecodeBack>(
        p.n_raw, p.n_raw, [p](uint64_t b) { return pack_find_row(p.starts, 0, 0, p.src.n - 1, b); },
        [p](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint8_t v[kDecodeGroup] = {};
            const uint32_t flags = decode_group(p.tab, p.src, p.starts, p.specials, lo, hi, e0, n_in, v);
            uint32_t w[4];  // (not store_bytes16: with it the kernel loses a wave of occupancy, profiles/tile_fill/README.md)
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                w[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
            if (n_in == kDecodeGroup) {  // raw is 16-byte aligned (checked by the launcher) and e0 a multiple of 16
                *reinterpret_cast<uint4*>(p.raw + e0) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {  // the tail of the last tile
                for (uint32_t q = 0; q < n_in; q++) p.raw[e0 + q] = v[q];
            }
            p.flags[e0 / kDecodeGroup] = flags;
        });
}

// row_offs[0..S] = the rows' raw starts; after the fill: every row start starts a run
__global__ __launch_bounds__(kDecodeBlock) void decode_rows_kernel(DecodeParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; i <= p.src.n_rows; i += (uint64_t)gridDim.x * kDecodeBlock) {
        const uint64_t r = p.starts[i < p.src.n_rows ? decode_row_first(p.src, i) : p.src.n];
        p.row_offs[i] = r;
        if (r < p.n_raw) atomicOr(p.flags + r / kDecodeGroup, 1u << (uint32_t)(r % kDecodeGroup));
    }
}

// codes[0..G): one slot of 16 raw bytes per thread; the replacement characters are added up, one atomic per block
__global__ __launch_bounds__(kDecodeBlock) void decode_utf8_kernel(DecodeParams p) {
    __shared__ unsigned long long part[kDecodeBlock / 64];
    const uint64_t n_groups = (p.n_raw + kDecodeGroup - 1) / kDecodeGroup;
    unsigned long long replaced = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * kDecodeBlock) {
        const uint32_t code = decode_utf8_slot(p.raw, p.flags, p.n_raw, g);
        p.codes[g] = code;
        replaced += decode_code_replaced(code);
    }
    for (int d = 32; d > 0; d >>= 1) replaced += __shfl_down(replaced, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = replaced;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kDecodeBlock / 64; k++) replaced += part[k];
        if (replaced) atomicAdd(p.n_replaced, replaced);
    }
}

// only after a replacement: the slots' bytes at their scanned positions
__global__ __launch_bounds__(kDecodeBlock) void decode_expand_kernel(DecodeParams p) {
    const uint64_t n_groups = (p.n_raw + kDecodeGroup - 1) / kDecodeGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * kDecodeBlock)
        decode_expand_slot(p.raw, p.n_raw, g, p.codes[g], p.out, p.gpos[g]);
}

__global__ __launch_bounds__(kDecodeBlock) void decode_final_rows_kernel(DecodeParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDecodeBlock + threadIdx.x; i <= p.src.n_rows; i += (uint64_t)gridDim.x * kDecodeBlock)
        p.row_offs[i] = decode_final_pos(p.gpos, p.codes, p.row_offs[i], p.n_raw);
}

}  // namespace

hipError_t decode_scan_temp_bytes(uint64_t n, size_t* bytes) {
    *bytes = 0;
    auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, MetaLen());
    return rocprim::exclusive_scan(nullptr, *bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>());
}

// meta must have room for n + 1 entries: entry n is set to 0 and scanned, so that starts[n] is the number of raw bytes
hipError_t launch_decode_meta(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    const uint64_t n = p.src.n;
    hipError_t e = hipMemsetAsync(p.meta + n, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_meta_kernel, dim3(grid_for(n, kDecodeBlock, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    auto len = rocprim::make_transform_iterator((const uint32_t*)p.meta, MetaLen());
    return rocprim::exclusive_scan(temp, temp_bytes, len, p.starts, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), stream);
}

// X, for a stream with live specials (the same temporary storage serves: the two scans have one type)
hipError_t launch_decode_specials(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    auto sp = rocprim::make_transform_iterator((const uint32_t*)p.meta, MetaSpecial());
    return rocprim::exclusive_scan(temp, temp_bytes, sp, p.specials, (uint64_t)0, (size_t)(p.src.n + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_decode_fill(const DecodeParams& p, hipStream_t stream) {
    if (p.n_raw == 0 || p.src.n == 0 || (reinterpret_cast<uintptr_t>(p.raw) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_fill_kernel, dim3(grid_for(p.n_raw, kDecodeTile, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_decode_rows(const DecodeParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(decode_rows_kernel, dim3(grid_for(p.src.n_rows + 1, kDecodeBlock, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_decode_utf8(const DecodeParams& p, hipStream_t stream) {
    if (p.n_raw == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_utf8_kernel, dim3(grid_for((p.n_raw + kDecodeGroup - 1) / kDecodeGroup, kDecodeBlock, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t decode_expand_temp_bytes(uint64_t n_groups, size_t* bytes) {
    *bytes = 0;
    auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, CodeBytes());
    return rocprim::exclusive_scan(nullptr, *bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n_groups + 1), rocprim::plus<uint64_t>());
}

// codes must have room for G + 1 entries: entry G is set to 0 and scanned, so that gpos[G] is the text's length
hipError_t launch_decode_positions(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    const uint64_t n_groups = (p.n_raw + kDecodeGroup - 1) / kDecodeGroup;
    const hipError_t e = hipMemsetAsync(p.codes + n_groups, 0, 4, stream);
    if (e != hipSuccess) return e;
    auto in = rocprim::make_transform_iterator((const uint32_t*)p.codes, CodeBytes());
    return rocprim::exclusive_scan(temp, temp_bytes, in, p.gpos, (uint64_t)0, (size_t)(n_groups + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_decode_expand(const DecodeParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(decode_expand_kernel, dim3(grid_for((p.n_raw + kDecodeGroup - 1) / kDecodeGroup, kDecodeBlock, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_final_rows_kernel, dim3(grid_for(p.src.n_rows + 1, kDecodeBlock, kDecodeMaxBlocks)), dim3(kDecodeBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tgx
