// Device-side scan helpers that more than one .hip shares: the block-wide exclusive sum and the 16-byte slot load of the
// byte kernels (front.hip, norm.hip) and the device-wide exclusive scans (rocPRIM) of front.hip, norm.hip, fim.hip and
// select.hip.  For translation units with kernels only: it includes rocPRIM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace tgx {

// exclusive sums of v over the block's BLOCK threads in thread order; *total: the block's sum.  part: u32[BLOCK / 64] of LDS
template <uint32_t BLOCK>
__device__ inline uint32_t block_exclusive_sum(uint32_t v, uint32_t* part, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; w++) {
        const uint32_t s = part[w];
        if (w < wave) base += s;
        all += s;
    }
    __syncthreads();  // part is rewritten by the next call
    *total = all;
    return base + incl - v;
}

// a slot's 16 bytes with one load (text is 16-byte aligned and readable to the end of the slot)
__device__ inline void load_slot(const uint8_t* text, uint64_t p0, uint8_t (&v)[16]) {
    const uint4 w = *reinterpret_cast<const uint4*>(text + p0);
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) v[q] = (uint8_t)(x[q >> 2] >> (8 * (q & 3)));
}

// out[0 .. n) = the exclusive 64-bit prefix sums of in[0 .. n); temp == NULL: temp_bytes = the room the scan needs.  (A
// template, so that a translation unit that does not call it gets none of the scan's kernels.)
template <class = void>
inline hipError_t sum_scan(const uint64_t* in, uint64_t* out, uint64_t n, void* temp, size_t& temp_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), stream);
}

// out[0 .. n) = the exclusive prefix sums of f(0), f(1), ..., f(n - 1), which are computed on the way: no array of them is
// written.  temp == NULL: temp_bytes = the room the scan needs, and f is not called
template <class F>
inline hipError_t scan_of(F f, uint64_t n, uint64_t* out, void* temp, size_t& temp_bytes, hipStream_t stream) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), f);
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), stream);
}

}  // namespace tgx
