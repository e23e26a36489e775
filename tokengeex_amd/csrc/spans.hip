// The part of its row's text that every token of a result covers (include/tgx.h: tgx_result_spans_device,
// tgx_result_pad_spans_device; spans.h has the index arithmetic).  The meta kernel looks one packed word up per element
// and keeps its value in the chosen unit: the token's bytes, or its bytes that start a character.  One device-wide
// 64-bit exclusive scan (rocPRIM, as decode.hip's) turns the values into P; a span is two differences against the row's
// base P[o[i]].  The padded writer takes one [start, end] pair per thread through the row mapping of the padded layout
// and writes it with one 8- or 16-byte store (the windowed writer the same through the window mapping, after a search
// of the windows' prefix sums for the pair's row); the flat writer walks tiles of 1024 consecutive elements, two threads
// finding the rows of the tile's ends and every thread then stepping a row cursor over its four elements, which go out
// as two 16-byte stores (four for i64).  Pure data movement: per element 4 B of ids and 2 B of table in, 4 B of values
// out and in again, 8 B of sums out and in, 8 or 16 B of spans out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "kernels.h"
#include "spans.h"

namespace tgx {

namespace {

constexpr uint32_t kSpanBlock = 256;
static_assert(kSpanGroup == 4 && kSpanBlock * kSpanGroup == kSpanTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kSpanMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

struct SpanValue {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v & ~kSpanValCont; }
};

// vals[0..T): one element per thread slot.  (The ids of a result are below V + n_specials; another id counts nothing.)
__global__ __launch_bounds__(kSpanBlock) void span_meta_kernel(SpanParams p) {
    const bool chars = (p.flags & kSpanChars) != 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kSpanBlock + threadIdx.x; j < p.n; j += (uint64_t)gridDim.x * kSpanBlock) {
        bool oob;
        p.vals[j] = span_val(p.tab, p.ids[j], chars, &oob);
    }
}

// the largest row total: one atomic per block that has one above 0
__global__ __launch_bounds__(kSpanBlock) void span_row_max_kernel(SpanParams p) {
    __shared__ unsigned long long part[kSpanBlock / 64];
    unsigned long long best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSpanBlock + threadIdx.x; i < p.n_rows; i += (uint64_t)gridDim.x * kSpanBlock) {
        const unsigned long long n = span_row_total(p.sums, p.offs, i);
        best = n > best ? n : best;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long y = __shfl_down(best, d, 64);
        best = y > best ? y : best;
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kSpanBlock / 64; w++) best = part[w] > best ? part[w] : best;
        if (best) atomicMax(p.row_max, best);
    }
}

// one pair as one store (VEC: the destination is aligned to a pair)
template <bool VEC>
__device__ inline void store_pair(int32_t* out, uint64_t e, const SpanPair& s) {
    if (VEC) {
        *reinterpret_cast<int2*>(out + 2 * e) = make_int2((int)s.start, (int)s.end);
    } else {
        out[2 * e] = (int32_t)s.start;
        out[2 * e + 1] = (int32_t)s.end;
    }
}
template <bool VEC>
__device__ inline void store_pair(int64_t* out, uint64_t e, const SpanPair& s) {
    if (VEC) {
        *reinterpret_cast<longlong2*>(out + 2 * e) = make_longlong2((long long)s.start, (long long)s.end);
    } else {
        out[2 * e] = s.start;
        out[2 * e + 1] = s.end;
    }
}

// total = S·L pairs, one per thread slot
template <class T, bool VEC>
__global__ __launch_bounds__(kSpanBlock) void span_pad_kernel(SpanParams p, uint64_t total) {
    const LayoutSeq seq = layout_seq(p.bos, p.eos, 0);
    const uint32_t* vals = (p.flags & kSpanChars) ? p.vals : nullptr;
    T* __restrict__ out = static_cast<T*>(p.out);
    for (uint64_t e = (uint64_t)blockIdx.x * kSpanBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kSpanBlock)
        store_pair<VEC>(out, e, span_pad_at(seq, p.offs, p.sums, vals, p.len, p.flags, e));
}

// total = W·L pairs, one per thread slot; each slot searches Wo for its window's row
template <class T, bool VEC>
__global__ __launch_bounds__(kSpanBlock) void span_window_kernel(SpanParams p, const uint64_t* __restrict__ wo, uint32_t stride, uint64_t total) {
    const LayoutSeq seq = layout_seq(p.bos, p.eos, 0);
    const uint32_t* vals = (p.flags & kSpanChars) ? p.vals : nullptr;
    T* __restrict__ out = static_cast<T*>(p.out);
    for (uint64_t e = (uint64_t)blockIdx.x * kSpanBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kSpanBlock)
        store_pair<VEC>(out, e, span_window_at(seq, p.offs, wo, p.n_rows, p.sums, vals, p.len, stride, p.flags, e));
}

// T pairs in tiles of 1024 consecutive elements: the tiled fill of DESIGN.md, section L.9, in a copy of its own
// (tile_fill.h's template measured slower here: profiles/tile_fill).  Two threads search all S rows for the owners of the tile's first and
// last element; the others then search between those two, which for rows of more than a few tokens is a handful of rows.
template <class T, bool VEC>
__global__ __launch_bounds__(kSpanBlock) void span_flat_kernel(SpanParams p) {
    __shared__ uint64_t s_row[2];
    const uint32_t* vals = (p.flags & kSpanChars) ? p.vals : nullptr;
    T* __restrict__ out = static_cast<T*>(p.out);
    const uint64_t n = p.n;
    const uint64_t n_tiles = (n + kSpanTile - 1) / kSpanTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kSpanTile;
        if (threadIdx.x < 2) s_row[threadIdx.x] = pack_find_row(p.offs, 0, 0, p.n_rows - 1, threadIdx.x ? tile_last(t0, kSpanTile, n) : t0);
        __syncthreads();
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kSpanGroup;
        if (e0 < n) {
            const uint32_t n_in = n - e0 < kSpanGroup ? (uint32_t)(n - e0) : kSpanGroup;
            SpanPair v[kSpanGroup] = {};
            span_group(p.offs, p.sums, vals, s_row[0], s_row[1], e0, n_in, v);
            if (VEC && n_in == kSpanGroup && sizeof(T) == 4) {  // e0 is a multiple of 4: 32 bytes at a 32-byte boundary
                int4* o = reinterpret_cast<int4*>(out + 2 * e0);
                o[0] = make_int4((int)v[0].start, (int)v[0].end, (int)v[1].start, (int)v[1].end);
                o[1] = make_int4((int)v[2].start, (int)v[2].end, (int)v[3].start, (int)v[3].end);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kSpanGroup; k++)
                    if (k < n_in) store_pair<VEC>(out, e0 + k, v[k]);
            }
        }
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

hipError_t span_scan_temp_bytes(uint64_t n, size_t* bytes) {
    *bytes = 0;
    auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, SpanValue());
    return rocprim::exclusive_scan(nullptr, *bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>());
}

// vals must have room for T + 1 entries: entry T is set to 0 and scanned, so that sums[T] is the stream's total
hipError_t launch_span_sums(const SpanParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (p.n == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p.vals + p.n, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(span_meta_kernel, dim3(grid_for(p.n, kSpanBlock, kSpanMaxBlocks)), dim3(kSpanBlock), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    auto in = rocprim::make_transform_iterator((const uint32_t*)p.vals, SpanValue());
    return rocprim::exclusive_scan(temp, temp_bytes, in, p.sums, (uint64_t)0, (size_t)(p.n + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_span_row_max(const SpanParams& p, hipStream_t stream) {
    if (p.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(span_row_max_kernel, dim3(grid_for(p.n_rows, kSpanBlock, kSpanMaxBlocks)), dim3(kSpanBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_span_flat(const SpanParams& p, hipStream_t stream) {
    if (p.n == 0 || p.n_rows == 0) return hipSuccess;
    const bool i64 = (p.flags & kLayoutI64) != 0;
    const bool vec = aligned(p.out, 16);
    const uint32_t grid = grid_for(p.n, kSpanTile, kSpanMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSpanBlock), 0, stream, p); };
    if (i64)
        vec ? launch(span_flat_kernel<int64_t, true>) : launch(span_flat_kernel<int64_t, false>);
    else
        vec ? launch(span_flat_kernel<int32_t, true>) : launch(span_flat_kernel<int32_t, false>);
    return hipGetLastError();
}

hipError_t launch_span_pad(const SpanParams& p, hipStream_t stream) {
    const uint64_t total = p.n_rows * (uint64_t)p.len;
    if (total == 0 || p.n == 0) return hipSuccess;
    const bool i64 = (p.flags & kLayoutI64) != 0;
    const bool vec = aligned(p.out, i64 ? 16 : 8);
    const uint32_t grid = grid_for(total, kSpanBlock, kSpanMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSpanBlock), 0, stream, p, total); };
    if (i64)
        vec ? launch(span_pad_kernel<int64_t, true>) : launch(span_pad_kernel<int64_t, false>);
    else
        vec ? launch(span_pad_kernel<int32_t, true>) : launch(span_pad_kernel<int32_t, false>);
    return hipGetLastError();
}

hipError_t launch_span_windows(const SpanParams& p, const uint64_t* wo, uint32_t stride, uint64_t n_windows, hipStream_t stream) {
    const uint64_t total = n_windows * (uint64_t)p.len;
    if (total == 0 || p.n == 0 || p.n_rows == 0) return hipSuccess;
    const bool i64 = (p.flags & kLayoutI64) != 0;
    const bool vec = aligned(p.out, i64 ? 16 : 8);
    const uint32_t grid = grid_for(total, kSpanBlock, kSpanMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSpanBlock), 0, stream, p, wo, stride, total); };
    if (i64)
        vec ? launch(span_window_kernel<int64_t, true>) : launch(span_window_kernel<int64_t, false>);
    else
        vec ? launch(span_window_kernel<int32_t, true>) : launch(span_window_kernel<int32_t, false>);
    return hipGetLastError();
}

}  // namespace tgx
