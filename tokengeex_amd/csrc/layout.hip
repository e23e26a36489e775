// A result's ids laid out for a model: [S, L] padded rows with an attention mask, or the documents concatenated and
// cut into [B, L] blocks, or long rows as overlapping [W, L] windows (include/tgx.h: tgx_result_pad_device,
// tgx_result_pack_device, tgx_result_window_pad_device).  Pure data movement: every
// thread slot owns four consecutive output elements, finds the rows they belong to (layout.h), reads each kept id
// once and writes the four with one 16-byte store (two for i64), the mask with one 4-byte store.  Destinations that
// are not 16-byte aligned take the same kernels with element-wide stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "layout.h"

namespace tgx {

namespace {

constexpr uint32_t kLayoutBlock = 256;
constexpr uint32_t kLayoutPerThread = kLayoutGroup;
constexpr uint32_t kLayoutTile = kLayoutBlock * kLayoutPerThread;
static_assert(kLayoutTile == kPackTile, "the host twin walks the kernel's tiles");
constexpr uint64_t kLayoutMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

__device__ inline void store4(int32_t* out, uint64_t e0, const uint32_t (&v)[4]) {
    *reinterpret_cast<int4*>(out + e0) = make_int4((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
}
__device__ inline void store4(int64_t* out, uint64_t e0, const uint32_t (&v)[4]) {
    longlong2* o = reinterpret_cast<longlong2*>(out + e0);
    o[0] = make_longlong2((long long)v[0], (long long)v[1]);
    o[1] = make_longlong2((long long)v[2], (long long)v[3]);
}

// sum / max over the block's 256 threads; the result is valid in thread 0
template <bool MAX>
__device__ inline unsigned long long block_reduce(unsigned long long x) {
    __shared__ unsigned long long part[kLayoutBlock / 64];
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long y = __shfl_down(x, d, 64);
        x = MAX ? (y > x ? y : x) : x + y;
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kLayoutBlock / 64; w++) x = MAX ? (part[w] > x ? part[w] : x) : x + part[w];
    }
    return x;
}

__global__ __launch_bounds__(kLayoutBlock) void layout_max_row_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                       unsigned long long* __restrict__ max_out) {
    unsigned long long best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kLayoutBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kLayoutBlock) {
        const unsigned long long n = offs[i + 1] - offs[i];
        best = n > best ? n : best;
    }
    best = block_reduce<true>(best);
    if (threadIdx.x == 0 && best) atomicMax(max_out, best);
}

// total = S·L elements, in groups of four
template <class T, bool VEC>
__global__ __launch_bounds__(kLayoutBlock) void layout_pad_kernel(LayoutParams p, uint64_t total) {
    const LayoutSeq seq = layout_seq(p.bos, p.eos, p.pad);
    const uint32_t L = p.len;
    T* __restrict__ out = static_cast<T*>(p.out);
    const uint64_t n_groups = (total + kLayoutPerThread - 1) / kLayoutPerThread;
    unsigned long long truncated = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * kLayoutBlock + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * kLayoutBlock) {
        const uint64_t e0 = g * kLayoutPerThread;
        const uint32_t n_in = total - e0 < kLayoutPerThread ? (uint32_t)(total - e0) : kLayoutPerThread;
        uint32_t v[kLayoutPerThread] = {0, 0, 0, 0};
        const uint32_t m = pad_group(seq, p.ids, p.offs, L, p.flags, e0, n_in, p.lengths, v, &truncated);
        if (VEC && n_in == kLayoutPerThread) {
            store4(out, e0, v);
            if (p.mask) *reinterpret_cast<uint32_t*>(p.mask + e0) = m;
        } else {
            for (uint32_t k = 0; k < n_in; k++) {
                out[e0 + k] = (T)v[k];
                if (p.mask) p.mask[e0 + k] = (uint8_t)(m >> (8 * k));
            }
        }
    }
    if (p.counter) {  // one atomic per block
        truncated = block_reduce<false>(truncated);
        if (threadIdx.x == 0 && truncated) atomicAdd(p.counter, truncated);
    }
}

// n_out elements in tiles of 1024 consecutive positions: the tiled fill of DESIGN.md, section L.9, in a copy of its own
// (tile_fill.h's template measured slower here and in layout_window_kernel: profiles/tile_fill).  Two threads search all
// S rows for the owners of the tile's first and last stream position; the others then search between those two, which
// for rows of more than a few tokens is a handful of rows.  The fill runs on over the padding of the last block.
template <class T, bool VEC>
__global__ __launch_bounds__(kLayoutBlock) void layout_pack_kernel(LayoutParams p, uint64_t n_stream, uint64_t n_out) {
    __shared__ uint64_t s_row[2];
    const LayoutSeq seq = layout_seq(p.bos, p.eos, p.pad);
    const uint64_t A = seq.extra;
    T* __restrict__ out = static_cast<T*>(p.out);
    const uint64_t n_tiles = (n_out + kLayoutTile - 1) / kLayoutTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kLayoutTile;
        if (threadIdx.x < 2 && t0 < n_stream) {
            uint64_t j = t0;
            if (threadIdx.x == 1) j = tile_last(t0, kLayoutTile, n_stream);
            s_row[threadIdx.x] = pack_find_row(p.offs, A, 0, p.n_rows - 1, j);
        }
        __syncthreads();
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kLayoutPerThread;
        if (e0 < n_out) {
            const uint32_t n_in = n_out - e0 < kLayoutPerThread ? (uint32_t)(n_out - e0) : kLayoutPerThread;
            uint32_t v[kLayoutPerThread] = {0, 0, 0, 0};
            int32_t doc[kLayoutPerThread] = {0, 0, 0, 0}, pos[kLayoutPerThread] = {0, 0, 0, 0};
            PackCursor cur;
#pragma unroll
            for (uint32_t k = 0; k < kLayoutPerThread; k++) {
                const uint64_t j = e0 + k;
                if (k < n_in && j < n_stream) {
                    const uint64_t i = pack_advance(cur, p.offs, A, s_row[0], s_row[1], j);
                    v[k] = pack_at(seq, p.ids, p.offs, i, j, &pos[k]);
                    doc[k] = (int32_t)i;
                } else {  // the tail of the last block
                    v[k] = seq.pad;
                    doc[k] = -1;
                    pos[k] = 0;
                }
            }
            if (VEC && n_in == kLayoutPerThread) {
                store4(out, e0, v);
                if (p.doc) *reinterpret_cast<int4*>(p.doc + e0) = make_int4(doc[0], doc[1], doc[2], doc[3]);
                if (p.pos) *reinterpret_cast<int4*>(p.pos + e0) = make_int4(pos[0], pos[1], pos[2], pos[3]);
            } else {
                for (uint32_t k = 0; k < n_in; k++) {
                    out[e0 + k] = (T)v[k];
                    if (p.doc) p.doc[e0 + k] = doc[k];
                    if (p.pos) p.pos[e0 + k] = pos[k];
                }
            }
        }
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

// counts[i] = the windows of row i; the longest row is reduced as in layout_max_row_kernel.  (A count that does not fit
// 32 bits belongs to a row of more than 2^31 tokens, which the caller refuses on the maximum.)
__global__ __launch_bounds__(kLayoutBlock) void layout_window_count_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t room,
                                                                            uint32_t step, uint32_t* __restrict__ counts,
                                                                            unsigned long long* __restrict__ max_out) {
    unsigned long long best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kLayoutBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kLayoutBlock) {
        const unsigned long long n = offs[i + 1] - offs[i];
        const uint64_t nw = window_count(n, room, step);
        counts[i] = nw < 0xFFFFFFFFull ? (uint32_t)nw : 0xFFFFFFFFu;
        best = n > best ? n : best;
    }
    best = block_reduce<true>(best);
    if (threadIdx.x == 0 && best) atomicMax(max_out, best);
}

// total = W·L elements in tiles of 1024 consecutive elements, as layout_pack_kernel: two threads search all S rows for
// the owners of the tile's first and last window, the others step a row cursor between those two over their four
// elements (win_group).
template <class T, bool VEC>
__global__ __launch_bounds__(kLayoutBlock) void layout_window_kernel(WindowParams q, uint64_t total) {
    __shared__ uint64_t s_row[2];
    const LayoutParams& p = q.base;
    const LayoutSeq seq = layout_seq(p.bos, p.eos, p.pad);
    const uint32_t L = p.len;
    T* __restrict__ out = static_cast<T*>(p.out);
    const uint64_t n_tiles = (total + kLayoutTile - 1) / kLayoutTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kLayoutTile;
        if (threadIdx.x < 2) {
            uint64_t e = t0;
            if (threadIdx.x == 1) e = tile_last(t0, kLayoutTile, total);
            s_row[threadIdx.x] = pack_find_row(q.wo, 0, 0, p.n_rows - 1, e / L);
        }
        __syncthreads();
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kLayoutPerThread;
        if (e0 < total) {
            const uint32_t n_in = total - e0 < kLayoutPerThread ? (uint32_t)(total - e0) : kLayoutPerThread;
            uint32_t v[kLayoutPerThread] = {0, 0, 0, 0};
            const uint32_t m = win_group(seq, p.ids, p.offs, q.wo, L, q.stride, p.flags, s_row[0], s_row[1], e0, n_in, p.lengths, q.window_row,
                                         q.window_first, v);
            if (VEC && n_in == kLayoutPerThread) {
                store4(out, e0, v);
                if (p.mask) *reinterpret_cast<uint32_t*>(p.mask + e0) = m;
            } else {
                for (uint32_t k = 0; k < n_in; k++) {
                    out[e0 + k] = (T)v[k];
                    if (p.mask) p.mask[e0 + k] = (uint8_t)(m >> (8 * k));
                }
            }
        }
        __syncthreads();  // s_row is rewritten for the next tile
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

hipError_t launch_layout_max_row(const uint64_t* offs, uint64_t n_rows, unsigned long long* max_out, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const uint32_t grid = grid_for(n_rows, kLayoutBlock, kLayoutMaxBlocks);
    hipLaunchKernelGGL(layout_max_row_kernel, dim3(grid), dim3(kLayoutBlock), 0, stream, offs, n_rows, max_out);
    return hipGetLastError();
}

hipError_t launch_layout_pad(const LayoutParams& p, hipStream_t stream) {
    const uint64_t total = p.n_rows * (uint64_t)p.len;
    if (total == 0) return hipSuccess;
    const bool i64 = (p.flags & kLayoutI64) != 0;
    const bool vec = aligned(p.out, 16) && aligned(p.mask, 4);
    const uint32_t grid = grid_for(total, kLayoutTile, kLayoutMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kLayoutBlock), 0, stream, p, total); };
    if (i64)
        vec ? launch(layout_pad_kernel<int64_t, true>) : launch(layout_pad_kernel<int64_t, false>);
    else
        vec ? launch(layout_pad_kernel<int32_t, true>) : launch(layout_pad_kernel<int32_t, false>);
    return hipGetLastError();
}

hipError_t launch_layout_pack(const LayoutParams& p, uint64_t n_stream, uint64_t n_out, hipStream_t stream) {
    if (n_out == 0) return hipSuccess;
    const bool i64 = (p.flags & kLayoutI64) != 0;
    const bool vec = aligned(p.out, 16) && aligned(p.doc, 16) && aligned(p.pos, 16);
    const uint32_t grid = grid_for(n_out, kLayoutTile, kLayoutMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kLayoutBlock), 0, stream, p, n_stream, n_out); };
    if (i64)
        vec ? launch(layout_pack_kernel<int64_t, true>) : launch(layout_pack_kernel<int64_t, false>);
    else
        vec ? launch(layout_pack_kernel<int32_t, true>) : launch(layout_pack_kernel<int32_t, false>);
    return hipGetLastError();
}

hipError_t launch_layout_window_count(const uint64_t* offs, uint64_t n_rows, uint32_t room, uint32_t step, uint32_t* counts,
                                      unsigned long long* max_out, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const uint32_t grid = grid_for(n_rows, kLayoutBlock, kLayoutMaxBlocks);
    hipLaunchKernelGGL(layout_window_count_kernel, dim3(grid), dim3(kLayoutBlock), 0, stream, offs, n_rows, room, step, counts, max_out);
    return hipGetLastError();
}

hipError_t launch_layout_windows(const WindowParams& q, uint64_t n_windows, hipStream_t stream) {
    const uint64_t total = n_windows * (uint64_t)q.base.len;
    if (total == 0 || q.base.n_rows == 0) return hipSuccess;
    const bool i64 = (q.base.flags & kLayoutI64) != 0;
    const bool vec = aligned(q.base.out, 16) && aligned(q.base.mask, 4);
    const uint32_t grid = grid_for(total, kLayoutTile, kLayoutMaxBlocks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kLayoutBlock), 0, stream, q, total); };
    if (i64)
        vec ? launch(layout_window_kernel<int64_t, true>) : launch(layout_window_kernel<int64_t, false>);
    else
        vec ? launch(layout_window_kernel<int32_t, true>) : launch(layout_window_kernel<int32_t, false>);
    return hipGetLastError();
}

}  // namespace tgx
