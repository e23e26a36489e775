// Runs of a byte mask replaced in a new resident corpus, on the device (include/tgx_redact.h: tgx_corpus_redact; redact.h
// has a byte's class, the head of a run, a lane's length, the table and the new offset of a row boundary; DESIGN.md,
// section L.19).  The kernels walk the bytes of all rows laid end to end with textstat_walk.h's walk, a lane a byte.
// redact_length_kernel sums what the 64 bytes of a chunk put out and writes one u64 per chunk; a rocPRIM exclusive sum
// gives every chunk its place in the new text; redact_offsets_kernel, a thread per row boundary, adds to the carry of the
// boundary's chunk what the at most 63 bytes in front of it put out; redact_fill_kernel recomputes the lengths, takes an
// exclusive sum inside the wave and writes: a copying lane its byte, a head its replacement out of LDS.
//
// The class of the byte before a lane's comes from a shuffle; lane 0 reads mask[pos - 1] when its byte is not its row's
// first.  The table, 8 x 64 bytes and 8 lengths, is copied into LDS once by every block.  No LDS beyond it, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "redact.h"
#include "scan_helpers.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

constexpr uint32_t kRedactRowBlock = 256;
constexpr uint64_t kRedactRowMaxBlocks = 4096;

__device__ inline void redact_load_table(const uint64_t* __restrict__ table, RedactTable& lds) {
    static_assert(kRedactTableWords <= kTextstatBlock, "a thread a word");
    if (threadIdx.x < kRedactTableWords) reinterpret_cast<uint64_t*>(&lds)[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
}

// what a lane's byte puts out (0 in a lane without a byte), and its class
__device__ inline uint32_t redact_lane(const uint8_t* __restrict__ mask, const TextLane& t, uint32_t lane, uint32_t n_repl, const uint8_t* lens, uint32_t* cls) {
    *cls = t.in ? redact_class(mask[t.pos], n_repl) : kRedactNone;
    uint32_t before = (uint32_t)__shfl_up((int)*cls, 1, 64);
    const bool row_first = t.pos == t.row_begin;
    if (lane == 0 && t.in && !row_first) before = redact_class(mask[t.pos - 1], n_repl);
    return t.in ? redact_len(*cls, before, row_first, lens) : 0u;
}
// the inclusive sum over the wave's lanes (at most 64 x 64, far inside 32 bits)
__device__ inline uint32_t redact_wave_sum(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += below;
    }
    return v;
}

__global__ __launch_bounds__(kTextstatBlock) void redact_length_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                       const uint8_t* __restrict__ mask, uint32_t n_repl, const uint64_t* __restrict__ table,
                                                                       uint64_t n_chunks, uint64_t* __restrict__ rec) {
    __shared__ RedactTable lds;
    redact_load_table(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t, uint64_t, const TextLane& t) {
        uint32_t cls;
        const uint32_t sum = redact_wave_sum(redact_lane(mask, t, lane, n_repl, lds.len, &cls), lane);
        if (lane == 63) {
            const uint64_t k = c0 / kTextstatChunk;
            rec[k] = sum;
            if (k + 1 == n_chunks) rec[n_chunks] = 0;
        }
    });
}

__global__ __launch_bounds__(kRedactRowBlock) void redact_offsets_kernel(const uint8_t* __restrict__ mask, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                         uint32_t n_repl, const uint64_t* __restrict__ table,
                                                                         const uint64_t* __restrict__ carry, uint64_t* __restrict__ new_offs) {
    const uint8_t* lens = reinterpret_cast<const RedactTable*>(table)->len;
    for (uint64_t r = (uint64_t)blockIdx.x * kRedactRowBlock + threadIdx.x; r <= n_rows; r += (uint64_t)gridDim.x * kRedactRowBlock)
        new_offs[r] = redact_row_offset(mask, offs, r, n_repl, lens, carry);
}

__global__ __launch_bounds__(kTextstatBlock) void redact_fill_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     const uint8_t* __restrict__ mask, uint32_t n_repl, const uint64_t* __restrict__ table,
                                                                     const uint64_t* __restrict__ carry, uint8_t* __restrict__ out) {
    __shared__ RedactTable lds;
    redact_load_table(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t, uint64_t, const TextLane& t) {
        uint32_t cls;
        const uint32_t len = redact_lane(mask, t, lane, n_repl, lds.len, &cls);
        uint8_t* at = out + carry[c0 / kTextstatChunk] + (redact_wave_sum(len, lane) - len);
        if (cls == kRedactNone) {
            if (t.in) *at = t.b;
        } else {
            for (uint32_t q = 0; q < len; q++) at[q] = lds.bytes[cls][q];
        }
    });
}

}  // namespace

hipError_t redact_scan_bytes(uint64_t n_recs, size_t* scan_bytes) {
    *scan_bytes = 0;
    return sum_scan(nullptr, nullptr, n_recs, nullptr, *scan_bytes, nullptr);
}

hipError_t launch_redact_lengths(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, uint64_t* rec, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint64_t n_chunks = (rows.n_elems + kTextstatChunk - 1) / kTextstatChunk;
    hipLaunchKernelGGL(redact_length_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, mask, n_repl, table,
                       n_chunks, rec);
    return hipGetLastError();
}

hipError_t launch_redact_scan(const uint64_t* rec, uint64_t* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    return sum_scan(rec, carry, n_recs, scan_tmp, scan_bytes, stream);
}

hipError_t launch_redact_offsets(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, const uint64_t* carry, uint64_t* new_offs,
                                 hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_rows + 1, kRedactRowBlock, kRedactRowMaxBlocks)), block(kRedactRowBlock);
    hipLaunchKernelGGL(redact_offsets_kernel, grid, block, 0, stream, mask, rows.offs, rows.n_rows, n_repl, table, carry, new_offs);
    return hipGetLastError();
}

hipError_t launch_redact_fill(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, const uint64_t* carry, uint8_t* out,
                              hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(redact_fill_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, mask, n_repl, table, carry,
                       out);
    return hipGetLastError();
}

}  // namespace tgx
