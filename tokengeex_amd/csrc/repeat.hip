// Repeated n-grams within a row on the device (include/tgx.h: tgx_*_repeat_stats_device; repeat.h has the definitions
// and the rules).  Four stages: repeat_keys_kernel walks the elements of all rows laid end to
// end (gram_walk.h) and writes every valid gram's row key and position to its slot; rocPRIM sorts the pairs by key,
// stably; repeat_runs_kernel, a thread a sorted slot, turns the runs of equal keys into one flag byte per element and
// the longest run per row; repeat_cover_kernel, the hot one, walks the elements again, a lane an element, and turns
// the flags into the rows' sums and covered elements with ballots.  No LDS, plain C++ and vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gram_walk.h"
#include "repeat.h"

namespace tgx {

namespace {

constexpr uint32_t kRepeatBlock = 256;
static_assert(kRepeatBlock == kGramTile && kGramTile == 4 * kGramChunk && kGramChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kRepeatMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

// keys_out / pos_out[g_offs[i] + t] = the row key / the element of the gram at element offs[i] + t, for every valid gram
template <bool kText>
__global__ __launch_bounds__(kRepeatBlock) void repeat_keys_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                   uint32_t width, uint64_t hs, const uint64_t* __restrict__ g_offs,
                                                                   uint64_t* __restrict__ keys_out, uint32_t* __restrict__ pos_out) {
    gram_walk<kText>(data_, offs, n_rows, width, hs, [=](uint64_t, uint32_t, const GramLane& g) {
        if (!g.valid) return;
        const uint64_t slot = g_offs[g.row] + (g.pos - offs[g.row]);
        keys_out[slot] = repeat_row_key(g.key, g.row);
        pos_out[slot] = (uint32_t)g.pos;
    });
}

// the table's pre-set: a thread a row
__global__ __launch_bounds__(kRepeatBlock) void repeat_preset_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t width,
                                                                     int64_t* __restrict__ stats) {
    for (uint64_t i = (uint64_t)blockIdx.x * kRepeatBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kRepeatBlock) {
        const uint64_t grams = gram_row_count(offs, n_rows, width, i);
#pragma unroll
        for (uint32_t k = 0; k < kRepeatN; k++) stats[k * n_rows + i] = 0;
        stats[kRpGrams * n_rows + i] = (int64_t)grams;
        stats[kRpTop * n_rows + i] = (int64_t)repeat_top_preset(grams);
    }
}

// flag[pos[t]] of every sorted slot t (each valid position is written exactly once; the launcher pre-set the array to
// 0).  The head of a run of two or more finds the run's end in log time and its row from its position, and maxes the
// run's length onto the row's `top` (pre-set to repeat_top_preset).  top may be NULL.
__global__ __launch_bounds__(kRepeatBlock) void repeat_runs_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint64_t n,
                                                                   const uint64_t* __restrict__ offs, uint64_t n_rows, uint8_t* __restrict__ flag,
                                                                   unsigned long long* top) {
    for (uint64_t t = (uint64_t)blockIdx.x * kRepeatBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kRepeatBlock) {
        const uint64_t k = keys[t];
        const bool head = t == 0 || keys[t - 1] != k, next_same = t + 1 < n && keys[t + 1] == k;
        const uint32_t p = pos[t];
        flag[p] = repeat_flag(head, next_same);
        if (top && head && next_same) {
            const unsigned long long len = repeat_run_end(keys, n, t) - t;
            const uint64_t row = pack_find_row(offs, 0, 0, n_rows - 1, p);
            atomicMax(&top[row], len);
        }
    }
}

// repeated, multi, covered and covered_all of every row.  A lane loads its element's flag and the flag 64 elements
// before it; ballots of the two bits give a window of 128 elements per bit, from which repeat_covered takes the lane's
// part.  The four ballots are then cut into the chunk's stretches of one row as gram_hits_kernel cuts its hits: the
// lane at which a stretch begins popcounts them and, by the rule of gram.h, stores plainly when the row lies inside the
// chunk and else adds to the row's sums (pre-set to 0).
__global__ __launch_bounds__(kRepeatBlock) void repeat_cover_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t width,
                                                                    const uint8_t* __restrict__ flag, unsigned long long* stats) {
    const uint32_t lane = threadIdx.x & 63u;
    gram_walk<true, false>(nullptr, offs, n_rows, width, 0, [=](uint64_t c0, uint32_t n_in, const GramLane& g) {
        const uint32_t f = g.in ? flag[g.pos] : 0u;
        const uint32_t fb = c0 ? flag[c0 - kGramChunk + lane] : 0u;  // (the chunk before is whole)
        const uint64_t rep = __ballot(f & kRepeatBitRepeat), mul = __ballot(f & kRepeatBitMulti);
        const uint64_t rep_b = __ballot(fb & kRepeatBitRepeat), mul_b = __ballot(fb & kRepeatBitMulti);
        const uint64_t rs = g.in ? offs[g.row] : 0;
        const uint64_t cov = __ballot(g.in && repeat_covered(rep_b, rep, lane, g.pos, rs, width));
        const uint64_t cov_all = __ballot(g.in && repeat_covered(mul_b, mul, lane, g.pos, rs, width));
        const uint32_t row_before = (uint32_t)__shfl_up((int)g.row, 1, 64);
        const bool begins = g.in && (lane == 0 || g.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~((2ull << lane) - 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const uint64_t stretch = ((end >= 64 ? 0ull : (1ull << end)) - 1) & ~((1ull << lane) - 1);  // lanes [lane, end)
            const bool inside = gram_row_inside(offs, g.row, c0);
            const uint64_t ballots[4] = {rep, mul, cov, cov_all};
            const uint32_t which[4] = {kRpRepeated, kRpMulti, kRpCovered, kRpCoveredAll};
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                const unsigned long long v = (unsigned long long)__popcll(ballots[q] & stretch);
                unsigned long long* dst = &stats[which[q] * n_rows + g.row];
                if (inside)
                    *dst = v;
                else if (gram_adds(v))
                    atomicAdd(dst, v);
            }
        }
    });
}

}  // namespace

hipError_t repeat_sort_bytes(uint64_t n, size_t* sort_bytes) {
    *sort_bytes = 0;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *sort_bytes, k, k, v, v, (size_t)n);
}

hipError_t launch_repeat_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, uint32_t* pos_out,
                              hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kRepeatMaxBlocks)), block(kRepeatBlock);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(repeat_keys_kernel<true>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out, pos_out);
    else
        hipLaunchKernelGGL(repeat_keys_kernel<false>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out, pos_out);
    return hipGetLastError();
}

hipError_t launch_repeat_sort(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* pos_in, uint32_t* pos_out, uint64_t n, void* sort_tmp,
                              size_t sort_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys_in, keys_out, pos_in, pos_out, (size_t)n, 0, 64, stream);
}

hipError_t launch_repeat_preset(const DedupRows& rows, uint32_t width, int64_t* stats, uint8_t* flag, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (rows.n_elems) {
        const hipError_t e = hipMemsetAsync(flag, 0, (size_t)rows.n_elems, stream);
        if (e != hipSuccess) return e;
    }
    if (!stats) return hipSuccess;
    hipLaunchKernelGGL(repeat_preset_kernel, dim3(grid_for(rows.n_rows, kRepeatBlock, kRepeatMaxBlocks)), dim3(kRepeatBlock), 0, stream, rows.offs,
                       rows.n_rows, width, stats);
    return hipGetLastError();
}

hipError_t launch_repeat_runs(const DedupRows& rows, const uint64_t* keys, const uint32_t* pos, uint64_t n, uint8_t* flag, int64_t* stats,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    unsigned long long* top = stats ? reinterpret_cast<unsigned long long*>(stats) + (uint64_t)kRpTop * rows.n_rows : nullptr;
    hipLaunchKernelGGL(repeat_runs_kernel, dim3(grid_for(n, kRepeatBlock, kRepeatMaxBlocks)), dim3(kRepeatBlock), 0, stream, keys, pos, n, rows.offs,
                       rows.n_rows, flag, top);
    return hipGetLastError();
}

hipError_t launch_repeat_cover(const DedupRows& rows, uint32_t width, const uint8_t* flag, int64_t* stats, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0 || !stats) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kRepeatMaxBlocks)), block(kRepeatBlock);
    hipLaunchKernelGGL(repeat_cover_kernel, grid, block, 0, stream, rows.offs, rows.n_rows, width, flag, reinterpret_cast<unsigned long long*>(stats));
    return hipGetLastError();
}

}  // namespace tgx
