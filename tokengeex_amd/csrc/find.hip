// Leftmost-first, non-overlapping matches over the bytes of every row on the device, and the counting of the distinct
// matches (include/tgx_find.h: tgx_corpus_find_device, tgx_corpus_mine_device; find.h has the table, the step, the walk
// byte, the maps and the order rule).  A wave owns whole segments, as in dfa64.hip:
//
//   find_walk_kernel, a lane per START byte.  A wave holds a chunk's 64 bytes and the 64 behind them in ONE register, a
//     lane two bytes; at trip t lane j reads the byte at j + t from lane (j + t) & 63 with one ds_bpermute and takes its
//     low or its high byte, and advances its walk with one ds_read_u8 of the table (state, tagged and dead in one
//     entry).  The loop runs while a ballot of the live lanes is non-empty, max_len trips at most; on ordinary text
//     nearly every lane dies on its first byte, so its time depends on the text.  It stores a walk byte per position,
//     forms the chunk's skip map with six more cross-lane reads (pointer doubling) and folds it into the segment's record
//     with dfa64's composition.  No text in LDS and no barrier after the table's copy.
//   launch_dfa64_scan (dfa64.hip, unchanged) scans the records from skip 0: every segment's entry skip.
//   find_replay_kernel, a lane per position again.  The wave carries the skip through its segment's chunks as an SGPR.
//     It doubles the chunk's pointers once more, now with the 64-bit set of the lanes passed under the same reads, takes
//     the set and the pointer of the lane at the entry skip with v_readlane: the visited positions and the next skip.
//     It clears the lengths of the positions not visited and sums the matches and the truncated walks per row by the
//     store / add rule of dfa64_count_kernel.
//   The mine: the matches' positions are compacted (textstat.hip's select), find_key_kernel hashes a match a lane,
//     the pairs are sorted by key, find_head_kernel and find_run_kernel turn runs of equal keys into (first position,
//     count), two stable sorts bring them into find_before's order and find_top_kernel gathers the first `top`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "find.h"
#include "minhash.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

constexpr uint32_t kFindBlockWaves = kDfa64BlockWaves;
constexpr uint32_t kFindBlock = kFindBlockWaves * 64;
constexpr uint32_t kFindFlat = 256;  // threads of the mine's element-wise kernels

struct alignas(16) FindLds {
    uint8_t next[kFindTableBytes];
};

__device__ inline void find_load_table(const uint8_t* __restrict__ table, FindLds& lds) {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    uint4* dst = reinterpret_cast<uint4*>(&lds);
    for (uint32_t i = threadIdx.x; i < kFindTableBytes / 16; i += kFindBlock) dst[i] = src[i];
    __syncthreads();
}

// the wave's run of consecutive segments, [begin, end) (dfa64_run's split)
struct FindRun {
    uint64_t begin, end;
};
__device__ inline FindRun find_run(uint64_t n_segs) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t waves = (uint64_t)gridDim.x * kFindBlockWaves, per = (n_segs + waves - 1) / waves;
    const uint64_t begin = ((uint64_t)blockIdx.x * kFindBlockWaves + wave) * per;
    return {begin < n_segs ? begin : n_segs, begin + per < n_segs ? begin + per : n_segs};
}

// What a lane knows of its position in the chunk at c0 of n_in bytes: the owners of the chunk's ends are galloped from
// the chunk before (hi, first: the wave's cursor), a lane's is searched between them.
struct FindLane {
    uint64_t pos, row, row_end;
    bool in;
};
__device__ inline FindLane find_lane(const uint64_t* __restrict__ offs, uint64_t n_rows, uint64_t c0, uint32_t n_in, uint32_t lane, uint64_t& hi, bool& first) {
    const uint64_t lo = first ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
    hi = dedup_find_from(offs, lo, n_rows - 1, c0 + n_in - 1);
    first = false;
    FindLane l = {c0 + lane, lo, 0, lane < n_in};
    if (l.in) {
        l.row = pack_find_row(offs, 0, lo, hi, l.pos);
        l.row_end = offs[l.row + 1];
    }
    return l;
}

// `a` then `b` of two maps, a lane a skip: lane r fetches b from lane a[r] (dfa64_then)
__device__ inline uint32_t find_then(uint32_t a, uint32_t b) { return (uint32_t)__shfl((int)b, (int)a, 64); }

// ---- the walk, the chunk's map and the segment's record -----------------------------------------------------------------
__global__ __launch_bounds__(kFindBlock) void find_walk_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows, uint64_t N,
                                                               uint32_t start, uint32_t max_len, const uint8_t* __restrict__ table, uint8_t* __restrict__ walk,
                                                               uint8_t* __restrict__ srec) {
    __shared__ FindLds lds;
    find_load_table(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const FindRun run = find_run(dfa64_segs(N));
    uint64_t hi = 0;
    bool first = true;
    for (uint64_t seg = run.begin; seg < run.end; seg++) {
        uint32_t seg_map = lane;
        for (uint32_t k = 0; k < kDfa64SegChunks; k++) {
            const uint64_t c0 = (seg * kDfa64SegChunks + k) * kDfa64Chunk;
            const uint32_t n_in = dfa64_chunk_bytes(c0, N);
            if (!n_in) break;  // (the chunks past the corpus's end have the identity)
            const FindLane l = find_lane(offs, n_rows, c0, n_in, lane, hi, first);
            // the chunk's bytes in the low byte and the 64 behind them in the high one
            const uint64_t behind = l.pos + kDfa64Chunk;
            const uint32_t two = (l.in ? (uint32_t)text[l.pos] : 0u) | (behind < N ? (uint32_t)text[behind] << 8 : 0u);
            const uint32_t limit = l.in ? find_limit(l.pos, l.row_end, max_len) : 0u;
            uint32_t q = start, len = 0, wb = 0;
            bool live = limit != 0;
            for (uint32_t t = 0; __ballot(live) != 0; t++) {
                const uint32_t v = (uint32_t)__shfl((int)two, (int)((lane + t) & 63u), 64);
                if (live) {
                    live = find_advance(lds.next, lane + t < kDfa64Chunk ? v & 255u : v >> 8, t, q, len);
                    if (!live) {
                        wb = len;
                    } else if (t + 1 == limit) {
                        wb = find_walk_byte(len, true, t + 1, max_len, l.pos, l.row_end);
                        live = false;
                    }
                }
            }
            if (l.in) walk[l.pos] = (uint8_t)wb;
            uint32_t ptr = lane + (l.in ? find_hop(wb) : 1u);
#pragma unroll
            for (uint32_t d = 0; d < kFindDoublings; d++) {
                const uint32_t far = (uint32_t)__shfl((int)ptr, (int)(ptr & 63u), 64);
                if (ptr < kDfa64Chunk) ptr = far;
            }
            seg_map = find_then(seg_map, ptr - kDfa64Chunk);
        }
        srec[seg * kDfa64Map + lane] = (uint8_t)seg_map;
    }
}

// ---- the replay ---------------------------------------------------------------------------------------------------------
// a row's sum of the chunk's stretch that begins at this lane, by the store / add rule
__device__ inline void find_row_sum(unsigned long long* out, uint64_t row, bool inside, uint64_t mask) {
    const unsigned long long v = textstat_popc(mask);
    if (inside)
        out[row] = v;
    else if (textstat_adds(v))
        atomicAdd(&out[row], v);
}

template <bool kSums>
__global__ __launch_bounds__(kFindBlock) void find_replay_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint64_t N, const uint8_t* walk,
                                                                 const uint8_t* __restrict__ sentry, uint8_t* lens, unsigned long long* count,
                                                                 unsigned long long* truncated) {
    const uint32_t lane = threadIdx.x & 63u;
    const FindRun run = find_run(dfa64_segs(N));
    uint64_t hi = 0;
    bool first = true;
    for (uint64_t seg = run.begin; seg < run.end; seg++) {
        uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)sentry[seg]);
        for (uint32_t k = 0; k < kDfa64SegChunks; k++) {
            const uint64_t c0 = (seg * kDfa64SegChunks + k) * kDfa64Chunk;
            const uint32_t n_in = dfa64_chunk_bytes(c0, N);
            if (!n_in) break;
            const uint64_t pos = c0 + lane;
            const bool in = lane < n_in;
            const uint32_t wb = in ? walk[pos] : 0u;
            uint32_t ptr = lane + (in ? find_hop(wb) : 1u);
            uint32_t reach_lo = lane < 32 ? 1u << lane : 0u, reach_hi = lane < 32 ? 0u : 1u << (lane - 32);
#pragma unroll
            for (uint32_t d = 0; d < kFindDoublings; d++) {
                const int src = (int)(ptr & 63u);
                const uint32_t far = (uint32_t)__shfl((int)ptr, src, 64);
                const uint32_t far_lo = (uint32_t)__shfl((int)reach_lo, src, 64), far_hi = (uint32_t)__shfl((int)reach_hi, src, 64);
                if (ptr < kDfa64Chunk) {
                    ptr = far;
                    reach_lo |= far_lo;
                    reach_hi |= far_hi;
                }
            }
            const uint64_t visited = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)reach_lo, (int)e) |
                                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)reach_hi, (int)e) << 32);
            e = (uint32_t)__builtin_amdgcn_readlane((int)ptr, (int)e) - kDfa64Chunk;
            const bool seen = in && ((visited >> lane) & 1ull);
            const uint32_t len = seen ? find_len(wb) : 0u;
            if (lens && in) lens[pos] = (uint8_t)len;
            if (kSums) {
                const FindLane l = find_lane(offs, n_rows, c0, n_in, lane, hi, first);
                const uint64_t emitted = __ballot(len != 0), cut = __ballot(seen && (wb & kFindTrunc));
                const uint32_t row_before = (uint32_t)__shfl_up((int)(uint32_t)l.row, 1, 64);
                const bool begins = in && (lane == 0 || (uint32_t)l.row != row_before);
                const uint64_t heads = __ballot(begins);
                if (begins) {
                    const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
                    const uint64_t span = textstat_span(lane, (above ? (uint32_t)__builtin_ctzll(above) : n_in) - 1);
                    const bool inside = textstat_row_inside(offs, l.row, c0);
                    if (count) find_row_sum(count, l.row, inside, emitted & span);
                    if (truncated) find_row_sum(truncated, l.row, inside, cut & span);
                }
            }
        }
    }
}

// ---- the mine -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFindFlat) void find_key_kernel(const uint8_t* __restrict__ text, const uint8_t* __restrict__ lens, const uint64_t* __restrict__ pos,
                                                             uint64_t n, uint64_t hs, uint64_t* __restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFindFlat + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFindFlat) {
        const uint64_t p = pos[i];
        const uint32_t len = lens[p];  // 1 .. 64
        uint64_t words[kMinhashMaxBytes / 8];
#pragma unroll
        for (uint32_t j = 0; j < kMinhashMaxBytes / 8; j++) {
            uint64_t w = 0;
            for (uint32_t b = 0; b < 8 && 8 * j + b < len; b++) w |= (uint64_t)text[p + 8 * j + b] << (8 * b);
            words[j] = w;
        }
        keys[i] = minhash_hash_words(words, len, hs);
    }
}

__global__ __launch_bounds__(kFindFlat) void find_head_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint8_t* __restrict__ heads) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFindFlat + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFindFlat)
        heads[i] = i == 0 || keys[i] != keys[i - 1];
}

__global__ __launch_bounds__(kFindFlat) void find_run_kernel(const uint64_t* __restrict__ head, uint64_t n_runs, uint64_t n, const uint64_t* __restrict__ pos,
                                                             uint64_t* __restrict__ run_pos, uint64_t* __restrict__ run_count) {
    for (uint64_t r = (uint64_t)blockIdx.x * kFindFlat + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * kFindFlat) {
        const uint64_t h = head[r];
        run_pos[r] = pos[h];  // (the sort is stable and the positions ascended: the run's first is its smallest)
        run_count[r] = (r + 1 < n_runs ? head[r + 1] : n) - h;
    }
}

__global__ __launch_bounds__(kFindFlat) void find_top_kernel(const uint64_t* __restrict__ run_pos, const uint64_t* __restrict__ run_count,
                                                             const uint8_t* __restrict__ lens, uint64_t n_top, uint64_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFindFlat + threadIdx.x; i < n_top; i += (uint64_t)gridDim.x * kFindFlat) {
        out[3 * i] = run_pos[i];
        out[3 * i + 1] = lens[run_pos[i]];
        out[3 * i + 2] = run_count[i];
    }
}

inline dim3 find_flat_grid(uint64_t n) { return dim3(grid_for(n, kFindFlat, 1u << 16)); }

}  // namespace

hipError_t launch_find_walk(const DedupRows& rows, uint32_t start, uint32_t max_len, const uint8_t* table, uint8_t* walk, uint8_t* srec, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(dfa64_grid(dfa64_segs(rows.n_elems), kTextstatMaxBlocks)), block(kFindBlock);
    hipLaunchKernelGGL(find_walk_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, rows.n_elems, start, max_len, table,
                       walk, srec);
    return hipGetLastError();
}

hipError_t launch_find_replay(const DedupRows& rows, const uint8_t* walk, const uint8_t* sentry, uint8_t* lens, int64_t* count, int64_t* truncated,
                              hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (count) e = hipMemsetAsync(count, 0, (size_t)rows.n_rows * 8, stream);
    if (e == hipSuccess && truncated) e = hipMemsetAsync(truncated, 0, (size_t)rows.n_rows * 8, stream);
    if (e != hipSuccess || rows.n_elems == 0) return e;
    const dim3 grid(dfa64_grid(dfa64_segs(rows.n_elems), kTextstatMaxBlocks)), block(kFindBlock);
    auto* c = reinterpret_cast<unsigned long long*>(count);
    auto* t = reinterpret_cast<unsigned long long*>(truncated);
    if (count || truncated)
        hipLaunchKernelGGL(find_replay_kernel<true>, grid, block, 0, stream, rows.offs, rows.n_rows, rows.n_elems, walk, sentry, lens, c, t);
    else
        hipLaunchKernelGGL(find_replay_kernel<false>, grid, block, 0, stream, rows.offs, rows.n_rows, rows.n_elems, walk, sentry, lens, c, t);
    return hipGetLastError();
}

hipError_t launch_find_keys(const uint8_t* text, const uint8_t* lens, const uint64_t* pos, uint64_t n, uint64_t seed, uint64_t* keys, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(find_key_kernel, find_flat_grid(n), dim3(kFindFlat), 0, stream, text, lens, pos, n, dedup_seed(minhash_hash_seed(seed)), keys);
    return hipGetLastError();
}

hipError_t find_sort_bytes(uint64_t n, size_t* bytes) {
    uint64_t* k = nullptr;
    size_t up = 0, down = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, up, k, k, k, k, (size_t)n);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs_desc(nullptr, down, k, k, k, k, (size_t)n);
    *bytes = up > down ? up : down;
    return e;
}

hipError_t launch_find_sort(const uint64_t* keys, uint64_t* keys_out, const uint64_t* pos, uint64_t* pos_out, uint64_t n, void* tmp, size_t bytes,
                            hipStream_t stream) {
    return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, pos, pos_out, (size_t)n, 0, 64, stream);
}

hipError_t launch_find_heads(const uint64_t* keys, uint64_t n, uint8_t* heads, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(find_head_kernel, find_flat_grid(n), dim3(kFindFlat), 0, stream, keys, n, heads);
    return hipGetLastError();
}

hipError_t launch_find_runs(const uint64_t* head, uint64_t n_runs, uint64_t n, const uint64_t* pos, uint64_t* run_pos, uint64_t* run_count, hipStream_t stream) {
    if (n_runs == 0) return hipSuccess;
    hipLaunchKernelGGL(find_run_kernel, find_flat_grid(n_runs), dim3(kFindFlat), 0, stream, head, n_runs, n, pos, run_pos, run_count);
    return hipGetLastError();
}

hipError_t launch_find_order(uint64_t* run_pos, uint64_t* run_count, uint64_t* pos_tmp, uint64_t* count_tmp, uint64_t n_runs, void* tmp, size_t bytes,
                             hipStream_t stream) {
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, run_pos, pos_tmp, run_count, count_tmp, (size_t)n_runs, 0, 64, stream);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs_desc(tmp, bytes, count_tmp, run_count, pos_tmp, run_pos, (size_t)n_runs, 0, 64, stream);
    return e;
}

hipError_t launch_find_top(const uint64_t* run_pos, const uint64_t* run_count, const uint8_t* lens, uint64_t n_top, uint64_t* out, hipStream_t stream) {
    if (n_top == 0) return hipSuccess;
    hipLaunchKernelGGL(find_top_kernel, find_flat_grid(n_top), dim3(kFindFlat), 0, stream, run_pos, run_count, lens, n_top, out);
    return hipGetLastError();
}

}  // namespace tgx
