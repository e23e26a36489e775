// Hashed n-gram features on the device (include/tgx_hashed.h: tgx_*_hashed_counts_device, tgx_*_hashed_scores_device;
// hashed.h has the feature, the keys of all widths from one window, the limits and the LDS budget; gram.h the chunk, the
// validity and the store / add rule).  The elements of all rows are laid end to end and a lane
// takes an element, as in gram.hip, but the walk is this file's own: a block is sixteen waves that share ONE table in LDS,
// and a wave takes a run of consecutive chunks, so that a long row stays with one wave.
//
// hashed_scores_kernel: the block copies the weights, laid out [B][KP] (KP: K padded to a power of two), into LDS.  A
// lane loads the longest valid window at its element once, forms the keys of all widths from it (hashed_keys), and per
// width reads the feature's KP weights with one wide LDS read and adds them to KP 64-bit sums in registers.  The lanes of
// a row are contiguous: a segmented scan over the wave (__shfl_up, as many doubling steps as the chunk's longest stretch
// needs) leaves a stretch's sum in its last lane, which stores or adds it by gram.h's rule.  A chunk that is a stretch
// of ONE row that goes on past it is not scanned at all: its lanes' sums are added to a carry, lane by lane, which is
// reduced and added to the row once, when the wave meets another row or its run ends.  The sums are integers, so the
// order of all this changes no bit.  Above the LDS budget the same kernel reads the table from memory (kLds = false).
//
// hashed_counts_kernel: the same walk with a histogram of 32-bit bins in LDS, flushed with 64-bit atomics when the block's
// run ends (hashed_bins_hold: a bin cannot wrap); above the budget 64-bit atomics on the counts themselves.  Text is
// Zipfian, and 64 adds to one address serialise: before it adds, a wave peels its first pending lane's bucket, counts
// the lanes that share it with a ballot and adds that number once, up to four times or until a peel finds a bucket of a
// single lane; what is left adds by itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram.h"
#include "hashed.h"
#include "shingle_load.h"

namespace tgx {

namespace {

constexpr uint64_t kHashedMaxBlocks = 512;  // a capped grid: two blocks of sixteen waves a CU
constexpr uint32_t kHashedNoRow = 0xFFFFFFFFu;
static_assert(kGramChunk == 64 && kHashedBlock == 1024, "a wave is a chunk; the host twin walks the same chunks");

// What a lane knows of its element: `in`, the element exists; row, its owner; the first n_valid widths own a gram there,
// whose keys are keys[0 .. n_valid).
struct HashedLane {
    uint64_t keys[kHashedMaxWidths];
    uint32_t row, n_valid;
    bool in;
};

// the chunks [begin, end) of this wave
__device__ inline void hashed_run(uint64_t n_elems, uint64_t& begin, uint64_t& end) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_chunks = (n_elems + kGramChunk - 1) / kGramChunk, per_wave = hashed_run_chunks(n_elems, gridDim.x);
    begin = ((uint64_t)blockIdx.x * kHashedWaves + wave) * per_wave;
    end = begin + per_wave < n_chunks ? begin + per_wave : n_chunks;
}

// The lane's part of the chunk at c0, whose ends' owners are lo and hi: one load of the longest valid window.
template <bool kText>
__device__ inline HashedLane hashed_lane(const void* __restrict__ data_, const uint64_t* __restrict__ offs, const HashedWidths& ws, uint64_t hs, uint64_t c0,
                                         uint64_t c_last, uint64_t lo, uint64_t hi, uint32_t lane) {
    HashedLane g = {{0, 0, 0, 0}, (uint32_t)lo, 0, false};
    const uint64_t pos = c0 + lane;
    g.in = pos <= c_last;
    if (g.in) {
        const uint64_t i = pack_find_row(offs, 0, lo, hi, pos);
        g.row = (uint32_t)i;
        g.n_valid = hashed_valid_widths(ws, pos, offs[i + 1]);
        if (g.n_valid) {
            uint64_t w[8];
            const uint32_t window = hashed_window(ws, g.n_valid);
            if constexpr (kText)
                minhash_load_text(static_cast<const uint8_t*>(data_), pos, window, w);
            else
                minhash_load_ids(static_cast<const uint32_t*>(data_), pos, window, w);
            hashed_keys(w, ws, kText ? 1u : 4u, g.n_valid, hs, g.keys);
        }
    }
    return g;
}

// acc[k] += the k-th weight of the feature's entry: KP consecutive i32, one read of 4, 8 or 16 bytes (KP = 8, 16: two, four)
template <uint32_t KP>
__device__ inline void hashed_add_weights(const int32_t* tab, uint64_t b, long long (&acc)[KP]) {
    const int32_t* p = tab + b * KP;
    if constexpr (KP == 1) {
        acc[0] += p[0];
    } else if constexpr (KP == 2) {
        const int2 v = *reinterpret_cast<const int2*>(p);
        acc[0] += v.x;
        acc[1] += v.y;
    } else {
#pragma unroll
        for (uint32_t t = 0; t < KP / 4; t++) {
            const int4 v = reinterpret_cast<const int4*>(p)[t];
            acc[4 * t] += v.x;
            acc[4 * t + 1] += v.y;
            acc[4 * t + 2] += v.z;
            acc[4 * t + 3] += v.w;
        }
    }
}

// the carry of a row that fills whole chunks: summed over the wave and added to the row's scores, then cleared
template <uint32_t KP>
__device__ inline void hashed_flush_carry(unsigned long long* scores, uint32_t n_vectors, uint32_t row, long long (&carry)[KP], uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < KP; k++) {
        long long v = carry[k];
#pragma unroll
        for (uint32_t d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0 && k < n_vectors && gram_adds((uint64_t)v)) atomicAdd(&scores[(uint64_t)row * n_vectors + k], (unsigned long long)v);
        carry[k] = 0;
    }
}

// table[b][k] = q[k][b], zero where k >= K
__global__ __launch_bounds__(256) void hashed_table_kernel(const int32_t* __restrict__ q, uint64_t buckets, uint32_t n_vectors, uint32_t kp,
                                                           int32_t* __restrict__ table) {
    const uint64_t n = buckets * kp;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t b = i / kp;
        const uint32_t k = (uint32_t)(i % kp);
        table[i] = k < n_vectors ? q[(uint64_t)k * buckets + b] : 0;
    }
}

template <bool kText, uint32_t KP, bool kLds>
__global__ __launch_bounds__(kHashedBlock) void hashed_scores_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     HashedWidths ws, uint64_t hs, uint64_t buckets, uint32_t n_vectors,
                                                                     const int32_t* __restrict__ table, unsigned long long* scores) {
    __shared__ __attribute__((aligned(16))) int32_t s_table[kLds ? kHashedLdsEntries : 4];
    const int32_t* tab = table;
    if constexpr (kLds) {
        const uint32_t n_entries = (uint32_t)buckets * KP;  // <= kHashedLdsEntries, by the launcher
        for (uint32_t i = threadIdx.x; i < n_entries; i += kHashedBlock) s_table[i] = table[i];
        __syncthreads();
        tab = s_table;
    }
    const uint64_t M = offs[n_rows];
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t begin, end, hi = 0;
    hashed_run(M, begin, end);
    long long carry[KP];
#pragma unroll
    for (uint32_t k = 0; k < KP; k++) carry[k] = 0;
    uint32_t carry_row = kHashedNoRow;
    for (uint64_t c = begin; c < end; c++) {
        const uint64_t c0 = c * kGramChunk, c_last = tile_last(c0, kGramChunk, M);
        const uint32_t n_in = (uint32_t)(c_last - c0) + 1;
        const uint64_t lo = c == begin ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(offs, lo, n_rows - 1, c_last);
        const HashedLane g = hashed_lane<kText>(data_, offs, ws, hs, c0, c_last, lo, hi, lane);
        long long p[KP];
#pragma unroll
        for (uint32_t k = 0; k < KP; k++) p[k] = 0;
#pragma unroll
        for (uint32_t j = 0; j < kHashedMaxWidths; j++)
            if (j < g.n_valid) hashed_add_weights<KP>(tab, hashed_bucket(g.keys[j], buckets), p);
        const uint32_t row_before = (uint32_t)__shfl_up((int)g.row, 1, 64);
        const uint64_t heads = __ballot(g.in && (lane == 0 || g.row != row_before));
        if (heads == 1ull && !gram_row_inside(offs, lo, c0)) {  // one row, and other chunks have more of it
            if (carry_row != (uint32_t)lo) {
                if (carry_row != kHashedNoRow) hashed_flush_carry<KP>(scores, n_vectors, carry_row, carry, lane);
                carry_row = (uint32_t)lo;
            }
#pragma unroll
            for (uint32_t k = 0; k < KP; k++) carry[k] += p[k];
            continue;
        }
        if (carry_row != kHashedNoRow) {
            hashed_flush_carry<KP>(scores, n_vectors, carry_row, carry, lane);
            carry_row = kHashedNoRow;
        }
        // the segmented scan: a lane adds the lane d before it while that lane is of its own stretch
        const uint64_t at_or_below = heads & ((2ull << lane) - 1);
        const uint32_t start = at_or_below ? 63u - (uint32_t)__builtin_clzll(at_or_below) : 0u;
#pragma unroll 1
        for (uint32_t d = 1; d < kGramChunk; d <<= 1) {
            const bool take = g.in && lane >= start + d;
            if (!__ballot(take)) break;  // no stretch is longer than d
#pragma unroll
            for (uint32_t k = 0; k < KP; k++) {
                const long long v = __shfl_up(p[k], d, 64);
                if (take) p[k] += v;
            }
        }
        const bool last = g.in && (lane + 1 == n_in || ((heads >> 1) >> lane) & 1ull);
        if (last) {
            unsigned long long* out = scores + (uint64_t)g.row * n_vectors;
            const bool inside = gram_row_inside(offs, g.row, c0);
#pragma unroll
            for (uint32_t k = 0; k < KP; k++) {
                if (k >= n_vectors) break;
                if (inside)
                    out[k] = (unsigned long long)p[k];
                else if (gram_adds((uint64_t)p[k]))
                    atomicAdd(&out[k], (unsigned long long)p[k]);
            }
        }
    }
    if (carry_row != kHashedNoRow) hashed_flush_carry<KP>(scores, n_vectors, carry_row, carry, lane);
}

// One add per pending lane to bins (u32 in LDS) or counts (u64 in memory), the lanes of a hot bucket first and as one.
template <class T>
__device__ inline void hashed_count_adds(T* bins, uint32_t b, bool active, uint32_t lane) {
    uint64_t todo = __ballot(active);
#pragma unroll 1
    for (uint32_t r = 0; r < 4 && todo; r++) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t b0 = (uint32_t)__shfl((int)b, (int)leader, 64);
        const uint64_t same = __ballot(active && b == b0) & todo;
        const uint32_t n = (uint32_t)__popcll(same);
        if (lane == leader) atomicAdd(&bins[b0], (T)n);
        todo &= ~same;
        if (n == 1) break;  // nothing hot at the front: the rest adds by itself
    }
    if ((todo >> lane) & 1ull) atomicAdd(&bins[b], (T)1);
}

template <bool kText, bool kLds>
__global__ __launch_bounds__(kHashedBlock) void hashed_counts_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     HashedWidths ws, uint64_t hs, uint64_t buckets, unsigned long long* counts) {
    __shared__ uint32_t s_bins[kLds ? kHashedLdsEntries : 1];
    if constexpr (kLds) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)buckets; i += kHashedBlock) s_bins[i] = 0;
        __syncthreads();
    }
    const uint64_t M = offs[n_rows];
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t begin, end, hi = 0;
    hashed_run(M, begin, end);
    for (uint64_t c = begin; c < end; c++) {
        const uint64_t c0 = c * kGramChunk, c_last = tile_last(c0, kGramChunk, M);
        const uint64_t lo = c == begin ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(offs, lo, n_rows - 1, c_last);
        const HashedLane g = hashed_lane<kText>(data_, offs, ws, hs, c0, c_last, lo, hi, lane);
#pragma unroll
        for (uint32_t j = 0; j < kHashedMaxWidths; j++) {
            if (j >= ws.n) break;  // (the whole wave)
            const uint32_t b = (uint32_t)hashed_bucket(g.keys[j], buckets);  // B <= 2^24
            if constexpr (kLds)
                hashed_count_adds(s_bins, b, j < g.n_valid, lane);
            else
                hashed_count_adds(counts, b, j < g.n_valid, lane);
        }
    }
    if constexpr (kLds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < (uint32_t)buckets; i += kHashedBlock) {
            const uint32_t n = s_bins[i];
            if (n) atomicAdd(&counts[i], (unsigned long long)n);
        }
    }
}

uint32_t hashed_grid(uint64_t n_elems) { return grid_for(n_elems, kHashedBlock, kHashedMaxBlocks); }

template <bool kText, uint32_t KP>
void hashed_scores_launch(bool lds, dim3 grid, hipStream_t stream, const DedupRows& rows, const HashedWidths& ws, uint64_t hs, uint64_t buckets,
                          uint32_t n_vectors, const int32_t* table, unsigned long long* scores) {
    if (lds)
        hipLaunchKernelGGL((hashed_scores_kernel<kText, KP, true>), grid, dim3(kHashedBlock), 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets,
                           n_vectors, table, scores);
    else
        hipLaunchKernelGGL((hashed_scores_kernel<kText, KP, false>), grid, dim3(kHashedBlock), 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets,
                           n_vectors, table, scores);
}

template <bool kText>
void hashed_scores_launch_kp(uint32_t kp, bool lds, dim3 grid, hipStream_t stream, const DedupRows& rows, const HashedWidths& ws, uint64_t hs,
                             uint64_t buckets, uint32_t n_vectors, const int32_t* table, unsigned long long* scores) {
    switch (kp) {
        case 1: return hashed_scores_launch<kText, 1>(lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, scores);
        case 2: return hashed_scores_launch<kText, 2>(lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, scores);
        case 4: return hashed_scores_launch<kText, 4>(lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, scores);
        case 8: return hashed_scores_launch<kText, 8>(lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, scores);
        default: return hashed_scores_launch<kText, 16>(lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, scores);
    }
}

}  // namespace

hipError_t launch_hashed_counts(const DedupRows& rows, const HashedWidths& ws, uint64_t buckets, uint64_t seed, int64_t* counts, bool* used_lds,
                                hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)buckets * 8, stream);
    if (e != hipSuccess) return e;
    const uint32_t n_blocks = hashed_grid(rows.n_elems);
    const bool lds = buckets <= hashed_lds_buckets(1) && hashed_bins_hold(rows.n_elems, n_blocks, ws.n);
    if (used_lds) *used_lds = lds;
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(n_blocks), block(kHashedBlock);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (rows.elem_bytes == 1) {
        if (lds)
            hipLaunchKernelGGL((hashed_counts_kernel<true, true>), grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets, cnt);
        else
            hipLaunchKernelGGL((hashed_counts_kernel<true, false>), grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets, cnt);
    } else {
        if (lds)
            hipLaunchKernelGGL((hashed_counts_kernel<false, true>), grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets, cnt);
        else
            hipLaunchKernelGGL((hashed_counts_kernel<false, false>), grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, ws, hs, buckets, cnt);
    }
    return hipGetLastError();
}

hipError_t launch_hashed_scores(const DedupRows& rows, const HashedWidths& ws, uint64_t buckets, uint32_t n_vectors, uint64_t seed, const int32_t* q,
                                int32_t* table, int64_t* scores, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(scores, 0, (size_t)rows.n_rows * n_vectors * 8, stream);
    if (e != hipSuccess) return e;
    if (rows.n_elems == 0) return hipSuccess;
    const uint32_t kp = hashed_padded(n_vectors);
    hipLaunchKernelGGL(hashed_table_kernel, dim3(grid_for(buckets * kp, 256, 1024)), dim3(256), 0, stream, q, buckets, n_vectors, kp, table);
    const dim3 grid(hashed_grid(rows.n_elems));
    const bool lds = buckets <= hashed_lds_buckets(n_vectors);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    unsigned long long* out = reinterpret_cast<unsigned long long*>(scores);
    if (rows.elem_bytes == 1)
        hashed_scores_launch_kp<true>(kp, lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, out);
    else
        hashed_scores_launch_kp<false>(kp, lds, grid, stream, rows, ws, hs, buckets, n_vectors, table, out);
    return hipGetLastError();
}

}  // namespace tgx
