// Duplicate spans across rows on the device (include/tgx_dupspans.h: tgx_*_dup_spans_device; dupspan.h has the
// definitions and the rules).  Four stages: dupspan_keys_kernel walks the elements of all rows
// laid end to end (gram_walk.h) and writes every valid gram's key and position to its slot; rocPRIM sorts the pairs
// stably by the key's low key_bits bits; dupspan_match_kernel, a lane a sorted slot, VERIFIES each slot against the
// earlier slots of its run of equal masked keys by comparing the elements, and flags the duplicates; dupspan_cover_kernel
// walks the elements again and turns the flags into the rows' sums and the covered elements with ballots.  No LDS,
// plain C++ and vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "dupspan.h"
#include "gram_walk.h"

namespace tgx {

namespace {

constexpr uint32_t kDupspanBlock = 256;
static_assert(kDupspanBlock == kGramTile && kGramTile == 4 * kGramChunk && kGramChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kDupspanMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

// keys_out / pos_out[g_offs[i] + t] = the key / the element of the gram at element offs[i] + t, for every valid gram
template <bool kText>
__global__ __launch_bounds__(kDupspanBlock) void dupspan_keys_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     uint32_t width, uint64_t hs, const uint64_t* __restrict__ g_offs,
                                                                     uint64_t* __restrict__ keys_out, uint32_t* __restrict__ pos_out) {
    gram_walk<kText>(data_, offs, n_rows, width, hs, [=](uint64_t, uint32_t, const GramLane& g) {
        if (!g.valid) return;
        const uint64_t slot = g_offs[g.row] + (g.pos - offs[g.row]);
        keys_out[slot] = g.key;
        pos_out[slot] = (uint32_t)g.pos;
    });
}

// the table's pre-set: a thread a row
__global__ __launch_bounds__(kDupspanBlock) void dupspan_preset_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t width,
                                                                       int64_t* __restrict__ table) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDupspanBlock + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * kDupspanBlock) {
        table[kDsGrams * n_rows + i] = (int64_t)gram_row_count(offs, n_rows, width, i);
        table[kDsDup * n_rows + i] = 0;
        table[kDsCovered * n_rows + i] = 0;
    }
}

// the words of the gram at element e, as gram_walk loads them: what lies past the gram's bytes is 0
template <bool kText>
__device__ inline void dupspan_load(const void* data_, uint64_t e, uint32_t width, uint64_t (&w)[8]) {
    if constexpr (kText)
        minhash_load_text(static_cast<const uint8_t*>(data_), e, width, w);
    else
        minhash_load_ids(static_cast<const uint32_t*>(data_), e, width, w);
}

// The match.  A lane takes sorted slot t, 64 consecutive slots to a wave, and its predecessor's key and position from
// the lane below (lane 0: from memory).  The head of a run is done at once and loads no data.  A candidate loads its
// own gram's words once and hands dupspan_walk_back a comparison of them with the gram at another position, loaded the
// same way: the loaders mask off what lies past the gram, so equal words are equal elements.  A duplicate stores bit 0
// at flag[pos[t]] (each position is in one slot; the launcher pre-set the array to 0).  Every position is that of a
// VALID gram, so the loads are gram_walk's: text may over-read into the corpus's zeroed slack, ids stay inside the gram.
template <bool kText>
__global__ __launch_bounds__(kDupspanBlock) void dupspan_match_kernel(const void* __restrict__ data_, uint32_t width, const uint64_t* __restrict__ keys,
                                                                      const uint32_t* __restrict__ pos, uint64_t n, uint64_t key_mask,
                                                                      uint8_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_bytes = width * (kText ? 1u : 4u);
    const uint64_t stride = (uint64_t)gridDim.x * kDupspanBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kDupspanBlock; base < n; base += stride) {  // (the bound is the block's: the wave stays whole)
        const uint64_t t = base + threadIdx.x;
        const bool live = t < n;
        const unsigned long long k = live ? keys[t] : 0ull;
        const uint32_t p = live ? pos[t] : 0u;
        unsigned long long prev_key = __shfl_up(k, 1, 64);
        uint32_t prev_pos = (uint32_t)__shfl_up((int)p, 1, 64);
        if (lane == 0 && live && t > 0) {
            prev_key = keys[t - 1];
            prev_pos = pos[t - 1];
        }
        if (live && dupspan_candidate(t, k, prev_key, key_mask)) {
            uint64_t mine[8];
            dupspan_load<kText>(data_, p, width, mine);
            const bool dup = dupspan_walk_back(keys, pos, t, k, key_mask, prev_pos, [&](uint32_t q) {
                uint64_t other[8];
                dupspan_load<kText>(data_, q, width, other);
                bool equal = true;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    if (8 * j < n_bytes) equal = equal && mine[j] == other[j];
                return equal;
            });
            if (dup) flag[p] = kDupspanBitDup;
        }
    }
}

// dup and covered of every row, and the mask's second bit.  repeat_cover_kernel's shape over the one bit: a lane loads
// its element's flag and the flag 64 elements before it; ballots of bit 0 give a window of 128 elements, from which
// repeat_covered takes the lane's part.  The two ballots are cut into the chunk's stretches of one row: the lane at
// which a stretch begins popcounts them and, by the rule of gram.h, stores plainly when the row lies inside the chunk
// and else adds to the row's sums (pre-set to 0).  With finish_mask a covered lane stores its own flag byte back with
// bit 1 set; the wave of the next chunk, perhaps of another block, may read that byte at the same time with a plain
// load, and it looks at bit 0 alone, which no store of this kernel changes.  That is an unsynchronised read and write of
// one location: it is right because a byte has one writer, its own lane, and because the hardware's byte stores are
// byte-granular and touch no neighbour.  repeat_cover_kernel, which only reads its flags, has no such dependence.
// table may be NULL.
__global__ __launch_bounds__(kDupspanBlock) void dupspan_cover_kernel(const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t width, uint8_t* flag,
                                                                      bool finish_mask, unsigned long long* table) {
    const uint32_t lane = threadIdx.x & 63u;
    gram_walk<true, false>(nullptr, offs, n_rows, width, 0, [=](uint64_t c0, uint32_t n_in, const GramLane& g) {
        const uint32_t f = g.in ? flag[g.pos] : 0u;
        const uint32_t fb = c0 ? flag[c0 - kGramChunk + lane] : 0u;  // (the chunk before is whole)
        const uint64_t dup = __ballot(f & kDupspanBitDup), dup_b = __ballot(fb & kDupspanBitDup);
        const uint64_t rs = g.in ? offs[g.row] : 0;
        const bool covered = g.in && repeat_covered(dup_b, dup, lane, g.pos, rs, width);
        const uint64_t cov = __ballot(covered);
        if (finish_mask && covered) flag[g.pos] = (uint8_t)(f | kDupspanBitCovered);
        if (!table) return;  // (the same for the whole grid)
        const uint32_t row_before = (uint32_t)__shfl_up((int)g.row, 1, 64);
        const bool begins = g.in && (lane == 0 || g.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~((2ull << lane) - 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const uint64_t stretch = ((end >= 64 ? 0ull : (1ull << end)) - 1) & ~((1ull << lane) - 1);  // lanes [lane, end)
            const bool inside = gram_row_inside(offs, g.row, c0);
            const uint64_t ballots[2] = {dup, cov};
            const uint32_t which[2] = {kDsDup, kDsCovered};
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                const unsigned long long v = (unsigned long long)__popcll(ballots[q] & stretch);
                unsigned long long* dst = &table[which[q] * n_rows + g.row];
                if (inside)
                    *dst = v;
                else if (gram_adds(v))
                    atomicAdd(dst, v);
            }
        }
    });
}

}  // namespace

hipError_t dupspan_sort_bytes(uint64_t n, uint32_t key_bits, size_t* sort_bytes) {
    *sort_bytes = 0;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *sort_bytes, k, k, v, v, (size_t)n, 0, key_bits);
}

hipError_t launch_dupspan_preset(const DedupRows& rows, uint32_t width, int64_t* table, uint8_t* flag, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (rows.n_elems) {
        const hipError_t e = hipMemsetAsync(flag, 0, (size_t)rows.n_elems, stream);
        if (e != hipSuccess) return e;
    }
    if (!table) return hipSuccess;
    hipLaunchKernelGGL(dupspan_preset_kernel, dim3(grid_for(rows.n_rows, kDupspanBlock, kDupspanMaxBlocks)), dim3(kDupspanBlock), 0, stream, rows.offs,
                       rows.n_rows, width, table);
    return hipGetLastError();
}

hipError_t launch_dupspan_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, uint32_t* pos_out,
                               hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kDupspanMaxBlocks)), block(kDupspanBlock);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(dupspan_keys_kernel<true>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out, pos_out);
    else
        hipLaunchKernelGGL(dupspan_keys_kernel<false>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out, pos_out);
    return hipGetLastError();
}

hipError_t launch_dupspan_sort(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* pos_in, uint32_t* pos_out, uint64_t n, uint32_t key_bits,
                               void* sort_tmp, size_t sort_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys_in, keys_out, pos_in, pos_out, (size_t)n, 0, key_bits, stream);
}

hipError_t launch_dupspan_match(const DedupRows& rows, uint32_t width, const uint64_t* keys, const uint32_t* pos, uint64_t n, uint32_t key_bits,
                                uint8_t* flag, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(grid_for(n, kDupspanBlock, kDupspanMaxBlocks)), block(kDupspanBlock);
    const uint64_t key_mask = dupspan_key_mask(key_bits);
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(dupspan_match_kernel<true>, grid, block, 0, stream, rows.data, width, keys, pos, n, key_mask, flag);
    else
        hipLaunchKernelGGL(dupspan_match_kernel<false>, grid, block, 0, stream, rows.data, width, keys, pos, n, key_mask, flag);
    return hipGetLastError();
}

hipError_t launch_dupspan_cover(const DedupRows& rows, uint32_t width, uint8_t* flag, bool finish_mask, int64_t* table, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0 || (!table && !finish_mask)) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kDupspanMaxBlocks)), block(kDupspanBlock);
    hipLaunchKernelGGL(dupspan_cover_kernel, grid, block, 0, stream, rows.offs, rows.n_rows, width, flag, finish_mask,
                       reinterpret_cast<unsigned long long*>(table));
    return hipGetLastError();
}

}  // namespace tgx
