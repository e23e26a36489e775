// Shared n-grams on the device (include/tgx.h: tgx_*_gramset_create, tgx_gramset_create_from_keys,
// tgx_*_gram_hits_device; gram.h has the definitions, the directory, the membership test and the rules; DESIGN.md,
// section L.12).  Two kernels walk the elements of all rows laid end to end, a lane an element (gram_walk.h, shared with
// repeat.hip): gram_keys_kernel writes the key of every valid gram to its slot (then rocPRIM sorts and uniques them and
// gram_dir_kernel writes the bucket directory), and gram_hits_kernel, the hot one, looks every valid gram's key up in a
// set and counts the hits per row.  A lookup is the two adjacent directory entries and then, in a bucket of about one
// key, the key itself: two dependent gathers beside a hash of some 40 cycles.  Neither kernel uses LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "gram.h"
#include "gram_walk.h"
#include "scan_helpers.h"

namespace tgx {

namespace {

constexpr uint32_t kGramBlock = 256;
static_assert(kGramBlock == kGramTile && kGramTile == 4 * kGramChunk && kGramChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kGramMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

struct GramCounts {
    const uint64_t* offs;
    uint64_t n_rows;
    uint32_t width;
    __host__ __device__ uint64_t operator()(uint64_t k) const { return gram_row_count(offs, n_rows, width, k); }
};

// keys_out[g_offs[i] + t] = the key of the gram at element offs[i] + t, for every valid gram
template <bool kText>
__global__ __launch_bounds__(kGramBlock) void gram_keys_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                               uint32_t width, uint64_t hs, const uint64_t* __restrict__ g_offs,
                                                               uint64_t* __restrict__ keys_out) {
    gram_walk<kText>(data_, offs, n_rows, width, hs, [=](uint64_t, uint32_t, const GramLane& g) {
        if (g.valid) keys_out[g_offs[g.row] + (g.pos - offs[g.row])] = g.key;
    });
}

// count[i] = the valid grams of row i whose key is in the set, mask[e] = 1 where the gram at element e is one of them.
// The mask is one byte per lane, coalesced.  For the counts a ballot of the hits is cut into the chunk's stretches of
// one row: the lane at which a stretch begins popcounts the stretch's part of the ballot and, by the rule of gram.h,
// stores it plainly when the row lies inside the chunk and else adds it to the row's count (pre-set to 0 by the launcher).
template <bool kText>
__global__ __launch_bounds__(kGramBlock) void gram_hits_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                               uint32_t width, uint64_t hs, const uint64_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ dir, uint32_t bits, unsigned long long* count,
                                                               uint8_t* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u;
    gram_walk<kText>(data_, offs, n_rows, width, hs, [=](uint64_t c0, uint32_t n_in, const GramLane& g) {
        const bool hit = g.valid && gram_contains(keys, dir, bits, g.key);
        if (mask && g.in) mask[g.pos] = hit ? 1 : 0;
        if (!count) return;
        const uint64_t hits = __ballot(hit);
        const uint32_t row_before = (uint32_t)__shfl_up((int)g.row, 1, 64);
        const bool begins = g.in && (lane == 0 || g.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~((2ull << lane) - 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const uint64_t stretch = ((end >= 64 ? 0ull : (1ull << end)) - 1) & ~((1ull << lane) - 1);  // lanes [lane, end)
            const unsigned long long n_hits = (unsigned long long)__popcll(hits & stretch);
            if (gram_row_inside(offs, g.row, c0))
                count[g.row] = n_hits;
            else if (gram_adds(n_hits))
                atomicAdd(&count[g.row], n_hits);
        }
    });
}

// dir[b] of every b in 0 .. 2^bits: one thread per entry
__global__ __launch_bounds__(kGramBlock) void gram_dir_kernel(const uint64_t* __restrict__ keys, uint64_t n_keys, uint32_t bits, uint32_t* __restrict__ dir) {
    const uint64_t n = (1ull << bits) + 1;
    for (uint64_t b = (uint64_t)blockIdx.x * kGramBlock + threadIdx.x; b < n; b += (uint64_t)gridDim.x * kGramBlock)
        dir[b] = gram_dir_entry(keys, n_keys, bits, b);
}

}  // namespace

hipError_t gram_scan_bytes(uint64_t n_rows, size_t* scan_bytes) {
    *scan_bytes = 0;
    uint64_t* out = nullptr;
    return scan_of(GramCounts{}, n_rows + 1, out, nullptr, *scan_bytes, nullptr);
}

hipError_t gram_sort_bytes(uint64_t n, size_t* sort_bytes, size_t* unique_bytes) {
    *sort_bytes = *unique_bytes = 0;
    uint64_t* k = nullptr;
    unsigned long long* count = nullptr;
    hipError_t e = rocprim::radix_sort_keys(nullptr, *sort_bytes, k, k, (size_t)n);
    if (e == hipSuccess) e = rocprim::unique(nullptr, *unique_bytes, k, k, count, (size_t)n);
    return e;
}

hipError_t launch_gram_offsets(const DedupRows& rows, uint32_t width, uint64_t* g_offs, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    return scan_of(GramCounts{rows.offs, rows.n_rows, width}, rows.n_rows + 1, g_offs, scan_tmp, scan_bytes, stream);
}

hipError_t launch_gram_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kGramMaxBlocks)), block(kGramBlock);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(gram_keys_kernel<true>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out);
    else
        hipLaunchKernelGGL(gram_keys_kernel<false>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, g_offs, keys_out);
    return hipGetLastError();
}

hipError_t launch_gram_sort_unique(const uint64_t* keys_in, uint64_t* sorted, uint64_t* unique_out, unsigned long long* d_count, uint64_t n,
                                   void* sort_tmp, size_t sort_bytes, void* unique_tmp, size_t unique_bytes, hipStream_t stream) {
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream);
    hipError_t e = rocprim::radix_sort_keys(sort_tmp, sort_bytes, keys_in, sorted, (size_t)n, 0, 64, stream);
    if (e != hipSuccess) return e;
    return rocprim::unique(unique_tmp, unique_bytes, sorted, unique_out, d_count, (size_t)n, rocprim::equal_to<uint64_t>(), stream);
}

hipError_t launch_gram_dir(const uint64_t* keys, uint64_t n_keys, uint32_t bits, uint32_t* dir, hipStream_t stream) {
    hipLaunchKernelGGL(gram_dir_kernel, dim3(grid_for((1ull << bits) + 1, kGramBlock, kGramMaxBlocks)), dim3(kGramBlock), 0, stream, keys, n_keys, bits, dir);
    return hipGetLastError();
}

hipError_t launch_gram_hits(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* keys, const uint32_t* dir, uint32_t bits,
                            int64_t* count, uint8_t* mask, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (count) {
        const hipError_t e = hipMemsetAsync(count, 0, (size_t)rows.n_rows * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kGramMaxBlocks)), block(kGramBlock);
    const uint64_t hs = dedup_seed(minhash_hash_seed(seed));
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(gram_hits_kernel<true>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, keys, dir, bits, cnt, mask);
    else
        hipLaunchKernelGGL(gram_hits_kernel<false>, grid, block, 0, stream, rows.data, rows.offs, rows.n_rows, width, hs, keys, dir, bits, cnt, mask);
    return hipGetLastError();
}

}  // namespace tgx
