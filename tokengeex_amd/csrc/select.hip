// Rows of a result or of a corpus selected and reordered on the device (include/tgx.h: tgx_result_select,
// tgx_corpus_select; select.h has the index arithmetic), the rows' lengths (tgx_result_lengths_device) and the seeded
// permutation (tgx_shuffled_rows_device).  Two steps, as fim.hip's: the new offsets (a device-wide exclusive scan,
// rocPRIM, over an iterator that computes a length from offs[rows[k]]: no length array is written) and the fill.  The fill
// is the tiled fill of tile_fill.h: a tile of consecutive output
// positions per block, the owners of the tile's ends found by two threads over the new offsets, every thread then walking
// its slot between those two and writing it with one 16-byte store.  A row is 0 to 10^5 elements, so no unit of work is
// a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.h"
#include "scan_helpers.h"
#include "select.h"

namespace tgx {

namespace {

constexpr uint32_t kSelectBlock = 256;
static_assert(kSelectBlock * kSelectGroup == kSelectTile && kSelectBlock * kSelectByteGroup == kSelectByteTile,
              "the host twins walk the kernels' tiles");
constexpr uint64_t kSelectMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest

// output row k -> its length; entry M (which the scan turns into T') is 0 and reads nothing
struct SelectOutLen {
    const uint64_t* offs;
    const int64_t* rows;
    uint64_t n_src, n_rows;
    __host__ __device__ uint64_t operator()(uint64_t k) const {
        if (k >= n_rows) return 0;
        return select_out_len(offs, n_src, rows, k);
    }
};

// the smallest k whose index is out of range: one thread per output row
__global__ __launch_bounds__(kSelectBlock) void select_check_kernel(SelectParams p, unsigned long long* bad) {
    for (uint64_t k = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x; k < p.n_rows; k += (uint64_t)gridDim.x * kSelectBlock)
        if (!select_in_range(p.rows[k], p.n_src)) atomicMin(bad, (unsigned long long)k);
}

// lengths[i] = n_i: one thread per row
__global__ __launch_bounds__(kSelectBlock) void select_lengths_kernel(const uint64_t* __restrict__ offs, uint64_t n_src,
                                                                      int64_t* __restrict__ lengths) {
    for (uint64_t i = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x; i < n_src; i += (uint64_t)gridDim.x * kSelectBlock)
        lengths[i] = (int64_t)(offs[i + 1] - offs[i]);
}

// keys[g] = tgx_shuffle_key(seed, g), vals[g] = g: one thread per row
__global__ __launch_bounds__(kSelectBlock) void shuffle_keys_kernel(uint64_t n, uint64_t seed, uint64_t* __restrict__ keys,
                                                                    int64_t* __restrict__ vals) {
    for (uint64_t g = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x; g < n; g += (uint64_t)gridDim.x * kSelectBlock) {
        keys[g] = shuffle_key(seed, g);
        vals[g] = (int64_t)g;
    }
}

// The five aligned dwords that cover the 16 text bytes from text + s on, and r = how far into the first of them they
// start.  The fifth is not read when r = 0.  Up to 3 bytes in front of the row's first byte and up to 3 behind its last
// are read: a corpus's text has 256 zeroed bytes of slack on either side in its allocation (corpus_create), and the
// aligned over-read rests on that slack.
__device__ inline uint32_t select_load5(const uint8_t* text, uint64_t s, uint32_t (&d)[5]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(text + s);
    const uint32_t r = (uint32_t)(a & 3u);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - r);
    d[0] = p[0];
    d[1] = p[1];
    d[2] = p[2];
    d[3] = p[3];
    d[4] = r ? p[4] : 0u;
    return r;
}

// T = uint32_t: ids, a slot of 4, dword loads at offs[rows[k]] + t.  T = uint8_t: text, a slot of 16 bytes; a slot inside
// one source row reads the aligned dwords that cover it and shifts them into place, a slot that crosses a row boundary
// (or the output's end) loads bytes through the cursor.
template <class T>
__global__ __launch_bounds__(kSelectBlock) void select_fill_kernel(SelectParams p) {
    constexpr bool kText = sizeof(T) == 1;
    constexpr uint32_t kGroup = kText ? kSelectByteGroup : kSelectGroup;
    constexpr uint32_t kTile = kText ? kSelectByteTile : kSelectTile;
    tiled_fill<kTile, kGroup>(
        p.n_out, p.n_out, [p](uint64_t j) { return pack_find_row(p.out_offs, 0, 0, p.n_rows - 1, j); },
        [p](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            const T* __restrict__ data = static_cast<const T*>(p.data);
            T* __restrict__ out = static_cast<T*>(p.out);
            if constexpr (kText) {
                SelectCursor cur;
                select_enter(cur, p.offs, p.rows, p.out_offs, lo, hi, e0);
                if (select_slot_inside(cur, e0, n_in)) {
                    uint32_t d[5], w[4];
                    const uint32_t r = select_load5(data, select_slot_source(cur, e0), d);
                    select_shift16(d, r, w);
                    *reinterpret_cast<uint4*>(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
                    uint8_t v[kSelectByteGroup] = {};
                    select_walk<kSelectByteGroup, uint8_t>(cur, data, p.offs, p.rows, p.out_offs, lo, hi, e0, n_in, v);
                    store_bytes16(out, e0, v, n_in);  // (the tail of the last tile: exactly n_out bytes are written)
                }
            } else {
                uint32_t v[kSelectGroup] = {0, 0, 0, 0};
                select_group<kSelectGroup, uint32_t>(data, p.offs, p.rows, p.out_offs, lo, hi, e0, n_in, v);
                store_ids4(out, e0, v, n_in);
            }
        });
}

template <class T>
hipError_t launch_fill(const SelectParams& p, uint64_t tile, hipStream_t stream) {
    if (p.n_out == 0) return hipSuccess;
    if (p.n_rows == 0 || p.n_src == 0 || (reinterpret_cast<uintptr_t>(p.out) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_fill_kernel<T>, dim3(grid_for(p.n_out, tile, kSelectMaxBlocks)), dim3(kSelectBlock), 0, stream, p);
    return hipGetLastError();
}

// out_offs[0 .. M]: the exclusive prefix sums of the selected rows' lengths, so out_offs[M] = T'.  temp == NULL: the size query
hipError_t offsets_scan(const SelectParams& p, void* temp, size_t& temp_bytes, hipStream_t stream) {
    return scan_of(SelectOutLen{p.offs, p.rows, p.n_src, p.n_rows}, p.n_rows + 1, p.out_offs, temp, temp_bytes, stream);
}

}  // namespace

hipError_t select_scan_temp_bytes(uint64_t n_rows, size_t* bytes) {
    SelectParams p = {};
    p.n_rows = n_rows;
    *bytes = 0;
    return offsets_scan(p, nullptr, *bytes, nullptr);
}

hipError_t launch_select_check(const SelectParams& p, unsigned long long* bad, hipStream_t stream) {
    if (p.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(select_check_kernel, dim3(grid_for(p.n_rows, kSelectBlock, kSelectMaxBlocks)), dim3(kSelectBlock), 0, stream, p, bad);
    return hipGetLastError();
}

hipError_t launch_select_offsets(const SelectParams& p, void* temp, size_t temp_bytes, hipStream_t stream) {
    return offsets_scan(p, temp, temp_bytes, stream);
}

hipError_t launch_select_fill_ids(const SelectParams& p, hipStream_t stream) { return launch_fill<uint32_t>(p, kSelectTile, stream); }
hipError_t launch_select_fill_text(const SelectParams& p, hipStream_t stream) { return launch_fill<uint8_t>(p, kSelectByteTile, stream); }

hipError_t launch_select_lengths(const uint64_t* offs, uint64_t n_src, int64_t* lengths, hipStream_t stream) {
    if (n_src == 0) return hipSuccess;
    hipLaunchKernelGGL(select_lengths_kernel, dim3(grid_for(n_src, kSelectBlock, kSelectMaxBlocks)), dim3(kSelectBlock), 0, stream, offs, n_src,
                       lengths);
    return hipGetLastError();
}

hipError_t shuffle_sort_temp_bytes(uint64_t n, size_t* bytes) {
    uint64_t* k = nullptr;
    int64_t* v = nullptr;
    size_t b = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, (size_t)n);
    *bytes = b;
    return e;
}

// rocPRIM's radix sort is stable, so equal keys keep their indices ascending: the order by (key, index)
hipError_t launch_shuffled_rows(uint64_t n, uint64_t seed, uint64_t* keys_in, uint64_t* keys_out, int64_t* vals_in, int64_t* rows, void* temp,
                                size_t temp_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(shuffle_keys_kernel, dim3(grid_for(n, kSelectBlock, kSelectMaxBlocks)), dim3(kSelectBlock), 0, stream, n, seed, keys_in,
                       vals_in);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, rows, (size_t)n, 0, 64, stream);
}

}  // namespace tgx
