// Exact row deduplication of a result or of a corpus on the device (include/tgx.h: tgx_corpus_first_equal_device,
// tgx_result_first_equal_device, tgx_*_row_hashes_device; dedup.h has the hash, the tiling and the rules; DESIGN.md,
// section L.10).  A round over a list of unresolved rows: the rows' hashes (a tiled loop over the rows' padded bytes,
// the bandwidth-bound kernel), a stable radix sort of (key, row) (rocPRIM), the compare of every candidate with its
// run's head (again a tiled loop, over the candidates' concatenated elements), and the resolve, which compacts the
// rows that differed from their head into the next round's list.  A row is 0 to 10^8 bytes, so no unit of work is a
// row.  Integer work throughout: the hash of a row is a SUM of terms that depend on a word and its place alone, so any
// number of threads add it up in any order to the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "dedup.h"
#include "scan_helpers.h"

namespace tgx {

namespace {

constexpr uint32_t kDedupBlock = 256;
static_assert(kDedupBlock * kDedupGroup == kDedupTile && kDedupBlock * kDedupCmpByteGroup == kDedupCmpByteTile &&
                  kDedupBlock * kDedupCmpGroup == kDedupCmpTile,
              "the host twin walks the kernels' tiles");
constexpr uint64_t kDedupMaxBlocks = 2048;  // memory-bound: a capped grid that strides over the rest
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

struct DedupPadLen {
    const uint64_t* offs;
    const uint32_t* list;
    uint64_t n_list;
    uint32_t elem_bytes;
    __host__ __device__ uint64_t operator()(uint64_t k) const { return dedup_pad_len(offs, elem_bytes, list, n_list, k); }
};
struct DedupCmpLen {
    const uint64_t* offs;
    const uint32_t *rows, *head_row;
    const uint8_t* flag;
    uint64_t n_list;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return dedup_cmp_len(offs, rows, head_row, flag, n_list, i); }
};
struct DedupListAt {
    const uint32_t* list;
    __host__ __device__ uint32_t operator()(uint64_t k) const { return (uint32_t)dedup_listed(list, k); }
};
struct DedupMarkAt {
    const uint32_t* list;
    const uint8_t* mark;
    __host__ __device__ uint8_t operator()(uint64_t k) const { return mark[dedup_listed(list, k)]; }
};

// The n_words = 1 or 2 little-endian words from text + s on, through the aligned dwords that cover them (2·n_words, and
// one more when s is not a multiple of 4).  Up to 3 bytes in front of text + s and up to 3 behind the last word are
// read, and a word may itself reach up to 7 bytes past its row: a corpus's text has 256 zeroed bytes of slack on either
// side in its allocation (corpus_create), and the aligned over-read rests on that slack.  The caller masks what lies
// past the row.
__device__ inline void dedup_load_text(const uint8_t* text, uint64_t s, uint32_t n_words, uint64_t (&w)[2]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(text + s);
    const uint32_t r = (uint32_t)(a & 3u), sh = 8 * r;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - r);
    uint32_t d[5] = {p[0], p[1], 0, 0, 0};
    if (n_words == 2) {
        d[2] = p[2];
        d[3] = p[3];
        if (r) d[4] = p[4];
    } else if (r) {
        d[2] = p[2];
    }
    uint32_t v[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) v[q] = sh ? (d[q] >> sh) | (d[q + 1] << (32 - sh)) : d[q];
    w[0] = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    w[1] = (uint64_t)v[2] | ((uint64_t)v[3] << 32);
}
// the low n < 8 bytes of w, or all of it
__device__ inline uint64_t dedup_keep_bytes(uint64_t w, uint64_t n) { return n >= 8 ? w : w & ((1ull << (8 * n)) - 1); }

// word j of a row of ids: dword loads inside the row only (an id buffer has no slack to over-read)
__device__ inline uint64_t dedup_load_ids(const uint32_t* ids, uint64_t begin, uint64_t end, uint64_t j) {
    const uint64_t x = begin + 2 * j;
    const uint64_t lo = ids[x], hi = x + 1 < end ? ids[x + 1] : 0u;
    return lo | (hi << 32);
}

// sums[k] = the sum of the terms of listed row k.  A block takes a tile of kDedupTile padded bytes, a thread two words.
// Inside a wave the terms of one row, which sit in consecutive lanes, are added up with shuffles; the wave's sums per row
// go to an LDS word named by where in the tile the row begins (word 0: before the tile).  The thread whose slot holds a
// row's beginning then stores the row's sum plainly when the row ends inside the tile, and adds it to the row's word with
// a 64-bit atomic when the row goes on into the next tile, as thread 0 does for the row that came in from the tile before:
// at most two atomics per tile.  sums is zeroed by the launcher; rows without bytes keep that zero.
template <bool kText>
__global__ __launch_bounds__(kDedupBlock) void dedup_hash_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs,
                                                                 const uint32_t* __restrict__ list, uint64_t n_list,
                                                                 const uint64_t* __restrict__ pad_offs, uint64_t s, unsigned long long* sums) {
    __shared__ uint64_t s_own[2];
    __shared__ unsigned long long s_sum[kDedupTile / 8 + 1];
    const uint64_t n_pad = pad_offs[n_list];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = threadIdx.x; i < kDedupTile / 8 + 1; i += kDedupBlock) s_sum[i] = 0;
    // a block takes consecutive tiles, so that a tile's owners are found from those of the tile before (dedup_find_from)
    const uint64_t n_tiles = (n_pad + kDedupTile - 1) / kDedupTile, per_block = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per_block, tile_end = tile_begin + per_block < n_tiles ? tile_begin + per_block : n_tiles;
    uint64_t lo = 0, hi = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t t0 = tile * kDedupTile;
        if (threadIdx.x < 2) {
            const uint64_t j = threadIdx.x ? tile_last(t0, kDedupTile, n_pad) : t0;
            s_own[threadIdx.x] = tile == tile_begin ? pack_find_row(pad_offs, 0, 0, n_list - 1, j) : dedup_find_from(pad_offs, hi, n_list - 1, j);
        }
        __syncthreads();  // s_own is written, s_sum is zero
        lo = s_own[0];
        hi = s_own[1];
        const uint64_t e0 = t0 + (uint64_t)threadIdx.x * kDedupGroup;
        const bool active = e0 < n_pad;
        DedupSlot sl = {};
        uint32_t key_a = kNoKey, key_b = kNoKey;  // the LDS words of the slot's first row and, when it has two rows, of the second
        unsigned long long val_a = 0, val_b = 0;
        bool begins_a = false;
        if (active) {
            dedup_slot(pad_offs, lo, hi, e0, n_pad - e0 < kDedupGroup ? (uint32_t)(n_pad - e0) : kDedupGroup, sl);
            const bool two_rows = sl.n == 2 && sl.k[1] != sl.k[0];
            uint64_t w[2] = {0, 0};
            const uint64_t r0 = dedup_listed(list, sl.k[0]), r1 = two_rows ? dedup_listed(list, sl.k[1]) : r0;
            if constexpr (kText) {
                const uint8_t* text = static_cast<const uint8_t*>(data_);
                const uint64_t b0 = offs[r0], n0 = offs[r0 + 1] - b0;
                if (two_rows) {
                    uint64_t x[2];
                    dedup_load_text(text, b0 + 8 * sl.j[0], 1, x);
                    w[0] = dedup_keep_bytes(x[0], n0 - 8 * sl.j[0]);
                    const uint64_t b1 = offs[r1], n1 = offs[r1 + 1] - b1;
                    dedup_load_text(text, b1 + 8 * sl.j[1], 1, x);
                    w[1] = dedup_keep_bytes(x[0], n1 - 8 * sl.j[1]);
                } else {
                    dedup_load_text(text, b0 + 8 * sl.j[0], sl.n, w);
                    w[0] = dedup_keep_bytes(w[0], n0 - 8 * sl.j[0]);
                    if (sl.n == 2) w[1] = dedup_keep_bytes(w[1], n0 - 8 * sl.j[1]);
                }
            } else {
                const uint32_t* ids = static_cast<const uint32_t*>(data_);
                w[0] = dedup_load_ids(ids, offs[r0], offs[r0 + 1], sl.j[0]);
                if (sl.n == 2) w[1] = dedup_load_ids(ids, offs[r1], offs[r1 + 1], sl.j[1]);
            }
            const uint64_t p0 = pad_offs[sl.k[0]];
            begins_a = p0 == e0;
            key_a = p0 < t0 ? 0u : (uint32_t)((p0 - t0) / 8) + 1;
            val_a = dedup_term(w[0], sl.j[0], s);
            if (sl.n == 2) {
                const uint64_t t1 = dedup_term(w[1], sl.j[1], s);
                if (two_rows) {
                    key_b = (uint32_t)((e0 + 8 - t0) / 8) + 1;
                    val_b = t1;
                } else {
                    val_a += t1;
                }
            }
        }
        // the sums of the runs of equal key_a over the wave's lanes, into each run's lowest lane (every lane takes part)
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const unsigned long long v = __shfl_down(val_a, off, 64);
            const uint32_t k = __shfl_down(key_a, off, 64);
            if (lane + off < 64 && k == key_a) val_a += v;
        }
        const uint32_t key_before = __shfl_up(key_a, 1, 64);
        if (active && (lane == 0 || key_before != key_a)) atomicAdd(&s_sum[key_a], val_a);
        if (key_b != kNoKey) atomicAdd(&s_sum[key_b], val_b);
        __syncthreads();  // s_sum holds the tile's sums
        // every word that was added to belongs to a row that begins in an active slot, or is word 0: its reader zeroes it
        if (active) {
            if (begins_a) {
                const unsigned long long v = s_sum[key_a];
                s_sum[key_a] = 0;
                if (pad_offs[sl.k[0] + 1] <= t0 + kDedupTile)
                    sums[sl.k[0]] = v;
                else
                    atomicAdd(&sums[sl.k[0]], v);
            }
            if (key_b != kNoKey) {
                const unsigned long long v = s_sum[key_b];
                s_sum[key_b] = 0;
                if (pad_offs[sl.k[1] + 1] <= t0 + kDedupTile)
                    sums[sl.k[1]] = v;
                else
                    atomicAdd(&sums[sl.k[1]], v);
            }
        }
        if (threadIdx.x == 0 && pad_offs[lo] < t0) {
            atomicAdd(&sums[lo], s_sum[0]);
            s_sum[0] = 0;
        }
        // (the next tile's first barrier stands between these reads and its additions, and s_own was read before the second)
    }
}

// out[k] = the key of listed row k from its sum, rows_out[k] = the row: one thread per listed row
__global__ __launch_bounds__(kDedupBlock) void dedup_finish_kernel(const uint64_t* __restrict__ offs, uint32_t elem_bytes,
                                                                   const uint32_t* __restrict__ list, uint64_t n_list, uint64_t s, uint32_t bits,
                                                                   const uint64_t* sums, uint64_t* out, uint32_t* __restrict__ rows_out) {
    for (uint64_t k = (uint64_t)blockIdx.x * kDedupBlock + threadIdx.x; k < n_list; k += (uint64_t)gridDim.x * kDedupBlock) {
        const uint64_t r = dedup_listed(list, k);
        out[k] = dedup_key(dedup_finish(sums[k], (offs[r + 1] - offs[r]) * elem_bytes, s), bits);
        if (rows_out) rows_out[k] = (uint32_t)r;
    }
}

// head_row[i] and flag[i] of sorted position i: one thread per listed row
__global__ __launch_bounds__(kDedupBlock) void dedup_runs_kernel(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ rows, uint64_t n_list, uint32_t* __restrict__ head_row,
                                                                 uint8_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDedupBlock + threadIdx.x; i < n_list; i += (uint64_t)gridDim.x * kDedupBlock) {
        const uint64_t h = dedup_run_head(keys, i);
        const uint32_t r = rows[i], hr = rows[h];
        head_row[i] = hr;
        flag[i] = (h != i && dedup_len_differs(offs, r, hr)) ? 1 : 0;
    }
}

// the aligned dwords that cover the 16 text bytes from text + s on, shifted into place (select.hip: select_load5)
__device__ inline uint4 dedup_load16(const uint8_t* text, uint64_t s) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(text + s);
    const uint32_t r = (uint32_t)(a & 3u), sh = 8 * r;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - r);
    const uint32_t d[5] = {p[0], p[1], p[2], p[3], r ? p[4] : 0u};
    uint32_t v[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) v[q] = sh ? (d[q] >> sh) | (d[q + 1] << (32 - sh)) : d[q];
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// Every candidate against its head: the tiled fill of tile_fill.h over the candidates' concatenated elements.  A slot
// inside one candidate compares 16 bytes at once; a slot that crosses candidates walks.  A slot that finds a difference
// stores 1 into the candidate's flag (every writer stores the same byte).
template <class T>
__global__ __launch_bounds__(kDedupBlock) void dedup_compare_kernel(const void* __restrict__ data_, const uint64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ rows, const uint32_t* __restrict__ head_row,
                                                                    const uint64_t* __restrict__ cmp_offs, uint64_t n_list, uint8_t* flag) {
    constexpr bool kText = sizeof(T) == 1;
    constexpr uint32_t kGroup = kText ? kDedupCmpByteGroup : kDedupCmpGroup;
    constexpr uint32_t kTile = kText ? kDedupCmpByteTile : kDedupCmpTile;
    const uint64_t n_cmp = cmp_offs[n_list];
    const T* __restrict__ data = static_cast<const T*>(data_);
    tiled_fill<kTile, kGroup>(
        n_cmp, n_cmp, [=](uint64_t j) { return pack_find_row(cmp_offs, 0, 0, n_list - 1, j); },
        [=](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            DedupCursor cur;
            dedup_enter(cur, offs, rows, head_row, cmp_offs, lo, hi, e0);
            if (dedup_slot_inside(cur, e0, n_in, kGroup)) {
                const uint64_t t = e0 - cur.start;
                uint4 x, y;
                if constexpr (kText) {
                    x = dedup_load16(data, cur.a + t);
                    y = dedup_load16(data, cur.b + t);
                } else {
                    x = make_uint4(data[cur.a + t], data[cur.a + t + 1], data[cur.a + t + 2], data[cur.a + t + 3]);
                    y = make_uint4(data[cur.b + t], data[cur.b + t + 1], data[cur.b + t + 2], data[cur.b + t + 3]);
                }
                if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) flag[cur.i] = 1;
            } else {
                dedup_compare_walk<T>(cur, data, offs, rows, head_row, cmp_offs, lo, hi, e0, n_in, flag);
            }
        });
}

// first[] of the heads and of the candidates that equal their head; mark[] of every listed row: one thread per row
__global__ __launch_bounds__(kDedupBlock) void dedup_resolve_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ head_row,
                                                                    const uint8_t* __restrict__ flag, uint64_t n_list, int64_t* __restrict__ first,
                                                                    uint8_t* __restrict__ mark, unsigned long long* n_heads) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDedupBlock + threadIdx.x; i < n_list; i += (uint64_t)gridDim.x * kDedupBlock) {
        const uint32_t r = rows[i], hr = head_row[i];
        const uint8_t f = flag[i];
        mark[r] = f;
        if (!f) first[r] = (int64_t)hr;
        if (hr == r) atomicAdd(n_heads, 1ull);
    }
}

inline uint32_t row_grid(uint64_t n) { return grid_for(n, kDedupBlock, kDedupMaxBlocks); }

}  // namespace

hipError_t dedup_temp_bytes(uint64_t n_rows, size_t* scan_bytes, size_t* sort_bytes, size_t* select_bytes) {
    *scan_bytes = *sort_bytes = *select_bytes = 0;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    unsigned long long* count = nullptr;
    hipError_t e = scan_of(DedupPadLen{}, n_rows + 1, k, nullptr, *scan_bytes, nullptr);
    size_t b = 0;
    if (e == hipSuccess) e = scan_of(DedupCmpLen{}, n_rows + 1, k, nullptr, b, nullptr);
    if (b > *scan_bytes) *scan_bytes = b;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, *sort_bytes, k, k, v, v, (size_t)n_rows);
    if (e == hipSuccess) {
        auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), DedupListAt{});
        auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), DedupMarkAt{});
        e = rocprim::select(nullptr, *select_bytes, in, flags, v, count, (size_t)n_rows);
    }
    return e;
}

hipError_t launch_dedup_hash(const DedupRows& rows, const uint32_t* list, uint64_t n_list, uint64_t seed, uint32_t bits, uint64_t* pad_offs,
                             void* scan_tmp, size_t scan_bytes, uint64_t* sums, uint64_t* out, uint32_t* rows_out, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    hipError_t e = scan_of(DedupPadLen{rows.offs, list, n_list, rows.elem_bytes}, n_list + 1, pad_offs, scan_tmp, scan_bytes, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sums, 0, (size_t)n_list * 8, stream)) != hipSuccess) return e;
    const uint64_t s = dedup_seed(seed);
    // (the padded total stays on the device: the grid comes from its bound, N bytes and up to 7 more per listed row)
    const uint64_t pad_bound = rows.n_elems * rows.elem_bytes + 7 * n_list;
    const dim3 grid(grid_for(pad_bound, kDedupTile, kDedupMaxBlocks)), block(kDedupBlock);
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(dedup_hash_kernel<true>, grid, block, 0, stream, rows.data, rows.offs, list, n_list, pad_offs, s,
                           reinterpret_cast<unsigned long long*>(sums));
    else
        hipLaunchKernelGGL(dedup_hash_kernel<false>, grid, block, 0, stream, rows.data, rows.offs, list, n_list, pad_offs, s,
                           reinterpret_cast<unsigned long long*>(sums));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dedup_finish_kernel, dim3(row_grid(n_list)), block, 0, stream, rows.offs, rows.elem_bytes, list, n_list, s, bits, sums, out,
                       rows_out);
    return hipGetLastError();
}

// rocPRIM's radix sort is stable, so equal keys keep their rows ascending: each run begins with its smallest row
hipError_t launch_dedup_sort(const DedupScratch& s, uint64_t n_list, uint32_t bits, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    if (bits == 0) {  // every key is 0: the order stays
        hipError_t e = hipMemcpyAsync(s.keys_b, s.keys_a, (size_t)n_list * 8, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.rows_b, s.rows_a, (size_t)n_list * 4, hipMemcpyDeviceToDevice, stream);
        return e;
    }
    size_t bytes = s.sort_bytes;
    return rocprim::radix_sort_pairs(s.sort_tmp, bytes, s.keys_a, s.keys_b, s.rows_a, s.rows_b, (size_t)n_list, 0, bits, stream);
}

hipError_t launch_dedup_compare(const DedupRows& rows, const DedupScratch& s, uint64_t n_list, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    const dim3 block(kDedupBlock);
    hipLaunchKernelGGL(dedup_runs_kernel, dim3(row_grid(n_list)), block, 0, stream, rows.offs, s.keys_b, s.rows_b, n_list, s.head_row, s.flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.scan_bytes;
    e = scan_of(DedupCmpLen{rows.offs, s.rows_b, s.head_row, s.flag, n_list}, n_list + 1, s.offs_tmp, s.scan_tmp, bytes, stream);
    if (e != hipSuccess) return e;
    // (the compare's total stays on the device: no candidate compares more than the source holds, but their sum may, so
    // the grid is the capped one whenever there is anything)
    if (rows.n_elems == 0) return hipSuccess;
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(dedup_compare_kernel<uint8_t>, dim3((uint32_t)kDedupMaxBlocks), block, 0, stream, rows.data, rows.offs, s.rows_b,
                           s.head_row, s.offs_tmp, n_list, s.flag);
    else
        hipLaunchKernelGGL(dedup_compare_kernel<uint32_t>, dim3((uint32_t)kDedupMaxBlocks), block, 0, stream, rows.data, rows.offs, s.rows_b,
                           s.head_row, s.offs_tmp, n_list, s.flag);
    return hipGetLastError();
}

hipError_t launch_dedup_resolve(const DedupScratch& s, const uint32_t* list, uint64_t n_list, uint32_t* list_out, int64_t* first,
                                hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(dedup_resolve_kernel, dim3(row_grid(n_list)), dim3(kDedupBlock), 0, stream, s.rows_b, s.head_row, s.flag, n_list, first,
                       s.mark, s.words + 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), DedupListAt{list});
    auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), DedupMarkAt{list, s.mark});
    size_t bytes = s.select_bytes;
    return rocprim::select(s.select_tmp, bytes, in, flags, list_out, s.words, (size_t)n_list, stream);
}

}  // namespace tgx
