// A deterministic automaton over the bytes of every row on the device (include/tgx_patterns.h:
// tgx_corpus_dfa_hits_device; dfa.h has the map, its composition, the constant map of a row's first byte, the table and
// the carry operator).  Two kernels walk the bytes of all rows laid end to end with
// textstat.hip's walk (textstat_walk.h), a lane a byte, and no lane ever walks its row: a wave scans the state maps of its
// 64 bytes in six doubling steps.  dfa_summary_kernel writes the map of every chunk as its record, a rocPRIM scan under
// DfaCarryOp turns the records into the map in front of each chunk, and dfa_kernel repeats the in-wave scan, reads every
// byte's state off its map and the chunk's carry, stores the state's tag and cuts the ballot of the tagged lanes into
// the chunk's stretches of one row, by the rule of the row sums of textstat.h.
//
// The table, the 256 maps and the 16 tags, is copied into LDS once by every block in front of its run of tiles: 2 KiB +
// 16 bytes at NS = 16, half the maps at NS = 8.  A lane's map is one LDS read indexed by its byte.  The cross-lane move of
// a step is __shfl_up, ds_bpermute_b32 (two for a 64-bit map), as in words.hip and for the same reason: DPP's row shifts
// stop at a row of 16 lanes.  No LDS beyond the table, no scratch.  The table's copy and the in-wave scan are in
// dfa_wave.h, which cover.hip shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "dfa.h"
#include "dfa_wave.h"
#include "scan_helpers.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

// rec[c] of every chunk c, and the identity behind the last
template <uint32_t NS>
__global__ __launch_bounds__(kTextstatBlock) void dfa_summary_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     uint32_t start, const uint64_t* __restrict__ table, uint64_t n_chunks,
                                                                     DfaMap<NS>* __restrict__ rec) {
    __shared__ DfaLds<NS> lds;
    dfa_load_table<NS>(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const DfaMap<NS> m = dfa_chunk<NS>(lds, t, lane, start);
        if (lane == n_in - 1) {
            const uint64_t k = c0 / kTextstatChunk;
            rec[k] = m;
            if (k + 1 == n_chunks) rec[n_chunks] = dfa_identity<NS>();
        }
    });
}

// ends[p] of every byte and count[i] of every nonempty row i (the launcher pre-set the counts to 0, which empty rows
// keep); either may be NULL.  The tags are one byte per lane, coalesced.  For the counts the ballot of the tagged lanes
// is cut into the chunk's stretches of one row: the lane at which a stretch begins popcounts the stretch's part and, by
// the rule of textstat.h, stores it plainly when the row lies inside the chunk and else adds it.
template <uint32_t NS>
__global__ __launch_bounds__(kTextstatBlock) void dfa_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                             uint32_t start, const uint64_t* __restrict__ table, const DfaMap<NS>* __restrict__ carry,
                                                             unsigned long long* count, uint8_t* __restrict__ ends) {
    __shared__ DfaLds<NS> lds;
    dfa_load_table<NS>(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const DfaMap<NS> m = dfa_chunk<NS>(lds, t, lane, start);
        const uint8_t tag = t.in ? lds.tag[dfa_state<NS>(m, carry[c0 / kTextstatChunk], start)] : (uint8_t)0;
        if (ends && t.in) ends[t.pos] = tag;
        if (!count) return;
        const uint64_t tagged = __ballot(tag != 0);
        const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
        const bool begins = t.in && (lane == 0 || t.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const unsigned long long v = textstat_popc(tagged & textstat_span(lane, end - 1));
            if (textstat_row_inside(offs, t.row, c0))
                count[t.row] = v;
            else if (textstat_adds(v))
                atomicAdd(&count[t.row], v);
        }
    });
}

template <uint32_t NS>
hipError_t dfa_scan_bytes(uint64_t n_recs, size_t* scan_bytes) {
    *scan_bytes = 0;
    DfaMap<NS>* p = nullptr;
    return rocprim::exclusive_scan(nullptr, *scan_bytes, p, p, dfa_identity<NS>(), (size_t)n_recs, DfaCarryOp<NS>());
}

template <uint32_t NS>
hipError_t dfa_summary(const DedupRows& rows, uint32_t start, const uint64_t* table, void* rec, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint64_t n_chunks = (rows.n_elems + kTextstatChunk - 1) / kTextstatChunk;
    hipLaunchKernelGGL(dfa_summary_kernel<NS>, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, start, table, n_chunks,
                       static_cast<DfaMap<NS>*>(rec));
    return hipGetLastError();
}

template <uint32_t NS>
hipError_t dfa_hits(const DedupRows& rows, uint32_t start, const uint64_t* table, const void* carry, int64_t* count, uint8_t* ends, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(dfa_kernel<NS>, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, start, table,
                       static_cast<const DfaMap<NS>*>(carry), reinterpret_cast<unsigned long long*>(count), ends);
    return hipGetLastError();
}

}  // namespace

hipError_t dfa_scan_bytes8(uint64_t n_recs, size_t* scan_bytes) { return dfa_scan_bytes<8>(n_recs, scan_bytes); }
hipError_t dfa_scan_bytes16(uint64_t n_recs, size_t* scan_bytes) { return dfa_scan_bytes<16>(n_recs, scan_bytes); }

hipError_t launch_dfa_summary(const DedupRows& rows, uint32_t width, uint32_t start, const uint64_t* table, void* rec, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    return width == 8 ? dfa_summary<8>(rows, start, table, rec, stream) : dfa_summary<16>(rows, start, table, rec, stream);
}

hipError_t launch_dfa_scan(uint32_t width, const void* rec, void* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (n_recs == 0) return hipSuccess;
    if (width == 8)
        return rocprim::exclusive_scan(scan_tmp, scan_bytes, static_cast<const uint32_t*>(rec), static_cast<uint32_t*>(carry), dfa_identity<8>(), (size_t)n_recs,
                                       DfaCarryOp<8>(), stream);
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, static_cast<const uint64_t*>(rec), static_cast<uint64_t*>(carry), dfa_identity<16>(), (size_t)n_recs,
                                   DfaCarryOp<16>(), stream);
}

hipError_t launch_dfa(const DedupRows& rows, uint32_t width, uint32_t start, const uint64_t* table, const void* carry, int64_t* count, uint8_t* ends,
                      hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (count) {
        const hipError_t e = hipMemsetAsync(count, 0, (size_t)rows.n_rows * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_elems == 0) return hipSuccess;
    return width == 8 ? dfa_hits<8>(rows, start, table, carry, count, ends, stream) : dfa_hits<16>(rows, start, table, carry, count, ends, stream);
}

}  // namespace tgx
