// Fixed-length sequences of byte classes on the device (include/tgx_shapes.h: tgx_corpus_shape_hits_device,
// tgx_corpus_shape_cover_device; shape.h has the word of position bits, the doubling step, the table, the ends and the
// cover's window).  Two kernels walk the bytes of all rows laid end to end with textstat.hip's
// walk (textstat_walk.h), a lane a byte.
//
// shape_ends_kernel is one pass: no summary, no scan over the corpus.  A wave keeps two registers of words, that of its
// own chunk's bytes and that of the chunk in front of it, the halo, each looked up in the B table in LDS, and doubles the
// window six times.  One rotate of the halo register by d serves both uses of a step: the halo's lanes >= d update
// themselves from it, and the own chunk's lanes < d take it where the lanes >= d take __shfl_up.  The halo's lanes below
// d go stale; they are never read again, because a step d reads the halo's lanes >= 64 - d from the own chunk and its
// lanes >= 2d - 1 hold whole windows.  The cross-lane moves are ds_bpermute_b32, two per 64 bits, as in dfa.hip.  The
// before-guard's byte comes from one shuffle per guarded pattern, at the wave-uniform distance len[k], of the guard bits
// of both registers' bytes; the after-guard's from lane + 1, and for lane 63 from one more load.  The ends are one byte
// per lane, coalesced, and the counts follow dfa_kernel's rule.
//
// shape_cover_kernel is kept apart so that it serves ends from any source: a lane reads the ends of its byte and of the
// byte 64 further on, every pattern in use costs a pair of ballots, and a lane is covered by pattern k iff the 128 lanes
// of the two ballots, shifted down by its own, have a bit within their low len[k].  No LDS, no table.
//
// No LDS beyond the table (3 160 bytes at NW = 1, 5 784 at NW = 2), no scratch, no lane that walks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_helpers.h"
#include "shape.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

// the block's copy of the table, word by word
template <uint32_t NW>
__device__ inline void shape_load_table(const uint64_t* __restrict__ table, ShapeTable<NW>& lds) {
    uint64_t* dst = reinterpret_cast<uint64_t*>(&lds);
    for (uint32_t i = threadIdx.x; i < kShapeTableWords<NW>; i += kTextstatBlock) dst[i] = table[i];
    __syncthreads();
}

// One doubling step of both registers.  rot is the halo's word of lane - d, which for an own lane < d is the word of the
// byte d before it: lane 64 + lane - d of the halo.
template <uint32_t NW, uint32_t D>
__device__ inline void shape_double(ShapeWord<NW>& own, ShapeWord<NW>& halo, uint32_t lane, const ShapeWord<NW>& z) {
    ShapeWord<NW> rot, below;
    for (uint32_t i = 0; i < NW; i++) {
        rot.w[i] = __shfl(halo.w[i], (int)((lane - D) & 63u), 64);
        below.w[i] = __shfl_up(own.w[i], D, 64);
    }
    if (lane >= D) halo = shape_step<NW>(halo, rot, D, z);
    own = shape_step<NW>(own, lane >= D ? below : rot, D, z);
}

// The row sums of a chunk's marked lanes, dfa_kernel's rule to the letter: the lane at which a stretch of one row begins
// popcounts the stretch's part of the ballot and stores it plainly when the row lies inside the chunk, else adds it.
__device__ inline void shape_row_sums(const uint64_t* __restrict__ offs, uint64_t c0, uint32_t n_in, const TextLane& t, uint32_t lane, bool marked_lane,
                                      unsigned long long* sums) {
    const uint64_t marked = __ballot(marked_lane);
    const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
    const bool begins = t.in && (lane == 0 || t.row != row_before);
    const uint64_t heads = __ballot(begins);
    if (begins) {
        const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
        const unsigned long long v = textstat_popc(marked & textstat_span(lane, end - 1));
        if (textstat_row_inside(offs, t.row, c0))
            sums[t.row] = v;
        else if (textstat_adds(v))
            atomicAdd(&sums[t.row], v);
    }
}

// ends[p] of every byte and count[i] of every nonempty row i (the launcher pre-set the counts to 0, which empty rows
// keep); either may be NULL.
template <uint32_t NW>
__global__ __launch_bounds__(kTextstatBlock) void shape_ends_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                    const uint64_t* __restrict__ table, unsigned long long* count,
                                                                    uint8_t* __restrict__ ends) {
    __shared__ ShapeTable<NW> lds;
    shape_load_table<NW>(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_patterns = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds.n_patterns);
    const uint32_t nb_used = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds.nb_used);
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        // the halo: the whole chunk in front of this one, which exists when this is not the corpus's first
        const bool has_halo = c0 >= kTextstatChunk;
        const uint8_t hb = has_halo ? text[c0 - kTextstatChunk + lane] : (uint8_t)0;
        ShapeWord<NW> own = t.in ? lds.b[t.b] : shape_zero<NW>();
        ShapeWord<NW> halo = has_halo ? lds.b[hb] : shape_zero<NW>();  // (no byte before the corpus: 0 before the OR)
        shape_double<NW, 1>(own, halo, lane, lds.z[0]);
        shape_double<NW, 2>(own, halo, lane, lds.z[1]);
        shape_double<NW, 4>(own, halo, lane, lds.z[2]);
        shape_double<NW, 8>(own, halo, lane, lds.z[3]);
        shape_double<NW, 16>(own, halo, lane, lds.z[4]);
        shape_double<NW, 32>(own, halo, lane, lds.z[5]);
        const uint64_t in_row = t.pos - t.row_begin;
        uint32_t e = 0;
        if (t.in) e = shape_last_bits<NW>(shape_and<NW>(own, lds.rowok[in_row < kShapeMaxLen - 1 ? in_row : kShapeMaxLen - 1]), lds.last, n_patterns);
        // the before-guards: the guard bits of the byte len[k] before, out of the own chunk or out of the halo
        const uint32_t guards = (t.in ? (uint32_t)lds.nb[t.b] : 0u) | (has_halo ? (uint32_t)lds.nb[hb] << 8 : 0u);
        for (uint32_t used = nb_used; used; used &= used - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(used), len = lds.len[k];
            const uint32_t from = (uint32_t)__shfl((int)guards, (int)((lane - len) & 63u), 64);
            const uint32_t g = lane >= len ? from : from >> 8;
            if (t.in && shape_guarded_before(in_row, len) && ((g >> k) & 1u)) e &= ~(1u << k);
        }
        // the after-guards: one byte serves every pattern
        uint32_t after = (uint32_t)__shfl_down((int)t.b, 1, 64);
        const bool more = t.in && t.pos + 1 < t.row_end;
        if (more && lane == 63) after = text[t.pos + 1];
        if (more) e &= ~(uint32_t)lds.na[after & 0xFFu];
        if (ends && t.in) ends[t.pos] = (uint8_t)e;
        if (count) shape_row_sums(offs, c0, n_in, t, lane, e != 0, count);
    });
}

// lens: byte k is len[k].  mask[p] of every byte and covered[i] of every nonempty row i (pre-set to 0 by the launcher); either may be NULL.
__global__ __launch_bounds__(kTextstatBlock) void shape_cover_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     uint64_t n_bytes, uint32_t n_patterns, uint64_t lens,
                                                                     const uint8_t* __restrict__ ends, unsigned long long* covered,
                                                                     uint8_t* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const uint64_t further = c0 + kTextstatChunk + lane;  // (the next chunk may be short, or not exist)
        const uint32_t e_own = t.in ? ends[t.pos] : 0u, e_next = further < n_bytes ? ends[further] : 0u;
        uint32_t m = 0;
        for (uint32_t k = 0; k < n_patterns; k++) {
            const uint64_t own = __ballot((e_own >> k) & 1u), next = __ballot((e_next >> k) & 1u);
            if ((own | next) && shape_covered(own, next, lane, (uint32_t)(lens >> (8 * k)) & 0xFFu)) m |= 1u << k;
        }
        if (!t.in) m = 0;
        if (mask && t.in) mask[t.pos] = (uint8_t)m;
        if (covered) shape_row_sums(offs, c0, n_in, t, lane, m != 0, covered);
    });
}

template <uint32_t NW>
hipError_t shape_ends(const DedupRows& rows, const uint64_t* table, int64_t* count, uint8_t* ends, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(shape_ends_kernel<NW>, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, table,
                       reinterpret_cast<unsigned long long*>(count), ends);
    return hipGetLastError();
}

// the sums' pre-set, which empty rows keep
hipError_t shape_preset(const DedupRows& rows, int64_t* sums, hipStream_t stream) {
    return sums ? hipMemsetAsync(sums, 0, (size_t)rows.n_rows * 8, stream) : hipSuccess;
}

}  // namespace

hipError_t launch_shape_ends(const DedupRows& rows, uint32_t nw, const uint64_t* table, int64_t* count, uint8_t* ends, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    const hipError_t e = shape_preset(rows, count, stream);
    if (e != hipSuccess || rows.n_elems == 0) return e;
    return nw == 1 ? shape_ends<1>(rows, table, count, ends, stream) : shape_ends<2>(rows, table, count, ends, stream);
}

hipError_t launch_shape_cover(const DedupRows& rows, uint32_t n_patterns, const uint32_t* len, const uint8_t* ends, int64_t* covered, uint8_t* mask,
                              hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    const hipError_t e = shape_preset(rows, covered, stream);
    if (e != hipSuccess || rows.n_elems == 0) return e;
    uint64_t lens = 0;
    for (uint32_t k = 0; k < n_patterns && k < kShapesMaxPatterns; k++) lens |= (uint64_t)len[k] << (8 * k);
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(shape_cover_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, rows.n_elems, n_patterns, lens,
                       ends, reinterpret_cast<unsigned long long*>(covered), mask);
    return hipGetLastError();
}

}  // namespace tgx
