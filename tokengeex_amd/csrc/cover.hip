// The bytes inside a match on the device (include/tgx_redact.h: tgx_corpus_dfa_cover_device; cover.h has the mirrored
// records, the state a byte reads off the backward side and the table; dfa.h the maps).  Two
// kernels walk the bytes of all rows laid end to end with textstat_walk.h's walk, a lane a byte, and scan state maps
// inside the wave in both directions: dfa_wave.h's forward scan for the automaton that runs left to right, and its
// mirror, __shfl_down and composition in front, for the one that runs right to left.  cover_summary_kernel reads the
// text once and writes both records of every chunk, the backward one at the mirrored index, so that dfa.hip's
// exclusive scan under DfaCarryOp serves both sides unchanged.  cover_kernel repeats both scans, reads f off the forward
// map and its chunk's carry and g off the map of the lane to its right and the mirrored carry, stores cover[f][g] and
// cuts the ballot of the covered lanes into the chunk's stretches of one row, as dfa_kernel does its tagged lanes.
//
// Each side takes the map width its automaton needs, so the kernels come in four builds, {8, 16} x {8, 16}.  LDS holds the
// forward table, the backward maps and the 256 bytes of the pair table: 4 KiB + 272 bytes at 16 x 16.  No LDS beyond the
// tables, no scratch, no lane that walks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cover.h"
#include "dfa_wave.h"
#include "scan_helpers.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

template <uint32_t NSF, uint32_t NSB>
struct CoverLds {
    DfaLds<NSF> fwd;
    DfaMap<NSB> back[256];
    uint8_t pair[kDfaMaxStates * kDfaMaxStates];
};
// thread t takes map t of either side and byte t of the pair table
template <uint32_t NSF, uint32_t NSB>
__device__ inline void cover_load_table(const uint64_t* __restrict__ table, CoverLds<NSF, NSB>& lds) {
    static_assert(kTextstatBlock == 256 && kDfaMaxStates * kDfaMaxStates == 256, "a thread a map and a pair");
    lds.back[threadIdx.x] = reinterpret_cast<const DfaMap<NSB>*>(table + kDfaTableWords<NSF>)[threadIdx.x];
    lds.pair[threadIdx.x] = reinterpret_cast<const uint8_t*>(table + kDfaTableWords<NSF> + kDfaTableWords<NSB>)[threadIdx.x];
    dfa_load_table<NSF>(table, lds.fwd);  // (ends in the block's barrier)
}

// rec_f[k] and rec_b[n_chunks - 1 - k] of every chunk k, and the identity behind the last of each
template <uint32_t NSF, uint32_t NSB>
__global__ __launch_bounds__(kTextstatBlock) void cover_summary_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                       uint32_t f_start, uint32_t b_start, const uint64_t* __restrict__ table,
                                                                       uint64_t n_chunks, DfaMap<NSF>* __restrict__ rec_f, DfaMap<NSB>* __restrict__ rec_b) {
    __shared__ CoverLds<NSF, NSB> lds;
    cover_load_table<NSF, NSB>(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const DfaMap<NSF> mf = dfa_chunk<NSF>(lds.fwd, t, lane, f_start);
        const DfaMap<NSB> mb = dfa_chunk_back<NSB>(lds.back, t, lane, b_start);
        const uint64_t k = c0 / kTextstatChunk;
        if (lane == n_in - 1) {
            rec_f[k] = mf;
            if (k + 1 == n_chunks) rec_f[n_chunks] = dfa_identity<NSF>();
        }
        if (lane == 0) {
            rec_b[cover_mirror(k, n_chunks)] = mb;
            if (k == 0) rec_b[n_chunks] = dfa_identity<NSB>();
        }
    });
}

// mask[p] of every byte and covered[i] of every nonempty row i (the launcher pre-set the counts to 0, which empty rows
// keep); either may be NULL.  The bytes are one store per lane, coalesced; the counts follow dfa_kernel's rule.
template <uint32_t NSF, uint32_t NSB>
__global__ __launch_bounds__(kTextstatBlock) void cover_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                               uint32_t f_start, uint32_t b_start, const uint64_t* __restrict__ table, uint64_t n_chunks,
                                                               const DfaMap<NSF>* __restrict__ carry_f, const DfaMap<NSB>* __restrict__ carry_b,
                                                               unsigned long long* covered, uint8_t* __restrict__ mask) {
    __shared__ CoverLds<NSF, NSB> lds;
    cover_load_table<NSF, NSB>(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const DfaMap<NSF> mf = dfa_chunk<NSF>(lds.fwd, t, lane, f_start);
        const DfaMap<NSB> mb = dfa_chunk_back<NSB>(lds.back, t, lane, b_start);
        const DfaMap<NSB> right = __shfl_down(mb, 1, 64);
        const uint64_t k = c0 / kTextstatChunk;
        uint8_t m = 0;
        if (t.in) {
            const uint32_t f = dfa_state<NSF>(mf, carry_f[k], f_start);
            const uint32_t g = cover_back_state<NSB>(right, lane == n_in - 1, t.pos + 1 == t.row_end, carry_b[cover_mirror(k, n_chunks)], b_start);
            m = lds.pair[kDfaMaxStates * f + g];
        }
        if (mask && t.in) mask[t.pos] = m;
        if (!covered) return;
        const uint64_t marked = __ballot(m != 0);
        const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
        const bool begins = t.in && (lane == 0 || t.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const unsigned long long v = textstat_popc(marked & textstat_span(lane, end - 1));
            if (textstat_row_inside(offs, t.row, c0))
                covered[t.row] = v;
            else if (textstat_adds(v))
                atomicAdd(&covered[t.row], v);
        }
    });
}

template <uint32_t NSF, uint32_t NSB>
hipError_t cover_summary(const DedupRows& rows, uint32_t f_start, uint32_t b_start, const uint64_t* table, void* rec_f, void* rec_b, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint64_t n_chunks = (rows.n_elems + kTextstatChunk - 1) / kTextstatChunk;
    hipLaunchKernelGGL((cover_summary_kernel<NSF, NSB>), grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, f_start,
                       b_start, table, n_chunks, static_cast<DfaMap<NSF>*>(rec_f), static_cast<DfaMap<NSB>*>(rec_b));
    return hipGetLastError();
}

template <uint32_t NSF, uint32_t NSB>
hipError_t cover_marks(const DedupRows& rows, uint32_t f_start, uint32_t b_start, const uint64_t* table, const void* carry_f, const void* carry_b,
                       int64_t* covered, uint8_t* mask, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint64_t n_chunks = (rows.n_elems + kTextstatChunk - 1) / kTextstatChunk;
    hipLaunchKernelGGL((cover_kernel<NSF, NSB>), grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, f_start, b_start,
                       table, n_chunks, static_cast<const DfaMap<NSF>*>(carry_f), static_cast<const DfaMap<NSB>*>(carry_b),
                       reinterpret_cast<unsigned long long*>(covered), mask);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cover_summary(const DedupRows& rows, uint32_t wf, uint32_t wb, uint32_t f_start, uint32_t b_start, const uint64_t* table, void* rec_f,
                                void* rec_b, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    if (wf == 8) return wb == 8 ? cover_summary<8, 8>(rows, f_start, b_start, table, rec_f, rec_b, stream) : cover_summary<8, 16>(rows, f_start, b_start, table, rec_f, rec_b, stream);
    return wb == 8 ? cover_summary<16, 8>(rows, f_start, b_start, table, rec_f, rec_b, stream) : cover_summary<16, 16>(rows, f_start, b_start, table, rec_f, rec_b, stream);
}

hipError_t launch_cover(const DedupRows& rows, uint32_t wf, uint32_t wb, uint32_t f_start, uint32_t b_start, const uint64_t* table, const void* carry_f,
                        const void* carry_b, int64_t* covered, uint8_t* mask, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (covered) {
        const hipError_t e = hipMemsetAsync(covered, 0, (size_t)rows.n_rows * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_elems == 0) return hipSuccess;
    if (wf == 8)
        return wb == 8 ? cover_marks<8, 8>(rows, f_start, b_start, table, carry_f, carry_b, covered, mask, stream)
                       : cover_marks<8, 16>(rows, f_start, b_start, table, carry_f, carry_b, covered, mask, stream);
    return wb == 8 ? cover_marks<16, 8>(rows, f_start, b_start, table, carry_f, carry_b, covered, mask, stream)
                   : cover_marks<16, 16>(rows, f_start, b_start, table, carry_f, carry_b, covered, mask, stream);
}

}  // namespace tgx
