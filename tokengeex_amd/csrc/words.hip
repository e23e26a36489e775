// Word ids on the device (include/tgx_word_ids.h: tgx_corpus_words; words.h has the definitions, the state, the doubling
// step, the record, the carry operator, the emit rule and the rule of the offsets).  Two kernels
// walk the bytes of all rows laid end to end with textstat.hip's walk (textstat_walk.h), a lane a byte, and no lane ever
// walks its word: a wave scans the segmented polynomial states of its 64 bytes in six doubling steps whose multipliers
// M, M^2 .. M^32 are compile-time constants.  words_summary_kernel writes one record per chunk, a rocPRIM scan under
// WordsCarryOp turns the records into each chunk's carry (and the totals, which visit the host to size the ids), and
// words_kernel repeats the in-wave scan and gives every word end its key and its place.  words_offsets_kernel, a lane a
// row, counts the word ends in front of each row's first byte.
//
// The cross-lane move of a step is __shfl_up on the 64-bit h, two ds_bpermute_b32: DPP's row shifts stop at a row of 16
// lanes, so the steps 16 and 32 would need a second mechanism, and bpermute serves all six alike without touching LDS
// memory.  The 64 powers M^(lane + 1) that a word from before the chunk multiplies its carry with are a register pair per
// lane, raised once per thread in front of the walk (seven multiplies), not an LDS table: a block walks many tiles, the
// power depends on the lane alone, and a table would cost a barrier for two registers.  The record's pow, M^(the open
// lanes), is one of the same 64 powers and comes from the lane that holds it by one __shfl a chunk (two bpermutes), which
// only the chunk's last lane uses: raising it there with words_pow would put up to fourteen 64-bit multiplies into every
// chunk of the wave for that one lane, and a table of the powers in memory a load.  Neither was measured against the
// shuffle.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "scan_helpers.h"
#include "textstat_walk.h"
#include "words.h"

namespace tgx {

namespace {

constexpr uint32_t kWordsOffsBlock = 256;

// What both kernels need of a chunk: its masks (wordstat.h's resets, non-space bytes and word ends) and every lane's
// scanned h.
struct WordsChunk {
    uint64_t resets, nonspace, ends;
    uint64_t h;
};
__device__ inline WordsChunk words_chunk(const uint8_t* __restrict__ text, const TextLane& t, uint32_t lane, bool fold) {
    const bool space = textstat_is_space(t.b), nonspace = t.in && !space;
    WordsChunk c;
    c.resets = __ballot(t.in && (space || t.pos == t.row_begin));
    c.nonspace = __ballot(nonspace);
    // word ends: the byte after the chunk's last lane is read only where the row goes on
    bool next_space = true;
    if (lane < 63)
        next_space = !((c.nonspace >> (lane + 1)) & 1ull);
    else if (t.in && t.pos + 1 < t.row_end)
        next_space = textstat_is_space(text[t.pos + 1]);
    c.ends = __ballot(nonspace && (t.pos + 1 == t.row_end || next_space));
    const uint32_t reach = words_reach(c.resets, lane);
    uint64_t h = nonspace ? words_digit(t.b, fold) : 0;
    h = words_step<1>(h, __shfl_up(h, 1, 64), reach);
    h = words_step<2>(h, __shfl_up(h, 2, 64), reach);
    h = words_step<4>(h, __shfl_up(h, 4, 64), reach);
    h = words_step<8>(h, __shfl_up(h, 8, 64), reach);
    h = words_step<16>(h, __shfl_up(h, 16, 64), reach);
    h = words_step<32>(h, __shfl_up(h, 32, 64), reach);
    c.h = h;
    return c;
}

// rec[c] of every chunk c, and the identity behind the last
__global__ __launch_bounds__(kTextstatBlock) void words_summary_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                       uint32_t fold, uint64_t n_chunks, WordsRec* __restrict__ rec) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pow_lane = words_pow(lane + 1);
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const WordsChunk c = words_chunk(text, t, lane, fold != 0);
        const uint64_t pow = __shfl(pow_lane, (int)words_open_lanes(c.resets, n_in) - 1, 64);
        if (lane == n_in - 1) {
            const uint64_t k = c0 / kTextstatChunk;
            rec[k] = words_record(c.resets, c.nonspace, c.ends, c.h, pow);
            if (k + 1 == n_chunks) rec[n_chunks] = words_identity();
        }
    });
}

// ids[place] of every word end.  (place < n_words by the records' own count; the test keeps a store inside the ids
// whatever happens.)
__global__ __launch_bounds__(kTextstatBlock) void words_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows, uint32_t fold,
                                                               uint64_t t_seed, const WordsRec* __restrict__ carry, uint32_t* __restrict__ ids,
                                                               uint64_t n_words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pow_lane = words_pow(lane + 1);
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t, uint64_t, const TextLane& t) {
        const WordsChunk c = words_chunk(text, t, lane, fold != 0);
        if (!((c.ends >> lane) & 1ull)) return;
        const WordsRec cy = carry[c0 / kTextstatChunk];
        const uint64_t place = words_end_place(c.ends, lane, cy);
        if (place < n_words) ids[place] = words_id(words_end_key(c.resets, c.nonspace, lane, c.h, pow_lane, cy, t_seed));
    });
}

// out_offs[k], k = 0 .. S
__global__ __launch_bounds__(kWordsOffsBlock) void words_offsets_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                        uint64_t n_bytes, const WordsRec* __restrict__ carry, uint64_t* __restrict__ out_offs) {
    for (uint64_t k = (uint64_t)blockIdx.x * kWordsOffsBlock + threadIdx.x; k <= n_rows; k += (uint64_t)gridDim.x * kWordsOffsBlock)
        out_offs[k] = words_row_offset(text, offs, k, n_bytes, carry);
}

}  // namespace

hipError_t words_scan_bytes(uint64_t n_recs, size_t* scan_bytes) {
    *scan_bytes = 0;
    WordsRec* p = nullptr;
    return rocprim::exclusive_scan(nullptr, *scan_bytes, p, p, words_identity(), (size_t)n_recs, WordsCarryOp());
}

hipError_t launch_words_summary(const DedupRows& rows, uint32_t flags, WordsRec* rec, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint64_t n_chunks = (rows.n_elems + kTextstatChunk - 1) / kTextstatChunk;
    hipLaunchKernelGGL(words_summary_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows,
                       (flags & kWordsFold) ? 1u : 0u, n_chunks, rec);
    return hipGetLastError();
}

hipError_t launch_words_scan(const WordsRec* rec, WordsRec* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (n_recs == 0) return hipSuccess;
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, rec, carry, words_identity(), (size_t)n_recs, WordsCarryOp(), stream);
}

hipError_t launch_words_emit(const DedupRows& rows, uint32_t flags, uint64_t seed, const WordsRec* carry, uint32_t* ids, uint64_t n_words, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0 || n_words == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(words_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, (flags & kWordsFold) ? 1u : 0u,
                       words_seed(seed), carry, ids, n_words);
    return hipGetLastError();
}

hipError_t launch_words_offsets(const DedupRows& rows, const WordsRec* carry, uint64_t* out_offs, hipStream_t stream) {
    const dim3 grid(grid_for(rows.n_rows + 1, kWordsOffsBlock, kTextstatMaxBlocks)), block(kWordsOffsBlock);
    hipLaunchKernelGGL(words_offsets_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, rows.n_elems, carry, out_offs);
    return hipGetLastError();
}

}  // namespace tgx
