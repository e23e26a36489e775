// Per-row text statistics and line starts on the device (include/tgx.h: tgx_corpus_text_stats_device, tgx_corpus_lines;
// textstat.h has the definitions, the summary, the carry operator and the rule of the row sums).
// Two kernels walk the bytes of all rows laid end to end, a lane a byte (textstat_walk.h: the walk, which the word
// statistics of wordstat.hip share): textstat_summary_kernel writes one word per
// chunk of 64 bytes, a rocPRIM scan under the segmented sum turns the words into each chunk's carry (the units of the
// line that is open at the chunk's first byte), and textstat_kernel, the hot one, cuts ballots of the byte classes, the
// line ends and the long lines into the chunk's stretches of one row.  A line's length is one popcount plus, for a line
// that began before the chunk, the carry: no lane ever walks back.  Neither kernel uses LDS, and a block keeps nothing
// between the tiles of its run but the owner its next search gallops from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_select.hpp>

#include "scan_helpers.h"
#include "textstat.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

// summary[c] of every chunk c (textstat.h)
template <bool kChars>
__global__ __launch_bounds__(kTextstatBlock) void textstat_summary_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                          uint64_t* __restrict__ summary) {
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t, uint64_t starts, const TextLane& t) {
        const uint64_t units = __ballot(t.in && textstat_is_unit(t.b, kChars ? kTextstatChars : 0u));
        if (lane == 0) summary[c0 / kTextstatChunk] = textstat_summary(starts, units);
    });
}

// stats[k][i] of every nonempty row i (the launcher pre-set the table to 0, which empty rows keep) and line_start[p] of
// every byte; either may be NULL.  The mask is one byte per lane, coalesced.  For the sums a ballot of each class is
// cut into the chunk's stretches of one row: the lane at which a stretch begins popcounts the stretch's part of every
// ballot and, by the rule of textstat.h, stores it plainly when the row lies inside the chunk and else adds it.  The
// longest line is a segmented maximum over the stretch's lanes, which its last lane stores or folds in likewise.
template <bool kChars>
__global__ __launch_bounds__(kTextstatBlock) void textstat_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                  uint64_t line_limit, const uint64_t* __restrict__ carry, unsigned long long* stats,
                                                                  uint8_t* __restrict__ line_start) {
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t starts, const TextLane& t) {
        if (line_start && t.in) line_start[t.pos] = (uint8_t)((starts >> lane) & 1ull);
        if (!stats) return;
        const bool is_nl = t.in && t.b == '\n';
        const bool is_end = t.in && (is_nl || t.pos + 1 == t.row_end);
        const uint64_t chars = __ballot(t.in && textstat_is_char(t.b));
        const uint64_t units = kChars ? chars : textstat_below(n_in);
        uint64_t len = 0;
        if (is_end) len = textstat_line_len(starts, units, lane, is_nl, carry[c0 / kTextstatChunk]);
        const uint64_t newlines = __ballot(is_nl), ends = __ballot(is_end), longs = __ballot(is_end && len > line_limit);
        const uint64_t alpha = __ballot(t.in && textstat_is_alpha(t.b)), digit = __ballot(t.in && textstat_is_digit(t.b));
        const uint64_t space = __ballot(t.in && textstat_is_space(t.b)), non_ascii = __ballot(t.in && textstat_is_non_ascii(t.b));
        const uint64_t control = __ballot(t.in && textstat_is_control(t.b));

        const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
        const bool begins = t.in && (lane == 0 || t.row != row_before);
        const uint64_t heads = __ballot(begins);
        const bool inside = t.in && textstat_row_inside(offs, t.row, c0);
        unsigned long long* const mine = stats + t.row;  // statistic k of this lane's row: mine[k * n_rows]
        if (t.in && t.pos == t.row_begin) mine[kTsBytes * n_rows] = t.row_end - t.row_begin;  // (its only writer)

        // the longest line of the stretch: a line is shorter than 2^32 (a row is), so the maximum travels as 32 bits
        const uint32_t head_lane = t.in ? textstat_top(heads & textstat_below(lane + 1)) : lane;
        uint32_t longest = (uint32_t)len;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)longest, off, 64);
            if (lane >= off && lane - off >= head_lane && y > longest) longest = y;
        }
        const bool is_tail = t.in && (lane + 1 == n_in || ((heads >> (lane + 1)) & 1ull));
        if (is_tail) {
            if (inside)
                mine[kTsMaxLine * n_rows] = longest;
            else if (textstat_adds(longest))
                atomicMax(&mine[kTsMaxLine * n_rows], (unsigned long long)longest);
        }
        if (begins) {
            const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const uint64_t stretch = textstat_span(lane, end - 1);
            const uint64_t ballots[kTextstatN] = {0, chars, newlines, ends, 0, longs, alpha, digit, space, non_ascii, control};
#pragma unroll
            for (uint32_t k = 0; k < kTextstatN; k++) {
                if (k == kTsBytes || k == kTsMaxLine) continue;
                const unsigned long long v = textstat_popc(ballots[k] & stretch);
                if (inside)
                    mine[k * n_rows] = v;
                else if (textstat_adds(v))
                    atomicAdd(&mine[k * n_rows], v);
            }
        }
    });
}

struct TextstatMark {
    __host__ __device__ unsigned long long operator()(uint8_t m) const { return m ? 1ull : 0ull; }
};

}  // namespace

hipError_t textstat_scan_bytes(uint64_t n_chunks, size_t* scan_bytes) {
    *scan_bytes = 0;
    uint64_t* p = nullptr;
    return rocprim::exclusive_scan(nullptr, *scan_bytes, p, p, (uint64_t)0, (size_t)n_chunks, TextstatCarryOp());
}

hipError_t textstat_lines_bytes(uint64_t n_bytes, size_t* count_bytes, size_t* select_bytes) {
    *count_bytes = *select_bytes = 0;
    const uint8_t* marks = nullptr;
    uint64_t* out = nullptr;
    unsigned long long* count = nullptr;
    hipError_t e = rocprim::reduce(nullptr, *count_bytes, rocprim::make_transform_iterator(marks, TextstatMark()), count, 0ull, (size_t)n_bytes,
                                   rocprim::plus<unsigned long long>());
    if (e == hipSuccess) e = rocprim::select(nullptr, *select_bytes, rocprim::counting_iterator<uint64_t>(0), marks, out, count, (size_t)n_bytes);
    return e;
}

hipError_t launch_textstat_summary(const DedupRows& rows, uint32_t flags, uint64_t* summary, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint8_t* text = static_cast<const uint8_t*>(rows.data);
    if (flags & kTextstatChars)
        hipLaunchKernelGGL(textstat_summary_kernel<true>, grid, block, 0, stream, text, rows.offs, rows.n_rows, summary);
    else
        hipLaunchKernelGGL(textstat_summary_kernel<false>, grid, block, 0, stream, text, rows.offs, rows.n_rows, summary);
    return hipGetLastError();
}

hipError_t launch_textstat_scan(const uint64_t* summary, uint64_t* carry, uint64_t n_chunks, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, summary, carry, (uint64_t)0, (size_t)n_chunks, TextstatCarryOp(), stream);
}

hipError_t launch_textstat(const DedupRows& rows, uint64_t line_limit, uint32_t flags, const uint64_t* carry, int64_t* stats, uint8_t* line_start,
                           hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (stats) {
        const hipError_t e = hipMemsetAsync(stats, 0, (size_t)rows.n_rows * kTextstatN * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint8_t* text = static_cast<const uint8_t*>(rows.data);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    if (flags & kTextstatChars)
        hipLaunchKernelGGL(textstat_kernel<true>, grid, block, 0, stream, text, rows.offs, rows.n_rows, line_limit, carry, st, line_start);
    else
        hipLaunchKernelGGL(textstat_kernel<false>, grid, block, 0, stream, text, rows.offs, rows.n_rows, line_limit, carry, st, line_start);
    return hipGetLastError();
}

hipError_t launch_textstat_count(const uint8_t* line_start, uint64_t n_bytes, unsigned long long* d_count, void* tmp, size_t tmp_bytes, hipStream_t stream) {
    return rocprim::reduce(tmp, tmp_bytes, rocprim::make_transform_iterator(line_start, TextstatMark()), d_count, 0ull, (size_t)n_bytes,
                           rocprim::plus<unsigned long long>(), stream);
}

hipError_t launch_textstat_compact(const uint8_t* line_start, uint64_t n_bytes, uint64_t* starts, unsigned long long* d_count, void* tmp, size_t tmp_bytes,
                                   hipStream_t stream) {
    return rocprim::select(tmp, tmp_bytes, rocprim::counting_iterator<uint64_t>(0), line_start, starts, d_count, (size_t)n_bytes, stream);
}

}  // namespace tgx
