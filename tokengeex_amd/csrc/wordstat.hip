// Per-row word statistics on the device (include/tgx_words.h: tgx_corpus_word_stats_device; wordstat.h has the
// definitions, the summary with its two carried states, the carry operator and the stop table's match; DESIGN.md, section
// L.15).  Two kernels walk the bytes of all rows laid end to end with textstat.hip's walk (textstat_walk.h), a lane a
// byte: wordstat_summary_kernel writes one word per chunk of 64 bytes, a rocPRIM scan under WordstatCarryOp turns the
// words into each chunk's carry (the word and the line that are open at the chunk's first byte), and wordstat_kernel
// cuts ballots of the word ends, the line ends and what they are into the chunk's stretches of one row, by textstat.h's
// store / add rule.  A word's length and flags are popcounts plus, for a word that began before the chunk, the carry; the
// nine bytes a lane looks back on come by shuffle, and for the chunk's first lanes from memory.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "scan_helpers.h"
#include "textstat_walk.h"
#include "wordstat.h"

namespace tgx {

namespace {

// the chunk's masks (wordstat.h) from its lanes
template <bool kChars>
__device__ inline WordMasks wordstat_masks(const TextLane& t, uint64_t starts) {
    const bool space = textstat_is_space(t.b), nonspace = t.in && !space;
    WordMasks m;
    m.resets = __ballot(t.in && (space || t.pos == t.row_begin));
    m.units = __ballot(nonspace && (!kChars || textstat_is_char(t.b)));
    m.alpha = __ballot(t.in && textstat_is_alpha(t.b));
    m.wide = __ballot(t.in && wordstat_is_wide(t.b));
    m.nonspace = __ballot(nonspace);
    m.starts = starts;
    return m;
}

// summary[c] of every chunk c (wordstat.h)
template <bool kChars>
__global__ __launch_bounds__(kTextstatBlock) void wordstat_summary_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                          uint64_t* __restrict__ summary) {
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t, uint64_t starts, const TextLane& t) {
        const WordMasks m = wordstat_masks<kChars>(t, starts);
        if (lane == 0) summary[c0 / kTextstatChunk] = wordstat_summary(m);
    });
}

// stats[k][i] of every nonempty row i (the launcher pre-set the table to 0, which empty rows keep) and marks[p] of every
// byte; either may be NULL.  A lane builds tail(p) and prev(p) of its byte from the (folded) bytes of the eight lanes
// below it; a lane nearer than that to the chunk's first reads the missing ones from memory, and a byte in front of the
// row's first reads as 0x20 for all.  The sums go as in textstat_kernel: a ballot of each count is cut into the chunk's
// stretches of one row, which the stretch's first lane stores or adds; the longest word is a segmented maximum that its
// last lane stores or folds in; the stop words' mask is the OR over the entries whose ballot meets the stretch.
template <bool kChars>
__global__ __launch_bounds__(kTextstatBlock) void wordstat_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                  uint64_t word_limit, uint32_t fold, const uint64_t* __restrict__ table, uint32_t n_stop,
                                                                  const uint64_t* __restrict__ carry, unsigned long long* stats, uint8_t* __restrict__ marks) {
    const uint32_t lane = threadIdx.x & 63u;
    // lane k keeps entry k of the stop table for the whole run: the loop over the entries reads that lane and loads nothing
    uint64_t lane_entry = 0;
    uint32_t lane_n = 0;
    if (lane < n_stop) {
        lane_entry = table[kWordstatStopWords * lane];
        lane_n = (uint32_t)table[kWordstatStopWords * lane + 1];
    }
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t starts, const TextLane& t) {
        const WordMasks m = wordstat_masks<kChars>(t, starts);
        const uint64_t cy = carry[c0 / kTextstatChunk];
        const bool nonspace = (m.nonspace >> lane) & 1ull;

        // tail(p) and prev(p)
        const uint8_t mine_b = fold ? wordstat_fold(t.b) : t.b;
        const uint64_t dist = t.pos - t.row_begin;  // the bytes of the row in front of this one
        uint64_t tail = mine_b;
        uint8_t prev = 0x20u;
#pragma unroll
        for (uint32_t k = 1; k <= 8; k++) {
            const uint8_t below = (uint8_t)__shfl_up((int)mine_b, k, 64);
            uint8_t v = 0x20u;
            if (t.in && dist >= k) {
                if (lane >= k) {
                    v = below;
                } else {  // (p - k >= row_begin: inside the text)
                    v = text[t.pos - k];
                    if (fold) v = wordstat_fold(v);
                }
            }
            if (k < 8)
                tail |= (uint64_t)v << (8 * k);
            else
                prev = v;
        }

        // word ends: the byte after the chunk's last lane is read only where the row goes on
        bool next_space = true;
        if (lane < 63)
            next_space = !((m.nonspace >> (lane + 1)) & 1ull);
        else if (t.in && t.pos + 1 < t.row_end)
            next_space = textstat_is_space(text[t.pos + 1]);
        const bool is_wend = nonspace && (t.pos + 1 == t.row_end || next_space);
        WordSoFar w = {0, false, false};
        if (is_wend) w = wordstat_word(m, lane, cy);
        const uint32_t nsb = wordstat_nsb(m, lane, cy);
        const bool is_nl = t.in && t.b == '\n';
        const bool is_lend = t.in && (is_nl || t.pos + 1 == t.row_end);
        const bool is_bullet = t.in && wordstat_is_bullet(tail, nsb);

        const uint64_t words = __ballot(is_wend), longs = __ballot(is_wend && w.units > word_limit);
        const uint64_t alpha_words = __ballot(is_wend && w.alpha), alpha_wide_words = __ballot(is_wend && (w.alpha || w.wide));
        const uint64_t hash = __ballot(t.in && t.b == '#'), ellipsis = __ballot(t.in && wordstat_is_ellipsis(tail));
        const uint64_t lines = __ballot(is_lend), bullets = __ballot(is_bullet);
        const uint64_t ellipsis_lines = __ballot(is_lend && wordstat_ellipsis_line(tail, is_nl)), punct_lines = __ballot(is_lend && wordstat_punct_line(tail, is_nl));

        // the chunk's stretches of one row
        const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
        const bool begins = t.in && (lane == 0 || t.row != row_before);
        const uint64_t heads = __ballot(begins);
        uint64_t stretch = 0;  // of the lane at which one begins
        if (begins) {
            const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
            stretch = textstat_span(lane, (above ? (uint32_t)__builtin_ctzll(above) : n_in) - 1);
        }

        // the stop words: matched on word ends only, an entry a step of the whole wave, read from the lane that keeps it
        uint64_t stop_ends = 0, stop_mask = 0;
        for (uint32_t k = 0; k < n_stop; k++) {
            const uint64_t entry = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(lane_entry >> 32), (int)k) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lane_entry, (int)k);
            const uint64_t hits = __ballot(is_wend && wordstat_matches(tail, prev, entry, (uint32_t)__builtin_amdgcn_readlane((int)lane_n, (int)k)));
            stop_ends |= hits;
            if (hits & stretch) stop_mask |= 1ull << k;
        }

        if (marks && t.in)
            marks[t.pos] = (uint8_t)((wordstat_is_word_start(tail) ? kWordMarkStart : 0u) | (is_wend ? kWordMarkEnd : 0u) |
                                     (((stop_ends >> lane) & 1ull) ? kWordMarkStop : 0u) | (is_bullet ? kWordMarkBullet : 0u));
        if (!stats) return;

        const bool inside = t.in && textstat_row_inside(offs, t.row, c0);
        unsigned long long* const mine = stats + t.row;  // statistic k of this lane's row: mine[k * n_rows]

        // the longest word of the stretch: a word is shorter than 2^32 (a row is), so the maximum travels as 32 bits
        const uint32_t head_lane = t.in ? textstat_top(heads & textstat_below(lane + 1)) : lane;
        uint32_t longest = (uint32_t)w.units;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)longest, off, 64);
            if (lane >= off && lane - off >= head_lane && y > longest) longest = y;
        }
        const bool is_tail = t.in && (lane + 1 == n_in || ((heads >> (lane + 1)) & 1ull));
        if (is_tail) {
            if (inside)
                mine[kWsMaxWord * n_rows] = longest;
            else if (textstat_adds(longest))
                atomicMax(&mine[kWsMaxWord * n_rows], (unsigned long long)longest);
        }
        if (begins) {
            const uint64_t ballots[kWordstatN] = {words, m.units, 0, longs, alpha_words, alpha_wide_words, hash, ellipsis, lines, bullets, ellipsis_lines, punct_lines, stop_ends, 0};
#pragma unroll
            for (uint32_t k = 0; k < kWordstatN; k++) {
                if (k == kWsMaxWord || k == kWsStopMask) continue;
                const unsigned long long v = textstat_popc(ballots[k] & stretch);
                if (inside)
                    mine[k * n_rows] = v;
                else if (textstat_adds(v))
                    atomicAdd(&mine[k * n_rows], v);
            }
            if (inside)
                mine[kWsStopMask * n_rows] = stop_mask;
            else if (textstat_adds(stop_mask))
                atomicOr(&mine[kWsStopMask * n_rows], (unsigned long long)stop_mask);
        }
    });
}

}  // namespace

hipError_t wordstat_scan_bytes(uint64_t n_chunks, size_t* scan_bytes) {
    *scan_bytes = 0;
    uint64_t* p = nullptr;
    return rocprim::exclusive_scan(nullptr, *scan_bytes, p, p, (uint64_t)0, (size_t)n_chunks, WordstatCarryOp());
}

hipError_t launch_wordstat_summary(const DedupRows& rows, uint32_t flags, uint64_t* summary, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint8_t* text = static_cast<const uint8_t*>(rows.data);
    if (flags & kWordstatChars)
        hipLaunchKernelGGL(wordstat_summary_kernel<true>, grid, block, 0, stream, text, rows.offs, rows.n_rows, summary);
    else
        hipLaunchKernelGGL(wordstat_summary_kernel<false>, grid, block, 0, stream, text, rows.offs, rows.n_rows, summary);
    return hipGetLastError();
}

hipError_t launch_wordstat_scan(const uint64_t* summary, uint64_t* carry, uint64_t n_chunks, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    return rocprim::exclusive_scan(scan_tmp, scan_bytes, summary, carry, (uint64_t)0, (size_t)n_chunks, WordstatCarryOp(), stream);
}

hipError_t launch_wordstat(const DedupRows& rows, uint64_t word_limit, uint32_t flags, const uint64_t* table, uint32_t n_stop, const uint64_t* carry,
                           int64_t* stats, uint8_t* marks, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    if (stats) {
        const hipError_t e = hipMemsetAsync(stats, 0, (size_t)rows.n_rows * kWordstatN * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    const uint8_t* text = static_cast<const uint8_t*>(rows.data);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    const uint32_t fold = (flags & kWordstatFold) ? 1u : 0u;
    if (flags & kWordstatChars)
        hipLaunchKernelGGL(wordstat_kernel<true>, grid, block, 0, stream, text, rows.offs, rows.n_rows, word_limit, fold, table, n_stop, carry, st, marks);
    else
        hipLaunchKernelGGL(wordstat_kernel<false>, grid, block, 0, stream, text, rows.offs, rows.n_rows, word_limit, fold, table, n_stop, carry, st, marks);
    return hipGetLastError();
}

}  // namespace tgx
