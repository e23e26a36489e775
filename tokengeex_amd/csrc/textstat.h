// Per-row text statistics and the line view of a resident corpus (include/tgx.h: tgx_corpus_text_stats_device,
// tgx_corpus_lines): what a line, its length and a byte's classes are, the tiling of the bytes, the summary of a chunk and
// the operator that turns the summaries into each chunk's carry, and the rule by which a row's sums reach its
// statistics.  The kernels of textstat.hip and the host twins in host_twins.cpp (tgx_text_stats_host, tgx_lines_host)
// both go through these functions; DESIGN.md, section L.13.
//
// Row i is the bytes text[offs[i] .. offs[i+1]).  Only '\n' ends a line ('\r' is an ordinary byte: a caller who wants
// CRLF folded runs the CRLF front end, tgx_corpus_split_specials with TGX_FRONT_CRLF, first).  Position p of row i is a
// LINE END iff text[p] == '\n' or p == offs[i+1] - 1, and a LINE START iff p == offs[i] or text[p - 1] == '\n' with
// p - 1 >= offs[i].  So no line continues from one row into the next, a trailing '\n' opens no empty last line, "\n" is
// one empty line and an empty row has no line.  The line that ends at p begins at the last line start at or before p;
// its length is the units of [start, p], less the '\n' itself.  A unit is a byte, or under TGX_TEXTSTAT_CHARS a
// character: a byte that is no UTF-8 continuation byte (span_is_cont of spans.h negated), so everything is defined by
// bytes alone, on invalid UTF-8 too.
//
// The bytes of all rows are laid end to end: a lane takes a byte, a wave a chunk of 64, a block of four waves a tile of
// 256, and a block a run of consecutive tiles.  offs itself is the array of starts, so the owner search steps over
// empty rows and they are never visited; their statistics keep the launcher's 0.
//
// The carry.  A line end whose line start lies in its own chunk gets its length from one popcount.  Any other needs the
// units between the line's start and the chunk's first byte, however many chunks back that start is.  A first pass
// writes one word per chunk, its SUMMARY: whether the chunk holds a line start, and the units from its last line start
// on (all its units without one).  An exclusive scan of the summaries under textstat_carry_op, the segmented sum, gives
// every chunk its CARRY: the units from the last line start before the chunk up to the chunk.  That is linear in the
// bytes whatever the lines' lengths are: nothing ever walks back over a line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dedup.h"
#include "spans.h"

namespace tgx {

constexpr uint32_t kTextstatChunk = 64;   // bytes of a wave's step
constexpr uint32_t kTextstatTile = 256;   // bytes of a block's step: four chunks
constexpr uint32_t kTextstatN = 11;       // TGX_TEXTSTAT_N
constexpr int kTextstatStages = 4;
constexpr uint64_t kTextstatMaxLines = 0xFFFFFFFEull;  // 2^32 - 1 lines are refused, as 2^32 - 1 rows are
constexpr uint32_t kTextstatChars = 1u;   // TGX_TEXTSTAT_CHARS

// the statistics' places in the table (include/tgx.h)
enum : uint32_t {
    kTsBytes = 0, kTsChars = 1, kTsNewlines = 2, kTsLines = 3, kTsMaxLine = 4, kTsLongLines = 5,
    kTsAlpha = 6, kTsDigit = 7, kTsSpace = 8, kTsNonAscii = 9, kTsControl = 10,
};

// ---- a byte's classes ---------------------------------------------------------------------------------------------
__host__ __device__ inline bool textstat_is_char(uint8_t b) { return !span_is_cont(b); }
__host__ __device__ inline bool textstat_is_alpha(uint8_t b) { return (uint8_t)((b | 0x20u) - 'a') < 26u; }
__host__ __device__ inline bool textstat_is_digit(uint8_t b) { return (uint8_t)(b - '0') < 10u; }
__host__ __device__ inline bool textstat_is_space(uint8_t b) { return b == 0x20u || (uint8_t)(b - 9u) < 5u; }
__host__ __device__ inline bool textstat_is_non_ascii(uint8_t b) { return b >= 0xC0u; }
__host__ __device__ inline bool textstat_is_control(uint8_t b) { return (b < 0x20u && !textstat_is_space(b)) || b == 0x7Fu; }
__host__ __device__ inline bool textstat_is_unit(uint8_t b, uint32_t flags) { return !(flags & kTextstatChars) || textstat_is_char(b); }

// ---- masks over a chunk's 64 lanes --------------------------------------------------------------------------------
// lanes [0, n), n <= 64
__host__ __device__ inline uint64_t textstat_below(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }
// lanes [a, b], a <= b < 64
__host__ __device__ inline uint64_t textstat_span(uint32_t a, uint32_t b) { return textstat_below(b + 1) & ~textstat_below(a); }
__host__ __device__ inline uint32_t textstat_popc(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(m);
#else
    return (uint32_t)__builtin_popcountll(m);
#endif
}
// the highest set lane of m != 0
__host__ __device__ inline uint32_t textstat_top(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 63u - (uint32_t)__clzll((long long)m);
#else
    return 63u - (uint32_t)__builtin_clzll(m);
#endif
}

// ---- the summary and the carry ------------------------------------------------------------------------------------
constexpr uint64_t kTextstatReset = 1ull << 63;  // the chunk holds a line start; the low 63 bits are units
// starts, units: the chunk's line starts and units as lane masks
__host__ __device__ inline uint64_t textstat_summary(uint64_t starts, uint64_t units) {
    if (!starts) return textstat_popc(units);
    return kTextstatReset | textstat_popc(units & ~textstat_below(textstat_top(starts)));
}
// the segmented sum: b after a.  Associative, not commutative; 0 is its identity.  (A line is shorter than 2^32.)
struct TextstatCarryOp {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return (b & kTextstatReset) ? b : a + b; }
};
__host__ __device__ inline uint64_t textstat_carry_units(uint64_t carry) { return carry & ~kTextstatReset; }

// The length of the line that ends at `lane`: starts and units as above, is_nl: the end is a '\n' (which is a unit in
// either unit and does not count), carry: the chunk's carry, used only by a line that began before the chunk.
__host__ __device__ inline uint64_t textstat_line_len(uint64_t starts, uint64_t units, uint32_t lane, bool is_nl, uint64_t carry) {
    const uint64_t upto = textstat_below(lane + 1), s = starts & upto;
    const uint64_t len = s ? textstat_popc(units & upto & ~textstat_below(textstat_top(s))) : textstat_carry_units(carry) + textstat_popc(units & upto);
    return len - (is_nl ? 1u : 0u);
}

// ---- the rule of the row sums -------------------------------------------------------------------------------------
// A wave that has the sums of a stretch of row `row` in the chunk that starts at byte c0 stores them plainly when every
// byte of the row lies in that chunk (no other wave has any), and otherwise adds them to the row's statistics (the
// longest line: takes the maximum with it), which were pre-set to 0; a sum of 0 adds nothing.  A row's chunks all take
// the same branch.
__host__ __device__ inline bool textstat_row_inside(const uint64_t* offs, uint64_t row, uint64_t c0) {
    return offs[row] >= c0 && offs[row + 1] <= c0 + kTextstatChunk;
}
__host__ __device__ inline bool textstat_adds(uint64_t v) { return v != 0; }

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// textstat.hip.  All pointers are device memory.
// the room that the scan of n_chunks summaries and the count and compaction of n_bytes marks need
hipError_t textstat_scan_bytes(uint64_t n_chunks, size_t* scan_bytes);
hipError_t textstat_lines_bytes(uint64_t n_bytes, size_t* count_bytes, size_t* select_bytes);
// summary u64[n_chunks] of the corpus's chunks
hipError_t launch_textstat_summary(const DedupRows& rows, uint32_t flags, uint64_t* summary, hipStream_t stream);
// carry u64[n_chunks] = the exclusive scan of the summaries under TextstatCarryOp
hipError_t launch_textstat_scan(const uint64_t* summary, uint64_t* carry, uint64_t n_chunks, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// stats i64[kTextstatN, S] (may be NULL; pre-set to 0 here) and line_start u8[n_bytes] (may be NULL)
hipError_t launch_textstat(const DedupRows& rows, uint64_t line_limit, uint32_t flags, const uint64_t* carry, int64_t* stats, uint8_t* line_start,
                           hipStream_t stream);
// *d_count = the marks of line_start u8[n_bytes]
hipError_t launch_textstat_count(const uint8_t* line_start, uint64_t n_bytes, unsigned long long* d_count, void* tmp, size_t tmp_bytes, hipStream_t stream);
// starts u64[the marks] = the marked positions, ascending; *d_count = their number
hipError_t launch_textstat_compact(const uint8_t* line_start, uint64_t n_bytes, uint64_t* starts, unsigned long long* d_count, void* tmp, size_t tmp_bytes,
                                   hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
