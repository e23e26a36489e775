// Runs of a byte mask replaced in a new resident corpus (include/tgx_redact.h: tgx_corpus_redact): a byte's class, the
// head of a run, the bytes a lane puts out, the table of replacements and the new offset of a row boundary.  The kernels
// of redact.hip and the host twin in host_twins.cpp (tgx_redact_host) both go through these functions; the tiling is
// textstat.h's.  DESIGN.md, section L.19.
//
// A byte's class is the index of its mask's lowest set bit, and none when the mask is 0 or the index is no replacement.
// A run is a maximal stretch of bytes of one row with the same class; its HEAD is its first byte: a byte with a class
// that sits on its row's first byte or whose byte before has another class or none.  A byte puts out 1 byte (itself)
// without a class, its class's replacement at a head, and nothing inside a run.  So the new text is an exclusive sum of
// lengths and a fill: a wave sums its 64 lengths, one scan of a u64 per chunk gives every chunk its place (positions are
// 64-bit throughout), and the fill recomputes the lengths and writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"
#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kRedactMaxClasses = 8;  // TGX_REDACT_MAX_CLASSES
constexpr uint32_t kRedactMaxRepl = 64;    // TGX_REDACT_MAX_REPL
constexpr uint32_t kRedactNone = kRedactMaxClasses;
constexpr int kRedactStages = 4;

__host__ __device__ inline uint32_t redact_class(uint8_t mask, uint32_t n_repl) {
    if (!mask) return kRedactNone;
    const uint32_t k = (uint32_t)__builtin_ctz(mask);
    return k < n_repl ? k : kRedactNone;
}
// the bytes that a byte of class cls puts out; before: the class of the byte before it, looked at only when it is not
// its row's first
__host__ __device__ inline uint32_t redact_len(uint32_t cls, uint32_t before, bool row_first, const uint8_t* lens) {
    if (cls == kRedactNone) return 1;
    return row_first || before != cls ? lens[cls] : 0u;
}

// ---- the table of a call --------------------------------------------------------------------------------------------
// kRedactTableWords 8-byte words: the replacements in slots of 64 bytes, then their eight lengths.
constexpr uint32_t kRedactTableWords = kRedactMaxClasses * kRedactMaxRepl / 8 + 1;
struct RedactTable {
    uint8_t bytes[kRedactMaxClasses][kRedactMaxRepl];
    uint8_t len[kRedactMaxClasses];
};
static_assert(sizeof(RedactTable) == kRedactTableWords * 8, "the table is uploaded as words");
// NULL, or what is wrong with the replacements; on NULL `words` holds the table
inline const char* redact_pack_table(const uint8_t* repl_bytes, const uint64_t* repl_offs, uint32_t n_repl, uint64_t* words) {
    if (n_repl < 1 || n_repl > kRedactMaxClasses) return "n_repl is outside 1 .. 8";
    if (!repl_offs) return "repl_offs is NULL";
    if (repl_offs[0] != 0) return "repl_offs does not begin at 0";
    for (uint32_t k = 0; k < n_repl; k++) {
        if (repl_offs[k + 1] < repl_offs[k]) return "repl_offs is not monotone";
        if (repl_offs[k + 1] - repl_offs[k] > kRedactMaxRepl) return "a replacement is longer than 64 bytes";
    }
    if (repl_offs[n_repl] && !repl_bytes) return "repl_bytes is NULL";
    RedactTable* t = reinterpret_cast<RedactTable*>(words);
    for (uint32_t k = 0; k < kRedactMaxClasses; k++) {
        const uint64_t n = k < n_repl ? repl_offs[k + 1] - repl_offs[k] : 0;
        t->len[k] = (uint8_t)n;
        for (uint32_t q = 0; q < kRedactMaxRepl; q++) t->bytes[k][q] = q < n ? repl_bytes[repl_offs[k] + q] : 0;
    }
    return nullptr;
}

// The new offset of row boundary r = 0 .. S: the carry of the chunk that holds position offs[r], plus what the at most 63
// bytes in front of it in that chunk put out.  carry: u64[n_chunks + 1], the exclusive sum of the chunks' lengths, so the
// entry behind the last chunk is the new text's length and offs[S] on a chunk's edge needs no case of its own; empty rows
// need none either.  The bytes in front belong to rows below r: the walk goes down and looks a row up when it crosses a
// row's first byte (pack_find_row steps over runs of empty rows).
__host__ __device__ inline uint64_t redact_row_offset(const uint8_t* mask, const uint64_t* offs, uint64_t r, uint32_t n_repl, const uint8_t* lens,
                                                      const uint64_t* carry) {
    const uint64_t p = offs[r], c0 = p - p % kTextstatChunk;
    uint64_t at = carry[c0 / kTextstatChunk];
    if (p == c0) return at;
    uint64_t row = pack_find_row(offs, 0, 0, r - 1, p - 1), begin = offs[row];
    for (uint64_t q = p; q-- > c0;) {
        if (q < begin) {
            row = pack_find_row(offs, 0, 0, row - 1, q);
            begin = offs[row];
        }
        const uint32_t before = q > begin ? redact_class(mask[q - 1], n_repl) : kRedactNone;
        at += redact_len(redact_class(mask[q], n_repl), before, q == begin, lens);
    }
    return at;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// redact.hip.  All pointers are device memory; the corpus has a row and a byte, n_chunks = ceil(n_bytes / 64), and table
// is kRedactTableWords words.
// the room that the exclusive sum of n_recs words needs
hipError_t redact_scan_bytes(uint64_t n_recs, size_t* scan_bytes);
// rec[n_chunks + 1]: what every chunk puts out, then 0
hipError_t launch_redact_lengths(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, uint64_t* rec, hipStream_t stream);
// carry[n_recs] = the exclusive sum of the records
hipError_t launch_redact_scan(const uint64_t* rec, uint64_t* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// new_offs[S + 1]
hipError_t launch_redact_offsets(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, const uint64_t* carry, uint64_t* new_offs,
                                 hipStream_t stream);
// out[carry[n_chunks]]: the new text
hipError_t launch_redact_fill(const DedupRows& rows, const uint8_t* mask, uint32_t n_repl, const uint64_t* table, const uint64_t* carry, uint8_t* out,
                              hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
