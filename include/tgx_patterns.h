/* tgx_patterns.h: byte patterns over character classes on a resident corpus, as a deterministic automaton run over every
 * row.  An addition to the C ABI of tgx.h, which it includes, in a header of its own, as tgx_words.h and tgx_phrases.h
 * are; the ABI version stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- a DFA over the bytes of every row (csrc/dfa.hip, csrc/dfa.h) -----------------------------------------------------
 * E-mail and IPv4 addresses, SSN-shaped numbers (the PII pass of BigCode / StarCoder), URLs per row, lines that end in
 * terminal punctuation (C4), runs of five or more digits: filters written as patterns over character classes, which the
 * literal phrases of tgx_phrases.h cannot express.  The ABI takes an automaton, not a syntax: a caller compiles its
 * patterns with whatever it has (Python: tokengeex_amd.patterns.compile_pattern; Rust: regex-automata) and hands over
 * the table.  Integer work, pinned here: the same bits on every machine and in every run.
 *
 * The automaton.  tgx_dfa is a plain struct, no handle, nothing resident between calls: n_states states, 1 .. 16; the
 *   state `start`; next[b][s], the state after byte b in state s; tag[s], 0 for a non-accepting state and otherwise a
 *   caller-defined non-zero byte (the Python surface uses one bit per pattern).  Entries of next and tag at s >= n_states
 *   are ignored.  It is checked on the host before anything is queued: n_states outside 1 .. 16, start >= n_states, a
 *   next[b][s] >= n_states with s < n_states, or tag[start] != 0 (a pattern that matches the empty string) is
 *   TGX_ERR_INVALID, with nothing written.
 *
 * Semantics, by bytes alone.  Row i is the bytes b_0 .. b_{n-1} = text[offs[i] .. offs[i+1]).  q_{-1} = start and
 *   q_j = next[b_j][q_{j-1}].  Every row begins in `start`: nothing carries from one row into the next, and an empty row
 *   has no positions.  With a search automaton (that of .*R for a pattern R) tag[q_j] != 0 says that a match of R ends
 *   at byte j.
 *
 * Outputs.  count[i], i64[S]: the number of positions j of row i with tag[q_j] != 0.  ends[p], u8[n_bytes]: tag[q_j] at
 *   every byte.  Either may be NULL, not both (TGX_ERR_INVALID); every byte of the others is written.  S = 0 writes
 *   nothing.
 *
 * tgx_corpus_dfa_hits_device(c, dfa, count, ends, stream): count and ends are caller-owned device memory on the corpus's
 *   device, checked before anything is queued; the pointer checks, the stream rule, the corpus's lock and the limit on S
 *   (S < 2^32 - 1) are those of tgx_corpus_word_stats_device.  The corpus is only read.
 *   A deterministic automaton's step is a function from states to states, and functions compose associatively.  A
 *   byte's map is a word of sixteen nibbles (eight in a 32-bit word when n_states <= 8), nibble s holding next[b][s]; the
 *   kernels lay the bytes of all rows end to end, 64 to a wave and a lane a byte, as the text statistics' do, and scan
 *   the maps inside the wave in six doubling steps.  A row's first byte has the constant map, every nibble
 *   next[b][start], which drops whatever precedes it by arithmetic: rows need no segmented state.  A first kernel writes
 *   one map per 64 bytes, one scan under composition turns them into the map in front of every chunk, and the second
 *   kernel repeats the in-wave scan and reads every byte's state off its map.  No lane ever walks: the time does not
 *   depend on the text, the rows' lengths or the automaton.  A row inside a wave's 64 bytes gets a plain store of its
 *   count, any other 64-bit atomic adds onto a count pre-set to 0, which empty rows keep.
 *
 * Host twin, no device, the argument checks of tgx_text_stats_host and the automaton's above:
 *   tgx_dfa_hits_host(text, offs, n_rows, dfa, count, ends).  It builds the same maps and walks the kernels' chunks,
 *   doubling steps, records, carry and store / add rule through csrc/dfa.h.
 *
 * tgx_dfa_last_times: device time per stage of the calling thread's last call, as tgx_words_last_times (the names are
 * listed without a call): dfa_summary_kernel, dfa_scan, dfa_kernel (the pre-set and the kernel). */
#ifndef TGX_PATTERNS_H
#define TGX_PATTERNS_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_DFA_MAX_STATES 16
typedef struct {
    uint32_t n_states; /* 1 .. 16 */
    uint32_t start;
    uint8_t next[256][16]; /* next[b][s] */
    uint8_t tag[16];
} tgx_dfa;
tgx_status tgx_corpus_dfa_hits_device(tgx_corpus *c, const tgx_dfa *dfa, int64_t *count, uint8_t *ends, void *stream);
tgx_status tgx_dfa_hits_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_dfa *dfa, int64_t *count, uint8_t *ends);
int tgx_dfa_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_PATTERNS_H */
