/* tgx_find.h: the non-overlapping, leftmost-first matches of a byte pattern in every row of a resident corpus, and the
 * most frequent distinct matches (idiom mining).  An addition to the C ABI of tgx.h in a header of its own, as
 * tgx_hashed.h is; it includes tgx_patterns64.h, whose automaton struct it reuses, and the ABI version stays 1.  Status
 * codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- what a regex engine's find_iter / re.finditer gives (csrc/find.hip, csrc/find.h) -------------------------------
 * tgx_corpus_dfa64_hits_device counts match ENDS over all overlapping matches.  This pass gives the segmentation that a
 * search loop gives: matches found left to right, each search starting where the last match ended.
 *
 * The automaton.  A tgx_dfa64, ANCHORED (the automaton of the pattern itself, not of .*pattern) and with a dead state:
 *   patterns.compile_pattern(..., find=True) builds it so that the LAST tagged state seen before the dead state is the
 *   leftmost-first match (alternatives in source order, greedy repeats).  Its checks are tgx_dfa64's; tag[s] != 0 is
 *   "tagged".  A state is DEAD when no tagged state is reachable from it; the library finds the dead states itself.
 *
 * The walk from a start byte.  Row i is text[r0 .. r1).  For a start a: q = start, and for t = 0, 1, ..: stop when
 *   a + t == r1; stop when t == max_len; q = next[text[a + t]][q]; stop when q is dead; if tag[q], len(a) = t + 1.
 *   len(a) is the last value set, or 0.  trunc(a) is true when the walk stopped on t == max_len with a + t < r1 and q
 *   not dead: a longer match might exist and is not served.
 *
 * The chain over a row.  p = r0; while p < r1: if len(p) > 0, emit the match (p, len(p)) and p += len(p); else p += 1.
 *   No match crosses a row's end.  The positions p that the loop stands on are the row's VISITED positions.
 *
 * max_len is 1 .. TGX_FIND_MAX_LEN (64, the widest tgx_gram_key); anything else is TGX_ERR_INVALID.
 *
 * tgx_corpus_find_device(c, dfa, max_len, count, lens, truncated, stream).  Caller-owned device memory on the corpus's
 *   device: lens, u8[n_bytes], the match length at every emitted start and 0 elsewhere; count, i64[S], the matches of
 *   every row; truncated, i64[S], the visited positions of the row with trunc.  Where truncated[i] is 0, row i's matches
 *   are exactly those of re.finditer.  Any of the three may be NULL, not all (TGX_ERR_INVALID); every byte of the others
 *   is written.  S = 0 writes nothing.  The automaton's checks, the pointer checks, the stream rule, the corpus's lock
 *   and the limit on S are those of tgx_corpus_dfa64_hits_device.  Unlike every other automaton pass, its time depends
 *   on the text: a lane per start byte walks until its automaton dies, a wave until its last lane has.
 *   Scratch (pooled): N bytes of walks when lens is NULL, and N/64 + N/4096 of segment records and entry skips.
 *
 * tgx_corpus_mine_device(c, dfa, max_len, top, seed, out_pos, out_len, out_count, n_out, n_distinct, n_matches, stream):
 *   synchronous.  Every emitted match gets tgx_gram_key of its bytes under `seed`; two matches are the same idiom iff
 *   their 64-bit keys are equal (as for gram sets: a collision merges two idioms, at odds of about n^2 / 2^65).  The
 *   distinct matches are ordered by count descending, then by the position of their first occurrence ascending, and the
 *   first min(top, n_distinct) are written to the HOST arrays out_pos (u64: the first occurrence's byte offset in the
 *   corpus's text), out_len (u32) and out_count (u64), each of capacity top; *n_out says how many.  *n_distinct and
 *   *n_matches (either may be NULL) are the distinct keys and the emitted matches.  top = 0 is TGX_ERR_INVALID.
 *   Truncation is not reported here: ask tgx_corpus_find_device.
 *
 * Host twins, no device, the argument checks of tgx_dfa64_hits_host and the checks above: tgx_find_host and
 * tgx_mine_host over text and offs in host memory.  They walk the kernels' chunks, doubling rounds, maps, fold, scan
 * and order rule through csrc/find.h.
 *
 * tgx_find_last_times: device time per stage of the calling thread's last find or mine call, as tgx_dfa64_last_times
 * (the names are listed without a call): find_walk_kernel, find_scan, find_replay_kernel, and the mine's find_keys (the
 * compaction and the keys), find_sort_runs, find_order. */
#ifndef TGX_FIND_H
#define TGX_FIND_H

#include "tgx_patterns64.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_FIND_MAX_LEN 64
tgx_status tgx_corpus_find_device(tgx_corpus *c, const tgx_dfa64 *dfa, uint32_t max_len, int64_t *count, uint8_t *lens, int64_t *truncated, void *stream);
tgx_status tgx_corpus_mine_device(tgx_corpus *c, const tgx_dfa64 *dfa, uint32_t max_len, uint64_t top, uint64_t seed, uint64_t *out_pos, uint32_t *out_len, uint64_t *out_count, uint64_t *n_out, uint64_t *n_distinct, uint64_t *n_matches, void *stream);
tgx_status tgx_find_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_dfa64 *dfa, uint32_t max_len, int64_t *count, uint8_t *lens, int64_t *truncated);
tgx_status tgx_mine_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_dfa64 *dfa, uint32_t max_len, uint64_t top, uint64_t seed, uint64_t *out_pos, uint32_t *out_len, uint64_t *out_count, uint64_t *n_out, uint64_t *n_distinct, uint64_t *n_matches);
int tgx_find_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_FIND_H */
