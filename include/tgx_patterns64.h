/* tgx_patterns64.h: byte patterns of up to 64 states on a resident corpus.  An addition to the C ABI of tgx.h in a header
 * of its own, as tgx_shapes.h and tgx_redact.h are; it includes tgx_patterns.h, whose automaton it widens, and the ABI
 * version stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- a DFA of up to 64 states over the bytes of every row (csrc/dfa64.hip, csrc/dfa64.h) ------------------------------
 * The sixteen states of tgx_dfa are sixteen nibbles in one word, and that form cannot grow.  A phone shape of 17 states,
 * an e-mail, an IPv4 and an SSN pattern in one automaton, a 32-digit hash, card and IBAN shapes with optional separators
 * are all beyond it.  tgx_dfa64 is the same automaton with 64 for 16, served by kernels of another shape: a lane per
 * state, then a lane per chunk.
 *
 * The automaton.  tgx_dfa64 is a plain struct, no handle, nothing resident between calls: n_states states, 1 .. 64; the
 *   state `start`; next[b][s], the state after byte b in state s; tag[s], 0 for a non-accepting state and otherwise a
 *   caller-defined non-zero byte.  Entries of next and tag at s >= n_states are ignored.  It is checked on the host before
 *   anything is queued: n_states outside 1 .. 64, start >= n_states, a next[b][s] >= n_states with s < n_states, or
 *   tag[start] != 0 (a pattern that matches the empty string) is TGX_ERR_INVALID, with nothing written.  Any n_states in
 *   1 .. 64 is served, an automaton that tgx_dfa would hold too.
 *
 * Semantics, by bytes alone: those of tgx_patterns.h.  Row i is the bytes b_0 .. b_{n-1} = text[offs[i] .. offs[i+1]).
 *   q_{-1} = start and q_j = next[b_j][q_{j-1}].  Every row begins in `start`: nothing carries from one row into the
 *   next, and an empty row has no positions.
 *
 * Outputs.  count[i], i64[S]: the number of positions j of row i with tag[q_j] != 0.  ends[p], u8[n_bytes]: tag[q_j] at
 *   every byte.  Either may be NULL, not both (TGX_ERR_INVALID); every byte of the others is written.  S = 0 writes
 *   nothing.
 *
 * tgx_corpus_dfa64_hits_device(c, dfa, count, ends, stream): count and ends are caller-owned device memory on the
 *   corpus's device, checked before anything is queued; the pointer checks, the stream rule, the corpus's lock and the
 *   limit on S (S < 2^32 - 1) are those of tgx_corpus_dfa_hits_device.  The corpus is only read.
 *   The bytes of all rows are laid end to end; a CHUNK is 64 of them and a SEGMENT 64 chunks (4 096 bytes).  A wave reads
 *   a chunk's byte, which is the same for all its lanes, and lane s advances the run that began in state s with one LDS
 *   lookup: after 64 bytes the lanes hold the chunk's state map, and `a then b` of two maps is one cross-lane read (lane
 *   s fetches b from lane a[s]).  A row's first byte sends every lane to `start` first, the constant map of
 *   tgx_patterns.h, so rows need no segmented state.  The chunks' maps fold into their segment's, the segments' maps are
 *   scanned from `start`, and a second kernel replays the text with a lane per chunk, 64 chunks side by side, each from
 *   its known state, and stores every byte's tag.  A last kernel counts the tags per row by tgx_patterns.h's rule.  The
 *   time does not depend on the text, the rows' lengths or the automaton.
 *   Scratch (pooled, nothing assumed of its contents): N bytes of chunk maps, N/8 of row-start masks and N/64 of segment
 *   records, about 9N/8 + N/64 bytes, and N more for the tags when ends is NULL.
 *
 * Host twin, no device, the argument checks of tgx_dfa_hits_host and the automaton's above:
 *   tgx_dfa64_hits_host(text, offs, n_rows, dfa, count, ends).  It walks the kernels' chunks, segments, row-start masks,
 *   fold, scan, chain and store / add rule through csrc/dfa64.h.
 *
 * tgx_dfa64_last_times: device time per stage of the calling thread's last call, as tgx_dfa_last_times (the names are
 * listed without a call): dfa64_map_kernel, dfa64_scan, dfa64_replay_kernel, dfa64_count_kernel (the pre-set and the
 * kernel). */
#ifndef TGX_PATTERNS64_H
#define TGX_PATTERNS64_H

#include "tgx_patterns.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_DFA64_MAX_STATES 64
typedef struct {
    uint32_t n_states; /* 1 .. 64 */
    uint32_t start;
    uint8_t next[256][64]; /* next[b][s] */
    uint8_t tag[64];
} tgx_dfa64;
tgx_status tgx_corpus_dfa64_hits_device(tgx_corpus *c, const tgx_dfa64 *dfa, int64_t *count, uint8_t *ends, void *stream);
tgx_status tgx_dfa64_hits_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_dfa64 *dfa, int64_t *count, uint8_t *ends);
int tgx_dfa64_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_PATTERNS64_H */
