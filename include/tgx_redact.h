/* tgx_redact.h: the bytes of a resident corpus that lie inside a match of a byte pattern, and a new resident corpus in
 * which runs of marked bytes are replaced by short strings.  An addition to the C ABI of tgx.h, in a header of its own as
 * tgx_patterns.h is, which it includes for tgx_dfa; the ABI version stays 1.  Status codes, threading, the stream rule
 * and last-error reporting are tgx.h's.
 *
 * ---- cover: a forward and a backward automaton and a pair table (csrc/cover.hip, csrc/cover.h) -----------------------
 * The PII pass of BigCode / StarCoder does not drop a file that holds an e-mail address: it replaces the address.  The
 * ends that tgx_corpus_dfa_hits_device marks cannot say which bytes a match holds, and an automaton run backwards from
 * the ends is alive on bytes that no match reaches.  Whether byte j lies inside a match depends on what is to its left
 * AND on what is to its right, so the call takes two automata and a table over the pairs of their states.
 *
 * tgx_dfa_cover: fwd, run from a row's first byte to its last (fwd.tag marks match ends as in tgx_patterns.h); bwd, run
 *   from a row's last byte to its first (bwd.tag is ignored); cover[f][g], a caller-defined byte (the Python surface:
 *   bit k for pattern k).  Both automata are checked as tgx_dfa is, bwd without the rule on tag[start]; a failure is
 *   TGX_ERR_INVALID with nothing written.  Entries of cover at f >= fwd.n_states or g >= bwd.n_states are ignored.
 *
 * Semantics, by bytes alone.  Row i is the bytes b_0 .. b_{n-1} = text[offs[i] .. offs[i+1]).
 *   f_{-1} = fwd.start and f_j = fwd.next[b_j][f_{j-1}]: the forward state AFTER byte j.
 *   g_{n-1} = bwd.start and g_{j-1} = bwd.next[b_j][g_j]: g_j is the backward state BEFORE byte j is consumed, that is,
 *   after every byte to its right in the row.
 *   mask[offs[i] + j] = cover[f_j][g_j], u8[n_bytes]; covered[i], i64[S]: the bytes of row i with a non-zero mask.
 *   Nothing carries across a row's end in either direction, and an empty row has no positions.  Either output may be
 *   NULL, not both (TGX_ERR_INVALID); every byte of the others is written.  S = 0 writes nothing.
 *   (tokengeex_amd.patterns.compile_pattern(cover=True) builds the three tables so that bit k of mask[p] says that byte p
 *   lies inside some match of pattern k.)
 *
 * tgx_corpus_dfa_cover_device(c, cov, covered, mask, stream): covered and mask are caller-owned device memory on the
 *   corpus's device; the pointer checks, the stream rule, the corpus's lock and the limit on S are those of
 *   tgx_corpus_dfa_hits_device.  The corpus is only read.  Both sides are scans of state maps under composition, the
 *   backward one mirrored, so no lane walks and the time does not depend on the text.
 * tgx_dfa_cover_host(text, offs, n_rows, cov, covered, mask): the host twin, no device, the kernels' chunks, doubling
 *   steps in both directions, records, mirrored carry and store / add rule through csrc/dfa.h and csrc/cover.h.
 *
 * ---- redact: runs of a byte mask replaced in a new resident corpus (csrc/redact.hip, csrc/redact.h) ------------------
 * mask is u8[n_bytes] from any source.  A byte's CLASS is the index of its mask's lowest set bit; a byte whose mask is 0
 *   or whose index is >= n_repl has no class.  A RUN is a maximal stretch of bytes of ONE row with the same class.  The
 *   new corpus has the same S rows in order; every run is replaced by replacement `class`, repl_bytes[repl_offs[class] ..
 *   repl_offs[class + 1]), 0 .. TGX_REDACT_MAX_REPL bytes (an empty one deletes the run), and a byte with no class is
 *   copied.  A row may become empty.
 *
 * tgx_corpus_redact(c, d_mask, repl_bytes, repl_offs, n_repl, flags, stream, out): d_mask is device memory on the
 *   corpus's device (it may be NULL when the corpus has no byte); the replacements are host memory.  flags != 0, n_repl
 *   outside 1 .. TGX_REDACT_MAX_CLASSES, a replacement over TGX_REDACT_MAX_REPL bytes or repl_offs that are not
 *   monotone from 0 are TGX_ERR_INVALID with nothing queued and *out = NULL.  The corpus is only read; *out is freed
 *   with tgx_corpus_free.  The new offsets visit the host once, as tgx_corpus_lines' do.
 * tgx_redact_host(text, offs, n_rows, mask, repl_bytes, repl_offs, n_repl, out_text, out_cap, out_offs, out_len): the
 *   host twin.  out_offs is u64[n_rows + 1] and always written when the arguments pass; *out_len is the new length;
 *   out_text, out_cap bytes of room, is written only when out_cap >= *out_len (else TGX_ERR_INVALID, with *out_len
 *   set, so a caller may ask with out_cap = 0 first).
 *
 * tgx_redact_last_times: device time per stage of the calling thread's last cover or redact call, as
 * tgx_dfa_last_times (the names are listed without a call): cover_summary_kernel, cover_scan, cover_kernel,
 * redact_length_kernel, redact_scan, redact_offsets_kernel, redact_fill_kernel.  A call sets its own stages and leaves
 * the other call's alone. */
#ifndef TGX_REDACT_H
#define TGX_REDACT_H

#include "tgx_patterns.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    tgx_dfa fwd;           /* run left to right; fwd.tag marks match ends */
    tgx_dfa bwd;           /* run right to left; bwd.tag is ignored */
    uint8_t cover[16][16]; /* cover[f][g] */
} tgx_dfa_cover;
tgx_status tgx_corpus_dfa_cover_device(tgx_corpus *c, const tgx_dfa_cover *cov, int64_t *covered, uint8_t *mask, void *stream);
tgx_status tgx_dfa_cover_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_dfa_cover *cov, int64_t *covered, uint8_t *mask);

#define TGX_REDACT_MAX_CLASSES 8
#define TGX_REDACT_MAX_REPL 64
tgx_status tgx_corpus_redact(tgx_corpus *c, const uint8_t *d_mask, const uint8_t *repl_bytes, const uint64_t *repl_offs, uint32_t n_repl, uint32_t flags,
                             void *stream, tgx_corpus **out);
tgx_status tgx_redact_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const uint8_t *mask, const uint8_t *repl_bytes,
                           const uint64_t *repl_offs, uint32_t n_repl, uint8_t *out_text, uint64_t out_cap, uint64_t *out_offs, uint64_t *out_len);
int tgx_redact_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_REDACT_H */
