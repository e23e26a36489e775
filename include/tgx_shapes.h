/* tgx_shapes.h: fixed-length sequences of byte classes ("shapes") on a resident corpus, as a windowed bit scan over
 * every row.  An addition to the C ABI of tgx.h, which it includes, in a header of its own, as tgx_patterns.h and
 * tgx_redact.h are; the ABI version stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- shapes over the bytes of every row (csrc/shape.hip, csrc/shape.h) ------------------------------------------------
 * API keys and tokens (AKIA[0-9A-Z]{16}, ghp_[0-9a-zA-Z]{36}, [0-9a-f]{32}), the <KEY> class of the PII pass of BigCode /
 * StarCoder: a literal prefix inside the class that follows it, or a long run of one class, makes the search automaton
 * of tgx_patterns.h remember every overlapping start, 33 to thousands of states where it serves 16.  These patterns have
 * no loop: whether a match ends at byte j depends on the last len bytes alone.  The ABI takes the classes, not a syntax
 * (Python: tokengeex_amd.patterns.compile_shapes).  Integer work: the same bits on every machine and in every run.
 *
 * The shapes.  tgx_shapes is a plain struct, no handle, nothing resident between calls: n_patterns, 1 .. 8; len[k],
 *   1 .. 64 each, their sum at most 128; cls[q], position q of the patterns laid end to end, a set of bytes (byte b is
 *   bit b & 7 of cls[q][b >> 3]); per pattern two guards, not_before[k] and not_after[k], sets of bytes in the same
 *   layout, all zero for no guard.  Pattern k owns positions first_k .. first_k + len[k] - 1 of cls, first_k being the sum
 *   of the lengths before it.  Entries of len, cls and the guards beyond those in use are ignored.  It is checked on the
 *   host before anything is queued: n_patterns outside 1 .. 8, a len outside 1 .. 64, a sum of lengths over 128 or an
 *   empty class at a used position is TGX_ERR_INVALID, with nothing written.
 *
 * Semantics, by bytes alone.  Row i is the bytes text[r0 .. r1), r0 = offs[i], r1 = offs[i + 1].  Pattern k MATCHES at
 *   start a of row i when
 *     a >= r0 and a + len[k] <= r1;
 *     text[a + t] is in cls[first_k + t] for every t in 0 .. len[k] - 1;
 *     a == r0, or text[a - 1] is not in not_before[k];
 *     a + len[k] == r1, or text[a + len[k]] is not in not_after[k].
 *   A guard never looks outside its row: a row's ends, and so the corpus's, pass every guard.
 *
 * Outputs.  ends[p], u8[n_bytes]: bit k is set when a match of pattern k ends at byte p (p = a + len[k] - 1).
 *   count[i], i64[S]: the positions of row i with ends != 0.  mask[p], u8[n_bytes]: bit k is set when byte p lies inside
 *   some match of pattern k; overlapping matches merge, as in tgx_redact.h (what tgx_corpus_redact takes).  covered[i],
 *   i64[S]: the bytes of row i with mask != 0.  Either output of a call may be NULL, not both (TGX_ERR_INVALID); every
 *   byte of the others is written.  An empty row has no positions; S = 0 writes nothing.
 *
 * tgx_corpus_shape_hits_device(c, shapes, count, ends, stream), tgx_corpus_shape_cover_device(c, shapes, covered, mask,
 *   stream): the outputs are caller-owned device memory on the corpus's device, checked before anything is queued; the
 *   pointer checks, the stream rule, the corpus's lock and the limit on S (S < 2^32 - 1) are those of
 *   tgx_corpus_dfa_hits_device.  The corpus is only read.
 *   Position q of the packed patterns is bit q of a word of 64 or 128 bits.  A byte's word says which positions it fits;
 *   the kernel lays the bytes of all rows end to end, 64 to a wave and a lane a byte, and ANDs every byte's word with
 *   the shifted word of the byte d before it, d = 1, 2, 4 .. 32 (Shift-And's state, built as a window): after six steps
 *   bit q says that the bytes up to this one fit their pattern up to q.  No state is older than 63 bytes, so a wave reads
 *   the 64 bytes in front of its own and needs no summary, no scan over the corpus and no second pass.  The cover reads
 *   the ends of a chunk and of the next one.  The time does not depend on the text, the rows or the classes.
 *
 * Host twins, no device, the argument checks of tgx_dfa_hits_host and the shapes' above:
 *   tgx_shape_hits_host, tgx_shape_cover_host(text, offs, n_rows, shapes, ...).  They build the same tables and walk the
 *   kernels' chunks, halo, doubling steps, guards, windows and store / add rule through csrc/shape.h.
 *
 * tgx_shapes_last_times: device time per stage of the calling thread's last hits or cover call, as tgx_dfa_last_times
 * (the names are listed without a call): shape_ends_kernel (the pre-set and the kernel), shape_cover_kernel.  A hits call
 * sets the first and leaves the second alone. */
#ifndef TGX_SHAPES_H
#define TGX_SHAPES_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_SHAPES_MAX_PATTERNS 8
#define TGX_SHAPE_MAX_LEN 64
#define TGX_SHAPES_MAX_BITS 128
typedef struct {
    uint32_t n_patterns;        /* 1 .. 8 */
    uint32_t len[8];            /* 1 .. 64 each; their sum <= 128 */
    uint8_t cls[128][32];       /* position q of the concatenation of the patterns: a set of bytes, bit (b & 7) of byte b >> 3 */
    uint8_t not_before[8][32];  /* per pattern; all zero: no guard */
    uint8_t not_after[8][32];
} tgx_shapes;
tgx_status tgx_corpus_shape_hits_device(tgx_corpus *c, const tgx_shapes *shapes, int64_t *count, uint8_t *ends, void *stream);
tgx_status tgx_corpus_shape_cover_device(tgx_corpus *c, const tgx_shapes *shapes, int64_t *covered, uint8_t *mask, void *stream);
tgx_status tgx_shape_hits_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_shapes *shapes, int64_t *count, uint8_t *ends);
tgx_status tgx_shape_cover_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const tgx_shapes *shapes, int64_t *covered, uint8_t *mask);
int tgx_shapes_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_SHAPES_H */
