/* tgx_dupspans.h: duplicate spans across rows of a resident corpus or result, with every match verified against the
 * elements.  An addition to the C ABI of tgx.h in a header of its own, as tgx_find.h, tgx_hashed.h and tgx_allow.h are;
 * the ABI version stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- which spans already occurred earlier in the corpus (csrc/dupspan.hip, csrc/dupspan.h) -------
 * The ExactSubstr question of Lee et al. 2021 ("Deduplicating Training Data Makes Language Models Better"), which
 * pipelines run after MinHash: a licence header pasted into many files, a boilerplate paragraph at the foot of every
 * page.  tgx_*_first_equal_device sees nothing (the rows differ), MinHash a similarity near 0, tgx_*_repeat_stats_device
 * mixes the row into the key on purpose, and tgx_*_gram_hits_device against the corpus's own set flags first
 * occurrences too.
 *
 * The source, the element size eb (1: a corpus's bytes; 4: a result's ids), the width w (1 <= w, w * eb <= 64), the
 *   validity of a gram (a row shorter than w owns none) and its key under `seed` are tgx_*_repeat_stats_device's.
 *   Elements are numbered globally, all rows end to end.
 * DUPLICATE.  The valid gram at element e is a duplicate iff some valid gram at an element e' < e, in an earlier row or
 *   earlier in the same row, has the same w elements.  Equality is of the ELEMENTS, compared on the device: the 64-bit
 *   key only brings candidates together, so there is no false positive, not even at 2^-64.  The first occurrence in
 *   corpus order is never a duplicate: row order decides which copy survives (tgx_*_select_device can put the best rows
 *   first).
 * COVERED.  Element e of row i is covered iff it lies inside at least one duplicate gram.  A gram lies inside its own
 *   row, so coverage never crosses a row's end.
 * key_bits, 1 .. 64: only the low key_bits bits of the key are sorted on.  The output is the same for every value; it is
 *   a speed knob: fewer radix passes against longer runs of equal masked keys to verify.  A slot of a run that mixes
 *   different grams costs up to the run's length, so the match is quadratic in such a run: with key_bits far below log2
 *   of the gram count it runs for a very long time.  Small values are for tests of small sources only.  64 never mixes
 *   but by a 64-bit collision; 40 was the fastest of 64, 48, 40 and 32 where it was measured (256 MiB, few duplicates)
 *   and is what the Python surface passes by default.  The C call has no default.
 *
 * tgx_corpus_dup_spans_device(c, width, key_bits, seed, flags, stream, d_table, d_mask) and
 * tgx_result_dup_spans_device(r, ...):
 *   d_table, i64[TGX_DUPSPAN_N = 3, S], each statistic contiguous: grams, dup (duplicate grams), covered (covered
 *     elements).  d_mask, u8[n_elems]: TGX_DUPSPAN_MASK_DUP (bit 0) where a duplicate gram begins,
 *     TGX_DUPSPAN_MASK_COVERED (bit 1) on every covered element, 0 elsewhere.  Either may be NULL, not both; every byte of
 *     the others is written.  S = 0 writes nothing.  The source is only read.
 *   Refused before a device is asked for (TGX_ERR_INVALID): width outside its range, key_bits outside 1 .. 64, flags
 *     other than 0, both outputs NULL.  Positions are u32: 2^32 - 1 elements or more are TGX_ERR_UNSUPPORTED, before
 *     anything is queued.  The pointer checks, the stream rule, the corpus's lock and the limit on S are
 *     tgx_corpus_gram_hits_device's.
 *   Four stages on the caller's stream, one host visit (the grams' total): the keys and positions of all valid grams;
 *     rocPRIM's stable radix sort over the bits [0, key_bits); dupspan_match_kernel, a lane a sorted slot, which compares
 *     a slot's elements with its predecessor's and, on a mismatch, walks back through its run of equal masked keys to
 *     the first equal gram or the run's head; the cover kernel, which turns the flags into the rows' sums and the mask's
 *     second bit.  Scratch: 24 bytes per gram, plus a byte per element when d_mask is NULL.
 *
 * Host twin, no device, the argument checks of tgx_repeat_stats_host and key_bits': tgx_dup_spans_host(data, elem_bytes,
 *   offs, n_rows, width, key_bits, seed, table, mask) over host arrays, through the kernels' header (csrc/dupspan.h): the
 *   keys, a stable sort on the masked key, the same walk-back rule, the kernel's chunks, window and store / add rule.
 *
 * tgx_dupspan_last_times: device time per stage of the calling thread's last tgx_*_dup_spans_device, as
 * tgx_repeat_last_times (the names are listed without a call): dupspan_keys_kernel (with the scan, the pre-sets and the
 * host visit), dupspan_sort, dupspan_match_kernel, dupspan_cover_kernel.
 *
 * Not here: a minimum RUN of consecutive duplicate grams, deleting elements of a result (re-encode the deduplicated
 * corpus), where the first occurrence is, row batching for sources whose scratch does not fit, 2^32 - 1 elements or
 * more, more than one device. */
#ifndef TGX_DUPSPANS_H
#define TGX_DUPSPANS_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_DUPSPAN_N 3
#define TGX_DUPSPAN_MASK_DUP 1
#define TGX_DUPSPAN_MASK_COVERED 2
tgx_status tgx_corpus_dup_spans_device(tgx_corpus *c, uint32_t width, uint32_t key_bits, uint64_t seed, uint32_t flags, void *stream, int64_t *d_table, uint8_t *d_mask);
tgx_status tgx_result_dup_spans_device(const tgx_result *r, uint32_t width, uint32_t key_bits, uint64_t seed, uint32_t flags, void *stream, int64_t *d_table, uint8_t *d_mask);
tgx_status tgx_dup_spans_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, uint32_t width, uint32_t key_bits, uint64_t seed, int64_t *table, uint8_t *mask);
int tgx_dupspan_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_DUPSPANS_H */
