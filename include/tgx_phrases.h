/* tgx_phrases.h: literal phrase matching on a resident corpus or result: blocklists and keyword filters.  An addition to
 * the C ABI of tgx.h, which it includes, in a header of its own, as tgx_words.h is; the ABI version stays 1.  Status codes,
 * threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- phrase sets and their occurrences (csrc/phrase.hip, csrc/phrase.h) ------------------------------------------------
 * Does a row contain one of a list of literal strings?  The BigCode recipe drops files that say "auto-generated" in
 * their first lines, C4 pages with a word of a bad-word list or "lorem ipsum" and lines with "javascript"; licence
 * headers, secret-key markers and URL blocklists are the same question.  A phrase set is a trie over the list in device
 * memory; a hits call gives per-row counts, the longest match at every element and the occurrences of each phrase.
 * Integer work, pinned here: the same bits on every machine and in every run.  Literals only: no character classes,
 * no Unicode case folding (a non-ASCII phrase matches by its bytes).
 *
 * Definitions.
 *   Sources and elements.  Row i of a source is the elements data[offs[i] .. offs[i+1]) of eb bytes each: eb = 1 a
 *     corpus's text, eb = 4 a result's ids in little-endian order, as for the gram sets of tgx.h.
 *   Phrases.  Phrase p is L_p elements, 1 <= L_p <= 255 and L_p * eb <= 256: a text phrase is at most 255 bytes, an id
 *     phrase at most 64 ids.  An empty or longer phrase: TGX_ERR_INVALID.
 *   Folding.  fold(b) = b | 0x20 for b in 'A' .. 'Z' and b otherwise under TGX_PHRASE_FOLD_CASE, the identity without
 *     it.  It applies to the phrases at creation and to the text when it is read.  0x40, 0x5B, 0x60, 0x7B and every
 *     byte >= 0x80 stay as they are.
 *   Occurrence.  Phrase p occurs at element e of row i iff e + L_p <= offs[i+1] and fold(data[e+k]) == fold(p[k]) for
 *     all k.  Under TGX_PHRASE_WHOLE_WORD also: the element before e is in front of the row's first element or is no
 *     word byte, and the element at e + L_p is past the row's last element or is no word byte.  A word byte is
 *     [A-Za-z0-9_] or any byte >= 0x80.  Another row's elements are never neighbours.
 *     Occurrences may overlap ("aa" occurs three times in "aaaa"), one phrase may occur inside another's occurrence, and
 *     no occurrence crosses a row's end.  For eb = 4 occurrences begin at element boundaries only: a phrase's bytes at a
 *     byte offset that is no multiple of 4 are no occurrence.
 *   Flags.  Both need eb = 1.  Either with eb = 4, or an unknown flag: TGX_ERR_INVALID.
 *   Duplicates.  Phrases that are equal after folding are one phrase: counted once per occurrence and credited to the
 *     lowest index among them; the others' per_phrase entries are 0.
 *   Outputs.  count[i], i64[S]: the number of (e, p) occurrences in row i.  longest[e], u8[n_elems]: the largest L_p of
 *     an occurrence at e, 0 without one.  per_phrase[p], i64[P]: the occurrences of p over all rows.  Any of the three
 *     may be NULL, not all three.  Every byte of a non-NULL output is written.  P = 0, S = 0 and N = 0 are valid and
 *     write what that implies (S = 0 still zeroes per_phrase).
 *
 * tgx_phraseset_create(device, phrases, phrase_offs, n_phrases, elem_bytes, flags, out): phrases and phrase_offs are
 *   host memory, phrase p being the elements [phrase_offs[p], phrase_offs[p+1]) of `phrases`; the flags are the set's
 *   and hold for every call on it.  The set is read-only after creation: calls and threads share it without a lock.
 *   The table is an XOR double-array of 8-byte label-checked records over the phrases' bytes (csrc/phrase.h) and a
 *   65 536-bit map of the byte pairs that begin a phrase.  A table of more than 2^24 slots: TGX_ERR_UNSUPPORTED (a set
 *   of 65 536 phrases with 1 MiB of bytes has about 10^6).
 * tgx_phraseset_info: any pointer may be NULL.  n_distinct: the phrases left after folding and the duplicate rule;
 *   max_len: the longest phrase in elements, 0 for an empty set; table_bytes: the set's device memory.
 * tgx_corpus_phrase_hits_device / tgx_result_phrase_hits_device(source, set, flags, stream, d_count, d_longest,
 *   d_per_phrase): the stream rule, the corpus's lock, the pointer checks and the errors are those of
 *   tgx_corpus_gram_hits_device.  The outputs are caller-owned device memory on the source's device; everything is
 *   checked before anything is queued.  An element size or a device that differs from the set's, host memory, or call
 *   flags other than 0: TGX_ERR_INVALID, with nothing queued or written.  The source is only read.
 *   The kernel lays the elements of all rows end to end, 64 to a wave and a lane a start position, on the tiling of the
 *   gram kernels.  A row that lies inside a wave's 64 elements gets a plain store of its count, any other one 64-bit
 *   atomic add per wave onto a count pre-set to 0; per_phrase takes 64-bit atomic adds.  Integer sums are order-free.
 *
 * Host twin, no device: tgx_phrase_hits_host(data, elem_bytes, offs, n_rows, phrases, phrase_offs, n_phrases, flags,
 *   count, longest, per_phrase), `flags` being the set's.  It builds the same table and walks the kernel's chunks,
 *   filter, records and store / add rule through csrc/phrase.h.
 *
 * tgx_phrase_last_times: device time per stage of the calling thread's last hits call, as tgx_gram_last_times (the names
 * are listed without a call): phrase_hits_kernel (the pre-sets and the kernel). */
#ifndef TGX_PHRASES_H
#define TGX_PHRASES_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_PHRASE_FOLD_CASE 1u
#define TGX_PHRASE_WHOLE_WORD 2u
typedef struct tgx_phraseset tgx_phraseset;
tgx_status tgx_phraseset_create(int device, const void *phrases, const uint64_t *phrase_offs, uint32_t n_phrases, uint32_t elem_bytes,
                                uint32_t flags, tgx_phraseset **out);
tgx_status tgx_phraseset_info(const tgx_phraseset *ps, uint32_t *n_phrases, uint32_t *n_distinct, uint32_t *elem_bytes, uint32_t *flags,
                              uint32_t *max_len, int *device, uint64_t *table_bytes);
void tgx_phraseset_free(tgx_phraseset *ps);
tgx_status tgx_corpus_phrase_hits_device(tgx_corpus *c, const tgx_phraseset *ps, uint32_t flags, void *stream, int64_t *d_count,
                                         uint8_t *d_longest, int64_t *d_per_phrase);
tgx_status tgx_result_phrase_hits_device(const tgx_result *r, const tgx_phraseset *ps, uint32_t flags, void *stream, int64_t *d_count,
                                         uint8_t *d_longest, int64_t *d_per_phrase);
tgx_status tgx_phrase_hits_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, const void *phrases,
                                const uint64_t *phrase_offs, uint32_t n_phrases, uint32_t flags, int64_t *count, uint8_t *longest,
                                int64_t *per_phrase);
int tgx_phrase_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_PHRASES_H */
