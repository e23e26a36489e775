/* tgx_word_ids.h: the words of a resident corpus as rows of a result, one id per white-space word.  An addition to the C
 * ABI of tgx.h in a header of its own, beside the word statistics of tgx_words.h, which it includes and whose words these
 * are; the ABI version stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- word ids (csrc/words.hip) --------------------------------------------------------------------------------------
 * Every n-gram pass over a result (tgx_result_minhash_device, the gram sets and hits, the repeat statistics, the id
 * phrases of tgx_phrases.h, first_equal, select, the layouts) counts the result's elements.  The recipes they serve
 * define their n-grams over WORDS: Gopher's repetition rules, 13-gram decontamination, the word 5-gram shingles of
 * MinHash dedup.  tgx_corpus_words gives a result whose row i holds one id per word of row i of the corpus, so each of
 * those passes works at word level as it stands, and two corpora encoded under different vocabularies compare by words.
 *
 * Definitions.  Space, word, word start and word end are exactly those of tgx_corpus_word_stats_device (tgx_words.h): a
 * space is 0x20 or 0x09 .. 0x0D, a word a maximal run of non-space bytes of one row, two rows with no space between them
 * are two words, and everything is defined by bytes alone, on invalid UTF-8 too.
 *   digit(b) = b + 1 (1 .. 256); under TGX_WORDS_FOLD b is lowered first if it is A-Z, and only then ('@' and '[' stay,
 *     and so does every byte >= 0x80).
 *   The polynomial of a word with the bytes b_0 .. b_{n-1}:  P = sum_j digit(b_j) * M^(n-1-j)  mod 2^64, with
 *     M = 0x9E3779B97F4A7C15 (odd).  No digit is 0, so a leading 0x00 counts: "\0a", "a" and "\0\0a" differ.
 *   R(x): the three xor-shift / multiply rounds of tgx_dropout_u01 (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27,
 *     x *= 0x94D049BB133111EB, x ^= x >> 31).
 *   key = R(P ^ R(t + n)), with t = R(seed + M) and n the word's length in bytes.
 *   id = key >> 33: below 2^31, and the result's vocab_size is 0x80000000, so the layout calls, which refuse ids of 2^31
 *     and more, take it.
 *   Two words are the same word iff their keys are equal: equal words always are, and different words are told apart
 *   with the probability of a 64-bit key (of a 31-bit id: D distinct words collide somewhere with probability about
 *   D^2 / 2^32), in the sense in which the gram hits are probabilistic.  The polynomial is taken mod 2^64 and is NOT robust
 *   against input made to collide.
 *
 * tgx_corpus_words(c, flags, seed, stream, &out) -> a new tgx_result on the corpus's device (free it with
 *   tgx_result_free): S rows, row i the ids of row i's words in order; an empty row and a row of spaces only are empty
 *   rows.  flags: 0 or TGX_WORDS_FOLD; anything else is TGX_ERR_INVALID with nothing queued.  The number of words visits
 *   the host once, between the scan and the emit kernel (it sizes the ids), as the number of lines does in
 *   tgx_corpus_lines; 2^32 - 1 words or more: TGX_ERR_UNSUPPORTED.  S = 0 or no word: an empty result with S rows.
 *   Stream rule, the corpus's lock and the limit on S (S < 2^32 - 1) as tgx_corpus_word_stats_device.  The corpus is
 *   only read.
 *   The kernels lay the bytes of all rows end to end, 64 to a wave and a lane a byte, as the word statistics' do, and no
 *   lane walks its word: the polynomial of a stretch of bytes is the state (h, M^len), `a` then `b` is
 *   (a.h * b.pow + b.h, a.pow * b.pow), and a space byte or a row's first byte drops what precedes it.  A wave scans its
 *   64 states in six doubling steps with the constant multipliers M, M^2 .. M^32; a first kernel writes the state that is
 *   open at each chunk's end with the chunk's number of word ends, one scan turns those into each chunk's carry, and the
 *   second kernel gives every word end its polynomial (plus carry.h * M^(lane + 1) for a word that began before the
 *   chunk), its key and its place, carry.ends + the word ends below the lane.  A third kernel writes the S + 1 offsets:
 *   the word ends in front of each row's first byte.  The time does not depend on the words' lengths.
 *
 * tgx_word_key(bytes, n, flags, seed) -> the key of the n bytes taken as ONE word (space bytes are not looked for;
 *   n = 0 has a key too), on the host, no device: what a caller needs to build id phrases and to look words up.  Only the
 *   TGX_WORDS_FOLD bit of flags is read.  The id is the key >> 33.
 *
 * Host twin, no device, the argument checks of tgx_word_stats_host: tgx_words_host(text, offs, n_rows, flags, seed,
 *   out_ids, ids_cap, out_offs, &n_words) writes out_offs u64[n_rows + 1] and out_ids u32[n_words], and sets n_words (also
 *   when it fails after counting).  ids_cap < n_words: TGX_ERR_INVALID with n_words set and nothing written, so a first
 *   call with ids_cap = 0 asks for the size.  It walks the kernels' chunks, doubling steps, summaries, carry, emit rule
 *   and offsets through csrc/words.h.
 *
 * tgx_words_last_times: device time per stage of the calling thread's last tgx_corpus_words, as tgx_wordstat_last_times
 * (the names are listed without a call): words_summary_kernel, words_scan, words_kernel, words_offsets_kernel. */
#ifndef TGX_WORD_IDS_H
#define TGX_WORD_IDS_H

#include "tgx_words.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_WORDS_FOLD 1u
#define TGX_WORDS_VOCAB_SIZE 0x80000000u
tgx_status tgx_corpus_words(tgx_corpus *c, uint32_t flags, uint64_t seed, void *stream, tgx_result **out);
uint64_t tgx_word_key(const uint8_t *bytes, uint64_t n, uint32_t flags, uint64_t seed);
tgx_status tgx_words_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, uint32_t flags, uint64_t seed, uint32_t *out_ids,
                          uint64_t ids_cap, uint64_t *out_offs, uint64_t *n_words);
int tgx_words_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_WORD_IDS_H */
