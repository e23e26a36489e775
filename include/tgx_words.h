/* tgx_words.h: per-row word statistics of a resident corpus, the counts of the Gopher quality rules.  An addition to the C
 * ABI of tgx.h, which it includes, in a header of its own; the ABI version stays 1.  Status codes, threading, the stream
 * rule and last-error reporting are tgx.h's.
 *
 * ---- per-row word statistics: the Gopher quality rules (csrc/wordstat.hip) ------------------------------------------
 * What the quality rules of Gopher / MassiveText (carried by RefinedWeb, FineWeb and Dolma: a document of 50 to 100 000
 * words, a mean word length of 3 to 10, at most 0.1 hashes or ellipses per word, at most 90 % of the lines beginning with
 * a bullet, at most 30 % ending with an ellipsis, at least 80 % of the words holding a letter, at least two of eight
 * stop words) and the terminal-punctuation share of C4 and FineWeb need per row: counts over words and over the first
 * and last bytes of lines.  One call gives them where the documents already lie.  Integer work, pinned here, the same
 * on every machine.  These words come from white space; Gopher's come from a word tokenizer.
 *
 * Definitions.  Row i is the bytes text[offs[i] .. offs[i+1]) of the corpus.  Everything is defined by bytes alone, on
 * invalid UTF-8 too.
 *   Space: 0x20 and 0x09 .. 0x0D, the bytes Python's bytes.split() splits on.  Non-ASCII spaces are ordinary bytes.
 *   Word: a maximal run of non-space bytes of one row.  p is a word start iff text[p] is no space and p is its row's first
 *     byte or text[p - 1] is a space; a word end iff text[p] is no space and p is its row's last byte or text[p + 1] is a
 *     space.  Two rows with no space between them are two words.
 *   Unit: a byte, or under TGX_WORDSTAT_CHARS a character, a byte b with (b & 0xC0) != 0x80.  A word's length is its units.
 *   Line, line start, line end: those of tgx_corpus_text_stats_device.  A line's content is the line without its '\n'.
 *   tail(p): the eight bytes text[p - 7 .. p], and prev(p) = text[p - 8]; any of them in front of the row's first byte
 *     reads as 0x20.  Every look-around below is backwards and at most nine bytes.
 *   nsb(p): the number of non-space bytes of p's line in front of p, saturated at 3.
 *
 * tgx_corpus_word_stats_device(c, word_limit, stop_bytes, stop_offs, n_stop, flags, stream, d_stats, d_marks) writes
 *   d_stats, int64 [TGX_WORDSTAT_N, S], each statistic contiguous over the rows:
 *      0 words             word ends
 *      1 word_units        units of non-space bytes: the sum of the word lengths
 *      2 max_word          the longest word's length; 0 without a word
 *      3 long_words        words longer than word_limit
 *      4 alpha_words       words with a byte in A-Z, a-z
 *      5 alpha_wide_words  words with a byte in A-Z, a-z or a byte >= 0x80 (the stand-in for the letters of other
 *                          scripts: the classes stay ASCII, as in the text statistics)
 *      6 hash              bytes equal to '#'
 *      7 ellipsis          positions p with text[p - 2 .. p] = "..." and text[p - 3] != '.' (a run of three or more dots,
 *                          counted once at its third dot), plus positions p with text[p - 2 .. p] = E2 80 A6 (U+2026)
 *      8 lines             line ends (the text statistics' `lines`: the shares below need no second call)
 *      9 bullet_lines      lines whose first non-space byte is '-' or '*', or whose first three non-space bytes are
 *                          E2 80 A2 (U+2022).  Counted at the bullet's last byte p: text[p] is '-' or '*' and nsb(p) = 0, or
 *                          text[p - 2 .. p] = E2 80 A2 and nsb(p) = 2
 *     10 ellipsis_lines    lines whose content ends in "..." or E2 80 A6.  Trailing spaces are not trimmed
 *     11 punct_lines       lines whose content's last byte is one of . ! ? "
 *     12 stop_words        word ends whose word is in the stop table
 *     13 stop_mask         bit k set iff stop word k occurs in the row
 *   and d_marks, u8[n_bytes]: bit 0 a word start, bit 1 a word end, bit 2 the end of a stop word, bit 3 the last byte of
 *   a line-leading bullet.  Every byte of both is written.  Either may be NULL, not both.
 *   The stop table is host memory, as the special tokens of tgx_corpus_split_specials are: n_stop <= 63 distinct words
 *   of 1 to 8 bytes, none holding a space byte, entry k being stop_bytes[stop_offs[k] .. stop_offs[k+1]).  n_stop = 0 is
 *   allowed (both pointers may then be NULL); statistics 12 and 13 stay 0.  Under TGX_WORDSTAT_FOLD the text's A-Z are
 *   lowered before the comparison, and only A-Z ('@' does not become '`'); an entry holding A-Z is then refused.  A word
 *   end p matches entry k of length n iff the last n bytes of (folded) tail(p) equal the entry and the byte before them
 *   (of tail, or prev when n = 8) is a space: "bathe" does not match "the".
 *   Both outputs are caller-owned device memory on the corpus's device, checked before anything is queued.  Host memory,
 *   a flag other than the two, or a bad table (an entry that is empty, longer than 8 bytes or holds a space byte, two equal
 *   entries, more than 63 entries, A-Z under TGX_WORDSTAT_FOLD): TGX_ERR_INVALID, with nothing queued or written.  Stream
 *   rule, the corpus's lock and the limit on S (S < 2^32 - 1) as tgx_corpus_text_stats_device.  S = 0 writes nothing.  The
 *   corpus is only read.
 *   The kernels lay the bytes of all rows end to end, 64 to a wave and a lane a byte, as the text statistics' do.  A first
 *   kernel writes one word per 64 bytes with two segmented states: the word that is open at the chunk's end (its units, a
 *   letter seen, a byte >= 0x80 seen; reset by a space byte or a row's first byte) and the line that is (its non-space
 *   bytes, saturated at 3; reset by a line start).  One scan turns the words into each chunk's carry, and the second
 *   kernel cuts ballots of the word ends, the line ends and what they are per row: a row inside the wave's 64 bytes gets
 *   plain stores, any other 64-bit atomic adds (max_word: an atomic maximum; stop_mask: an atomic or) onto the table,
 *   which was pre-set to 0 and which empty rows keep.  The time does not depend on the words' or the lines' lengths.
 *
 * Host twin, no device, the argument checks of tgx_text_stats_host and the table's above: tgx_word_stats_host(text, offs,
 *   n_rows, word_limit, stop_bytes, stop_offs, n_stop, flags, stats, marks) writes stats i64[TGX_WORDSTAT_N, n_rows] and
 *   marks u8[offs[n_rows]] (either may be NULL, not both).  It walks the kernel's chunks, masks, summaries, carry and
 *   store / add rule through csrc/wordstat.h.
 *
 * tgx_wordstat_last_times: device time per stage of the calling thread's last call, as tgx_textstat_last_times (the
 * names are listed without a call): wordstat_summary_kernel, wordstat_scan, wordstat_kernel (the pre-set and the
 * kernel). */
#ifndef TGX_WORDS_H
#define TGX_WORDS_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_WORDSTAT_N 14
#define TGX_WORDSTAT_CHARS 1u
#define TGX_WORDSTAT_FOLD 2u
tgx_status tgx_corpus_word_stats_device(tgx_corpus *c, uint64_t word_limit, const uint8_t *stop_bytes, const uint64_t *stop_offs,
                                        uint32_t n_stop, uint32_t flags, void *stream, int64_t *d_stats, uint8_t *d_marks);
tgx_status tgx_word_stats_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, uint64_t word_limit,
                               const uint8_t *stop_bytes, const uint64_t *stop_offs, uint32_t n_stop, uint32_t flags, int64_t *stats,
                               uint8_t *marks);
int tgx_wordstat_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_WORDS_H */
