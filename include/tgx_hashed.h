/* tgx_hashed.h: hashed n-gram features of the rows of a resident corpus or result: how many n-grams fall into each of B
 * hash buckets, and per row the sum of fixed-point weights looked up by bucket, for K weight vectors.  An addition to
 * the C ABI of tgx.h, which it includes, in a header of its own, as tgx_patterns.h and tgx_shapes.h are; the ABI version
 * stays 1.  Status codes, threading, the stream rule and last-error reporting are tgx.h's.
 *
 * ---- features over the elements of every row (csrc/hashed.hip, csrc/hashed.h) ------------------------------------------
 * The two primitives of a model over hashed n-gram features: DSIR's importance weights over hashed unigrams and bigrams,
 * a hashing-TF linear quality classifier, a multinomial naive-Bayes classifier.  FIT is counts, SCORE is scores.
 *
 * The source.  S rows, row i the elements data[offs[i] .. offs[i + 1]): a corpus's bytes (eb = 1) or a result's u32 ids
 *   (eb = 4; the word ids of tgx_corpus_words among them, so word n-grams are id n-grams).
 * The widths.  n_widths in 1 .. 4 widths w_j, ascending and distinct, each with 1 <= w_j and w_j·eb <= 64.
 * The feature.  The gram of width w at element e (a global element index) of row i is the w elements from e on, and it is
 *   VALID iff e + w <= offs[i + 1], as for tgx_*_gram_hits_device: a row shorter than w owns no gram of that width.  Its
 *   key is tgx_gram_key of its w·eb bytes (ids little-endian) under `seed`, and its bucket is
 *   tgx_hashed_bucket(key, B) = floor(key · B / 2^64), the high 64 bits of the 128-bit product.
 * The limits.  1 <= B, 1 <= K <= 16, K·B <= 2^24.
 *
 * counts[b], i64[B]: the valid grams, over all rows and all widths, whose bucket is b.
 * scores[i][k], i64[S][K]: the sum of Q[k][bucket(g)] over all valid grams g, of all widths, of row i.  Q is i32[K][B],
 *   fixed point: Q = rint(w · 2^24) with |w| < 128, so a score is its i64 times 2^-24.  The sums are exact integers and
 *   do not depend on the order of the additions: the same bits whatever the grid, in every run and on every machine.
 *   There is no floating-point variant.
 *
 * tgx_result_hashed_counts_device, tgx_corpus_hashed_counts_device(src, widths, n_widths, buckets, seed, flags, stream,
 *   d_counts) and tgx_result_hashed_scores_device, tgx_corpus_hashed_scores_device(src, widths, n_widths, buckets,
 *   n_vectors, seed, d_q, flags, stream, d_scores): widths is host memory; d_q, d_counts and d_scores are caller-owned
 *   device memory on the source's device, checked before anything is queued; flags must be 0.  The pointer checks, the
 *   stream rule, the corpus's lock and the limit on S (S < 2^32 - 1) are those of tgx_corpus_gram_hits_device.  The source
 *   and d_q are only read; every entry of the output is written, whatever it held.  S = 0 writes nothing.  A source
 *   without a valid gram gives zeros.  Widths that are none or more than 4, do not ascend or are out of range, an
 *   n_vectors outside 1 .. 16 and a B outside 1 .. 2^24 / K are TGX_ERR_INVALID, with a message that names the value and
 *   nothing written.
 *   The elements of all rows are laid end to end, 64 to a wave and a lane an element.  A lane loads the longest valid
 *   window at its element once and forms the keys of all widths from it.  Up to tgx_hashed_info's lds_max_buckets the
 *   weights (laid out [B][K'], K' = K padded to a power of two, so that a feature's weights are one wide read) or the
 *   counts' 32-bit bins live in the LDS of a block of sixteen waves; above it the kernels read the weights from memory
 *   and add to the counts in memory.  A row's lanes are contiguous: a segmented scan over the wave sums them, and the
 *   last lane of a stretch stores the sums when the row lies inside the wave's 64 elements and adds them to the pre-set
 *   zeros otherwise.
 *
 * tgx_hashed_bucket(key, buckets): the bucket of a key (0 for buckets = 0).
 * tgx_hashed_info(n_vectors, lds_max_entries, lds_max_buckets): the 32-bit entries of the LDS table, and the largest B
 *   that the LDS path serves for n_vectors vectors (n_vectors = 1: the counts too); either may be NULL.
 *
 * Host twins, no device, the same argument checks: tgx_hashed_counts_host, tgx_hashed_scores_host(data, elem_bytes, offs,
 *   n_rows, widths, n_widths, buckets, [n_vectors,] seed, [q,] out), everything in host memory.  They walk the kernels'
 *   chunks, form the keys of all widths from the longest valid window and follow the store / add rule through
 *   csrc/hashed.h and csrc/gram.h.
 *
 * tgx_hashed_last_times: device time of the calling thread's last counts call and last scores call, as
 * tgx_gram_last_times (the names are listed without a call): hashed_counts_kernel, hashed_scores_kernel, each with its
 * pre-set (and the scores' with the transposition of the weights). */
#ifndef TGX_HASHED_H
#define TGX_HASHED_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_HASHED_MAX_WIDTHS 4
#define TGX_HASHED_MAX_VECTORS 16
#define TGX_HASHED_MAX_ENTRIES (1ull << 24)
tgx_status tgx_result_hashed_counts_device(const tgx_result *r, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint64_t seed, uint32_t flags, void *stream, int64_t *d_counts);
tgx_status tgx_corpus_hashed_counts_device(tgx_corpus *c, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint64_t seed, uint32_t flags, void *stream, int64_t *d_counts);
tgx_status tgx_result_hashed_scores_device(const tgx_result *r, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors, uint64_t seed, const int32_t *d_q, uint32_t flags, void *stream, int64_t *d_scores);
tgx_status tgx_corpus_hashed_scores_device(tgx_corpus *c, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors, uint64_t seed, const int32_t *d_q, uint32_t flags, void *stream, int64_t *d_scores);
uint64_t tgx_hashed_bucket(uint64_t key, uint64_t buckets);
tgx_status tgx_hashed_info(uint32_t n_vectors, uint64_t *lds_max_entries, uint64_t *lds_max_buckets);
tgx_status tgx_hashed_counts_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint64_t seed, int64_t *counts);
tgx_status tgx_hashed_scores_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, const uint32_t *widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors, uint64_t seed, const int32_t *q, int64_t *scores);
int tgx_hashed_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_HASHED_H */
