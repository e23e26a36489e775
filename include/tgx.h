/*
 * tgx.h — C ABI of the MI355X-native TokenGeeX Unigram encode / E-step path.
 *
 * This is the drop-in boundary: a Rust `extern "C"` block, a
 * C++ host or Python/ctypes bind exactly these symbols.  Plain pointers and
 * sizes only; no exceptions or unwinding cross it; every function returns a
 * tgx_status.  All reference citations are relative to the TokenGeeX source tree.
 *
 * Batch format (replaces Vec<&str> / &[&str] of the reference's batch loops):
 *   text  : uint8_t[N]      all samples' bytes back to back (already processed
 *                           by the tokenizer's processors, as in cli.rs:276-287)
 *   offs  : uint64_t[S+1]   sample i = text[offs[i] .. offs[i+1])
 * Result format (replaces Vec<Vec<u32>>):
 *   ids   : uint32_t[T]     token ids of all samples back to back
 *   ooffs : uint64_t[S+1]   sample i's ids = ids[ooffs[i] .. ooffs[i+1])
 *
 * The library fails loudly (TGX_ERR_DEVICE) when no gfx950 device is usable;
 * there is no CPU fallback behind these entry points.
 */
#ifndef TGX_H
#define TGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGX_ABI_VERSION 1

/* tokengeex::Error — src/lib.rs:219-224 (+ build-specific codes >= 5) */
typedef enum tgx_status {
    TGX_OK = 0,
    TGX_ERR_IO = 1,                 /* Error::IO                                   */
    TGX_ERR_JSON = 2,               /* Error::SerdeJSON                            */
    TGX_ERR_TOKEN_ID_OOB = 3,       /* Error::TokenIdOutOfBounds(id)               */
    TGX_ERR_NO_PATH = 4,            /* Error::NoPath(pos, len), src/model.rs:119   */
    TGX_ERR_DEVICE = 5,             /* HIP runtime / no GPU / kernel failure       */
    TGX_ERR_Z_NOT_NORMAL = 6,       /* the panic at src/prune.rs:90-96             */
    TGX_ERR_INVALID = 7,            /* bad argument                                */
    TGX_ERR_UNSUPPORTED = 8         /* e.g. a token longer than TGX_MAX_TOKEN_LEN  */
} tgx_status;

/* Longest vocabulary token (bytes) the device lattice handles.  The reference's
 * recipes use 16 (README.md:161) to 24 (cli.rs:723). */
#define TGX_MAX_TOKEN_LEN 64

/* E-step snippet length: const MAX_SAMPLE_LENGTH = 8192 * 10, src/prune.rs:75 */
#define TGX_ESTEP_SNIPPET_LEN 81920

typedef struct tgx_model tgx_model;   /* Model: vocab + trie, src/model.rs:8-12   */
typedef struct tgx_corpus tgx_corpus; /* a packed batch resident in HBM            */
typedef struct tgx_result tgx_result; /* ids + offsets of one encode pass          */

/* ---- error reporting ----------------------------------------------------- */
/* Message of the last failure on the calling thread, formatted like the
 * reference's Display impl (src/lib.rs:238-249), e.g.
 * "no path to position 12/12", "token id 7 is out of bounds". */
const char *tgx_last_error(void);
/* Details of the last TGX_ERR_NO_PATH / TGX_ERR_Z_NOT_NORMAL: the LOWEST failing
 * sample index (the reference leaves it unspecified, src/tokenizer.rs:107-110),
 * and (pos, len) of Error::NoPath. */
void tgx_last_error_detail(uint64_t *sample, uint64_t *pos, uint64_t *len);
int tgx_abi_version(void);
/* Number of usable gfx950 devices (0 when none; never fails). */
int tgx_device_count(void);

/* ---- Model ---------------------------------------------------------------- */
/* Model::from(vocab) — src/model.rs:16-30.  Token i = bytes[offs[i]..offs[i+1]),
 * id = i, scores[i] = vocab[i].score passed as raw f64 (never re-parsed).
 * Later duplicates overwrite earlier ones (src/trie.rs:19); empty tokens never
 * match (src/trie.rs:53-61).  Flattens the byte trie into an XOR double-array in
 * HBM on `device`.  The handle is immutable and may be used concurrently; mutation
 * = build a new handle (as `*model = Model::from(vocab)`, src/prune.rs:48,53). */
tgx_status tgx_model_create(const uint8_t *bytes, const uint64_t *offs, const double *scores,
                            uint32_t vocab_size, int device, tgx_model **out);
/* As tgx_model_create; flags: TGX_MODEL_FOR_ESTEP builds the tables of the E-step's backward sweep on a second
 * host thread during creation instead of at the first tgx_estep call (Model::from is rebuilt for every EM
 * sub-iteration, src/prune.rs:48). */
#define TGX_MODEL_FOR_ESTEP 1u
tgx_status tgx_model_create_ex(const uint8_t *bytes, const uint64_t *offs, const double *scores,
                               uint32_t vocab_size, int device, uint32_t flags, tgx_model **out);

/* A model for a SUBSET of `parent`'s vocabulary (keep_ids: ascending ids of the parent's tokens; the new id of a token
 * is its position in keep_ids) with new scores, on the parent's double-arrays: nothing is rebuilt, the tokens that are
 * gone lose their terminal marks — a trie with dead branches gives the same matches.  What `prune` needs three times
 * per iteration (src/prune.rs:36-56: a model per EM sub-iteration and one for the pruning step, each a subset of the one
 * before).  Same flags as tgx_model_create_ex; the parent stays valid.  TGX_ERR_UNSUPPORTED when the parent's vocabulary
 * has duplicate tokens (build the model with tgx_model_create_ex then). */
tgx_status tgx_model_create_derived(const tgx_model *parent, const uint32_t *keep_ids, uint32_t n_keep,
                                    const double *scores, uint32_t flags, tgx_model **out);
void tgx_model_destroy(tgx_model *m);
uint32_t tgx_model_vocab_size(const tgx_model *m);     /* Model::vocab_size, src/model.rs:179 */
uint32_t tgx_model_max_token_len(const tgx_model *m);
uint64_t tgx_model_trie_bytes(const tgx_model *m);     /* size of the device table */
int tgx_model_device(const tgx_model *m);

/* Model::common_prefix_search — src/model.rs:132-138 / src/trie.rs:44-64 (host
 * twin of the device walk over the same flattened table).  Writes up to cap
 * (id, len) pairs in ascending length; *count = number found. */
tgx_status tgx_common_prefix_search(const tgx_model *m, const uint8_t *s, uint64_t n,
                                    uint32_t *ids, uint32_t *lens, uint64_t cap, uint64_t *count);

/* ---- Tokenizer front and back over packed buffers (host code, no device; csrc/frontback.cpp) ----------
 * The reference runs these per sample on its rayon workers: the special-token splitter
 * (src/tokenizer.rs:299-347), CrlfProcessor::preprocess (src/processor.rs:46-54), the assembly of a
 * sample's ids from its segments (src/tokenizer.rs:65-90) and decode_batch (src/tokenizer.rs:126-187 over
 * src/model.rs:146-160, String::from_utf8_lossy per run of base ids).  Strings cross as UTF-8 bytes +
 * u64 offsets.  Arrays returned through pointer-to-pointer arguments are malloc'd: tgx_free. */
tgx_status tgx_split_specials(const uint8_t *text, const uint64_t *offs, uint64_t n_samples,
                              const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                              uint64_t *seg_offs, uint64_t **seg_begin, uint64_t **seg_end,
                              int32_t **seg_special, uint64_t *n_segments);
tgx_status tgx_pack_segments(const uint8_t *text, const uint64_t *seg_begin, const uint64_t *seg_end,
                             const int32_t *seg_special, uint64_t n, int crlf, uint8_t *out_text,
                             uint64_t *out_offs, uint64_t *n_out);
/* UnicodeProcessor::preprocess (src/processor.rs:124-137) over packed segments: form 0 NFD, 1 NFC, 2 NFKD, 3 NFKC (UAX #15;
 * tables of Unicode tgx_unidata_version()).  Bytes that are not UTF-8 pass through unchanged.  out_text / out_offs are
 * malloc'd (tgx_free): n_segs segments back to back, offsets u64[n_segs + 1]. */
tgx_status tgx_normalize_segments(uint32_t form, const uint8_t *text, const uint64_t *seg_begin, const uint64_t *seg_end,
                                  uint64_t n_segs, uint8_t **out_text, uint64_t **out_offs);
const char *tgx_unidata_version(void);
tgx_status tgx_assemble_ids(const uint64_t *seg_offs, const int32_t *seg_special, uint64_t n_samples,
                            const uint32_t *ids, const uint64_t *id_offs, uint32_t vocab_size,
                            uint32_t *out_ids, uint64_t *out_offs);
tgx_status tgx_decode_batch(const uint8_t *vocab_bytes, const uint64_t *vocab_offs, uint32_t vocab_size,
                            const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                            const uint32_t *ids, const uint64_t *id_offs, uint64_t n_samples,
                            int include_special, uint8_t **out_text, uint64_t *out_offs,
                            uint64_t *bad_sample, uint64_t *bad_id);
uint64_t tgx_utf8_lossy(const uint8_t *s, uint64_t n, uint8_t *out);

/* ---- `generate`: document frequencies of substrings on the device (csrc/generate.hip) ----------------
 * VocabularyGenerator::feed (src/generate.rs:54-139): in how many samples does every char-aligned substring of
 * at most max_token_length (<= 32) bytes occur?  Parts are the byte ranges the windows may lie in (the samples,
 * or the matches of the split regex), sorted, disjoint, with ascending sample ids; part_origin[k] = where the part's
 * sample begins in `text` (NULL: every part is a sample of its own).  Every OCCURRENCE is kept with probability
 * insert_probability, as in the reference's loops (src/generate.rs:84-89, 108-113; a substring with k occurrences in a
 * sample counts for it with probability 1 - (1 - p)^k): occurrence (sample, offset o in the sample, length l) is kept iff
 * tgx_generate_u01(seed, sample, o << 8 | l) < insert_probability (the reference draws from an unseeded thread RNG).  Out: one entry per distinct substring — position and length of one occurrence, number
 * of samples — malloc'd (tgx_free).  Two different substrings in one 64-bit sort key are detected (every entry of a run is
 * compared with the run's first, byte by byte) and resolved: the pass is sorted again under a second, independent hash of
 * the windows' bytes (up to three times; *n_collisions = entries that had met a foreign run in the discarded attempts).
 * More than 2^32 - 1 kept windows in one call: TGX_ERR_UNSUPPORTED ("feed smaller batches"). */
tgx_status tgx_substring_df(int device, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_begin,
                            const uint64_t *part_end, const uint32_t *part_sample, const uint64_t *part_origin, uint64_t n_parts,
                            uint32_t max_token_length, double insert_probability, uint64_t seed,
                            uint64_t **out_pos, uint32_t **out_len, uint32_t **out_df, uint64_t *n_out,
                            uint64_t *n_windows, uint64_t *n_collisions);
/* The same with only the top_k most frequent substrings leaving the device, in descending frequency (top_k = 0:
 * all): VocabularyGenerator::generate keeps the most frequent substrings (src/generate.rs:150-152, 199-213), and
 * copying every distinct substring of a corpus to the host (254 M for 64 MiB of text) is what bounded `feed`.
 * *n_distinct = distinct substrings counted; *cutoff_df = the frequency of the most frequent substring NOT
 * returned (0 when nothing was cut): whatever is missing from the output occurs in at most that many samples. */
tgx_status tgx_substring_df_top(int device, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_begin,
                                const uint64_t *part_end, const uint32_t *part_sample, const uint64_t *part_origin, uint64_t n_parts,
                                uint32_t max_token_length, double insert_probability, uint64_t seed,
                                uint64_t top_k, uint64_t **out_pos, uint32_t **out_len, uint32_t **out_df,
                                uint64_t *n_out, uint64_t *n_windows, uint64_t *n_collisions,
                                uint64_t *n_distinct, uint32_t *cutoff_df);
double tgx_generate_u01(uint64_t seed, uint64_t sample, uint64_t window_hash);

/* ---- host-only trie introspection (no device needed) ------------------------
 * The same flattening tgx_model_create uploads, built on the host alone, so that
 * the layout can be validated (and inspected) on machines without a GPU. */
typedef struct tgx_flat_trie tgx_flat_trie;
tgx_status tgx_flat_trie_build(const uint8_t *bytes, const uint64_t *offs, const double *scores,
                               uint32_t vocab_size, tgx_flat_trie **out);
void tgx_flat_trie_free(tgx_flat_trie *t);
/* as tgx_common_prefix_search; returns the number of matches */
uint64_t tgx_flat_trie_search(const tgx_flat_trie *t, const uint8_t *s, uint64_t n, uint32_t *ids,
                              uint32_t *lens, uint64_t cap);
void tgx_flat_trie_stats(const tgx_flat_trie *t, uint64_t *n_slots, uint64_t *n_nodes,
                         uint32_t *max_token_len);
/* The same search over the 8-byte label-checked records encode5_kernel walks (built from the same slot
 * assignment: the walk keeps only the record and compares its label with the text byte), plus figures of the
 * score table for a copy of max_hot values in LDS: *n_hot = values in that copy (ranks 1..n_hot of the
 * vocabulary's distinct score values), *n_cold terminal slots whose value is outside it (read from HBM / L2 by
 * the kernels), *hot_coverage the expected share of matches the copy serves.  Any out pointer may be NULL.
 * Returns the number of matches, or UINT64_MAX when the records cannot be built (more than 65 535 distinct
 * score values, or more than 2^21 slots). */
uint64_t tgx_flat_trie_search8(const tgx_flat_trie *t, const uint8_t *bytes, const uint64_t *offs,
                               const double *scores, uint32_t max_hot, const uint8_t *s, uint64_t n,
                               uint32_t *ids, uint32_t *lens, uint64_t cap, uint32_t *n_hot,
                               uint64_t *n_cold, double *hot_coverage);
/* copies the slot table: check[n_slots], base_flags[n_slots] (bit 31 = terminal), tokid[n_slots] */
void tgx_flat_trie_copy(const tgx_flat_trie *t, uint32_t *check, uint32_t *base_flags, uint32_t *tokid);
/* Builds the token-bytes -> id table the trace kernel probes and looks every token up again through it
 * (host only).  TGX_OK and *mismatches == 0 when every token of <= 32 bytes maps back to the id the trie
 * gives it; TGX_ERR_UNSUPPORTED when the table cannot be built (a token longer than 32 bytes, or no
 * collision-free seed) — the model then keeps the one-sample-per-wave kernel. */
tgx_status tgx_tok_hash_selftest(const uint8_t *bytes, const uint64_t *offs, uint32_t vocab_size,
                                 uint32_t *seed, uint64_t *mismatches);
/* out-of-line copy of tgx_dropout_u01 (below) for bindings that cannot inline C */
double tgx_dropout_u01_host(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len);

/* ---- encode: Tokenizer::encode_ordinary_batch / the rayon loop ----------- */
/* src/tokenizer.rs:102-123 over src/model.rs:59-129.  Host buffers in, result
 * handle out (host-readable).  dropout/seed: see tgx_dropout_u01.  On
 * TGX_ERR_NO_PATH *out is NULL and tgx_last_error_detail names the sample. */
tgx_status tgx_encode_batch(tgx_model *m, const uint8_t *text, const uint64_t *offs,
                            uint64_t n_samples, double dropout, uint64_t seed, tgx_result **out);
/* The same with host buffers on both sides: the ids are written to ids_out (room for ids_cap entries; the
 * number of bytes of the batch always suffices) and the exclusive token offsets to offs_out[n_samples + 1].
 * Large batches are cut at sample boundaries into chunks that go through three stages — upload, kernels,
 * download — on three host threads and two copy streams, so the link works in both directions beside the kernels.  Errors as tgx_encode_batch (the lowest failing sample of the batch is reported). */
tgx_status tgx_encode_batch_host(tgx_model *m, const uint8_t *text, const uint64_t *offs, uint64_t n_samples,
                                 double dropout, uint64_t seed, uint32_t *ids_out, uint64_t ids_cap,
                                 uint64_t *offs_out, uint64_t *n_tokens);

/* The same from ONE host process over SEVERAL devices: `models` holds one handle per GPU (tgx_model_create with
 * device = 0 .. n - 1, the same vocabulary), the batch is cut at sample boundaries into byte-balanced shards, every shard
 * runs tgx_encode_batch_host on a host thread of its own, and ids / offsets come back packed in sample order — what the
 * reference's single-call batch (src/tokenizer.rs:102-111) becomes on a node with several GPUs.  No collective.
 * ids_out must hold one id per input byte (ids_cap >= bytes).  With dropout > 0 the keep decisions hash a sample's index
 * in its shard.  The lowest failing sample of the batch is reported. */
tgx_status tgx_encode_batch_multi(tgx_model *const *models, uint32_t n_models, const uint8_t *text, const uint64_t *offs,
                                  uint64_t n_samples, double dropout, uint64_t seed, uint32_t *ids_out, uint64_t ids_cap,
                                  uint64_t *offs_out, uint64_t *n_tokens);

uint64_t tgx_result_num_samples(const tgx_result *r);
uint64_t tgx_result_num_tokens(const tgx_result *r);
/* Host pointers (copied from the device on first use); valid until tgx_result_free. */
const uint32_t *tgx_result_ids(tgx_result *r);
const uint64_t *tgx_result_offsets(tgx_result *r);
/* The same arrays copied from the device straight into caller-owned memory (a binding's Vec<u32> / numpy
 * array: no intermediate host copy); `cap` = elements available at dst, at least num_tokens resp.
 * num_samples + 1, else TGX_ERR_INVALID. */
tgx_status tgx_result_copy_ids(const tgx_result *r, uint32_t *dst, uint64_t cap);
tgx_status tgx_result_copy_offsets(const tgx_result *r, uint64_t *dst, uint64_t cap);
/* Device pointers of the same arrays (for callers that keep ids in HBM). */
const void *tgx_result_ids_device(const tgx_result *r);
const void *tgx_result_offsets_device(const tgx_result *r);
void tgx_result_free(tgx_result *r);
/* The device the result's arrays live on. */
int tgx_result_device(const tgx_result *r);
/* Every id of the result is below it: the vocabulary size of the model that wrote it (plus the number of special
 * tokens for the result of tgx_assemble_result). */
uint32_t tgx_result_vocab_size(const tgx_result *r);

/* ---- layouts for a model: the ids of a result as padded rows or packed blocks, written on the device ----------
 * A result of encode, sampling or n-best (n-best rows are just rows) laid out in caller-owned DEVICE memory, e.g. a
 * torch tensor's data_ptr(), by the kernels of csrc/layout.hip: the ids never visit the host.  Row i has the tokens
 * t_i[0..n_i), n_i = ooffs[i+1] - ooffs[i].  bos_id / eos_id: TGX_NO_ID = none; A = how many of the two are present.
 * Every id written, pad_id included, must be below 2^31 (TGX_ERR_INVALID otherwise).  Elements are int32_t, or
 * int64_t with TGX_LAYOUT_I64.  All element indices are 64-bit.
 *
 * Padded, row_len = L (L >= 1 and L >= A, else TGX_ERR_INVALID): keep_i = min(n_i, L - A) tokens are kept, the first
 *   keep_i, or the last keep_i with TGX_LAYOUT_TRUNC_LEFT; seq_i = [bos] + kept + [eos], len_i = keep_i + A;
 *   out[i, 0:len_i] = seq_i and the rest of the row is pad_id, or out[i, L-len_i:L] = seq_i with TGX_LAYOUT_PAD_LEFT.
 *   d_mask (NULL or u8[S·L]): 1 on seq_i, 0 on padding.  d_lengths (NULL or i32[S]): len_i.  *n_truncated (NULL or
 *   host): rows with n_i > L - A.  S = 0 writes nothing.
 * Packed, block_len = L >= 1: the rows' sequences [bos] + t_i + [eos] back to back; row i starts at stream position
 *   P_i = ooffs[i] + i·A, n_stream = T + S·A, *n_blocks = ceil(n_stream / L) (0 for an empty stream) and n_blocks·L
 *   elements are written: position j < n_stream belongs to the row i with P_i <= j < P_{i+1} (rows with n_i = 0 and
 *   A = 0 own no position), d_doc[j] = i and d_pos[j] = j - P_i (each NULL or i32[n_blocks·L]); in the tail of the
 *   last block ids = pad_id, doc = -1, pos = 0.  2^31 rows or more: TGX_ERR_UNSUPPORTED.
 * tgx_result_layout_info sizes the destinations: *max_row_len = max_i n_i + A (A when S = 0; a device reduction, one
 *   word is read back), *n_stream as above.  Either out pointer may be NULL.  The reduction runs on the library's
 *   stream (see below), so it also waits for work queued earlier on the device's null stream although it reads the
 *   result's offsets only: a cost in time, not a dependency.  It is skipped when max_row_len is NULL.
 *
 * stream is a hipStream_t: pass the stream the destination's allocator orders its memory on (torch's current
 * stream); NULL selects a stream of the library.  That one is a blocking stream (hipStreamDefault): its work starts
 * after everything queued earlier on the device's null stream, so NULL is also right for a caller whose stream IS the
 * null stream, whose handle is 0 (torch's default stream).  The work is queued on the chosen stream and the call
 * returns only after the stream has reached its end.  Two rules rest on this: a caching allocator may hand out a
 * block that work still queued on its stream reads, so writing it from an unordered stream would race; and the result
 * may be freed, and its pooled buffers reused, as soon as the call returns.  The destinations must be device memory on
 * the result's device (checked with hipPointerGetAttributes: TGX_ERR_INVALID otherwise).  Only where a destination
 * lies can be checked, not how large it is: room for every element written (S·row_len ids and mask bytes, S lengths;
 * n_blocks·block_len ids, docs and positions) is the caller's responsibility.  NULL arguments are refused before any
 * device call.  The calling thread's current device is the same after the call as before. */
#define TGX_NO_ID 0xFFFFFFFFu
#define TGX_LAYOUT_PAD_LEFT 1u
#define TGX_LAYOUT_TRUNC_LEFT 2u
#define TGX_LAYOUT_I64 4u
tgx_status tgx_result_layout_info(const tgx_result *r, uint32_t bos_id, uint32_t eos_id,
                                  uint64_t *max_row_len, uint64_t *n_stream);
tgx_status tgx_result_pad_device(const tgx_result *r, uint32_t row_len, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id,
                                 uint32_t flags, void *stream, void *d_ids, uint8_t *d_mask, int32_t *d_lengths,
                                 uint64_t *n_truncated);
tgx_status tgx_result_pack_device(const tgx_result *r, uint32_t block_len, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id,
                                  uint32_t flags, void *stream, void *d_ids, int32_t *d_doc, int32_t *d_pos, uint64_t *n_blocks);
/* Host twins over host arrays (ids u32[T], may be NULL when T = 0; offs u64[n_rows + 1], offs[0] = 0, ascending):
 * the same semantics through the same row mapping (csrc/layout.h), no device — for callers of tgx_encode_batch_host
 * and for validation on machines without a GPU.  Here every id of `ids` that is written is checked against 2^31.
 * The packed form writes ceil((T + n_rows·A) / block_len) · block_len elements. */
tgx_status tgx_layout_pad_host(const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t row_len, uint32_t pad_id,
                               uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *out_ids, uint8_t *out_mask,
                               int32_t *out_lengths, uint64_t *n_truncated);
tgx_status tgx_layout_pack_host(const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t block_len, uint32_t pad_id,
                                uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *out_ids, int32_t *out_doc,
                                int32_t *out_pos, uint64_t *n_blocks);

/* ---- overflow windows: a row longer than row_len as overlapping [W, L] windows, written on the device ------------
 * What truncation with a stride and "return overflowing tokens" give: every token of a long row, in windows of row_len
 * elements that each repeat `stride` tokens of the window before, each tagged with the row it came from.  Kernels of
 * csrc/layout.hip over the window mapping of csrc/layout.h; ids, flags, elements and the stream rule as in the layouts
 * above.
 *
 * With row_len = L and A as above: room = L - A tokens per window, step = room - stride.  L >= A + 1 and
 *   0 <= stride < room, else TGX_ERR_INVALID before anything is queued.
 * Row i with n_i tokens has nw_i = 1 windows if n_i <= room, else 1 + ceil((n_i - room) / step): an empty row is one
 *   window of padding.  Windows are ordered by row, then by k = 0 .. nw_i - 1: Wo[i] = the exclusive prefix sum of nw,
 *   W = Wo[S]; window w belongs to the largest i with Wo[i] <= w, and k = w - Wo[i].
 * Window k keeps the row's tokens [k·step, min(n_i, k·step + room)); with TGX_LAYOUT_TRUNC_LEFT the windows run from the
 *   row's end: tokens [n_i - min(n_i, k·step + room), n_i - k·step).  first_w = the first kept index, keep_w the count.
 * Row w of out[W, L] holds [bos] + kept + [eos], len_w = keep_w + A elements, at its start, or at its end with
 *   TGX_LAYOUT_PAD_LEFT; the rest of the row is pad_id.  d_mask (NULL or u8[W·L]): 1 on the sequence, 0 on padding.
 *   d_lengths (NULL or i32[W]): len_w.  d_window_row (NULL or i32[W]): i, the overflow-to-sample mapping.
 *   d_window_first (NULL or i32[W]): first_w.
 * So window 0 of row i is row i of the padded form, and when no row is longer than room, W = S and every output equals
 *   that of tgx_result_pad_device / tgx_result_pad_spans_device for the same arguments.
 * tgx_result_window_spans_device writes d_spans[W, L, 2], aligned element for element with the ids: a kept token gets
 *   exactly the span tgx_result_spans_device gives it, relative to its whole row's text (bytes, or TGX_SPAN_CHARS), so
 *   the pairs index the sample; bos, eos and padding get (0, 0).  Model, specials, units and the int32 rule for a row's
 *   total are those of the spans section below.
 * tgx_result_window_info gives *n_windows = W for sizing the destinations: a count kernel, a scan over the S rows and
 *   one read-back, on the library's stream.  The other two calls take the W the caller sized its buffers for as
 *   n_windows, compute W again (nothing is kept on the result) and return TGX_ERR_INVALID, with nothing written, when
 *   the two differ.  W >= 2^31, or a row of 2^31 tokens or more: TGX_ERR_UNSUPPORTED, nothing written.  S = 0: W = 0,
 *   TGX_OK, nothing written.
 * Host twins (tgx_layout_windows_host, tgx_window_spans_host; arrays as for the twins above and tgx_spans_host): the
 *   same semantics through the same window mapping, no device.  They first compute W and store it to *n_windows_out;
 *   with out_ids / out NULL that is all they do.  Otherwise n_windows must equal W as above. */
tgx_status tgx_result_window_info(const tgx_result *r, uint32_t row_len, uint32_t stride, uint32_t bos_id, uint32_t eos_id,
                                  uint32_t flags, uint64_t *n_windows);
tgx_status tgx_result_window_pad_device(const tgx_result *r, uint32_t row_len, uint32_t stride, uint32_t pad_id,
                                        uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *stream, uint64_t n_windows,
                                        void *d_ids, uint8_t *d_mask, int32_t *d_lengths, int32_t *d_window_row,
                                        int32_t *d_window_first);
tgx_status tgx_result_window_spans_device(tgx_model *m, const tgx_result *r, const uint8_t *special_bytes,
                                          const uint64_t *special_offs, uint32_t n_specials, uint32_t row_len,
                                          uint32_t stride, uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *stream,
                                          uint64_t n_windows, void *d_spans);
tgx_status tgx_layout_windows_host(const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t row_len,
                                   uint32_t stride, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id, uint32_t flags,
                                   uint64_t n_windows, void *out_ids, uint8_t *out_mask, int32_t *out_lengths,
                                   int32_t *out_window_row, int32_t *out_window_first, uint64_t *n_windows_out);
tgx_status tgx_window_spans_host(const uint8_t *vocab_bytes, const uint64_t *vocab_offs, uint32_t vocab_size,
                                 const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                                 const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t row_len,
                                 uint32_t stride, uint32_t bos_id, uint32_t eos_id, uint32_t flags, uint64_t n_windows,
                                 void *out, uint64_t *n_windows_out);

/* ---- assembly: a sample-level result with the special tokens' ids, put together on the device ----------------
 * The special-aware encode (Tokenizer::encode_batch, src/tokenizer.rs:65-90) splits every sample at its special tokens,
 * encodes the segments between them and concatenates, per sample, the special tokens' ids and the segments' ids.
 * tgx_assemble_ids does the last step on host arrays; tgx_assemble_result does it in HBM (csrc/assemble.hip), so that
 * the ids of a batch with special tokens reach the layouts above without visiting the host.
 *   A model with base vocabulary size V.
 *   segs: a result over E rows with T ids and offsets o[0..E] — the encode or sampling result over the non-special
 *     segments, in order.
 *   seg_offs u64[S+1]: sample i owns segments [seg_offs[i], seg_offs[i+1]); K = seg_offs[S].
 *   seg_special i32[K]: a value >= 0 is an index into the special tokens, any negative value means "the next encoded
 *     segment" (what tgx_split_specials returns).  n_specials: the number of special tokens.
 * Let enc(k) = seg_special[k] < 0 and r_k = the number of k' < k with enc(k'); r_K must equal E.  Segment k starts at
 * output position D_k = o[r_k] + (k - r_k); D_K = T + (K - E) = T'.  Then
 *   out_offs[i] = D_{seg_offs[i]} for i = 0..S, and
 *   for D_k <= j < D_{k+1}: out_ids[j] = enc(k) ? ids[o[r_k] + (j - D_k)] : V + seg_special[k].
 * An encoded segment with no ids, and a sample with no segments, own no position.  This is what tgx_assemble_ids
 * computes.  All element and segment indices are 64-bit.
 *
 * tgx_assemble_result runs on the model's stream, uploads the two host arrays, and returns after the stream has
 * reached its end: *out has n_samples = S rows, T' ids, vocabulary size V + n_specials (what the layouts check ids
 * against) and lives on the model's device; every entry point that takes a result takes it.  segs is only read and
 * stays valid; the caller frees both results.  tgx_last_kernel_times reports the stage's kernels.  TGX_ERR_INVALID,
 * before anything is launched: seg_offs[0] != 0 or seg_offs not non-decreasing; a special index >= n_specials; the
 * number of encoded segments differs from segs' row count (so an n-best result, which has n_samples · nbest rows, is
 * refused: combining n-best rows across segments stays with the caller); segs is NULL although E > 0 (segs is NULL
 * iff E == 0; a result without rows is accepted too); segs is on another device or was written by a model with a
 * different vocabulary size; V + n_specials > 0xFFFFFFFE.  S = 0 gives TGX_OK and an empty result with offsets [0].
 * tgx_assemble_host is the host twin over host arrays (ids may be NULL when T = 0, id_offs when n_encoded = 0): the
 * same checks, plus id_offs[0] = 0 and ascending, and ids_cap >= T'; no device — it walks the kernel's tiles through
 * the same index arithmetic (csrc/assemble.h).  out_offs u64[S+1]. */
tgx_status tgx_assemble_result(tgx_model *m, const tgx_result *segs, const uint64_t *seg_offs, const int32_t *seg_special,
                               uint64_t n_samples, uint32_t n_specials, tgx_result **out);
tgx_status tgx_assemble_host(const uint32_t *ids, const uint64_t *id_offs, uint64_t n_encoded,
                             const uint64_t *seg_offs, const int32_t *seg_special, uint64_t n_samples,
                             uint32_t vocab_size, uint32_t n_specials,
                             uint32_t *out_ids, uint64_t ids_cap, uint64_t *out_offs);

/* ---- fill-in-the-middle on the device: PSM / SPM rows from a result (csrc/fim.hip) ---------------------------------
 * Code LMs are trained on documents whose tokens are cut into prefix, middle and suffix and re-ordered behind three
 * sentinels (Bavarian et al. 2022, "Efficient Training of Language Models to Fill in the Middle"): PSM is prefix,
 * suffix, middle and SPM suffix, prefix, middle.  tgx_result_fim does that to the rows of a result in HBM, between
 * encode (or the assembly above) and the layouts, so the ids do not visit the host.
 *
 * In: a result r with S rows, row i with the tokens t_i[0..n_i); three pairwise distinct sentinel ids PRE, SUF, MID
 * (prefix_id, suffix_id, middle_id); rate and spm_rate in [0, 1]; seed; first_row.
 *
 * The uniform.  tgx_fim_u01(seed, row, draw): x = seed ^ TGX_FIM_SALT ^ row·0x9E3779B97F4A7C15 ^
 * draw·0xC2B2AE3D27D4EB4F, the three xor-shift / multiply rounds of tgx_dropout_u01, u = (x >> 11) · 2^-53 in f64, so u
 * lies in [0, 1).
 *
 * Row i, with g = first_row + i (all arithmetic on g wraps at 2^64):
 *   The row is REARRANGED iff n_i >= 1 and u01(seed, g, 0) < rate: rate = 0 rearranges nothing, rate = 1 every
 *     non-empty row.
 *   A rearranged row is SPM iff u01(seed, g, 1) < spm_rate, otherwise PSM.
 *   The cuts are c_d = min(n_i, (uint64_t)(u01(seed, g, d) · (double)(n_i + 1))) for d = 2, 3; a = min(c_2, c_3),
 *     b = max(c_2, c_3).  The multiplication and the conversion are the plain IEEE f64 operations, so host and device
 *     agree bit for bit; the clamp is there because the product can round up to n_i + 1.
 *   prefix = t[0:a), middle = t[a:b), suffix = t[b:n_i); any of them may be empty.
 *   A PSM row is  PRE prefix SUF suffix MID middle,  an SPM row  PRE SUF suffix MID prefix middle:  n_i + 3 tokens.
 *   A row that is not rearranged is copied.
 * first_row makes a shard of a larger batch draw what the whole batch draws: rows [k, S) with first_row = k give the
 * tail of what all rows give with first_row = 0.
 *
 * Out: a new result with S rows, T' = T + 3 · n_applied ids and offsets from 0, on r's device, whose vocabulary size is
 * max(tgx_result_vocab_size(r), 1 + max(PRE, SUF, MID)) — so a result of ordinary encoding, whose ids are all below V,
 * takes sentinels at V + k.  r is only read and stays valid; the caller frees both.  Every entry point that takes a
 * result takes the new one.  An n-best result is accepted: its rows are rows.  S = 0 gives an empty result with
 * offsets [0].  Optional host outputs: mode (NULL or u8[S]): 0 copied, 1 PSM, 2 SPM; cuts (NULL or u64[2S]): a and b,
 * (0, 0) for a copied row; n_applied (NULL or u64*).
 *
 * TGX_ERR_INVALID, before anything is queued: r or out NULL; rate or spm_rate NaN or outside [0, 1]; a sentinel equal
 * to TGX_NO_ID; two equal sentinels.  No model is needed.  stream: as in the layouts above — the work is queued on it
 * (NULL: the library's stream) and the call returns only after the stream has reached its end.  One word visits the
 * host in between: T', the last of the new offsets, which sizes the id buffer.  The calling thread's current device is
 * the same after the call as before.
 *
 * tgx_fim_host is the host twin over host arrays (ids u32[T], may be NULL when T = 0; offs u64[n_rows + 1]): the same
 * checks, plus offs[0] = 0 and ascending, every id below vocab_size, vocab_size <= 0xFFFFFFFE and ids_cap >= T'; no
 * device — it walks the kernel's tiles and thread slots through the same index arithmetic (csrc/fim.h).  out_offs
 * u64[n_rows + 1]; out_ids may be NULL when T' = 0.
 *
 * tgx_result_from_ids makes a result on `device` from host arrays: pre-tokenised corpora are what fill-in-the-middle is
 * most often applied to, and the layouts and decode become usable on ids that came from elsewhere.  It is checked on
 * the host as the twin checks its input (TGX_ERR_INVALID); the arrays are copied, the caller keeps its own.
 *
 * tgx_fim_last_times: device time of the calling thread's last tgx_result_fim per stage (the offsets' scan, fim_fill_kernel,
 * fim_info_kernel), as tgx_front_last_times; for tools/fim_bench.py. */
#define TGX_FIM_SALT 0xA0761D6478BD642FULL
int tgx_fim_last_times(const char **names, float *ms, int cap);
double tgx_fim_u01(uint64_t seed, uint64_t row, uint64_t draw);
tgx_status tgx_result_fim(const tgx_result *r, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id, double rate,
                          double spm_rate, uint64_t seed, uint64_t first_row, void *stream, uint8_t *mode, uint64_t *cuts,
                          uint64_t *n_applied, tgx_result **out);
tgx_status tgx_fim_host(const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t vocab_size,
                        uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id, double rate, double spm_rate,
                        uint64_t seed, uint64_t first_row, uint32_t *out_ids, uint64_t ids_cap, uint64_t *out_offs,
                        uint8_t *mode, uint64_t *cuts, uint64_t *n_applied);
tgx_status tgx_result_from_ids(int device, const uint32_t *ids, const uint64_t *offs, uint64_t n_rows,
                               uint32_t vocab_size, tgx_result **out);

/* ---- rows selected and reordered on the device: of a result or of a corpus (csrc/select.hip) ------------------------
 * A resident result or corpus is otherwise consumed whole and in the order it was produced.  A new document order per
 * epoch, dropping rows (length or quality filters) and taking some rows (a mini-batch, a split, length-grouped batches)
 * are one primitive: a new result (or corpus) whose row k is row rows[k] of the old one — any order, any subset,
 * repeats allowed.  The indices come from anywhere (torch's argsort, nonzero or masks on the device; the seeded
 * permutation below); moving the ragged rows through them happens in HBM.
 *
 * tgx_result_select(r, rows, M, flags, stream, &out).  In: a result r with S rows, T ids and offsets o[0..S], row i with
 * n_i = o[i+1] - o[i] ids; rows, int64_t[M]; flags; stream.
 *   Out: a new result with M rows, on r's device and with r's vocabulary size:
 *     out_offs[k] = the sum of n_{rows[k']} over k' < k,  T' = out_offs[M],
 *     out_ids[out_offs[k] + t] = ids[o[rows[k]] + t]  for t < n_{rows[k]}.
 *   r is only read and stays valid; the caller frees both.  Every entry point that takes a result takes the new one.  An
 *   n-best result is accepted: its rows are rows (selecting by sample while keeping the nbest grouping is the caller's:
 *   select the sample's rows).  M = 0 gives an empty result with offsets [0], also when S = 0; rows may then be NULL.
 *   rows is host memory and is uploaded by the call; with TGX_SELECT_ROWS_DEVICE it is device memory on r's device, read
 *   in stream order.  That is checked with hipPointerGetAttributes before anything is queued, as the layouts check their
 *   destinations: the flag with a pointer that is not device memory there gives TGX_ERR_INVALID.
 *   Every index must satisfy 0 <= rows[k] < S.  Otherwise the call returns TGX_ERR_INVALID with *out = NULL, and
 *   tgx_last_error names the smallest offending k and its value.  Host rows are checked on the host before any device
 *   call.  Device rows are checked by the device: an index out of range contributes length 0, and the smallest such k
 *   comes back in a word read together with T' — before the id buffer is sized, so a bad index never becomes an address.
 *   TGX_ERR_INVALID also for r, out or (with M > 0) rows NULL and for unknown flags.
 *   stream: the stream rule of the layouts above — the work is queued on it (NULL: the library's blocking stream), the
 *   call returns after the stream has reached its end, and the calling thread's current device is the same after the
 *   call as before.  One host visit in between: T' and the bad-index word.
 *   Token spans of a selected result keep their meaning only against the equally selected corpus or text.
 *
 * tgx_result_lengths_device(r, stream, d_lengths) writes n_i for i < S as int64 into caller-owned device memory on r's
 * device (checked as the layouts' destinations; S = 0 writes nothing): what a caller filters and sorts on without a host
 * trip.
 *
 * tgx_corpus_select(c, rows, M, flags, stream, &out): the same mapping over the corpus's text bytes and byte offsets.
 * The output is a corpus like any other: every pass accepts it (encode, sampling, n-best, stats, the E-step, the counts,
 * tgx_corpus_split_specials, tgx_corpus_normalize).  Index checks, flag, stream rule and M = 0 as above; with device rows
 * the M + 1 new offsets visit the host too (a corpus keeps them there).  The limits of tgx_corpus_upload apply:
 * M >= 2^32 - 1 gives TGX_ERR_UNSUPPORTED.  c is only read; the call holds the corpus's lock, as
 * tgx_corpus_split_specials does.
 *
 * The seeded permutation: the same on every machine, on the host and for a caller without torch.
 *   tgx_shuffle_key(seed, g): x = seed ^ TGX_SHUFFLE_SALT ^ g·0x9E3779B97F4A7C15 (wrapping at 2^64), then the three
 *   xor-shift / multiply rounds of tgx_fim_u01; all 64 bits are the key.
 *   The permutation of n rows is 0 .. n-1 sorted ascending by (key, index).
 *   tgx_shuffled_rows_device(device, n, seed, stream, d_rows) writes it as int64[n] into caller-owned device memory on
 *   `device` (checked as above): a key kernel, then a stable radix sort of the keys with the indices as values.  Stream
 *   rule as above.  tgx_shuffled_rows_host(n, seed, rows) is the host twin.  n = 0 writes nothing; n >= 2^31 gives
 *   TGX_ERR_UNSUPPORTED.
 *
 * Host twins, no device: tgx_select_host over ids u32[T] (may be NULL when T = 0) and offs u64[n_rows + 1], and
 * tgx_select_text_host over text bytes u8[N] — the same checks, plus offs[0] = 0 and ascending offsets and cap >= T'
 * (nothing is written otherwise); they walk the kernels' tiles and thread slots through the same index arithmetic
 * (csrc/select.h).  out_offs u64[n_select + 1]; out may be NULL when T' = 0.
 *
 * tgx_select_last_times: device time of the calling thread's last tgx_result_select or tgx_corpus_select per stage (the
 * check of device rows, the offsets' scan, the fill), as tgx_fim_last_times; for tools/select_bench.py. */
#define TGX_SELECT_ROWS_DEVICE 1u
#define TGX_SHUFFLE_SALT 0xD6E8FEB86659FD93ULL
int tgx_select_last_times(const char **names, float *ms, int cap);
tgx_status tgx_result_select(const tgx_result *r, const int64_t *rows, uint64_t n_select, uint32_t flags, void *stream,
                             tgx_result **out);
tgx_status tgx_result_lengths_device(const tgx_result *r, void *stream, int64_t *d_lengths);
tgx_status tgx_corpus_select(tgx_corpus *c, const int64_t *rows, uint64_t n_select, uint32_t flags, void *stream,
                             tgx_corpus **out);
uint64_t tgx_shuffle_key(uint64_t seed, uint64_t g);
tgx_status tgx_shuffled_rows_device(int device, uint64_t n, uint64_t seed, void *stream, int64_t *d_rows);
tgx_status tgx_shuffled_rows_host(uint64_t n, uint64_t seed, int64_t *rows);
tgx_status tgx_select_host(const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, const int64_t *rows,
                           uint64_t n_select, uint32_t *out_ids, uint64_t ids_cap, uint64_t *out_offs);
tgx_status tgx_select_text_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, const int64_t *rows,
                                uint64_t n_select, uint8_t *out_text, uint64_t text_cap, uint64_t *out_offs);

/* ---- exact row deduplication on the device: of a result or of a corpus (csrc/dedup.hip) ------------------------------
 * The mask that drops duplicate documents, made where the documents are.  For a corpus c, S rows are given by byte
 * offsets o[0..S] over its text; for a result r, S rows by id offsets over its u32 ids.  Two rows are EQUAL iff they have
 * the same length and the same elements; two empty rows are equal.
 *
 *     first[k] = min { i : row i equals row k }        (int64, 0 <= first[k] <= k)
 *     n_unique = #{ k : first[k] == k }
 *
 * The result is exact: a hash only finds candidates, and every first[k] != k rests on an element-by-element comparison.
 * first == arange(S) selects the unique rows (tgx_result_select, tgx_corpus_select), and a histogram of first gives the
 * group sizes.
 *
 * tgx_corpus_first_equal_device(c, flags, stream, d_first, &n_unique), tgx_result_first_equal_device(r, ...):
 *   d_first is caller-owned device memory on the object's device, int64[S], checked with hipPointerGetAttributes before
 *   anything is queued, as the destination of tgx_result_lengths_device.  S = 0 writes nothing, and d_first may then be
 *   NULL.  n_unique is host memory and may be NULL.  flags must be 0.  The stream rule is that of the select block: the
 *   work is queued on stream (NULL: the library's blocking stream), the call returns after the stream has reached its
 *   end, and the calling thread's current device is unchanged.  The object is only read; the corpus call holds the
 *   corpus's lock, as tgx_corpus_select does.  An n-best result is accepted: its rows are rows.
 *   Without a device: TGX_ERR_DEVICE (asked first).  A NULL handle, unknown flags, d_first NULL with S > 0 or memory of
 *   the wrong kind: TGX_ERR_INVALID.  S >= 2^32 - 1: TGX_ERR_UNSUPPORTED.  Out of device memory: TGX_ERR_DEVICE, with
 *   nothing kept.  Scratch is about 46 bytes per row plus the sort's temporaries, allocated once per call.
 *   Rounds over a list of unresolved rows, ascending by row, all rows at first: (1) the key of every listed row, the top
 *   bits of tgx_row_hash with the round's number as seed; (2) a stable radix sort of (key, row), so each run of equal keys
 *   begins with its smallest row, its head; (3) every other row of a run compared with the head, lengths first; (4) a head
 *   gets first = itself, a row equal to its head first = the head, and the rows that differ form the next round's list.
 *   One host visit per round reads how many are left.  Equal rows share a key in every round and so the same verdict
 *   against the same head: the unresolved rows are closed under equality, a head has no equal row before it, and
 *   first is the minimum.  Every round resolves its heads, so the rounds end; with 64 key bits a second round takes a
 *   collision of two 64-bit hashes.
 *
 * tgx_row_hash(bytes, n, seed), an exported function, the same on every machine.  All arithmetic wraps at 2^64;
 *   R(x) is the three xor-shift / multiply rounds of tgx_dropout_u01 (x ^= x>>30; x *= 0xBF58476D1CE4E5B9; x ^= x>>27;
 *   x *= 0x94D049BB133111EB; x ^= x>>31).
 *     s    = R(seed ^ TGX_DEDUP_SALT)
 *     w_j  = bytes[8j .. 8j+8) as a little-endian u64, bytes past n read as 0,   j < W = ceil(n/8)
 *     acc  = the sum over j < W of  R( w_j ^ ((j+1)·0x9E3779B97F4A7C15) ^ s )
 *     hash = R( acc ^ (n·0xC2B2AE3D27D4EB4F) ^ s )
 *   A term depends only on a word and its position in the row, so a row of any length is hashed by any number of
 *   threads in any order, and integer addition gives the same bits every time.  A row of a result is hashed as the 4·n_i
 *   little-endian bytes of its ids.  (Rows that differ only in trailing zero bytes have equal sums: n tells them apart.)
 * tgx_corpus_row_hashes_device(c, seed, stream, d_hashes), tgx_result_row_hashes_device(r, ...) write the hash of every
 *   row as u64[S] into caller-owned device memory; checks and stream rule as above.  With an all-gather they are a
 *   probabilistic deduplication across ranks; an exact one is not offered.
 *
 * tgx_first_equal_host(data, elem_bytes, offs, n_rows, hash_bits, first, &n_unique, &n_rounds): the host twin, no
 *   device, over data of elem_bytes 1 (bytes) or 4 (u32, 4-byte aligned) and offs u64[n_rows + 1] in elements (offs[0] = 0
 *   and ascending, as the select twins check).  It runs the device's rounds through the same header (csrc/dedup.h: the
 *   hash in the kernel's tiles, the key of hash_bits bits, the run, compare and resolve rules); n_rounds is how many it
 *   took.  hash_bits 0 makes every row collide: the rounds then number the distinct contents.  hash_bits > 64 or another
 *   elem_bytes gives TGX_ERR_INVALID.  n_unique and n_rounds may be NULL; first may be NULL when n_rows = 0.
 *
 * tgx_dedup_last_times: device time of the calling thread's last first_equal call per stage, summed over its rounds, as
 * tgx_select_last_times (the names are listed without a call): dedup_hash_kernel (the padded offsets' scan, the hash
 * kernel, the keys), dedup_sort, dedup_compare_kernel (the runs, the compare offsets' scan, the compare), dedup_resolve
 * (first, and the next list's compaction).  tgx_dedup_last_rounds: the rounds that call took. */
#define TGX_DEDUP_SALT 0xA0761D6478BD642FULL
tgx_status tgx_corpus_first_equal_device(tgx_corpus *c, uint32_t flags, void *stream, int64_t *d_first,
                                         uint64_t *n_unique);
tgx_status tgx_result_first_equal_device(const tgx_result *r, uint32_t flags, void *stream, int64_t *d_first,
                                         uint64_t *n_unique);
uint64_t tgx_row_hash(const uint8_t *bytes, uint64_t n, uint64_t seed);
tgx_status tgx_corpus_row_hashes_device(tgx_corpus *c, uint64_t seed, void *stream, uint64_t *d_hashes);
tgx_status tgx_result_row_hashes_device(const tgx_result *r, uint64_t seed, void *stream, uint64_t *d_hashes);
tgx_status tgx_first_equal_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows,
                                uint32_t hash_bits, int64_t *first, uint64_t *n_unique, uint32_t *n_rounds);
int tgx_dedup_last_times(const char **names, float *ms, int cap);
uint32_t tgx_dedup_last_rounds(void);

/* ---- near-duplicate rows on the device: MinHash signatures, LSH bands, clusters (csrc/minhash.hip) --------------------
 * What the exact deduplication above leaves: rows that are almost each other's copies (a licence header with another
 * year, a fork with one line changed).  Three calls: a signature per row, the band keys and bucket heads of the
 * signatures, and the clusters.  Everything is integer work, pinned here, the same bits on every machine.  All
 * arithmetic wraps at 2^64; R is the three rounds of tgx_row_hash, G = 0x9E3779B97F4A7C15.
 *
 * Signatures.  tgx_result_minhash_device(r, width, n_perm, seed, flags, stream, d_sig), tgx_corpus_minhash_device(c, ...):
 *   row i has n_i elements of eb bytes (eb = 1: a corpus's text bytes; eb = 4: a result's u32 ids, an n-best result's
 *   rows being rows).  With w = width (1 <= w, w·eb <= 64) and K = n_perm (1 <= K <= 1024), row i has
 *   m_i = max(1, n_i - w + 1) shingles, shingle t the elements [t, t + min(w, n_i)): a row shorter than w, the empty row
 *   included, has exactly one shingle, its whole content.  Every row has a signature; no value is special.
 *     h(i,t)    = tgx_row_hash of the shingle's min(w, n_i)·eb little-endian bytes under the seed  seed ^ TGX_MINHASH_SALT
 *                 (the length in its last step tells short rows with trailing zeros apart)
 *     s         = R(seed ^ TGX_MINHASH_SALT)
 *     a_k       = R(s ^ (2k+1)·G) | 1,     b_k = R(s ^ (2k+2)·G)
 *     v_k(h)    = (uint32_t)((a_k·h + b_k) >> 32)                     (multiply-add-shift)
 *     sig[i][k] = min over t < m_i of v_k(h(i,t))
 *   d_sig is caller-owned device memory on the object's device, u32[S, K] row-major.  The destination check, the stream
 *   rule, the locks, flags == 0 and the limit on S (S < 2^32 - 1, else TGX_ERR_UNSUPPORTED) are those of
 *   tgx_corpus_first_equal_device.  w = 0, w·eb > 64, K = 0 or K > 1024: TGX_ERR_INVALID.  S = 0 writes nothing.  The
 *   object is only read.  A minimum may be taken in any order and in any number of parts, so the kernel tiles the
 *   concatenated shingle positions of all rows, 64 to a wave, and a row of any length gets the same bits.
 * tgx_minhash_value(h, k, seed) is v_k(h), exported so that a caller on another machine can extend a signature.
 *
 * Bands.  tgx_minhash_bands_device(device, d_sig, S, K, bands, seed, stream, d_keys, d_heads): B = bands must divide K
 *   (else TGX_ERR_INVALID), r = K / B.
 *     key[i][b]  = tgx_row_hash of the 4r little-endian bytes of sig[i][b·r .. (b+1)·r) under the seed
 *                  (seed ^ TGX_MINHASH_SALT) + b + 1                                 -> d_keys, u64[S, B]
 *     head[i][b] = min { j : key[j][b] == key[i][b] }                                -> d_heads, int64[S, B]
 *   Either output may be NULL, not both.  All pointers are device memory on `device`, checked before anything is queued;
 *   stream rule as above.  Per band the heads are a stable radix sort of (key, row) and the run rule of the exact
 *   deduplication, every band through one scratch set (8·S·B bytes of band-major keys, 16 bytes per row, the sort's
 *   temporaries).  The keys alone are what a caller all-gathers for a pass across ranks.  Two rows of Jaccard similarity J
 *   share at least one bucket with probability 1 - (1 - J^r)^B.
 *
 * Clusters.  tgx_minhash_near_first_device(device, d_sig, S, K, d_heads, B, min_agree, stream, d_first, &n_clusters):
 *     agree(i,j) = #{ k : sig[i][k] == sig[j][k] }                              (agree / K estimates J)
 *     first0[i]  = min( {i} + { head[i][b] : b < B, head[i][b] < i, agree(i, head[i][b]) >= min_agree } )
 *     first[i]   = the root of i's chain under first0 (first0[i] <= i, so the chains end)   -> d_first, int64[S]
 *     n_clusters = #{ i : first[i] == i }                                       (host memory, may be NULL)
 *   1 <= min_agree <= K and 1 <= B <= K, else TGX_ERR_INVALID.  A head that is no row before i is never followed, so
 *   heads from elsewhere cannot make the call read outside d_sig.  This is a STAR per bucket: a row is compared with
 *   its bucket's head only, and transitivity comes from the chains alone; two rows of one bucket that both fail against
 *   the head are not compared with each other.  The roots are found by pointer doubling between d_first and a scratch of
 *   its size, one host visit per round.  first == arange(S) is the keep-mask, exactly as with first_equal.
 *
 * Host twins, no device, the same argument checks as tgx_first_equal_host: tgx_minhash_host(data, elem_bytes, offs,
 *   n_rows, width, n_perm, seed, sig) walks the kernel's tiles, chunks and flush rule through csrc/minhash.h;
 *   tgx_minhash_bands_host(sig, n_rows, n_perm, bands, seed, keys, heads); tgx_minhash_near_first_host(sig, n_rows, n_perm,
 *   heads, bands, min_agree, first, &n_clusters).
 *
 * tgx_minhash_last_times: device time per stage of the calling thread's last calls, as tgx_dedup_last_times (the names
 * are listed without a call).  Each of the three calls sets the stages it runs and leaves the others: minhash_sig_kernel
 * (the positions' scan, the pre-set, the kernel); minhash_band_keys, minhash_sort, minhash_heads (summed over the bands);
 * minhash_verify (first0), minhash_roots (the doubling rounds and the count). */
#define TGX_MINHASH_SALT 0xD6E8FEB86659FD93ULL
tgx_status tgx_result_minhash_device(const tgx_result *r, uint32_t width, uint32_t n_perm, uint64_t seed, uint32_t flags,
                                     void *stream, uint32_t *d_sig);
tgx_status tgx_corpus_minhash_device(tgx_corpus *c, uint32_t width, uint32_t n_perm, uint64_t seed, uint32_t flags,
                                     void *stream, uint32_t *d_sig);
uint32_t tgx_minhash_value(uint64_t h, uint32_t k, uint64_t seed);
tgx_status tgx_minhash_bands_device(int device, const uint32_t *d_sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands,
                                    uint64_t seed, void *stream, uint64_t *d_keys, int64_t *d_heads);
tgx_status tgx_minhash_near_first_device(int device, const uint32_t *d_sig, uint64_t n_rows, uint32_t n_perm,
                                         const int64_t *d_heads, uint32_t bands, uint32_t min_agree, void *stream,
                                         int64_t *d_first, uint64_t *n_clusters);
tgx_status tgx_minhash_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, uint32_t width,
                            uint32_t n_perm, uint64_t seed, uint32_t *sig);
tgx_status tgx_minhash_bands_host(const uint32_t *sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed,
                                  uint64_t *keys, int64_t *heads);
tgx_status tgx_minhash_near_first_host(const uint32_t *sig, uint64_t n_rows, uint32_t n_perm, const int64_t *heads,
                                       uint32_t bands, uint32_t min_agree, int64_t *first, uint64_t *n_clusters);
int tgx_minhash_last_times(const char **names, float *ms, int cap);

/* ---- shared n-grams on the device: gram sets and per-row contamination hits (csrc/gram.hip) ---------------------------
 * Decontamination: which rows of a large source share an n-gram with a small held-out set (a benchmark, test files),
 * and how many.  first_equal compares whole rows and MinHash whole-row similarity; a 2 KB problem pasted into a 200 KB
 * file is seen by neither.  Two steps: a gram set of the held-out source, and a probe of the large one against it.
 * Integer work, pinned here, the same bits on every machine.
 *
 * Definitions.  Row i of a source is the elements data[offs[i] .. offs[i+1]), of eb bytes (eb = 1: a corpus's text
 *   bytes; eb = 4: a result's u32 ids).  With w = width (1 <= w, w·eb <= 64) the gram AT ELEMENT e of row i (e a global
 *   element index) is the w elements from e on, and it is VALID iff e + w <= offs[i+1].  A row shorter than w owns no
 *   gram: unlike MinHash, where every row owns one short shingle, an empty held-out row does not flag every empty row.
 *     key(e) = tgx_row_hash of the gram's w·eb little-endian bytes under the seed  seed ^ TGX_MINHASH_SALT
 *   which is MinHash's h(i,t) of a full shingle.  tgx_gram_key(bytes, n_bytes, seed) is that hash of any bytes, exported
 *   so that another machine can build keys.
 *   A GRAM SET is the ascending, distinct u64 keys of all valid grams of a source, in device memory, with a bucket
 *   directory:  bits = n_keys <= 1 ? 0 : min(28, ceil_log2(n_keys));  dir is u32[2^bits + 1];  dir[b] = the lower bound of
 *   the first key whose top `bits` bits are >= b;  dir[2^bits] = n_keys.  Key k is a member iff a binary search of
 *   keys[dir[b] .. dir[b+1]), b = the top bits of k, finds it: a bucket holds about one key, and one that an adversary
 *   filled costs its logarithm.  Membership is by 64-bit key, as with tgx_*_row_hashes_device: PROBABILISTIC in that two
 *   different grams may share a key (about n_keys / 2^64 per probed gram); hits are not verified against the elements.
 *
 * Sets.  tgx_result_gramset_create(r, width, seed, flags, stream, &gs), tgx_corpus_gramset_create(c, ...): the rows' gram
 *   counts max(0, n_i - w + 1) and their scan, a kernel that writes every valid gram's key to its slot, a radix sort, a
 *   unique, a host visit for n_keys and the directory kernel (the scan's total, which sizes the sort, is a host visit
 *   too).  flags must be 0; stream rule, locks and the limit on S as tgx_corpus_first_equal_device.  The source is only
 *   read.  A source without a valid gram gives a valid set that contains nothing.
 *   tgx_gramset_create_from_keys(device, host_keys, n, width, elem_bytes, seed, &gs): keys in any order, duplicates
 *   allowed, sorted and made unique on the device (the library's stream of `device`): how the sets of several sources
 *   are united, and how a test builds a hostile set.  width, elem_bytes and seed are what a probe hashes with.
 *   w = 0, w·eb > 64, an elem_bytes other than 1 and 4: TGX_ERR_INVALID.  2^32 - 1 distinct keys or more:
 *   TGX_ERR_UNSUPPORTED.  A set is read-only after creation, so concurrent hit calls may share it.
 *   tgx_gramset_size: n_keys.  tgx_gramset_info(gs, &width, &elem_bytes, &seed, &device, &dir_bits): any may be NULL.
 *   tgx_gramset_keys(gs, host_out): the n_keys keys, ascending, to host memory.  tgx_gramset_free.
 *
 * Hits.  tgx_result_gram_hits_device(r, gs, flags, stream, d_count, d_mask), tgx_corpus_gram_hits_device(c, ...), under
 *   the set's width and seed:
 *     count[i] = #{ valid grams of row i whose key is in the set }      -> d_count, i64[S]
 *     mask[e]  = 1 where the gram at element e is valid and in the set, else 0   -> d_mask, u8[n_elems]
 *   Every byte of both is written.  Either may be NULL, not both.  Both are caller-owned device memory on the source's
 *   device, checked before anything is queued.  The source's element size or device differing from the set's, host
 *   memory, nonzero flags: TGX_ERR_INVALID, with nothing queued or written.  S = 0 writes nothing.  The source is only
 *   read.  Rows with count above a limit are dropped with tgx_*_select, of the corpus and of its result alike.
 *   The kernel lays the elements of all rows end to end, 64 to a wave and a lane an element: the validity test, the
 *   loads (an invalid position loads nothing), the hash, the two directory entries, the bucket.  A ballot of the hits is
 *   cut per row: a row inside the wave's 64 elements gets a plain store, any other a 64-bit atomic add onto the count,
 *   which was pre-set to 0 and which empty rows keep.
 *
 * Host twins, no device, the argument checks of tgx_first_equal_host: tgx_gram_keys_host(data, elem_bytes, offs, n_rows,
 *   width, seed, keys_out, &n_keys) writes the ascending distinct keys (keys_out has room for n_elems = offs[n_rows]);
 *   tgx_gram_hits_host(data, elem_bytes, offs, n_rows, width, seed, keys, n_keys, count, mask) takes keys in any order,
 *   builds the directory and walks the kernel's chunks, tiles and store / add rule through csrc/gram.h;
 *   tgx_gram_contains_host(keys, n_keys, probes, n_probes, out) is the membership test alone, out u8[n_probes].
 *
 * tgx_gram_last_times: device time per stage of the calling thread's last calls, as tgx_minhash_last_times: a create
 * sets gram_keys_kernel (the counts' scan and the kernel; 0 from keys), gram_sort (sort and unique) and gram_dir; a hits
 * call sets gram_hits_kernel (the pre-set and the kernel). */
typedef struct tgx_gramset tgx_gramset;
uint64_t tgx_gram_key(const uint8_t *bytes, uint64_t n_bytes, uint64_t seed);
tgx_status tgx_result_gramset_create(const tgx_result *r, uint32_t width, uint64_t seed, uint32_t flags, void *stream,
                                     tgx_gramset **out);
tgx_status tgx_corpus_gramset_create(tgx_corpus *c, uint32_t width, uint64_t seed, uint32_t flags, void *stream,
                                     tgx_gramset **out);
tgx_status tgx_gramset_create_from_keys(int device, const uint64_t *keys, uint64_t n, uint32_t width, uint32_t elem_bytes,
                                        uint64_t seed, tgx_gramset **out);
uint64_t tgx_gramset_size(const tgx_gramset *gs);
tgx_status tgx_gramset_info(const tgx_gramset *gs, uint32_t *width, uint32_t *elem_bytes, uint64_t *seed, int *device,
                            uint32_t *dir_bits);
tgx_status tgx_gramset_keys(const tgx_gramset *gs, uint64_t *keys_out);
void tgx_gramset_free(tgx_gramset *gs);
tgx_status tgx_result_gram_hits_device(const tgx_result *r, const tgx_gramset *gs, uint32_t flags, void *stream,
                                       int64_t *d_count, uint8_t *d_mask);
tgx_status tgx_corpus_gram_hits_device(tgx_corpus *c, const tgx_gramset *gs, uint32_t flags, void *stream,
                                       int64_t *d_count, uint8_t *d_mask);
tgx_status tgx_gram_keys_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, uint32_t width,
                              uint64_t seed, uint64_t *keys_out, uint64_t *n_keys);
tgx_status tgx_gram_hits_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, uint32_t width,
                              uint64_t seed, const uint64_t *keys, uint64_t n_keys, int64_t *count, uint8_t *mask);
tgx_status tgx_gram_contains_host(const uint64_t *keys, uint64_t n_keys, const uint64_t *probes, uint64_t n_probes,
                                  uint8_t *out);
int tgx_gram_last_times(const char **names, float *ms, int cap);

/* ---- per-row text statistics and the line view of a resident corpus (csrc/textstat.hip) --------------------------------
 * The heuristic quality filters of code corpora (a longest line over 1000 characters, a mean line length over 100, an
 * alphanumeric share under 0.25, the share of duplicate lines) need per row a handful of counts and the lines
 * themselves.  Two calls give both where the documents already lie.  Integer work, pinned here, the same on every machine.
 *
 * Definitions.  Row i is the bytes text[offs[i] .. offs[i+1]) of the corpus.
 *   Terminator: only '\n' (0x0A) ends a line; '\r' is an ordinary byte.  A caller who wants CRLF folded runs the CRLF
 *     front end first (tgx_corpus_split_specials with TGX_FRONT_CRLF).
 *   Line end: position p of row i is a line end iff text[p] == '\n' or p == offs[i+1] - 1.
 *   Line start: the line ending at p begins at max(offs[i], q + 1), q being the last '\n' before p at or after offs[i].
 *   So no line continues from one row into the next, a trailing '\n' opens no empty last line, "\n" is one empty line,
 *     and an empty row has no line.
 *   Line length: without its '\n'; in bytes, or under TGX_TEXTSTAT_CHARS in characters.
 *   Character: a byte b with (b & 0xC0) != 0x80, so everything is defined by bytes alone, on invalid UTF-8 too.
 *
 * tgx_corpus_text_stats_device(c, line_limit, flags, stream, d_stats, d_line_start) writes d_stats, int64
 *   [TGX_TEXTSTAT_N, S], each statistic contiguous over the rows:
 *      0 bytes       offs[i+1] - offs[i]
 *      1 chars       characters
 *      2 newlines    bytes equal to '\n'
 *      3 lines       line ends
 *      4 max_line    the longest line's length in the unit; 0 without a line
 *      5 long_lines  lines whose length in the unit is greater than line_limit
 *      6 alpha       A-Z, a-z
 *      7 digit       0-9
 *      8 space       0x20 and 0x09 .. 0x0D
 *      9 non_ascii   bytes >= 0xC0: the characters that are not ASCII
 *     10 control     bytes < 0x20 that are not space, and 0x7F
 *   and d_line_start, u8[n_bytes]: 1 where a line begins (a nonempty row's first byte, or a byte after a '\n' within its
 *   row), else 0.  Every byte of both is written.  Either may be NULL, not both.  Both are caller-owned device memory on
 *   the corpus's device, checked before anything is queued; host memory or a flag other than TGX_TEXTSTAT_CHARS:
 *   TGX_ERR_INVALID, with nothing queued or written.  Stream rule, the corpus's lock and the limit on S (S < 2^32 - 1) as
 *   tgx_corpus_gram_hits_device.  S = 0 writes nothing.  The corpus is only read.
 *   The kernels lay the bytes of all rows end to end, 64 to a wave and a lane a byte.  A first kernel writes one word per
 *   64 bytes (has the chunk a line start; the units from its last line start on), a scan under the segmented sum turns
 *   the words into the units of the line that is open at each chunk's first byte, and the second kernel cuts ballots of
 *   the classes, the line ends and the long lines per row: a row inside the wave's 64 bytes gets plain stores, any other
 *   64-bit atomic adds (max_line: an atomic maximum) onto the table, which was pre-set to 0 and which empty rows keep.  A
 *   line's length never costs a walk back over the line: the time does not depend on the lines' lengths.
 *
 * tgx_corpus_lines(c, flags, stream, &out): a new corpus whose rows are the lines of c, in order, each with its '\n' if
 *   it has one: the same bytes as c, its offsets the line starts plus n_bytes.  flags must be 0.  The line starts above
 *   are compacted on the device; their number and then the offsets visit the host, as in tgx_corpus_select.  2^32 - 1
 *   lines or more: TGX_ERR_UNSUPPORTED.  A corpus with no line gives an empty corpus.  The row a line came from needs no
 *   call: it is repeat_interleave(arange(S), lines).
 *
 * Host twins, no device, the argument checks of the select twins (offs[0] = 0 and ascending): tgx_text_stats_host(text,
 *   offs, n_rows, line_limit, flags, stats, line_start) writes stats i64[TGX_TEXTSTAT_N, n_rows] and line_start
 *   u8[offs[n_rows]] (either may be NULL, not both); tgx_lines_host(text, offs, n_rows, out_offs, cap, &n_lines) writes
 *   the n_lines + 1 offsets of the line view into out_offs u64[cap] (cap < n_lines + 1: TGX_ERR_INVALID, with n_lines
 *   set).  Both walk the kernel's chunks, tiles, summaries, carry and store / add rule through csrc/textstat.h.
 *
 * tgx_textstat_last_times: device time per stage of the calling thread's last call, as tgx_gram_last_times (the names are
 * listed without a call): textstat_summary_kernel, textstat_scan, textstat_kernel (the pre-set and the kernel), and
 * textstat_lines (the count and the compaction of the line starts; 0 after a statistics call). */
#define TGX_TEXTSTAT_N 11
#define TGX_TEXTSTAT_CHARS 1u
tgx_status tgx_corpus_text_stats_device(tgx_corpus *c, uint64_t line_limit, uint32_t flags, void *stream, int64_t *d_stats,
                                        uint8_t *d_line_start);
tgx_status tgx_corpus_lines(tgx_corpus *c, uint32_t flags, void *stream, tgx_corpus **out);
tgx_status tgx_text_stats_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, uint64_t line_limit, uint32_t flags,
                               int64_t *stats, uint8_t *line_start);
tgx_status tgx_lines_host(const uint8_t *text, const uint64_t *offs, uint64_t n_rows, uint64_t *out_offs, uint64_t cap,
                          uint64_t *n_lines);
int tgx_textstat_last_times(const char **names, float *ms, int cap);

/* ---- repeated n-grams within a row: the Gopher repetition statistics (csrc/repeat.hip) ---------------------------------
 * Which n-grams of row i occur earlier in row i: what the Gopher / MassiveText repetition rules (the share of a
 * document taken by its most frequent 2- to 4-gram, the share covered by repeated 5- to 10-grams) need, for a result
 * (token n-grams) or a corpus (byte n-grams) that stays in HBM.
 *
 * Definitions (csrc/repeat.h, used by the kernels and the host twin).  The source, the width w (1 <= w, w·eb <= 64), the
 *   gram AT ELEMENT e, its validity (a row shorter than w owns no gram) and its key(e) are those of the shared n-grams
 *   above.  The ROW KEY of a valid gram at element e of row i is
 *     rkey(e) = mix(key(e) ^ ((i + 1) · 0x9E3779B97F4A7C15))        (mix: tgx_row_hash's 64-bit finaliser, a bijection)
 *   so within a row two grams are EQUAL iff their keys are equal: probabilistic by the 64-bit key exactly as gram hits
 *   are, and not verified against the elements; across rows equal grams get different row keys except by a 64-bit
 *   collision.  An OCCURRENCE CLASS is the set of the valid grams of one row with one row key.  Its first member by
 *   position is its FIRST occurrence, every other member is a REPEAT, and a class of two or more members is MULTI.
 *
 * tgx_result_repeat_stats_device(r, width, seed, flags, stream, d_stats, d_mask), tgx_corpus_repeat_stats_device(c, ...)
 *   write d_stats, int64 [TGX_REPEAT_N, S], each statistic contiguous over the rows:
 *     0 grams        valid grams of the row, max(0, n_i - w + 1)
 *     1 repeated     valid grams that are repeats (grams - repeated = the distinct grams)
 *     2 multi        valid grams that belong to a MULTI class (first occurrences included)
 *     3 top          members of the row's largest class: 0 for a row without a gram, 1 when all its grams are distinct
 *     4 covered      elements of the row that lie inside at least one REPEAT (each once, however many overlap it): what
 *                    a pipeline that deletes repeats would delete
 *     5 covered_all  elements that lie inside at least one member of a MULTI class (the Gopher paper's literal reading)
 *   and d_mask, u8[n_elems]: bit 0 (TGX_REPEAT_MASK_REPEAT) where a repeat begins, bit 1 (TGX_REPEAT_MASK_MULTI) where a
 *   member of a MULTI class begins, every other position 0, invalid positions included.  Every byte of both is written;
 *   either may be NULL, not both.  Destinations are device memory of the source's device, checked before anything is
 *   queued; host memory, a nonzero flag or a bad width: TGX_ERR_INVALID.  2^32-1 rows or more, or 2^32-1 elements or more
 *   (positions are u32): TGX_ERR_UNSUPPORTED, before anything is queued.  Stream rule, corpus lock and pooled scratch as
 *   tgx_corpus_gram_hits_device; S = 0 writes nothing.  The source is only read.
 *   Pipeline: the rows' gram counts and their scan; a kernel that writes every valid gram's row key and position to its
 *   slot; a stable radix sort of the pairs by key (so a class's first slot is its first occurrence); a kernel over the
 *   sorted slots that writes the mask's byte of every valid position and maxes the length of every run onto `top`; a
 *   kernel over the elements that turns the mask into the rows' sums and coverage.  One host visit reads the grams'
 *   total, which sizes the sort.  Scratch: 24 bytes per gram, a byte per element without d_mask, 8 (S + 1) bytes and
 *   rocPRIM's temporaries.
 *
 * Host twin, no device, the argument checks of tgx_gram_hits_host: tgx_repeat_stats_host(data, elem_bytes, offs, n_rows,
 *   width, seed, stats, mask) goes through csrc/repeat.h: the same row keys, a stable sort, the run rule and the run's
 *   end, and the kernel's chunks with the two-chunk coverage window and the store / add rule.
 *
 * tgx_repeat_last_times: device time per stage of the calling thread's last call, as tgx_gram_last_times (the names are
 * listed without a call): repeat_keys_kernel (the counts' scan, the pre-sets and the kernel), repeat_sort,
 * repeat_runs_kernel and repeat_cover_kernel (0 without d_stats). */
#define TGX_REPEAT_N 6
#define TGX_REPEAT_MASK_REPEAT 1u
#define TGX_REPEAT_MASK_MULTI 2u
tgx_status tgx_result_repeat_stats_device(const tgx_result *r, uint32_t width, uint64_t seed, uint32_t flags, void *stream,
                                          int64_t *d_stats, uint8_t *d_mask);
tgx_status tgx_corpus_repeat_stats_device(tgx_corpus *c, uint32_t width, uint64_t seed, uint32_t flags, void *stream,
                                          int64_t *d_stats, uint8_t *d_mask);
tgx_status tgx_repeat_stats_host(const void *data, uint32_t elem_bytes, const uint64_t *offs, uint64_t n_rows, uint32_t width,
                                 uint64_t seed, int64_t *stats, uint8_t *mask);
int tgx_repeat_last_times(const char **names, float *ms, int cap);

/* ---- the front end on the device: a resident corpus split at special tokens, CRLF applied (csrc/front.hip) --------
 * What tgx_split_specials and tgx_pack_segments compute on host threads, for a corpus that is already in HBM (an upload,
 * or tgx_corpus_from_text of a decoded text), with the plan kept on the device for tgx_assemble_result_plan: a resident
 * text is encoded as Tokenizer::encode_batch encodes it without its bytes or the plan visiting the host.
 *
 * tgx_corpus_split_specials(c, specials, n_specials, flags, &segs, &plan).  The special tokens are host arrays as in
 * tgx_split_specials (special_offs u64[n_specials + 1], any base).  With S samples of N bytes in c:
 *   The plan is exactly what tgx_split_specials returns for the samples of c: a sample is scanned from its start; at a
 *   position the FIRST special token in list order that the text starts with and that ends inside the sample matches
 *   (not the longest); the earliest position wins, and the scan goes on behind the match.  The non-empty text in front of
 *   a match is a segment of its own, and so is a non-empty tail; an empty sample has no segments.  seg_offs u64[S+1]
 *   (sample i owns segments [seg_offs[i], seg_offs[i+1]); K = seg_offs[S]) and seg_special i32[K] (the special's index, or
 *   -1 for a segment that is encoded) stay in HBM (pooled buffers) until tgx_plan_free; E = segments with seg_special < 0.
 *   A special token never matches across a sample's end.
 *   *segs is a resident corpus of the E encoded segments, in order: exactly what tgx_pack_segments(..., crlf = flags &
 *   TGX_FRONT_CRLF) packs.  With TGX_FRONT_CRLF a '\r' is dropped iff the next byte is '\n' AND lies in the same segment:
 *   a '\r' that ends a segment is kept whatever follows it in the buffer, and a special token that contains "\r\n" is
 *   matched on the raw text.  Row k of *segs is segment k of the packed batch the host route builds, so dropout and
 *   sampling hash the same (seed, row, position) and agree bit for bit.  *segs is an ordinary corpus: every entry point
 *   that takes one takes it.  It is built as tgx_corpus_from_text builds one: the E + 1 offsets visit the host for the
 *   longest-first order, beside three counters (candidates, K, E); no text byte and no plan array does.
 *   n_specials = 0 is allowed: every non-empty sample is one encoded segment.
 * Errors, before anything is queued: TGX_ERR_INVALID for NULL arguments, unknown flags, special_offs that decrease and an
 *   empty special token (tgx_split_specials' message); TGX_ERR_UNSUPPORTED for more than 4096 special tokens or more than
 *   65 536 bytes of them (the kernels' tables; tgx_split_specials has no such limit).
 * c is only read and the call holds the corpus's lock, as a pass does.  S = 0 or N = 0: TGX_OK, a plan without segments
 *   and a corpus without samples.  Stream rule: that of tgx_corpus_from_text (the library's blocking stream; the call
 *   returns after the stream has reached its end; the caller's current device is restored).
 * Candidates can overlap (special "aa" on "aaaaa"): they are resolved by the sequential rule above, one thread per run of
 *   overlapping candidates, so a text that is one long run (10^6 x 'a') is slow but correct.
 *
 * tgx_plan_copy copies the plan to host arrays (seg_offs u64[S+1], seg_special i32[K]; caps in elements).
 * tgx_assemble_result_plan is tgx_assemble_result with the plan read in HBM: the same result; TGX_ERR_INVALID when E
 *   differs from segs' row count (so an n-best result is refused), segs is NULL although E > 0, the plan, segs and the
 *   model are not on one device, segs was written for another vocabulary size, V + n_specials > 0xFFFFFFFE, or n_specials
 *   is not the count the plan was made with.
 * tgx_corpus_copy_text / tgx_corpus_copy_offsets copy a resident corpus's bytes (N) and offsets (u64[S+1], from 0) to the
 *   host (caps in elements).
 * tgx_front_host is the host twin over host arrays (offs[0] = 0), no device: the same checks and limits, the kernels'
 *   tiles and thread slots through the same index arithmetic (csrc/front.h).  seg_offs u64[S+1] is the caller's;
 *   *seg_special (i32[K]), *out_text and *out_offs (u64[E+1]) are malloc'd (tgx_free).
 * tgx_front_last_times: device milliseconds of the calling thread's last tgx_corpus_split_specials, per stage (mark,
 *   resolve, segments, keep, pack: events on the call's stream around each stage's kernels and scans); returns the
 *   number of entries written (at most cap).  For tools/front_bench.py. */
typedef struct tgx_plan tgx_plan;
#define TGX_FRONT_CRLF 1u
tgx_status tgx_corpus_split_specials(tgx_corpus *c, const uint8_t *special_bytes, const uint64_t *special_offs,
                                     uint32_t n_specials, uint32_t flags, tgx_corpus **segs, tgx_plan **plan);
uint64_t tgx_plan_num_samples(const tgx_plan *p);
uint64_t tgx_plan_num_segments(const tgx_plan *p);
uint64_t tgx_plan_num_encoded(const tgx_plan *p);
int tgx_plan_device(const tgx_plan *p);
tgx_status tgx_plan_copy(const tgx_plan *p, uint64_t *seg_offs, uint64_t offs_cap, int32_t *seg_special, uint64_t special_cap);
void tgx_plan_free(tgx_plan *p);
tgx_status tgx_assemble_result_plan(tgx_model *m, const tgx_result *segs, const tgx_plan *plan, uint32_t n_specials,
                                    tgx_result **out);
int tgx_front_last_times(const char **names, float *ms, int cap);
tgx_status tgx_corpus_copy_text(const tgx_corpus *c, uint8_t *dst, uint64_t cap);
tgx_status tgx_corpus_copy_offsets(const tgx_corpus *c, uint64_t *dst, uint64_t cap);
tgx_status tgx_front_host(const uint8_t *text, const uint64_t *offs, uint64_t n_samples, const uint8_t *special_bytes,
                          const uint64_t *special_offs, uint32_t n_specials, uint32_t flags, uint64_t *seg_offs,
                          int32_t **seg_special, uint64_t *n_segments, uint8_t **out_text, uint64_t **out_offs,
                          uint64_t *n_encoded);

/* ---- Unicode normalisation on the device: a resident corpus to a resident corpus (csrc/norm.hip) -----------------
 * What tgx_normalize_segments computes on host threads, for a corpus that is already in HBM.
 *
 * tgx_corpus_normalize(c, form, &out, &n_pieces).  form as tgx_normalize_segments: 0 NFD, 1 NFC, 2 NFKD, 3 NFKC.  With E
 * rows in c, *out is a resident corpus of E rows on c's device, and row k holds exactly the bytes tgx_normalize_segments
 * produces for row k.
 *   Units.  A row is read as units by the strict UTF-8 decoder of csrc/unicode_norm.cpp (no overlong forms, no
 *   surrogates, <= 0x10FFFF): a unit is a scalar value, or an offending byte that travels alone as a raw byte.  Decoding
 *   is bounded by the row's end, so a UTF-8 sequence cut by a row end is raw bytes on both sides.  Raw bytes are never
 *   changed and nothing combines with them.
 *   Active units.  Under a form a scalar value cp is ACTIVE when ccc(cp) != 0, or normalising cp alone under the form
 *   changes it, or (NFC and NFKC only) cp is the second of a primary composition pair, a Hangul V jamo (U+1161..U+1175)
 *   or a Hangul T jamo (U+11A8..U+11C2).  Everything else is INERT: raw bytes, all of ASCII, and the rest.  With the
 *   Unicode 13.0.0 data of csrc/unicode_tables.h: 14 101 active scalar values under NFD, 2 060 under NFC, 17 776 under
 *   NFKD, 5 747 under NFKC.  The property is built once per process from that data and the normaliser itself, as a
 *   two-stage table over cp >> 8 whose block 0 is "all inert", and uploaded once per device.
 *   Pieces.  A piece starts at a HEAD: an inert unit whose next unit in the same row is active, or an active unit that
 *   is the first of its row.  It runs through the active units that follow the head.  Every byte outside a piece is
 *   copied verbatim; every piece is replaced by its normalisation in isolation.  Pieces never cross rows.
 *   Window.  One thread normalises a piece as a stream and keeps only the decomposed stream since its last starter: one
 *   starter and the non-starters after it.  A source scalar's full decomposition is fed one scalar at a time; a
 *   non-starter is appended to the window; on a starter the window's marks are put in canonical order (a stable sort by
 *   class) and, for the composed forms, composed as tgx_normalize_segments composes them; if the window is then a single
 *   starter that composes with the new one, the composite replaces it; otherwise the window is emitted and a new one
 *   starts with the starter.  The window holds 32 scalars (a starter and 31 non-starters; UAX #15 Stream-Safe text has
 *   at most 30 non-starters in a row, and one scalar's decomposition adds at most 3).  A row that needs more is refused.
 *   Result.  *out is an ordinary corpus, built as tgx_corpus_split_specials builds *segs: only the E + 1 offsets and
 *   three counters visit the host.  Row count and row order are kept and no non-empty row becomes empty, so dropout and
 *   sampling hash the same (seed, row, position) as the host route.  *n_pieces = the number of pieces; with 0 pieces the
 *   output is a device-to-device copy.  E = 0 or no bytes: TGX_OK and a copy.
 * Errors, before anything is queued: TGX_ERR_INVALID for NULL arguments and for form > 3.  After the length pass, with
 *   nothing returned: TGX_ERR_UNSUPPORTED for a window overflow (tgx_last_error names the limit; the sample of
 *   tgx_last_error_detail is the LOWEST offending row, a device minimum, so it does not depend on timing).
 * c is only read and the call holds the corpus's lock.  Stream rule and device restoration: those of
 *   tgx_corpus_split_specials.
 *
 * tgx_normalize_host is the host twin over host arrays (offs u64[n_rows + 1], offs[0] = 0), no device: the kernels'
 *   tiles, thread slots and pieces through the same decoder, stream machine and index arithmetic (csrc/norm.h); the same
 *   limit and the same error.  *out_text (at least one byte) and *out_offs (u64[n_rows + 1]) are malloc'd (tgx_free).
 * tgx_norm_last_times: device milliseconds of the calling thread's last tgx_corpus_normalize, per stage (mark, pieces,
 *   length, places, write), as tgx_front_last_times.  For tools/norm_bench.py. */
tgx_status tgx_corpus_normalize(tgx_corpus *c, uint32_t form, tgx_corpus **out, uint64_t *n_pieces);
tgx_status tgx_normalize_host(uint32_t form, const uint8_t *text, const uint64_t *offs, uint64_t n_rows,
                              uint8_t **out_text, uint64_t **out_offs, uint64_t *n_pieces);
int tgx_norm_last_times(const char **names, float *ms, int cap);

/* ---- decode on the device: a result's ids or a padded id tensor to UTF-8 text (csrc/decode.hip) -------------------
 * What tgx_decode_batch computes, with ids, text and row offsets all in HBM.
 *
 * Input: a stream of N elements in S rows.
 *   Offsets form (tgx_decode_result): a result; u32 ids, row i = elements [ooffs[i], ooffs[i+1]); every element is live.
 *   Padded form (tgx_decode_padded): caller-owned device memory, S = n_rows rows of L = row_len elements, contiguous and
 *     row-major, int32_t or (flags: TGX_LAYOUT_I64) int64_t; row i = elements [i·L, (i+1)·L).  Element (i, c) is live iff
 *     (d_mask == NULL || d_mask[i·L + c] != 0) && (d_lengths == NULL || c < d_lengths[i]) && (skip_id == TGX_NO_ID ||
 *     element != skip_id); d_mask is u8[S·L], d_lengths i32[S] with a negative length counting as 0.  An element that
 *     is not live is absent: it is not checked, owns no byte and does not end a run.
 * Classes: with V the model's vocabulary size, a live element x with 0 <= x < V is a base id, V <= x < V + n_specials
 *   special token x - V (special_bytes / special_offs: host arrays as in tgx_decode_batch), anything else — negative
 *   values and values >= 2^32 of int64 rows included — is out of bounds.
 * Out of bounds: TGX_ERR_TOKEN_ID_OOB and no text.  *bad_sample = the lowest row that holds such an element, *bad_id =
 *   the first such element of that row (a negative value as its two's complement), tgx_last_error() = "token id {x} is
 *   out of bounds" with a negative x printed signed.
 * Row i's text: walk its live elements in order.  A maximal stretch of consecutive base ids is a run; its tokens' bytes
 *   are concatenated and passed through String::from_utf8_lossy.  A special token ends the run before it and starts a new
 *   one after it; with include_special its bytes are emitted verbatim, without it nothing is emitted and it still
 *   separates the two runs.  Tokens of length 0 own no byte and do not end a run; row ends end runs.
 * from_utf8_lossy replaces every maximal invalid subpart by EF BF BD.  It is applied as a rule local to a byte: inside a
 *   run, byte p contributes 0, 1 or 3 output bytes, decided from at most 3 bytes before and after p inside the run.  For
 *   a byte c = s[p] that is no continuation byte (80..BF), sub(p) = (consumed, valid): c < 80: (1, valid); C0, C1,
 *   F5..FF: (1, invalid); a lead byte needs 2 (C2..DF), 3 (E0..EF) or 4 (F0..F4) bytes, its second byte in 80..BF except
 *   E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F, all later ones in 80..BF; k = the bytes that exist inside the run
 *   and fit; k == needed: (needed, valid), else (k, invalid).  A non-continuation byte contributes 1 if sub(p) is valid,
 *   else 3.  A continuation byte at p: q = the nearest non-continuation byte with p - q <= 3 inside the run; if q
 *   exists and q + consumed(q) > p, p contributes 1 when sub(q) is valid and 0 when not; otherwise p is a stray: 3.
 *   tgx_text_num_replaced = the replacement characters written.
 * Stream rule: that of the layouts above.  `stream` is a hipStream_t, NULL the library's blocking stream; the work is
 *   queued there and the call returns after the stream has reached its end.  d_ids, d_mask and d_lengths are checked with
 *   hipPointerGetAttributes before anything is queued (device memory on the model's device, else TGX_ERR_INVALID); NULL
 *   arguments are refused before any device call; the caller's current device is restored.
 * tgx_decode_result: r on the model's device and tgx_result_vocab_size(r) <= V + n_specials, else TGX_ERR_INVALID; r is
 *   only read.  S = 0 or N = 0: TGX_OK and a text with offsets all 0.  The model's token bytes go to its device on the
 *   first decode.  tgx_last_kernel_times is not touched: the kernels run on the caller's stream.
 * A tgx_text holds the bytes and u64 offsets[S+1] in HBM (pooled buffers) until tgx_text_free.  tgx_corpus_from_text:
 *   a resident corpus over its rows, by a device-to-device copy (only the S + 1 offsets visit the host).
 * tgx_decode_rows_host is the host twin over host arrays: the same semantics through the kernels' index arithmetic
 *   (csrc/decode.h), no device.  id_kind: 0 = u32, 1 = i32, 2 = i64 elements; id_offs != NULL selects the offsets form
 *   (mask, lengths, skip_id and row_len are then ignored).  *out_text is malloc'd (tgx_free), out_offs u64[n_rows + 1]. */
typedef struct tgx_text tgx_text;
tgx_status tgx_decode_result(tgx_model *m, const tgx_result *r, const uint8_t *special_bytes, const uint64_t *special_offs,
                             uint32_t n_specials, int include_special, void *stream, tgx_text **out,
                             uint64_t *bad_sample, uint64_t *bad_id);
tgx_status tgx_decode_padded(tgx_model *m, const void *d_ids, uint64_t n_rows, uint64_t row_len, uint32_t flags,
                             const uint8_t *d_mask, const int32_t *d_lengths, uint32_t skip_id,
                             const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                             int include_special, void *stream, tgx_text **out, uint64_t *bad_sample, uint64_t *bad_id);
uint64_t tgx_text_num_rows(const tgx_text *t);
uint64_t tgx_text_num_bytes(const tgx_text *t);
uint64_t tgx_text_num_replaced(const tgx_text *t);
int tgx_text_device(const tgx_text *t);
tgx_status tgx_text_copy_bytes(const tgx_text *t, uint8_t *dst, uint64_t cap);
tgx_status tgx_text_copy_offsets(const tgx_text *t, uint64_t *dst, uint64_t cap);
const void *tgx_text_bytes_device(const tgx_text *t);
const void *tgx_text_offsets_device(const tgx_text *t);
void tgx_text_free(tgx_text *t);
tgx_status tgx_corpus_from_text(const tgx_text *t, tgx_corpus **out);
tgx_status tgx_decode_rows_host(const uint8_t *vocab_bytes, const uint64_t *vocab_offs, uint32_t vocab_size,
                                const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                                const void *ids, uint32_t id_kind, const uint64_t *id_offs, uint64_t n_rows,
                                uint64_t row_len, const uint8_t *mask, const int32_t *lengths, uint32_t skip_id,
                                int include_special, uint8_t **out_text, uint64_t *out_offs, uint64_t *n_replaced,
                                uint64_t *bad_sample, uint64_t *bad_id);

/* ---- token spans on the device: the part of its row's text that every token covers (csrc/spans.hip) ----------------
 * The offsets mapping of a result, in bytes or in characters, written into caller-owned DEVICE memory: neither the ids nor
 * any text visit the host, and no text is needed on the device.  The spans are a function of the ids and the vocabulary.
 *
 * Input: a model with base vocabulary size V; n_specials special tokens (special_bytes / special_offs: host arrays as in
 *   tgx_decode_result); a result r with rows i = 0..S, ids x[0..T) and offsets o[0..S], on the model's device and with
 *   tgx_result_vocab_size(r) <= V + n_specials (TGX_ERR_INVALID otherwise).  Results of encode, sampling, n-best, a
 *   resident corpus and tgx_assemble_result are all taken.
 * For an id x: bytes(x) = its token's bytes, for x >= V those of special token x - V; len(x) = |bytes(x)|; leads(x) = the
 *   number of bytes of bytes(x) that are not in 80..BF; cont(x) = 1 iff len(x) > 0 and the first byte is in 80..BF.
 * Row i's raw text is the concatenation of bytes(x[j]) for o[i] <= j < o[i+1]: with no processors the input sample byte
 *   for byte, with CRLF or NFC the processed sample (what decode gives for valid UTF-8, special tokens included).
 * Byte unit: b_j = the sum of len(x[k]) over o[i] <= k < j, e_j = b_j + len(x[j]); the span of token j is (b_j, e_j).
 * Character unit (flags: TGX_SPAN_CHARS): c(p) = the number of bytes not in 80..BF among the first p bytes of the row's
 *   raw text; the span is (c(b_j) - cont(x[j]), c(e_j)) for len(x[j]) > 0, the smallest range of code points whose bytes
 *   cover the token (two byte tokens that split one CJK character both get that character), and (c(b_j), c(b_j)) for a
 *   token of length 0.  On valid UTF-8 this indexes a Python str.  On invalid bytes it is the same definition over
 *   bytes and nothing more: a token that starts with a byte in 80..BF is attributed to the character before it, and
 *   where there is none (the row's text starts with such bytes) its start is -1.  Only the specials' lengths are read
 *   in the byte unit (special_bytes is not looked at); the character unit reads their bytes.
 * Spans are relative to the whole row, truncated or not.
 * Flat form (tgx_result_spans_device): d_spans[T, 2], element (j, 0) the start and (j, 1) the end of token j.
 * Padded form (tgx_result_pad_spans_device): d_spans[S, L, 2], aligned element for element with what
 *   tgx_result_pad_device writes for the same row_len = L, bos_id, eos_id, TGX_LAYOUT_PAD_LEFT and
 *   TGX_LAYOUT_TRUNC_LEFT (the same row mapping, csrc/layout.h): a kept token gets its span; bos, eos and padding get
 *   (0, 0).  L >= 1 and L >= A, bos_id / eos_id below 2^31 or TGX_NO_ID, else TGX_ERR_INVALID.
 * Elements are int32_t, or int64_t with TGX_LAYOUT_I64.  All sums on the device are 64-bit (a batch holds more than 2^32
 *   bytes long before a row does).  With int32_t, if some row's total in the chosen unit is >= 2^31 the call returns
 *   TGX_ERR_UNSUPPORTED and nothing is written: a device reduction over the rows, of which one word is read back, and
 *   only for int32_t.
 * Stream rule: that of the layouts above.  `stream` is a hipStream_t: pass the stream the destination's allocator
 *   orders its memory on; NULL selects the library's blocking stream.  The work is queued on the chosen stream and the
 *   call returns only after the stream has reached its end.  d_spans must be device memory on the result's device
 *   (checked with hipPointerGetAttributes before anything is queued: TGX_ERR_INVALID otherwise); room for every element
 *   written is the caller's responsibility.  NULL arguments are refused before any device call.  The calling thread's
 *   current device is the same after the call as before.
 * S = 0 or T = 0: TGX_OK; the padded form still fills its S·L·2 elements with 0.  The model's token words (16 bits per
 *   token) go to its device on the first call.  tgx_last_kernel_times is not touched.
 * tgx_spans_host is the host twin over host arrays (vocab_bytes / vocab_offs u64[V+1]; ids u32[T], may be NULL when
 *   T = 0; offs u64[n_rows + 1], offs[0] = 0, ascending): the same semantics through the kernels' index arithmetic
 *   (csrc/spans.h), no device.  row_len = 0 selects the flat form (bos_id, eos_id and the two side flags are then
 *   ignored), out is [T, 2] or [n_rows, row_len, 2].  An id >= V + n_specials: TGX_ERR_TOKEN_ID_OOB. */
#define TGX_SPAN_CHARS 8u
tgx_status tgx_result_spans_device(tgx_model *m, const tgx_result *r, const uint8_t *special_bytes,
                                   const uint64_t *special_offs, uint32_t n_specials, uint32_t flags, void *stream,
                                   void *d_spans);
tgx_status tgx_result_pad_spans_device(tgx_model *m, const tgx_result *r, const uint8_t *special_bytes,
                                       const uint64_t *special_offs, uint32_t n_specials, uint32_t row_len,
                                       uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *stream, void *d_spans);
tgx_status tgx_spans_host(const uint8_t *vocab_bytes, const uint64_t *vocab_offs, uint32_t vocab_size,
                          const uint8_t *special_bytes, const uint64_t *special_offs, uint32_t n_specials,
                          const uint32_t *ids, const uint64_t *offs, uint64_t n_rows, uint32_t row_len,
                          uint32_t bos_id, uint32_t eos_id, uint32_t flags, void *out);

/* ---- resident corpus: the prune / merge training loops -------------------- */
/* The reference holds `samples: &[&str]` in RAM across all EM / merge passes
 * (src/prune.rs:23, src/merge.rs:33); here the batch is uploaded once and stays
 * in HBM while models change.  Samples are processed longest-first. */
tgx_status tgx_corpus_upload(int device, const uint8_t *text, const uint64_t *offs,
                             uint64_t n_samples, tgx_corpus **out);
void tgx_corpus_free(tgx_corpus *c);
uint64_t tgx_corpus_num_samples(const tgx_corpus *c);
uint64_t tgx_corpus_num_bytes(const tgx_corpus *c);

/* Model::encode over every sample of the corpus; result stays in HBM until the
 * host pointers are asked for. */
tgx_status tgx_encode_corpus(tgx_model *m, tgx_corpus *c, double dropout, uint64_t seed,
                             tgx_result **out);

/* ---- subword regularisation: a segmentation drawn from the lattice ---------
 * Kudo 2018 (SentencePiece's enable_sampling, nbest_size = -1): every sample gets one segmentation x drawn with
 * probability P(x | text) ∝ exp(alpha · Σ_{t ∈ x} score(t)) instead of the Viterbi path.  alpha = 0 is uniform over
 * the segmentations; a large alpha approaches encode.  The draw is forward filtering, backward sampling: with
 * A[0] = 0 and A[p] = logsumexp over the matches (q, len), q + len = p, of A[q] + alpha · score, the token ending at
 * p is the match with the largest key A[q] + alpha · score − log(−log u), u = tgx_sample_u01(seed, sample, q, len),
 * exact ties going to the longer token; the path is the back-trace from n.  `sample` is the sample's index in the
 * batch (the corpus form: as uploaded), `q` the match's first byte in the sample, `len` its length in bytes.
 *   alpha must be finite and >= 0 (else TGX_ERR_INVALID); a model with a non-finite score gives
 *   TGX_ERR_UNSUPPORTED; an unreachable end gives TGX_ERR_NO_PATH exactly as tgx_encode_batch on the same batch.
 *   logz (NULL or f64[n_samples], input order) receives every sample's log Z = A[n] under alpha.
 *   Ids and offsets come back in the usual tgx_result. */
/* the uniform of the race: x = seed ^ 0xD6E8FEB86659FD93 ^ sample·0x9E3779B97F4A7C15 ^ pos·0xC2B2AE3D27D4EB4F ^
 * len·0x165667B19E3779F9, the three xor-shift / multiply rounds of tgx_dropout_u01, u = ((x >> 11) + 0.5) · 2^-53 in
 * f64, except that the one value this rounds to 1.0 (x >> 11 = 2^53 − 1) gives the largest double below 1: never 0 or 1 */
double tgx_sample_u01(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len);
tgx_status tgx_encode_batch_sample(tgx_model *m, const uint8_t *text, const uint64_t *offs,
                                   uint64_t n_samples, double alpha, uint64_t seed,
                                   double *logz, tgx_result **out);
tgx_status tgx_encode_corpus_sample(tgx_model *m, tgx_corpus *c, double alpha, uint64_t seed,
                                    double *logz, tgx_result **out);

/* ---- lattice statistics: log Z, expected score and expected token count per sample ---
 * A forward-only sweep over the lattice sampling draws from: for a sample of n bytes the matches are what encode sees
 * with dropout 0, and P(x) ∝ exp(alpha · Σ_{t ∈ x} score(t)) over the segmentations x of the sample.  Per sample:
 *   logz    = log Σ_x exp(alpha · score(x)): the A[n] that tgx_encode_batch_sample reports, log P(text) at alpha = 1;
 *   escore  = E_P[Σ_t score(t)], on the raw scores (not multiplied by alpha);
 *   etokens = E_P[number of tokens of x].
 * The entropy of P is logz − alpha · escore (nats).  Nothing is drawn, traced or returned as ids: the sweep carries the
 * expectation semiring (a, r, c) with r[p] = Σ (r[q]·w + a[q]·w·s), c[p] = Σ (c[q]·w + a[q]·w) over the matches
 * (q, len, w = exp(alpha · s)) ending at p, escore = r[n] / a[n], etokens = c[n] / a[n].
 *   logz, escore, etokens: each NULL or f64[n_samples] in host memory, input order.
 *   An empty sample gives 0, 0, 0.  A sample whose end no path reaches gives logz = −inf and escore = etokens = NaN;
 *   the call still returns TGX_OK, and the number of such samples goes to *n_no_path (NULL or one u64).
 *   alpha must be finite and >= 0, and alpha · score finite for every token (else TGX_ERR_INVALID); a non-finite
 *   score gives TGX_ERR_UNSUPPORTED: the statuses of tgx_encode_batch_sample.  alpha = 0 is the uniform distribution:
 *   logz = log(number of segmentations).  A later duplicate token overrides an earlier one, as in the model.
 *   tgx_lattice_stats_host is the twin: plain f64 on the host over the vocabulary arrays (vocab_offs u64[vocab_size + 1],
 *   any base), in the log-domain formulation of the generic kernel; no device, no model. */
tgx_status tgx_lattice_stats_corpus(tgx_model *m, tgx_corpus *c, double alpha,
                                    double *logz, double *escore, double *etokens, uint64_t *n_no_path);
tgx_status tgx_lattice_stats_batch(tgx_model *m, const uint8_t *text, const uint64_t *offs, uint64_t n_samples,
                                   double alpha, double *logz, double *escore, double *etokens, uint64_t *n_no_path);
tgx_status tgx_lattice_stats_host(const uint8_t *vocab_bytes, const uint64_t *vocab_offs, const double *scores,
                                  uint32_t vocab_size, const uint8_t *text, const uint64_t *offs, uint64_t n_samples,
                                  double alpha, double *logz, double *escore, double *etokens, uint64_t *n_no_path);

/* ---- n-best segmentation: the k highest-scoring segmentations per sample ---
 * SentencePiece's NBestEncode (and the list that SampleEncode with nbest_size > 1 draws from).  For a sample of n
 * bytes the matches are what encode sees with dropout 0: a match is (q, len, id, s), s = score[id].  Every position p
 * gets a list L[p] of at most k entries (score, q, r):
 *   L[0] = [(0.0, -, -)];
 *   L[p] = the top k, in the order below, of all candidates (L[q][r].score + s, q, r) over every match (q, len) with
 *          q + len = p and every r < |L[q]|; the addition is the f64 add encode forms, left to right;
 *   order: score descending, then q ascending (the longer last token first), then r ascending — a strict total
 *          order, so the lists do not depend on how they are merged.
 * Row r of a sample is the back-trace from L[n][r].  Row 0 is tgx_encode_batch's path (encode keeps the first,
 * longest match on a tie); rows are pairwise distinct segmentations with non-increasing scores; and the rows for k
 * are the first k rows for any k' > k (fl(a + s) is monotone in a, and r breaks the ties rounding creates).
 *   *out has n_samples · nbest rows: row s · nbest + r is the r-th best segmentation of sample s, samples in input
 *     order; tgx_result_num_samples returns that row count and the result accessors work unchanged.  Rows at or
 *     beyond n_found are empty.  An empty sample has one empty row of score 0.0.
 *   scores (NULL or f64[n_samples · nbest]): each row's path score, -inf for rows at or beyond n_found.
 *   n_found (NULL or u32[n_samples]): min(nbest, the number of segmentations of the sample).
 *   nbest = 0 or > TGX_MAX_NBEST gives TGX_ERR_INVALID; a model with a non-finite score, or with 2^22 tokens or
 *   more, gives TGX_ERR_UNSUPPORTED; an unreachable end gives TGX_ERR_NO_PATH exactly as tgx_encode_batch on the
 *   same batch.  Any token length up to TGX_MAX_TOKEN_LEN; dropout does not apply. */
#define TGX_MAX_NBEST 16
tgx_status tgx_encode_batch_nbest(tgx_model *m, const uint8_t *text, const uint64_t *offs, uint64_t n_samples,
                                  uint32_t nbest, double *scores, uint32_t *n_found, tgx_result **out);
tgx_status tgx_encode_corpus_nbest(tgx_model *m, tgx_corpus *c, uint32_t nbest,
                                   double *scores, uint32_t *n_found, tgx_result **out);

/* Frequency pass of prune_vocab — src/prune.rs:205-244: freq[id] += 1 for every
 * Viterbi token (dropout 0.0).  freq[vocab_size] is ACCUMULATED into (host). */
tgx_status tgx_count_tokens(tgx_model *m, tgx_corpus *c, uint64_t *freq);

/* Pair scan of merge — src/merge.rs:53-76: adjacent id pairs inside each sample.
 * Returns malloc'd arrays sorted by key = (a << 32) | b; free with tgx_free. */
tgx_status tgx_count_pairs(tgx_model *m, tgx_corpus *c, uint64_t **keys, uint64_t **counts,
                           uint64_t *n_pairs);
/* The same scan, but only the max_pairs MOST FREQUENT pairs come back, ordered by descending count and
 * ascending key among equal counts — the order in which the merge loop consumes them (src/merge.rs:84-126);
 * *n_total = number of distinct pairs.  Saves the copy and the host sort of a table of millions. */
tgx_status tgx_count_pairs_top(tgx_model *m, tgx_corpus *c, uint64_t max_pairs, uint64_t **keys,
                               uint64_t **counts, uint64_t *n_pairs, uint64_t *n_total);

/* run_e_step — src/prune.rs:64-120 over src/model.rs:34-55 + src/lattice.rs:245-333:
 * each sample cut into <= snippet_len-byte snippets, forward/backward in f64
 * log-space, expected[vocab_size] ACCUMULATED into (host), *logz_sum = sum of z.
 * TGX_ERR_Z_NOT_NORMAL where the reference would panic (nothing of the failed
 * pass is added to expected[]).  Tokens of up to 16 bytes, and of up to 32 bytes
 * (vocabularies after `merge`), run the four-snippets-per-wave kernels; longer
 * ones the generic kernel. */
tgx_status tgx_estep(tgx_model *m, tgx_corpus *c, uint64_t snippet_len, double dropout,
                     uint64_t seed, double *expected, double *logz_sum);

void tgx_free(void *p);
/* Scratch and result buffers are recycled through a per-process pool of device buffers (at most a quarter of
 * the device's memory; flushed and retried automatically when an allocation fails).  tgx_pool_trim returns every
 * pooled buffer of `device` (all devices if negative) to the HIP runtime, e.g. before another library needs
 * the memory. */
void tgx_pool_trim(int device);
/* A test knob ("Hostile memory"): with TGX_KNOBS=1 and TGX_POOL_FILL=<0..255> every device buffer the
 * library allocates for itself is set to that byte, over its whole pooled size, before its owner sees it.
 * tgx_pool_filled_bytes: the bytes so filled since the process started; 0 forever without the knob. */
uint64_t tgx_pool_filled_bytes(void);
/* Page-locked host memory for the buffers a caller hands to tgx_encode_batch_host / tgx_corpus_upload and
 * receives ids in: copies from and to such memory are DMA transfers at the link's rate, copies from and to
 * ordinary (pageable) memory go through the driver's staging buffers at about half of it.  NULL (and
 * tgx_last_error) on failure.  (The reference has no counterpart: its tokenizer runs on the host.) */
void *tgx_host_alloc(uint64_t bytes);
void tgx_host_free(void *p);

/* ---- prune host logic (no device needed) ---------------------
 * The O(V) steps of ModelVocabularyPruner between the corpus passes above. */
double tgx_digamma(double x);                                        /* src/prune.rs:322-335 */
/* run_m_step — src/prune.rs:124-170: tokens with expected < 0.5 and !keep are dropped, the
 * others get score = digamma(max(freq, 0.5)) - digamma(sum).  out_* need room for V entries. */
tgx_status tgx_prune_m_step(const double *expected, const uint8_t *keep, uint32_t vocab_size,
                            uint32_t *out_idx, double *out_score, uint32_t *out_n);
/* prune_vocab, first half — src/prune.rs:179-203 over Lattice::nbest(2) (src/lattice.rs:152-238):
 * always_keep[V]; alternatives in CSR form, *alt_ids malloc'd (tgx_free). */
tgx_status tgx_prune_alternatives(const tgx_flat_trie *trie, const uint8_t *bytes, const uint64_t *offs,
                                  const double *scores, uint32_t vocab_size, uint8_t *always_keep,
                                  uint32_t *alt_offs, uint32_t **alt_ids);
/* The same for the vocabulary of a model, over the model's own table (no second trie is built). */
tgx_status tgx_model_prune_alternatives(const tgx_model *m, uint8_t *always_keep, uint32_t *alt_offs, uint32_t **alt_ids);
/* prune_vocab, second half — src/prune.rs:246-318: ids of the pruned vocabulary in its final
 * order (score descending).  out_idx needs room for V entries. */
tgx_status tgx_prune_select(const uint64_t *freq, const uint8_t *keep, const uint8_t *always_keep,
                            const uint32_t *alt_offs, const uint32_t *alt_ids, const double *scores,
                            uint32_t vocab_size, uint64_t n_samples, uint32_t pruned_size,
                            uint32_t *out_idx, uint32_t *out_n);

/* ---- measurement ---------------------------------------------------------- */
/* Per-kernel GPU time of the last pass on this model's stream, measured with
 * hipEvents recorded on that stream around each launch.  names[i] are static
 * strings.  Returns the number of kernels written (<= cap). */
int tgx_last_kernel_times(const tgx_model *m, const char **names, float *ms, int cap);
/* Algorithmic bytes of the last pass, SURVEY.md §8(d): encode N + 4T + 16(S+1). */
uint64_t tgx_last_algorithmic_bytes(const tgx_model *m);
/* waves per CU the last four-samples-per-wave encode launch really had resident (occupancy query for
 * its kernel variant, block size and LDS): a self-check that the launch geometry fits the device. */
uint32_t tgx_last_encode_waves_per_cu(const tgx_model *m);
/* samples the last encode of a vocabulary with tokens of 17..32 bytes had to redo with the
 * two-samples-per-wave kernel because a wave ran out of overflow entries for long matches (0 = none). */
uint64_t tgx_last_encode_redo_samples(const tgx_model *m);
/* samples of the last encode pass that had a block of their own (the long-sample kernel) */
uint64_t tgx_last_encode_long_samples(const tgx_model *m);
/* pieces the last tgx_estep pass cut its snippets into at positions no token match crosses (the lattice factorises
 * there, so expected counts and log Z of the pieces add up to the snippets': csrc/cuts.hip); 0: snippets uncut. */
uint64_t tgx_last_estep_pieces(const tgx_model *m);
/* stretches of text the last tgx_estep pass on estep7_kernel (one walk per position: every trip of 16 .. 64 positions a
 * lattice of its own between two positions no match crosses) could not close within a trip and handed to its redo
 * pass (csrc/estep7.hip); 0: none. */
uint64_t tgx_last_estep_redo(const tgx_model *m);
/* CUs the long-sample kernel had to itself while encode5_kernel ran on the others in the last encode pass
 * (batches of a few hundred MB whose longest samples bound either kernel alone); 0: the kernels ran one after the other. */
uint32_t tgx_last_encode_corun_cus(const tgx_model *m);
/* co-run passes of this model whose host-side wait for the resident blocks of encode5_kernel ran into its 2 ms limit
 * (0 in a healthy setup; after the first one the model launches its two encode kernels one after the other). */
uint32_t tgx_encode_corun_timeouts(const tgx_model *m);
/* distinct score values of the vocabulary as the rows5 encode kernels rank them (0: the model has no 8-byte
 * records — tokens longer than 16 bytes, non-finite scores, more than 65 535 distinct values — or has not
 * encoded yet when it was created for E-step passes), and how many of them the last encode5_kernel launch
 * kept in its block's LDS (the rest are read from L2 by the relaxing lanes). */
uint32_t tgx_model_score_values(const tgx_model *m);
uint32_t tgx_last_encode_hot_values(const tgx_model *m);
/* Which of the lean items the kernels of the last rows5 encode pass were built with (a self-check: results do not
 * depend on it): bits 0-7 encode5_kernel's, bits 8-15 encode6_kernel's, of 1 = lean relaxation step, 2 = broadcast
 * through the compiler's builtin and 4 = one-instruction score fetch.  0: the kernels
 * as they were (dropout, tokens longer than 16 bytes, TGX_E5_LEAN=0, or another encode path).  Bit 0 is set only for
 * the build that has the lean step (every token its own score at three positions per lane) and only for a model
 * whose scores all have a magnitude below 2^960; other models run that build without the step. */
uint32_t tgx_last_encode_lean_items(const tgx_model *m);
/* 1 when the last encode pass wrote its ids in place (a self-check: results do not depend on it): encode5_kernel
 * counted every sample's tokens in its relaxation, the counts were scanned into the result's offsets and the trace
 * wrote each id where it belongs — no scratch of 4 bytes per text byte, no compaction.  0: the pass went through that
 * scratch and compact_kernel (dropout, tokens longer than 16 bytes, samples sent to encode6_kernel, a sample of 2^24
 * bytes or more, a build of encode5_kernel that does not count, TGX_IDS_IN_PLACE=0, or another encode path). */
int tgx_last_encode_ids_in_place(const tgx_model *m);
/* 1 when the last encode pass's encode5_kernel was a top-table build (a self-check: results do not depend on it): a
 * walk's first two trie levels came from one table indexed by the first two text bytes, and the block's LDS held no copy
 * of the root's records — room for more hot score values, or for one more wave.  0: the kernel kept its root copy
 * (dropout, tokens longer than 16 bytes, TGX_E5_TOP=0), was not launched, or the pass took another encode path. */
int tgx_last_encode_top_table(const tgx_model *m);

/* ---- dropout ---------------------------------------------------------------
 * The reference draws rand::random::<f64>() from an unseeded thread RNG
 * (src/model.rs:48,100), so dropout > 0 is not reproducible there.  This build
 * replaces it with a counter hash of (seed, sample index, byte position, token
 * length) so that runs are reproducible and the CPU oracle and the HIP kernels
 * make identical decisions.  encode keeps a multi-byte match iff dropout < u
 * (model.rs:100); populate_nodes skips it iff u < dropout (model.rs:48). */
static inline double tgx_dropout_u01(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len) {
    uint64_t x = seed ^ (sample * 0x9E3779B97F4A7C15ULL) ^ (pos * 0xC2B2AE3D27D4EB4FULL) ^
                 ((uint64_t)len * 0x165667B19E3779F9ULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

#ifdef __cplusplus
}
#endif
#endif /* TGX_H */
