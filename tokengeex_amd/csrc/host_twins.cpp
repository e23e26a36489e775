// The *_host twins of the result-side device entry points (include/tgx.h): tgx_layout_pad_host, tgx_layout_pack_host,
// tgx_layout_windows_host, tgx_assemble_host, tgx_fim_host, tgx_select_host, tgx_select_text_host, tgx_shuffled_rows_host, tgx_first_equal_host, tgx_minhash_host, tgx_minhash_bands_host, tgx_minhash_near_first_host, tgx_gram_keys_host, tgx_gram_hits_host, tgx_gram_contains_host, tgx_repeat_stats_host, tgx_text_stats_host, tgx_lines_host, tgx_word_stats_host (include/tgx_words.h), tgx_phrase_hits_host (include/tgx_phrases.h), tgx_decode_rows_host, tgx_spans_host, tgx_window_spans_host, tgx_front_host,
// tgx_normalize_host and tgx_lattice_stats_host, and the
// argument checks they share with the device entry points of tgx_api.cpp.  A twin goes through the same index arithmetic as its kernels (layout.h, assemble.h,
// fim.h, select.h, dedup.h, minhash.h, gram.h, repeat.h, textstat.h, wordstat.h, decode.h, spans.h, front.h, norm.h) on host memory.  Nothing in this file calls a HIP function, so it builds and runs without the
// handles, the pool or a device.
#define TGX_HOST_ONLY  // tile_fill.h: the host loop, no kernel side
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "api_internal.h"
#include "assemble.h"
#include "decode.h"
#include "dedup.h"
#include "fim.h"
#include "front.h"
#include "gram.h"
#include "layout.h"
#include "minhash.h"
#include "norm.h"
#include "phrase.h"
#include "repeat.h"
#include "select.h"
#include "spans.h"
#include "textstat.h"
#include "unicode_tables.h"
#include "wordstat.h"
#include "../../include/tgx_phrases.h"
#include "../../include/tgx_words.h"

using namespace tgx::host;

// ---- argument checks ----------------------------------------------------------------

namespace {

// A packed list of n items: offs[0 .. n] does not decrease, and starts at 0 where from_zero.  `name` is what the messages
// call the argument and `plural` its entries.  offs may be NULL only for an empty list that need not start at 0.
tgx_status check_packed_list(const char* who, const char* name, const char* plural, const uint64_t* offs, uint64_t n, bool from_zero) {
    if (!offs && (n || from_zero)) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, name);
    if (from_zero && offs[0] != 0) return fail(TGX_ERR_INVALID, "%s: %s[0] must be 0", who, name);
    for (uint64_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i]) return fail(TGX_ERR_INVALID, "%s: %s not monotone at %llu", who, plural, (unsigned long long)i);
    return TGX_OK;
}

// the special tokens' ids follow the vocabulary's, and TGX_NO_ID is none of them
tgx_status check_id_room(const char* who, uint32_t vocab_size, uint32_t n_specials) {
    if ((uint64_t)vocab_size + n_specials > 0xFFFFFFFEull)
        return fail(TGX_ERR_INVALID, "%s: %u tokens and %u special tokens leave no room for their ids", who, vocab_size, n_specials);
    return TGX_OK;
}

}  // namespace

namespace tgx::host {

// a padded row holds at least one element, and its bos / eos (extra: tgx::LayoutSeq::extra)
tgx_status layout_check_row_len(const char* who, uint32_t row_len, uint32_t extra) {
    if (row_len < 1 || row_len < extra) return fail(TGX_ERR_INVALID, "%s: row_len %u (needs >= 1 and >= %u for bos / eos)", who, row_len, extra);
    return TGX_OK;
}

// TGX_OK when every id a layout writes besides the tokens' is below 2^31 (pad always, bos / eos when present)
tgx_status layout_check_ids(const char* who, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id) {
    if (pad_id >= 0x80000000u) return fail(TGX_ERR_INVALID, "%s: pad_id %u is not below 2^31", who, pad_id);
    if (bos_id != TGX_NO_ID && bos_id >= 0x80000000u) return fail(TGX_ERR_INVALID, "%s: bos_id %u is not below 2^31", who, bos_id);
    if (eos_id != TGX_NO_ID && eos_id >= 0x80000000u) return fail(TGX_ERR_INVALID, "%s: eos_id %u is not below 2^31", who, eos_id);
    return TGX_OK;
}

tgx_status layout_check_flags(const char* who, uint32_t flags, uint32_t allowed) {
    if (flags & ~allowed) return fail(TGX_ERR_INVALID, "%s: unknown flags 0x%x", who, flags & ~allowed);
    return TGX_OK;
}

// a window holds its bos / eos and at least one token, and moves on by at least one token
tgx_status window_check_args(const char* who, uint32_t row_len, uint32_t stride, uint32_t extra) {
    if (row_len < extra + 1) return fail(TGX_ERR_INVALID, "%s: row_len %u (needs >= %u: bos / eos and one token)", who, row_len, extra + 1);
    if (stride >= row_len - extra)
        return fail(TGX_ERR_INVALID, "%s: stride %u (needs < %u, the tokens of a window)", who, stride, row_len - extra);
    return TGX_OK;
}

tgx_status window_check_totals(const char* who, uint64_t max_row, uint64_t n_windows, const uint64_t* sized_for) {
    if (max_row >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: a row of %llu tokens (2^31 or more)", who, (unsigned long long)max_row);
    if (n_windows >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: %llu windows (2^31 or more)", who, (unsigned long long)n_windows);
    if (sized_for && *sized_for != n_windows)
        return fail(TGX_ERR_INVALID, "%s: %llu windows, the caller's n_windows is %llu", who, (unsigned long long)n_windows,
                    (unsigned long long)*sized_for);
    return TGX_OK;
}

tgx_status layout_check_host(const char* who, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows) {
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    if (offs[n_rows] && !ids) return fail(TGX_ERR_INVALID, "%s: ids is NULL", who);
    return TGX_OK;
}

tgx_status fim_check(const char* who, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id, double rate, double spm_rate) {
    if (!(rate >= 0.0 && rate <= 1.0)) return fail(TGX_ERR_INVALID, "%s: rate %g is not in [0, 1]", who, rate);
    if (!(spm_rate >= 0.0 && spm_rate <= 1.0)) return fail(TGX_ERR_INVALID, "%s: spm_rate %g is not in [0, 1]", who, spm_rate);
    if (prefix_id == TGX_NO_ID || suffix_id == TGX_NO_ID || middle_id == TGX_NO_ID)
        return fail(TGX_ERR_INVALID, "%s: a sentinel id is TGX_NO_ID", who);
    if (prefix_id == suffix_id || prefix_id == middle_id || suffix_id == middle_id)
        return fail(TGX_ERR_INVALID, "%s: the sentinel ids %u, %u, %u are not pairwise distinct", who, prefix_id, suffix_id, middle_id);
    return TGX_OK;
}

uint32_t fim_vocab_size(uint32_t vocab_size, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id) {
    return std::max(vocab_size, 1u + std::max(prefix_id, std::max(suffix_id, middle_id)));  // (no sentinel is 0xFFFFFFFF)
}

tgx_status result_check_host(const char* who, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t vocab_size) {
    const tgx_status st = layout_check_host(who, ids, offs, n_rows);
    if (st != TGX_OK) return st;
    if (vocab_size > 0xFFFFFFFEu) return fail(TGX_ERR_INVALID, "%s: vocab_size %u leaves no room for TGX_NO_ID", who, vocab_size);
    for (uint64_t j = 0, T = offs[n_rows]; j < T; j++)
        if (ids[j] >= vocab_size) return fail(TGX_ERR_INVALID, "%s: id %u at %llu is not below vocab_size %u", who, ids[j], (unsigned long long)j, vocab_size);
    return TGX_OK;
}

// What tgx_assemble_result and tgx_assemble_host check of a split plan before anything runs.  n_rows: the rows of the
// segment-level result (0 without one).  *n_segs = K.
tgx_status assemble_check(const char* who, const uint64_t* seg_offs, const int32_t* seg_special, uint64_t n_samples, uint32_t vocab_size,
                          uint32_t n_specials, bool have_segs, uint64_t n_rows, uint64_t* n_segs) {
    tgx_status st = check_packed_list(who, "seg_offs", "seg_offs", seg_offs, n_samples, true);
    if (st != TGX_OK) return st;
    const uint64_t K = seg_offs[n_samples];
    if (K && !seg_special) return fail(TGX_ERR_INVALID, "%s: seg_special is NULL", who);
    if ((st = check_id_room(who, vocab_size, n_specials)) != TGX_OK) return st;
    uint64_t E = 0;
    for (uint64_t k = 0; k < K; k++) {
        if (seg_special[k] < 0)
            E++;
        else if ((uint32_t)seg_special[k] >= n_specials)
            return fail(TGX_ERR_INVALID, "%s: segment %llu is special token %d of %u", who, (unsigned long long)k, seg_special[k], n_specials);
    }
    if (E && !have_segs) return fail(TGX_ERR_INVALID, "%s: %llu encoded segments and no result over them", who, (unsigned long long)E);
    if (E != n_rows)
        return fail(TGX_ERR_INVALID, "%s: %llu encoded segments, the result over them has %llu rows", who, (unsigned long long)E,
                    (unsigned long long)n_rows);
    *n_segs = K;
    return TGX_OK;
}

// lengths and 16-byte slots of a vocabulary's tokens: what the kernels (device copies) and the host twin read
tgx_status decode_build_tables(const char* who, const uint8_t* bytes, const uint64_t* offs, uint32_t V, std::vector<uint8_t>* len,
                               std::vector<tgx::DecodeSlot>* slots) {
    const tgx_status st = check_packed_list(who, "vocabulary offsets", "vocabulary offsets", offs, V, false);
    if (st != TGX_OK) return st;
    len->assign(V, 0);
    slots->assign(V, tgx::DecodeSlot{0, 0});
    for (uint32_t i = 0; i < V; i++) {
        const uint64_t n = offs[i + 1] - offs[i];
        if (n > TGX_MAX_TOKEN_LEN) return fail(TGX_ERR_UNSUPPORTED, "%s: token of %llu bytes exceeds TGX_MAX_TOKEN_LEN (%d)", who, (unsigned long long)n, TGX_MAX_TOKEN_LEN);
        (*len)[i] = (uint8_t)n;
        if (n > tgx::kDecodeSlotLen) continue;
        tgx::DecodeSlot& sl = (*slots)[i];
        for (uint64_t k = 0; k < n; k++) (k < 8 ? sl.lo : sl.hi) |= (uint64_t)bytes[offs[i] + k] << (8 * (k & 7));
    }
    return TGX_OK;
}

tgx_status decode_check_specials(const char* who, uint32_t vocab_size, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials) {
    tgx_status st = check_packed_list(who, "special_offs", "special_offs", special_offs, n_specials, false);
    if (st == TGX_OK) st = check_id_room(who, vocab_size, n_specials);
    if (st != TGX_OK) return st;
    for (uint32_t k = 0; k < n_specials; k++)
        if (special_offs[k + 1] - special_offs[k] >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: special token %u is 2 GiB or longer", who, k);
    if (n_specials && special_offs[n_specials] > special_offs[0] && !special_bytes) return fail(TGX_ERR_INVALID, "%s: special_bytes is NULL", who);
    return TGX_OK;
}

tgx_status decode_oob(uint32_t kind, int64_t x, uint64_t row, uint64_t* bad_sample, uint64_t* bad_id) {
    if (bad_sample) *bad_sample = row;
    if (bad_id) *bad_id = (uint64_t)x;
    g_err_sample = row;
    g_err_pos = (uint64_t)x;
    if (kind == tgx::kDecodeU32) return fail(TGX_ERR_TOKEN_ID_OOB, "token id %llu is out of bounds", (unsigned long long)x);
    return fail(TGX_ERR_TOKEN_ID_OOB, "token id %lld is out of bounds", (long long)x);
}

// one word per token of a vocabulary: what the meta kernel (a device copy) and the host twin read
tgx_status span_build_words(const char* who, const uint8_t* bytes, const uint64_t* offs, uint32_t V, std::vector<uint16_t>* words) {
    const tgx_status st = check_packed_list(who, "vocabulary offsets", "vocabulary offsets", offs, V, false);
    if (st != TGX_OK) return st;
    words->assign(V, 0);
    for (uint32_t i = 0; i < V; i++) {
        const uint64_t n = offs[i + 1] - offs[i];
        if (n > TGX_MAX_TOKEN_LEN) return fail(TGX_ERR_UNSUPPORTED, "%s: token of %llu bytes exceeds TGX_MAX_TOKEN_LEN (%d)", who, (unsigned long long)n, TGX_MAX_TOKEN_LEN);
        (*words)[i] = tgx::span_word(bytes + offs[i], (uint32_t)n);
    }
    return TGX_OK;
}

// the special tokens' words; the byte unit reads no byte of theirs
void span_special_words(const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials, bool chars, std::vector<uint64_t>* words) {
    words->assign((size_t)n_specials + 1, 0);
    for (uint32_t k = 0; k < n_specials; k++)
        (*words)[k] = tgx::span_special_word(chars ? special_bytes + special_offs[k] : nullptr, special_offs[k + 1] - special_offs[k]);
}

// flags, specials and the padded form's arguments: what the device entry points and the host twin check alike
tgx_status span_check_args(const char* who, uint32_t vocab_size, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials,
                           bool padded, uint32_t row_len, uint32_t bos_id, uint32_t eos_id, uint32_t flags) {
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_I64 | TGX_SPAN_CHARS | (padded ? TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT : 0u));
    static const uint8_t unread = 0;  // the byte unit does not look at special_bytes, which may then be NULL
    if (st == TGX_OK) st = decode_check_specials(who, vocab_size, (flags & TGX_SPAN_CHARS) ? special_bytes : &unread, special_offs, n_specials);
    if (st == TGX_OK && padded) st = layout_check_ids(who, 0, bos_id, eos_id);
    if (st != TGX_OK) return st;
    return padded ? layout_check_row_len(who, row_len, tgx::layout_seq(bos_id, eos_id, 0).extra) : TGX_OK;
}

tgx_status span_too_long(const char* who, uint64_t row_max, bool chars) {
    return fail(TGX_ERR_UNSUPPORTED, "%s: a row of %llu %s does not fit int32 spans (TGX_LAYOUT_I64 takes it)", who, (unsigned long long)row_max,
                chars ? "characters" : "bytes");
}

// The special tokens as the front kernels read them (front.h: FrontTables), from 0: what tgx_corpus_split_specials uploads
// and tgx_front_host reads.  An empty special is refused as tgx_split_specials refuses it.
tgx_status front_build_tables(const char* who, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials, FrontHostTables* t) {
    tgx_status st = check_packed_list(who, "special_offs", "special_offs", special_offs, n_specials, false);
    if (st != TGX_OK) return st;
    const uint64_t total = n_specials ? special_offs[n_specials] - special_offs[0] : 0;
    if (total && !special_bytes) return fail(TGX_ERR_INVALID, "%s: special_bytes is NULL", who);
    for (uint32_t k = 0; k < n_specials; k++)
        if (special_offs[k + 1] == special_offs[k]) return fail(TGX_ERR_INVALID, "empty special token (the reference's splitter would never advance)");
    if (n_specials > tgx::kFrontMaxSpecials || total > tgx::kFrontMaxSpecialBytes)
        return fail(TGX_ERR_UNSUPPORTED, "%s: %u special tokens of %llu bytes (at most %u of %llu bytes)", who, n_specials, (unsigned long long)total,
                    tgx::kFrontMaxSpecials, (unsigned long long)tgx::kFrontMaxSpecialBytes);
    t->first_mask.assign(8, 0);
    t->first_start.assign(257, 0);
    t->by_first.assign(n_specials, 0);
    t->sp_offs.assign((size_t)n_specials + 1, 0);
    t->sp_bytes.assign(special_bytes ? special_bytes + (n_specials ? special_offs[0] : 0) : nullptr,
                       special_bytes ? special_bytes + (n_specials ? special_offs[0] : 0) + total : nullptr);
    t->max_len = 0;
    for (uint32_t k = 0; k < n_specials; k++) {
        t->sp_offs[k + 1] = (uint32_t)(special_offs[k + 1] - special_offs[0]);
        const uint32_t b = t->sp_bytes[t->sp_offs[k]];
        t->first_mask[b >> 5] |= 1u << (b & 31);
        t->first_start[b + 1]++;
        t->max_len = std::max(t->max_len, t->sp_offs[k + 1] - t->sp_offs[k]);
    }
    t->firsts.clear();
    for (uint32_t b = 0; b < 256; b++) {
        if (t->first_start[b + 1]) t->firsts.push_back((uint8_t)b);
        t->first_start[b + 1] += t->first_start[b];
    }
    std::vector<uint32_t> at(t->first_start.begin(), t->first_start.end() - 1);
    for (uint32_t k = 0; k < n_specials; k++) t->by_first[at[t->sp_bytes[t->sp_offs[k]]]++] = k;  // ascending k: list order
    return TGX_OK;
}

// the tables over the given copies of the arrays (host memory for the twin, device memory for the kernels)
tgx::FrontTables front_tables(const FrontHostTables& t, const uint32_t* first_mask, const uint32_t* first_start, const uint32_t* by_first,
                              const uint32_t* sp_offs, const uint8_t* sp_bytes) {
    tgx::FrontTables tab = {first_mask, first_start, by_first, sp_offs, sp_bytes, (uint32_t)t.firsts.size(), {0, 0, 0, 0}};
    for (size_t k = 0; k < t.firsts.size() && k < tgx::kFrontFirstBytes; k++) tab.first_bytes[k] = t.firsts[k];
    return tab;
}

}  // namespace tgx::host

// ---- layouts ----------------------------------------------------------------------

namespace {

template <class T>
tgx_status layout_pad_host(const tgx::LayoutSeq& seq, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t L, uint32_t flags,
                           T* out, uint8_t* mask, int32_t* lengths, uint64_t* n_truncated) {
    // as the kernel: the flat [S, L] output in groups of kLayoutGroup consecutive elements, each walked by pad_group
    const uint64_t total = n_rows * (uint64_t)L;
    unsigned long long truncated = 0;
    for (uint64_t e0 = 0; e0 < total; e0 += tgx::kLayoutGroup) {
        const uint32_t n_in = total - e0 < tgx::kLayoutGroup ? (uint32_t)(total - e0) : tgx::kLayoutGroup;
        uint32_t v[tgx::kLayoutGroup] = {0, 0, 0, 0};
        const uint32_t m = tgx::pad_group(seq, ids, offs, L, flags, e0, n_in, lengths, v, &truncated);
        for (uint32_t k = 0; k < n_in; k++) {
            if (v[k] >= 0x80000000u)
                return fail(TGX_ERR_INVALID, "tgx_layout_pad_host: id %u of row %llu is not below 2^31", v[k], (unsigned long long)((e0 + k) / L));
            out[e0 + k] = (T)v[k];
            if (mask) mask[e0 + k] = (uint8_t)(m >> (8 * k));
        }
    }
    if (n_truncated) *n_truncated = truncated;
    return TGX_OK;
}

template <class T>
tgx_status layout_pack_host(const tgx::LayoutSeq& seq, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint64_t n_stream,
                            uint64_t n_out, T* out, int32_t* doc, int32_t* pos) {
    // as the kernel: the tiled fill over the stream's positions, which runs on over the padding of the last block
    tgx_status st = TGX_OK;
    tgx::tiled_fill_host(
        n_out, n_stream, tgx::kPackTile, tgx::kLayoutGroup, 0, [&](uint64_t j) { return tgx::pack_find_row(offs, seq.extra, 0, n_rows - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            tgx::PackCursor cur;
            for (uint32_t k = 0; k < n_in; k++) {
                const uint64_t j = e0 + k;
                uint32_t id = seq.pad;
                int32_t d = -1, q = 0;
                if (j < n_stream) {
                    const uint64_t i = tgx::pack_advance(cur, offs, seq.extra, lo, hi, j);
                    id = tgx::pack_at(seq, ids, offs, i, j, &q);
                    d = (int32_t)i;
                    if (id >= 0x80000000u) {
                        st = fail(TGX_ERR_INVALID, "tgx_layout_pack_host: id %u of row %llu is not below 2^31", id, (unsigned long long)i);
                        return false;
                    }
                }
                out[j] = (T)id;
                if (doc) doc[j] = d;
                if (pos) pos[j] = q;
            }
            return true;
        });
    return st;
}

}  // namespace

tgx_status tgx_layout_pad_host(const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t row_len, uint32_t pad_id,
                               uint32_t bos_id, uint32_t eos_id, uint32_t flags, void* out_ids, uint8_t* out_mask,
                               int32_t* out_lengths, uint64_t* n_truncated) {
    const char* who = "tgx_layout_pad_host";
    if (!out_ids && n_rows) return fail(TGX_ERR_INVALID, "%s: out_ids is NULL", who);
    tgx_status st = layout_check_host(who, ids, offs, n_rows);
    if (st == TGX_OK) st = layout_check_flags(who, flags, TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT | TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    if ((st = layout_check_row_len(who, row_len, seq.extra)) != TGX_OK) return st;
    if (flags & TGX_LAYOUT_I64)
        return layout_pad_host(seq, ids, offs, n_rows, row_len, flags, static_cast<int64_t*>(out_ids), out_mask, out_lengths, n_truncated);
    return layout_pad_host(seq, ids, offs, n_rows, row_len, flags, static_cast<int32_t*>(out_ids), out_mask, out_lengths, n_truncated);
}

tgx_status tgx_layout_pack_host(const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t block_len, uint32_t pad_id,
                                uint32_t bos_id, uint32_t eos_id, uint32_t flags, void* out_ids, int32_t* out_doc,
                                int32_t* out_pos, uint64_t* n_blocks) {
    const char* who = "tgx_layout_pack_host";
    if (!n_blocks) return fail(TGX_ERR_INVALID, "%s: n_blocks is NULL", who);
    tgx_status st = layout_check_host(who, ids, offs, n_rows);
    if (st == TGX_OK) st = layout_check_flags(who, flags, TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    if (block_len < 1) return fail(TGX_ERR_INVALID, "%s: block_len is 0", who);
    if (n_rows >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^31 rows or more", who);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    const uint64_t n_stream = offs[n_rows] + n_rows * seq.extra;
    const uint64_t nb = (n_stream + block_len - 1) / block_len;
    *n_blocks = nb;
    if (nb == 0) return TGX_OK;
    if (!out_ids) return fail(TGX_ERR_INVALID, "%s: out_ids is NULL", who);
    if (flags & TGX_LAYOUT_I64)
        return layout_pack_host(seq, ids, offs, n_rows, n_stream, nb * block_len, static_cast<int64_t*>(out_ids), out_doc, out_pos);
    return layout_pack_host(seq, ids, offs, n_rows, n_stream, nb * block_len, static_cast<int32_t*>(out_ids), out_doc, out_pos);
}

namespace {

// as the count kernel and the scan: Wo[0 .. S] and the longest row
void windows_host_offsets(const uint64_t* offs, uint64_t n_rows, uint32_t room, uint32_t step, std::vector<uint64_t>* wo, uint64_t* max_row) {
    wo->assign((size_t)n_rows + 1, 0);
    *max_row = 0;
    for (uint64_t i = 0; i < n_rows; i++) {
        const uint64_t n = offs[i + 1] - offs[i], nw = tgx::window_count(n, room, step);
        (*wo)[i + 1] = (*wo)[i] + (nw < 0xFFFFFFFFull ? nw : 0xFFFFFFFFull);
        *max_row = std::max(*max_row, n);
    }
}

template <class T>
tgx_status layout_windows_host(const tgx::LayoutSeq& seq, const uint32_t* ids, const uint64_t* offs, const uint64_t* wo, uint64_t n_rows,
                               uint64_t n_windows, uint32_t L, uint32_t stride, uint32_t flags, T* out, uint8_t* mask, int32_t* lengths,
                               int32_t* window_row, int32_t* window_first) {
    // as the kernel: the tiled fill over the elements of the flat [W, L] output, whose owners are the rows of their windows
    const uint64_t total = n_windows * (uint64_t)L;
    tgx_status st = TGX_OK;
    tgx::tiled_fill_host(
        total, total, tgx::kPackTile, tgx::kLayoutGroup, 0, [&](uint64_t e) { return tgx::pack_find_row(wo, 0, 0, n_rows - 1, e / L); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint32_t v[tgx::kLayoutGroup] = {0, 0, 0, 0};
            const uint32_t m = tgx::win_group(seq, ids, offs, wo, L, stride, flags, lo, hi, e0, n_in, lengths, window_row, window_first, v);
            for (uint32_t k = 0; k < n_in; k++) {
                if (v[k] >= 0x80000000u) {
                    st = fail(TGX_ERR_INVALID, "tgx_layout_windows_host: id %u of window %llu is not below 2^31", v[k],
                              (unsigned long long)((e0 + k) / L));
                    return false;
                }
                out[e0 + k] = (T)v[k];
                if (mask) mask[e0 + k] = (uint8_t)(m >> (8 * k));
            }
            return true;
        });
    return st;
}

}  // namespace

tgx_status tgx_layout_windows_host(const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t row_len, uint32_t stride, uint32_t pad_id,
                                   uint32_t bos_id, uint32_t eos_id, uint32_t flags, uint64_t n_windows, void* out_ids, uint8_t* out_mask,
                                   int32_t* out_lengths, int32_t* out_window_row, int32_t* out_window_first, uint64_t* n_windows_out) {
    const char* who = "tgx_layout_windows_host";
    if (!n_windows_out) return fail(TGX_ERR_INVALID, "%s: n_windows_out is NULL", who);
    tgx_status st = layout_check_host(who, ids, offs, n_rows);
    if (st == TGX_OK) st = layout_check_flags(who, flags, TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT | TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    if ((st = window_check_args(who, row_len, stride, seq.extra)) != TGX_OK) return st;
    std::vector<uint64_t> wo;
    uint64_t max_row = 0;
    windows_host_offsets(offs, n_rows, row_len - seq.extra, row_len - seq.extra - stride, &wo, &max_row);
    const uint64_t W = wo[n_rows];
    if ((st = window_check_totals(who, max_row, W, nullptr)) != TGX_OK) return st;
    *n_windows_out = W;
    if (!out_ids) return TGX_OK;
    if ((st = window_check_totals(who, max_row, W, &n_windows)) != TGX_OK || W == 0) return st;
    if (flags & TGX_LAYOUT_I64)
        return layout_windows_host(seq, ids, offs, wo.data(), n_rows, W, row_len, stride, flags, static_cast<int64_t*>(out_ids), out_mask,
                                   out_lengths, out_window_row, out_window_first);
    return layout_windows_host(seq, ids, offs, wo.data(), n_rows, W, row_len, stride, flags, static_cast<int32_t*>(out_ids), out_mask,
                               out_lengths, out_window_row, out_window_first);
}

// ---- assembly ---------------------------------------------------------------------

tgx_status tgx_assemble_host(const uint32_t* ids, const uint64_t* id_offs, uint64_t n_encoded, const uint64_t* seg_offs,
                             const int32_t* seg_special, uint64_t n_samples, uint32_t vocab_size, uint32_t n_specials, uint32_t* out_ids,
                             uint64_t ids_cap, uint64_t* out_offs) {
    const char* who = "tgx_assemble_host";
    if (!out_offs) return fail(TGX_ERR_INVALID, "%s: out_offs is NULL", who);
    uint64_t K = 0;
    tgx_status st = assemble_check(who, seg_offs, seg_special, n_samples, vocab_size, n_specials, id_offs != nullptr, n_encoded, &K);
    if (st != TGX_OK) return st;
    static const uint64_t kNoOffs[1] = {0};
    if (!id_offs) id_offs = kNoOffs;
    if ((st = layout_check_host(who, ids, id_offs, n_encoded)) != TGX_OK) return st;
    const uint64_t n_out = id_offs[n_encoded] + (K - n_encoded);
    if (ids_cap < n_out) return fail(TGX_ERR_INVALID, "%s: %llu ids, room for %llu", who, (unsigned long long)n_out, (unsigned long long)ids_cap);
    if (n_out && !out_ids) return fail(TGX_ERR_INVALID, "%s: out_ids is NULL", who);
    // as the device: the ranks, the starts with the samples' offsets, then the kernel's tiles and thread slots
    std::vector<uint64_t> rank(K + 1), starts(K + 1);
    for (uint64_t k = 0, r = 0; k <= K; k++) {
        rank[k] = r;
        if (k < K && seg_special[k] < 0) r++;
    }
    for (uint64_t k = 0; k <= K; k++) starts[k] = tgx::assemble_seg_start(id_offs, rank.data(), k);
    for (uint64_t i = 0; i <= n_samples; i++) out_offs[i] = tgx::assemble_seg_start(id_offs, rank.data(), seg_offs[i]);
    tgx::tiled_fill_host(
        n_out, n_out, tgx::kAssembleTile, tgx::kAssembleGroup, 0, [&](uint64_t j) { return tgx::pack_find_row(starts.data(), 0, 0, K - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint32_t v[tgx::kAssembleGroup] = {0, 0, 0, 0};
            tgx::assemble_group(ids, starts.data(), rank.data(), seg_special, vocab_size, lo, hi, e0, n_in, v);
            for (uint32_t q = 0; q < n_in; q++) out_ids[e0 + q] = v[q];
            return true;
        });
    return TGX_OK;
}

// ---- fill-in-the-middle -------------------------------------------------------------

double tgx_fim_u01(uint64_t seed, uint64_t row, uint64_t draw) { return tgx::fim_u01(seed, row, draw); }

tgx_status tgx_fim_host(const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t vocab_size, uint32_t prefix_id, uint32_t suffix_id,
                        uint32_t middle_id, double rate, double spm_rate, uint64_t seed, uint64_t first_row, uint32_t* out_ids, uint64_t ids_cap,
                        uint64_t* out_offs, uint8_t* mode, uint64_t* cuts, uint64_t* n_applied) {
    const char* who = "tgx_fim_host";
    if (!out_offs) return fail(TGX_ERR_INVALID, "%s: out_offs is NULL", who);
    tgx_status st = fim_check(who, prefix_id, suffix_id, middle_id, rate, spm_rate);
    if (st == TGX_OK) st = result_check_host(who, ids, offs, n_rows, vocab_size);
    if (st != TGX_OK) return st;
    // as the device: the new offsets from the rows' output lengths, then the kernel's tiles and thread slots
    uint64_t n_out = 0;
    for (uint64_t i = 0; i < n_rows; i++) n_out += tgx::fim_out_len(seed, first_row + i, offs[i + 1] - offs[i], rate);
    if (ids_cap < n_out) return fail(TGX_ERR_INVALID, "%s: %llu ids, room for %llu", who, (unsigned long long)n_out, (unsigned long long)ids_cap);
    if (n_out && !out_ids) return fail(TGX_ERR_INVALID, "%s: out_ids is NULL", who);
    out_offs[0] = 0;
    for (uint64_t i = 0; i < n_rows; i++) out_offs[i + 1] = out_offs[i] + tgx::fim_out_len(seed, first_row + i, offs[i + 1] - offs[i], rate);
    const tgx::FimArgs f = {seed, first_row, rate, spm_rate, prefix_id, suffix_id, middle_id};
    tgx::tiled_fill_host(
        n_out, n_out, tgx::kFimTile, tgx::kFimGroup, 0, [&](uint64_t j) { return tgx::pack_find_row(out_offs, 0, 0, n_rows - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint32_t v[tgx::kFimGroup] = {0, 0, 0, 0};
            tgx::fim_group(f, ids, offs, out_offs, lo, hi, e0, n_in, v);
            for (uint32_t q = 0; q < n_in; q++) out_ids[e0 + q] = v[q];
            return true;
        });
    for (uint64_t i = 0; i < n_rows && (mode || cuts); i++) {  // as fim_info_kernel
        const tgx::FimRow r = tgx::fim_row(seed, first_row + i, offs[i + 1] - offs[i], rate, spm_rate);
        if (mode) mode[i] = (uint8_t)r.mode;
        if (cuts) {
            cuts[2 * i] = r.a;
            cuts[2 * i + 1] = r.b;
        }
    }
    if (n_applied) *n_applied = (n_out - offs[n_rows]) / 3;
    return TGX_OK;
}

// ---- row selection and the seeded permutation -----------------------------------------

namespace tgx::host {

tgx_status select_index_error(const char* who, uint64_t k, int64_t value, uint64_t n_src) {
    return fail(TGX_ERR_INVALID, "%s: rows[%llu] = %lld is not a row of %llu", who, (unsigned long long)k, (long long)value, (unsigned long long)n_src);
}

tgx_status select_check_rows(const char* who, const int64_t* rows, uint64_t n_select, uint64_t n_src) {
    if (n_select && !rows) return fail(TGX_ERR_INVALID, "%s: rows is NULL", who);
    for (uint64_t k = 0; k < n_select; k++)
        if (!tgx::select_in_range(rows[k], n_src)) return select_index_error(who, k, rows[k], n_src);
    return TGX_OK;
}

}  // namespace tgx::host

namespace {

// What the two select twins share.  T = uint32_t: as select_fill_kernel<uint32_t>.  T = uint8_t: as
// select_fill_kernel<uint8_t>, whose slots inside one source row go through the aligned dwords' shift; the twin takes
// those dwords byte by byte (zero outside the text, where the device reads its allocation's zeroed slack), with the
// source index in the place of the address.
template <class T>
tgx_status select_host(const char* who, const char* what, const T* data, const uint64_t* offs, uint64_t n_rows, const int64_t* rows, uint64_t M, T* out,
                       uint64_t cap, uint64_t* out_offs) {
    constexpr bool kText = sizeof(T) == 1;
    constexpr uint32_t kGroup = kText ? tgx::kSelectByteGroup : tgx::kSelectGroup;
    constexpr uint32_t kTile = kText ? tgx::kSelectByteTile : tgx::kSelectTile;
    if (!out_offs) return fail(TGX_ERR_INVALID, "%s: out_offs is NULL", who);
    tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    const uint64_t n_data = offs[n_rows];
    if (n_data && !data) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, what);
    if ((st = select_check_rows(who, rows, M, n_rows)) != TGX_OK) return st;
    uint64_t n_out = 0;
    for (uint64_t k = 0; k < M; k++) n_out += tgx::select_out_len(offs, n_rows, rows, k);
    if (cap < n_out) return fail(TGX_ERR_INVALID, "%s: %llu elements, room for %llu", who, (unsigned long long)n_out, (unsigned long long)cap);
    if (n_out && !out) return fail(TGX_ERR_INVALID, "%s: the destination is NULL", who);
    out_offs[0] = 0;
    for (uint64_t k = 0; k < M; k++) out_offs[k + 1] = out_offs[k] + tgx::select_out_len(offs, n_rows, rows, k);
    tgx::tiled_fill_host(
        n_out, n_out, kTile, kGroup, 0, [&](uint64_t j) { return tgx::pack_find_row(out_offs, 0, 0, M - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            T v[kGroup] = {};
            tgx::SelectCursor cur;
            tgx::select_enter(cur, offs, rows, out_offs, lo, hi, e0);
            if (kText && tgx::select_slot_inside(cur, e0, n_in)) {
                const uint64_t s = tgx::select_slot_source(cur, e0), base = s & ~3ull;
                uint32_t d[5] = {0, 0, 0, 0, 0}, w[4];
                for (uint32_t b = 0; b < 20; b++)
                    if (base + b < n_data) d[b / 4] |= (uint32_t)data[base + b] << (8 * (b % 4));
                tgx::select_shift16(d, (uint32_t)(s & 3u), w);
                for (uint32_t q = 0; q < kGroup; q++) v[q] = (T)(w[q / 4] >> (8 * (q % 4)));
            } else {
                tgx::select_walk<kGroup, T>(cur, data, offs, rows, out_offs, lo, hi, e0, n_in, v);
            }
            for (uint32_t q = 0; q < n_in; q++) out[e0 + q] = v[q];
            return true;
        });
    return TGX_OK;
}

}  // namespace

tgx_status tgx_select_host(const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, const int64_t* rows, uint64_t n_select, uint32_t* out_ids,
                           uint64_t ids_cap, uint64_t* out_offs) {
    return select_host<uint32_t>("tgx_select_host", "ids", ids, offs, n_rows, rows, n_select, out_ids, ids_cap, out_offs);
}

tgx_status tgx_select_text_host(const uint8_t* text, const uint64_t* offs, uint64_t n_rows, const int64_t* rows, uint64_t n_select, uint8_t* out_text,
                                uint64_t text_cap, uint64_t* out_offs) {
    return select_host<uint8_t>("tgx_select_text_host", "text", text, offs, n_rows, rows, n_select, out_text, text_cap, out_offs);
}

uint64_t tgx_shuffle_key(uint64_t seed, uint64_t g) { return tgx::shuffle_key(seed, g); }

tgx_status tgx_shuffled_rows_host(uint64_t n, uint64_t seed, int64_t* rows) {
    const char* who = "tgx_shuffled_rows_host";
    if (n >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^31 rows or more", who);
    if (n == 0) return TGX_OK;
    if (!rows) return fail(TGX_ERR_INVALID, "%s: rows is NULL", who);
    std::vector<uint64_t> keys(n);
    for (uint64_t g = 0; g < n; g++) {
        keys[g] = tgx::shuffle_key(seed, g);
        rows[g] = (int64_t)g;
    }
    std::stable_sort(rows, rows + n, [&keys](int64_t a, int64_t b) { return keys[a] < keys[b]; });
    return TGX_OK;
}

// ---- exact row deduplication -----------------------------------------------------------

uint64_t tgx_row_hash(const uint8_t* bytes, uint64_t n, uint64_t seed) { return tgx::dedup_row_hash_host(n ? bytes : nullptr, bytes ? n : 0, seed); }

namespace {

// the compare of one round: the candidates' concatenated elements in the kernel's tiles and slots, every slot walked
// element by element (the kernel compares a slot inside one candidate 16 bytes at once, to the same flags)
template <class T>
void dedup_compare_host(const void* data, const uint64_t* offs, const uint32_t* rows, const uint32_t* head_row, const uint64_t* cmp_offs, uint64_t L,
                        uint8_t* flag) {
    constexpr bool kText = sizeof(T) == 1;
    const uint64_t n_cmp = cmp_offs[L];
    tgx::tiled_fill_host(
        n_cmp, n_cmp, kText ? tgx::kDedupCmpByteTile : tgx::kDedupCmpTile, kText ? tgx::kDedupCmpByteGroup : tgx::kDedupCmpGroup, 0,
        [&](uint64_t j) { return tgx::pack_find_row(cmp_offs, 0, 0, L - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            tgx::DedupCursor cur;
            tgx::dedup_compare_walk<T>(cur, static_cast<const T*>(data), offs, rows, head_row, cmp_offs, lo, hi, e0, n_in, flag);
            return true;
        });
}

}  // namespace

tgx_status tgx_first_equal_host(const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t hash_bits, int64_t* first,
                                uint64_t* n_unique, uint32_t* n_rounds) {
    const char* who = "tgx_first_equal_host";
    if (n_unique) *n_unique = 0;
    if (n_rounds) *n_rounds = 0;
    if (elem_bytes != 1 && elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, elem_bytes);
    if (hash_bits > 64) return fail(TGX_ERR_INVALID, "%s: hash_bits %u is more than 64", who, hash_bits);
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    const uint64_t S = n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (offs[S] && !data) return fail(TGX_ERR_INVALID, "%s: data is NULL", who);
    if (S && !first) return fail(TGX_ERR_INVALID, "%s: first is NULL", who);
    const uint8_t* bytes = static_cast<const uint8_t*>(data);
    std::vector<uint32_t> list, next, rows_a(S), rows_b(S), head_row(S), order(S);
    std::vector<uint64_t> keys_a(S), keys_b(S), offs_tmp(S + 1);
    std::vector<uint8_t> flag(S), mark(S);
    const uint32_t* lp = nullptr;  // round 0: every row
    uint64_t L = S, heads = 0;
    uint32_t round = 0;
    while (L) {
        // the hash: the sums over the padded bytes in the kernel's tiles and slots, then the keys
        const uint64_t s = tgx::dedup_seed(round);
        offs_tmp[0] = 0;
        for (uint64_t k = 0; k < L; k++) offs_tmp[k + 1] = offs_tmp[k] + tgx::dedup_pad_len(offs, elem_bytes, lp, L, k);
        std::fill(keys_a.begin(), keys_a.begin() + L, 0);
        const uint64_t n_pad = offs_tmp[L];
        uint64_t owner_before = 0;  // the tiles' edges ascend: each owner is found from the one before, as the kernel's
        tgx::tiled_fill_host(
            n_pad, n_pad, tgx::kDedupTile, tgx::kDedupGroup, 0,
            [&](uint64_t j) { return owner_before = tgx::dedup_find_from(offs_tmp.data(), owner_before, L - 1, j); },
            [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
                tgx::DedupSlot sl;
                tgx::dedup_slot(offs_tmp.data(), lo, hi, e0, n_in, sl);
                for (uint32_t q = 0; q < sl.n; q++) {
                    const uint64_t r = tgx::dedup_listed(lp, sl.k[q]);
                    keys_a[sl.k[q]] += tgx::dedup_term(tgx::dedup_word_host(bytes + offs[r] * elem_bytes, (offs[r + 1] - offs[r]) * elem_bytes, sl.j[q]), sl.j[q], s);
                }
                return true;
            });
        for (uint64_t k = 0; k < L; k++) {
            const uint64_t r = tgx::dedup_listed(lp, k);
            keys_a[k] = tgx::dedup_key(tgx::dedup_finish(keys_a[k], (offs[r + 1] - offs[r]) * elem_bytes, s), hash_bits);
            rows_a[k] = (uint32_t)r;
            order[k] = (uint32_t)k;
        }
        // the stable sort by key: each run begins with its smallest row
        std::stable_sort(order.begin(), order.begin() + L, [&keys_a](uint32_t x, uint32_t y) { return keys_a[x] < keys_a[y]; });
        for (uint64_t i = 0; i < L; i++) {
            keys_b[i] = keys_a[order[i]];
            rows_b[i] = rows_a[order[i]];
        }
        // the runs, the compare of every candidate with its head, the resolve
        for (uint64_t i = 0; i < L; i++) {
            const uint64_t h = tgx::dedup_run_head(keys_b.data(), i);
            head_row[i] = rows_b[h];
            flag[i] = (h != i && tgx::dedup_len_differs(offs, rows_b[i], rows_b[h])) ? 1 : 0;
        }
        offs_tmp[0] = 0;
        for (uint64_t i = 0; i < L; i++) offs_tmp[i + 1] = offs_tmp[i] + tgx::dedup_cmp_len(offs, rows_b.data(), head_row.data(), flag.data(), L, i);
        if (elem_bytes == 1)
            dedup_compare_host<uint8_t>(data, offs, rows_b.data(), head_row.data(), offs_tmp.data(), L, flag.data());
        else
            dedup_compare_host<uint32_t>(data, offs, rows_b.data(), head_row.data(), offs_tmp.data(), L, flag.data());
        for (uint64_t i = 0; i < L; i++) {
            const uint32_t r = rows_b[i];
            mark[r] = flag[i];
            if (!flag[i]) first[r] = (int64_t)head_row[i];
            if (head_row[i] == r) heads++;
        }
        next.clear();
        for (uint64_t k = 0; k < L; k++) {
            const uint64_t r = tgx::dedup_listed(lp, k);
            if (mark[r]) next.push_back((uint32_t)r);
        }
        list.swap(next);
        lp = list.data();
        L = list.size();
        round++;
    }
    if (n_unique) *n_unique = heads;
    if (n_rounds) *n_rounds = round;
    return TGX_OK;
}

// ---- near-duplicate rows ---------------------------------------------------------------

uint32_t tgx_minhash_value(uint64_t h, uint32_t k, uint64_t seed) {
    uint64_t a, b;
    tgx::minhash_perm(tgx::minhash_perm_seed(seed), k, a, b);
    return tgx::minhash_value(a, b, h);
}

namespace {

tgx_status minhash_check_sig_host(const char* who, const uint32_t* sig, uint64_t n_rows, uint32_t n_perm) {
    if (n_perm == 0 || n_perm > tgx::kMinhashMaxPerm) return fail(TGX_ERR_INVALID, "%s: n_perm %u is not in 1 .. %u", who, n_perm, tgx::kMinhashMaxPerm);
    if (n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (n_rows && !sig) return fail(TGX_ERR_INVALID, "%s: sig is NULL", who);
    return TGX_OK;
}

}  // namespace

// The kernel's walk: the positions in tiles of four chunks, the owners of a chunk's ends galloped from the chunk before,
// every position's owner searched between them, the minima flushed when the owner changes and at the chunk's end, by
// the kernel's rule (a plain store for a row inside the chunk, which would lose the other chunks' part if the rule were wrong).
tgx_status tgx_minhash_host(const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t width, uint32_t n_perm, uint64_t seed,
                            uint32_t* sig) {
    const char* who = "tgx_minhash_host";
    if (elem_bytes != 1 && elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, elem_bytes);
    if (width == 0 || (uint64_t)width * elem_bytes > tgx::kMinhashMaxBytes)
        return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, width, elem_bytes, tgx::kMinhashMaxBytes / elem_bytes);
    if (n_perm == 0 || n_perm > tgx::kMinhashMaxPerm) return fail(TGX_ERR_INVALID, "%s: n_perm %u is not in 1 .. %u", who, n_perm, tgx::kMinhashMaxPerm);
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    const uint64_t S = n_rows, K = n_perm;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (offs[S] && !data) return fail(TGX_ERR_INVALID, "%s: data is NULL", who);
    if (S && !sig) return fail(TGX_ERR_INVALID, "%s: sig is NULL", who);
    if (S == 0) return TGX_OK;
    const uint8_t* bytes = static_cast<const uint8_t*>(data);
    std::vector<uint64_t> sh_offs(S + 1), a(K), b(K);
    std::vector<uint32_t> mn(K, tgx::kMinhashNoSig);
    sh_offs[0] = 0;
    for (uint64_t k = 0; k < S; k++) sh_offs[k + 1] = sh_offs[k] + tgx::minhash_row_positions(offs, S, width, k);
    const uint64_t M = sh_offs[S], hs = tgx::dedup_seed(tgx::minhash_hash_seed(seed)), ps = tgx::minhash_perm_seed(seed);
    for (uint32_t k = 0; k < K; k++) tgx::minhash_perm(ps, k, a[k], b[k]);
    std::fill(sig, sig + S * K, tgx::kMinhashNoSig);
    uint64_t hi = 0;
    for (uint64_t t0 = 0; t0 < M; t0 += tgx::kMinhashTile) {
        for (uint64_t c0 = t0; c0 < M && c0 < t0 + tgx::kMinhashTile; c0 += tgx::kMinhashChunk) {
            const uint64_t c_last = tgx::tile_last(c0, tgx::kMinhashChunk, M);
            const uint64_t lo = tgx::dedup_find_from(sh_offs.data(), hi, S - 1, c0);
            hi = tgx::dedup_find_from(sh_offs.data(), lo, S - 1, c_last);
            uint64_t cur = lo;
            auto flush = [&](uint64_t r) {
                const bool inside = tgx::minhash_row_inside(sh_offs.data(), r, c0);
                for (uint64_t k = 0; k < K; k++) {
                    sig[r * K + k] = inside ? mn[k] : std::min(sig[r * K + k], mn[k]);
                    mn[k] = tgx::kMinhashNoSig;
                }
            };
            for (uint64_t pos = c0; pos <= c_last; pos++) {
                const uint64_t i = tgx::pack_find_row(sh_offs.data(), 0, lo, hi, pos);
                const uint64_t t = pos - sh_offs[i];
                const uint32_t n_bytes = tgx::minhash_shingle_len(offs[i + 1] - offs[i], width) * elem_bytes;
                uint64_t w[tgx::kMinhashMaxBytes / 8] = {};
                for (uint32_t j = 0; 8 * j < n_bytes; j++) w[j] = tgx::dedup_word_host(bytes + (offs[i] + t) * elem_bytes, n_bytes, j);
                const uint64_t h = tgx::minhash_hash_words(w, n_bytes, hs);
                if (i != cur) {
                    flush(cur);
                    cur = i;
                }
                for (uint64_t k = 0; k < K; k++) mn[k] = std::min(mn[k], tgx::minhash_value(a[k], b[k], h));
            }
            flush(cur);
        }
    }
    return TGX_OK;
}

tgx_status tgx_minhash_bands_host(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed, uint64_t* keys, int64_t* heads) {
    const char* who = "tgx_minhash_bands_host";
    const tgx_status st = minhash_check_sig_host(who, sig, n_rows, n_perm);
    if (st != TGX_OK) return st;
    if (bands == 0 || n_perm % bands) return fail(TGX_ERR_INVALID, "%s: bands %u does not divide n_perm %u", who, bands, n_perm);
    if (!keys && !heads) return fail(TGX_ERR_INVALID, "%s: keys and heads are both NULL", who);
    const uint64_t S = n_rows, B = bands;
    const uint32_t r = n_perm / bands;
    std::vector<uint64_t> col(S), sorted(S);
    std::vector<uint32_t> order(S);
    for (uint32_t b = 0; b < bands; b++) {
        for (uint64_t i = 0; i < S; i++) {
            col[i] = tgx::minhash_band_key(sig + i * n_perm, r, b, seed);
            if (keys) keys[i * B + b] = col[i];
            order[i] = (uint32_t)i;
        }
        if (!heads) continue;
        // the stable sort by key: each run begins with its smallest row
        std::stable_sort(order.begin(), order.end(), [&col](uint32_t x, uint32_t y) { return col[x] < col[y]; });
        for (uint64_t i = 0; i < S; i++) sorted[i] = col[order[i]];
        for (uint64_t i = 0; i < S; i++) heads[(uint64_t)order[i] * B + b] = (int64_t)order[tgx::dedup_run_head(sorted.data(), i)];
    }
    return TGX_OK;
}

tgx_status tgx_minhash_near_first_host(const uint32_t* sig, uint64_t n_rows, uint32_t n_perm, const int64_t* heads, uint32_t bands, uint32_t min_agree,
                                       int64_t* first, uint64_t* n_clusters) {
    const char* who = "tgx_minhash_near_first_host";
    if (n_clusters) *n_clusters = 0;
    const tgx_status st = minhash_check_sig_host(who, sig, n_rows, n_perm);
    if (st != TGX_OK) return st;
    if (bands == 0 || bands > n_perm) return fail(TGX_ERR_INVALID, "%s: bands %u is not in 1 .. n_perm %u", who, bands, n_perm);
    if (min_agree == 0 || min_agree > n_perm) return fail(TGX_ERR_INVALID, "%s: min_agree %u is not in 1 .. n_perm %u", who, min_agree, n_perm);
    const uint64_t S = n_rows, K = n_perm, B = bands;
    if (S == 0) return TGX_OK;
    if (!heads) return fail(TGX_ERR_INVALID, "%s: heads is NULL", who);
    if (!first) return fail(TGX_ERR_INVALID, "%s: first is NULL", who);
    for (uint64_t i = 0; i < S; i++) {
        uint64_t best = i;
        for (uint64_t b = 0; b < B; b++) {
            const int64_t head = heads[i * B + b];
            if (!tgx::minhash_looks_at(head, best)) continue;
            uint32_t agree = 0;
            for (uint64_t k = 0; k < K; k++) agree += sig[i * K + k] == sig[(uint64_t)head * K + k];
            if (tgx::minhash_takes(agree, min_agree)) best = (uint64_t)head;
        }
        first[i] = (int64_t)best;
    }
    // pointer doubling between two buffers, until a round moves nothing
    std::vector<int64_t> other(S);
    for (bool changed = true; changed;) {
        changed = false;
        for (uint64_t i = 0; i < S; i++) {
            other[i] = tgx::minhash_hop(first, i);
            changed = changed || other[i] != first[i];
        }
        std::copy(other.begin(), other.end(), first);
    }
    uint64_t n = 0;
    for (uint64_t i = 0; i < S; i++) n += first[i] == (int64_t)i;
    if (n_clusters) *n_clusters = n;
    return TGX_OK;
}

// ---- shared n-grams --------------------------------------------------------------------

uint64_t tgx_gram_key(const uint8_t* bytes, uint64_t n_bytes, uint64_t seed) { return tgx::dedup_row_hash_host(bytes, n_bytes, tgx::minhash_hash_seed(seed)); }

namespace {

tgx_status gram_check_source_host(const char* who, const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t width) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, elem_bytes);
    if (width == 0 || (uint64_t)width * elem_bytes > tgx::kMinhashMaxBytes)
        return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, width, elem_bytes, tgx::kMinhashMaxBytes / elem_bytes);
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    if (n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (offs[n_rows] && !data) return fail(TGX_ERR_INVALID, "%s: data is NULL", who);
    return TGX_OK;
}

// The kernels' walk over the elements of all rows laid end to end: tiles of four chunks, the owners of a chunk's ends
// galloped from the chunk before, every element's owner searched between them.  at(c0, e, i, valid, key) sees every
// element e, in order, with its row i and the validity and key of the gram that begins there.
template <class At>
void gram_walk_host(const uint8_t* bytes, uint32_t elem_bytes, const uint64_t* offs, uint64_t S, uint32_t width, uint64_t seed, At at) {
    const uint64_t M = S ? offs[S] : 0, hs = tgx::dedup_seed(tgx::minhash_hash_seed(seed));
    const uint32_t n_bytes = width * elem_bytes;
    uint64_t hi = 0;
    for (uint64_t t0 = 0; t0 < M; t0 += tgx::kGramTile) {
        for (uint64_t c0 = t0; c0 < M && c0 < t0 + tgx::kGramTile; c0 += tgx::kGramChunk) {
            const uint64_t c_last = tgx::tile_last(c0, tgx::kGramChunk, M);
            const uint64_t lo = tgx::dedup_find_from(offs, hi, S - 1, c0);
            hi = tgx::dedup_find_from(offs, lo, S - 1, c_last);
            for (uint64_t e = c0; e <= c_last; e++) {
                const uint64_t i = tgx::pack_find_row(offs, 0, lo, hi, e);
                const bool valid = tgx::gram_valid(e, width, offs[i + 1]);
                uint64_t key = 0;
                if (valid) {  // (an invalid position reads nothing)
                    uint64_t w[tgx::kMinhashMaxBytes / 8] = {};
                    for (uint32_t j = 0; 8 * j < n_bytes; j++) w[j] = tgx::dedup_word_host(bytes + e * elem_bytes, n_bytes, j);
                    key = tgx::minhash_hash_words(w, n_bytes, hs);
                }
                at(c0, e, i, valid, key);
            }
        }
    }
}

// the directory of ascending keys
std::vector<uint32_t> gram_dir_host(const std::vector<uint64_t>& keys, uint32_t bits) {
    std::vector<uint32_t> dir(((size_t)1 << bits) + 1);
    for (uint64_t b = 0; b < dir.size(); b++) dir[b] = tgx::gram_dir_entry(keys.data(), keys.size(), bits, b);
    return dir;
}

// keys in any order, duplicates allowed -> ascending and distinct, with their directory
tgx_status gram_set_host(const char* who, const uint64_t* keys, uint64_t n_keys, std::vector<uint64_t>* sorted, std::vector<uint32_t>* dir, uint32_t* bits) {
    if (n_keys && !keys) return fail(TGX_ERR_INVALID, "%s: keys is NULL", who);
    sorted->assign(keys, keys + n_keys);
    std::sort(sorted->begin(), sorted->end());
    sorted->erase(std::unique(sorted->begin(), sorted->end()), sorted->end());
    if (sorted->size() > tgx::kGramMaxKeys) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-2 keys", who);
    *bits = tgx::gram_dir_bits(sorted->size());
    *dir = gram_dir_host(*sorted, *bits);
    return TGX_OK;
}

}  // namespace

tgx_status tgx_gram_keys_host(const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t width, uint64_t seed,
                              uint64_t* keys_out, uint64_t* n_keys) {
    const char* who = "tgx_gram_keys_host";
    if (n_keys) *n_keys = 0;
    const tgx_status st = gram_check_source_host(who, data, elem_bytes, offs, n_rows, width);
    if (st != TGX_OK) return st;
    if (!n_keys) return fail(TGX_ERR_INVALID, "%s: n_keys is NULL", who);
    if (offs[n_rows] && !keys_out) return fail(TGX_ERR_INVALID, "%s: keys_out is NULL", who);
    // every valid gram's key to its slot, as gram_keys_kernel; then the sort and the unique
    std::vector<uint64_t> g_offs(n_rows + 1, 0);
    for (uint64_t k = 0; k < n_rows; k++) g_offs[k + 1] = g_offs[k] + tgx::gram_row_count(offs, n_rows, width, k);
    std::vector<uint64_t> raw(g_offs[n_rows]);
    gram_walk_host(static_cast<const uint8_t*>(data), elem_bytes, offs, n_rows, width, seed, [&](uint64_t, uint64_t e, uint64_t i, bool valid, uint64_t key) {
        if (valid) raw[g_offs[i] + (e - offs[i])] = key;
    });
    std::sort(raw.begin(), raw.end());
    raw.erase(std::unique(raw.begin(), raw.end()), raw.end());
    if (raw.size() > tgx::kGramMaxKeys) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-2 keys", who);
    std::copy(raw.begin(), raw.end(), keys_out);
    *n_keys = raw.size();
    return TGX_OK;
}

tgx_status tgx_gram_hits_host(const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t width, uint64_t seed,
                              const uint64_t* keys, uint64_t n_keys, int64_t* count, uint8_t* mask) {
    const char* who = "tgx_gram_hits_host";
    tgx_status st = gram_check_source_host(who, data, elem_bytes, offs, n_rows, width);
    if (st != TGX_OK) return st;
    if (!count && !mask) return fail(TGX_ERR_INVALID, "%s: count and mask are both NULL", who);
    std::vector<uint64_t> sorted;
    std::vector<uint32_t> dir;
    uint32_t bits = 0;
    if ((st = gram_set_host(who, keys, n_keys, &sorted, &dir, &bits)) != TGX_OK) return st;
    if (n_rows == 0) return TGX_OK;
    if (count) std::fill(count, count + n_rows, 0);  // the launcher's pre-set
    // a stretch of one row inside a chunk ends when the owner or the chunk changes: then the kernel's store / add rule
    uint64_t cur_c0 = 0, cur_row = 0, n_hits = 0;
    bool open = false;
    auto flush = [&]() {
        if (!open || !count) return;
        if (tgx::gram_row_inside(offs, cur_row, cur_c0))
            count[cur_row] = (int64_t)n_hits;
        else if (tgx::gram_adds(n_hits))
            count[cur_row] += (int64_t)n_hits;
    };
    gram_walk_host(static_cast<const uint8_t*>(data), elem_bytes, offs, n_rows, width, seed, [&](uint64_t c0, uint64_t e, uint64_t i, bool valid, uint64_t key) {
        if (!open || c0 != cur_c0 || i != cur_row) {
            flush();
            open = true;
            cur_c0 = c0;
            cur_row = i;
            n_hits = 0;
        }
        const bool hit = valid && tgx::gram_contains(sorted.data(), dir.data(), bits, key);
        if (mask) mask[e] = hit ? 1 : 0;
        n_hits += hit;
    });
    flush();
    return TGX_OK;
}

tgx_status tgx_gram_contains_host(const uint64_t* keys, uint64_t n_keys, const uint64_t* probes, uint64_t n_probes, uint8_t* out) {
    const char* who = "tgx_gram_contains_host";
    std::vector<uint64_t> sorted;
    std::vector<uint32_t> dir;
    uint32_t bits = 0;
    const tgx_status st = gram_set_host(who, keys, n_keys, &sorted, &dir, &bits);
    if (st != TGX_OK) return st;
    if (n_probes && (!probes || !out)) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, probes ? "out" : "probes");
    for (uint64_t p = 0; p < n_probes; p++) out[p] = tgx::gram_contains(sorted.data(), dir.data(), bits, probes[p]) ? 1 : 0;
    return TGX_OK;
}

// ---- literal phrase matching (include/tgx_phrases.h) --------------------------------------------

tgx_status tgx_phrase_hits_host(const void* data_, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, const void* phrases,
                                const uint64_t* phrase_offs, uint32_t n_phrases, uint32_t flags, int64_t* count, uint8_t* longest,
                                int64_t* per_phrase) {
    const char* who = "tgx_phrase_hits_host";
    tgx::PhraseTable table;
    const char* why = nullptr;
    const tgx::PhraseBuild built = tgx::phrase_build_table(phrases, phrase_offs, n_phrases, elem_bytes, flags, &table, &why);
    if (built != tgx::kPhraseOk) return fail(built == tgx::kPhraseInvalid ? TGX_ERR_INVALID : TGX_ERR_UNSUPPORTED, "%s: %s", who, why);
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    if (n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (offs[n_rows] && !data_) return fail(TGX_ERR_INVALID, "%s: data is NULL", who);
    if (!count && !longest && !per_phrase) return fail(TGX_ERR_INVALID, "%s: count, longest and per_phrase are all NULL", who);
    const uint8_t* data = static_cast<const uint8_t*>(data_);
    const uint64_t S = n_rows, M = offs[S];
    const uint32_t eb = elem_bytes, max_bytes = table.max_len * eb;
    const bool fold = flags & tgx::kPhraseFoldCase, whole = flags & tgx::kPhraseWholeWord;
    if (count) std::fill(count, count + S, 0);  // the launcher's pre-sets
    if (per_phrase) std::fill(per_phrase, per_phrase + n_phrases, 0);
    // a stretch of one row inside a chunk ends when the owner or the chunk changes: then the kernel's store / add rule
    uint64_t hi = 0;
    for (uint64_t t0 = 0; t0 < M; t0 += tgx::kGramTile) {
        for (uint64_t c0 = t0; c0 < M && c0 < t0 + tgx::kGramTile; c0 += tgx::kGramChunk) {
            const uint64_t c_last = tgx::tile_last(c0, tgx::kGramChunk, M);
            const uint64_t lo = tgx::dedup_find_from(offs, hi, S - 1, c0);
            hi = tgx::dedup_find_from(offs, lo, S - 1, c_last);
            uint64_t cur_row = 0, n_hits = 0;
            bool open = false;
            auto flush = [&]() {
                if (!open || !count) return;
                if (tgx::gram_row_inside(offs, cur_row, c0))
                    count[cur_row] = (int64_t)n_hits;
                else if (tgx::gram_adds(n_hits))
                    count[cur_row] += (int64_t)n_hits;
            };
            for (uint64_t pos = c0; pos <= c_last; pos++) {
                const uint64_t row = tgx::pack_find_row(offs, 0, lo, hi, pos);
                if (!open || row != cur_row) {
                    flush();
                    open = true;
                    cur_row = row;
                    n_hits = 0;
                }
                const uint64_t left = (offs[row + 1] - pos) * eb;
                const uint32_t avail = left > max_bytes ? max_bytes + 1 : (uint32_t)left;
                const uint8_t* s = data + pos * eb;
                auto get = [&](uint32_t k) { return tgx::phrase_fold(s[k], fold); };
                const uint32_t b0 = get(0), b1 = avail >= 2 ? get(1) : 0u;
                bool go = tgx::phrase_filter_pass(table.filter.data(), b0, b1);
                if (whole && go) go = pos == offs[row] || !tgx::phrase_word_byte(tgx::phrase_fold(s[-1], fold));
                tgx::PhraseHit h = {0, 0};
                if (go)
                    h = tgx::phrase_walk(table.rec.data(), table.root_base, eb, avail, max_bytes, whole, get, [&](uint32_t p) {
                        if (per_phrase) per_phrase[p]++;
                    });
                if (longest) longest[pos] = (uint8_t)h.longest;
                n_hits += h.count;
            }
            flush();
        }
    }
    return TGX_OK;
}

// ---- repeated n-grams within a row ------------------------------------------------------------

tgx_status tgx_repeat_stats_host(const void* data, uint32_t elem_bytes, const uint64_t* offs, uint64_t n_rows, uint32_t width, uint64_t seed,
                                 int64_t* stats, uint8_t* mask) {
    const char* who = "tgx_repeat_stats_host";
    const tgx_status st = gram_check_source_host(who, data, elem_bytes, offs, n_rows, width);
    if (st != TGX_OK) return st;
    if (!stats && !mask) return fail(TGX_ERR_INVALID, "%s: stats and mask are both NULL", who);
    const uint64_t S = n_rows;
    if (S == 0) return TGX_OK;
    const uint64_t N = offs[S];
    if (N > tgx::kRepeatMaxElems) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^32-1 elements or more", who);
    // the pre-sets
    std::vector<uint8_t> own_flag(mask ? 0 : N);
    uint8_t* flag = mask ? mask : own_flag.data();
    std::fill(flag, flag + N, 0);
    std::vector<uint64_t> g_offs(S + 1, 0);
    for (uint64_t k = 0; k < S; k++) {
        const uint64_t grams = tgx::gram_row_count(offs, S, width, k);
        g_offs[k + 1] = g_offs[k] + grams;
        if (!stats) continue;
        for (uint32_t q = 0; q < tgx::kRepeatN; q++) stats[q * S + k] = 0;
        stats[tgx::kRpGrams * S + k] = (int64_t)grams;
        stats[tgx::kRpTop * S + k] = (int64_t)tgx::repeat_top_preset(grams);
    }
    // every valid gram's row key and position to its slot, as repeat_keys_kernel; then the stable sort by key
    const uint64_t G = g_offs[S];
    std::vector<uint64_t> keys_a(G), keys(G);
    std::vector<uint32_t> pos_a(G), pos(G), order(G);
    gram_walk_host(static_cast<const uint8_t*>(data), elem_bytes, offs, S, width, seed, [&](uint64_t, uint64_t e, uint64_t i, bool valid, uint64_t key) {
        if (!valid) return;
        const uint64_t slot = g_offs[i] + (e - offs[i]);
        keys_a[slot] = tgx::repeat_row_key(key, i);
        pos_a[slot] = (uint32_t)e;
    });
    for (uint64_t t = 0; t < G; t++) order[t] = (uint32_t)t;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys_a[a] < keys_a[b]; });
    for (uint64_t t = 0; t < G; t++) {
        keys[t] = keys_a[order[t]];
        pos[t] = pos_a[order[t]];
    }
    // the runs, as repeat_runs_kernel
    for (uint64_t t = 0; t < G; t++) {
        const bool head = t == 0 || keys[t - 1] != keys[t], next_same = t + 1 < G && keys[t + 1] == keys[t];
        flag[pos[t]] = tgx::repeat_flag(head, next_same);
        if (stats && head && next_same) {
            const int64_t len = (int64_t)(tgx::repeat_run_end(keys.data(), G, t) - t);
            int64_t& top = stats[tgx::kRpTop * S + tgx::pack_find_row(offs, 0, 0, S - 1, pos[t])];
            top = std::max(top, len);
        }
    }
    if (!stats) return TGX_OK;
    // the cover and the row sums, as repeat_cover_kernel: its chunks, the window of two chunks, the store / add rule
    uint64_t hi = 0;
    for (uint64_t c0 = 0; c0 < N; c0 += tgx::kGramChunk) {
        const uint64_t c_last = tgx::tile_last(c0, tgx::kGramChunk, N);
        const uint64_t lo = tgx::dedup_find_from(offs, hi, S - 1, c0);
        hi = tgx::dedup_find_from(offs, lo, S - 1, c_last);
        const uint32_t n_in = (uint32_t)(c_last - c0) + 1;
        uint64_t row[tgx::kGramChunk], ballots[4] = {0, 0, 0, 0}, rep_b = 0, mul_b = 0;
        for (uint32_t l = 0; l < tgx::kGramChunk; l++) {
            if (l < n_in) {
                row[l] = tgx::pack_find_row(offs, 0, lo, hi, c0 + l);
                if (flag[c0 + l] & tgx::kRepeatBitRepeat) ballots[0] |= 1ull << l;
                if (flag[c0 + l] & tgx::kRepeatBitMulti) ballots[1] |= 1ull << l;
            }
            if (c0) {  // (the chunk before is whole)
                if (flag[c0 - tgx::kGramChunk + l] & tgx::kRepeatBitRepeat) rep_b |= 1ull << l;
                if (flag[c0 - tgx::kGramChunk + l] & tgx::kRepeatBitMulti) mul_b |= 1ull << l;
            }
        }
        for (uint32_t l = 0; l < n_in; l++) {
            if (tgx::repeat_covered(rep_b, ballots[0], l, c0 + l, offs[row[l]], width)) ballots[2] |= 1ull << l;
            if (tgx::repeat_covered(mul_b, ballots[1], l, c0 + l, offs[row[l]], width)) ballots[3] |= 1ull << l;
        }
        const uint32_t which[4] = {tgx::kRpRepeated, tgx::kRpMulti, tgx::kRpCovered, tgx::kRpCoveredAll};
        for (uint32_t a = 0; a < n_in;) {  // the stretch [a, b] of one row
            uint32_t b = a;
            while (b + 1 < n_in && row[b + 1] == row[a]) b++;
            const uint64_t i = row[a], stretch = ((b >= 63 ? 0ull : (1ull << (b + 1))) - 1) & ~((1ull << a) - 1);  // lanes [a, b]
            const bool inside = tgx::gram_row_inside(offs, i, c0);
            for (uint32_t q = 0; q < 4; q++) {
                const uint64_t v = (uint64_t)__builtin_popcountll(ballots[q] & stretch);
                if (inside)
                    stats[which[q] * S + i] = (int64_t)v;
                else if (tgx::gram_adds(v))
                    stats[which[q] * S + i] += (int64_t)v;
            }
            a = b + 1;
        }
    }
    return TGX_OK;
}

// ---- text statistics and the line view ------------------------------------------------------

namespace {

tgx_status textstat_check_source_host(const char* who, const uint8_t* text, const uint64_t* offs, uint64_t n_rows) {
    const tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    if (n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (offs[n_rows] && !text) return fail(TGX_ERR_INVALID, "%s: text is NULL", who);
    return TGX_OK;
}

// The kernels' walk over the bytes of all rows laid end to end: tiles of four chunks, the owners of a chunk's ends
// galloped from the chunk before, every byte's owner searched between them.  body(c0, n_in, starts, row) sees every
// chunk, in order, with the mask of its line starts and its lanes' owners.
template <class Body>
void textstat_walk_host(const uint8_t* text, const uint64_t* offs, uint64_t S, Body body) {
    const uint64_t M = S ? offs[S] : 0;
    uint64_t hi = 0;
    for (uint64_t t0 = 0; t0 < M; t0 += tgx::kTextstatTile) {
        for (uint64_t c0 = t0; c0 < M && c0 < t0 + tgx::kTextstatTile; c0 += tgx::kTextstatChunk) {
            const uint64_t c_last = tgx::tile_last(c0, tgx::kTextstatChunk, M);
            const uint64_t lo = tgx::dedup_find_from(offs, hi, S - 1, c0);
            hi = tgx::dedup_find_from(offs, lo, S - 1, c_last);
            const uint32_t n_in = (uint32_t)(c_last - c0) + 1;
            uint64_t row[tgx::kTextstatChunk], nl = 0, starts = 0;
            for (uint32_t l = 0; l < n_in; l++) {
                row[l] = tgx::pack_find_row(offs, 0, lo, hi, c0 + l);
                if (text[c0 + l] == '\n') nl |= 1ull << l;
            }
            const uint64_t after_nl = (nl << 1) | (c0 > 0 && text[c0 - 1] == '\n' ? 1ull : 0ull);
            for (uint32_t l = 0; l < n_in; l++)
                if (c0 + l == offs[row[l]] || ((after_nl >> l) & 1ull)) starts |= 1ull << l;
            body(c0, n_in, starts, row);
        }
    }
}

// a class's mask over the n_in bytes from c0 on
template <class Is>
uint64_t textstat_mask_host(const uint8_t* text, uint64_t c0, uint32_t n_in, Is is) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < n_in; l++)
        if (is(text[c0 + l])) m |= 1ull << l;
    return m;
}

// What the two twins share: the summaries, their scan, and the second kernel with its store / add rule.  The source has
// been checked, n_rows > 0; stats and line_start may each be NULL.
void textstat_host(const uint8_t* text, const uint64_t* offs, uint64_t S, uint64_t line_limit, uint32_t flags, int64_t* stats, uint8_t* line_start) {
    const uint64_t N = offs[S], n_chunks = (N + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk;
    auto units_of = [&](uint64_t c0, uint32_t n_in) { return textstat_mask_host(text, c0, n_in, [&](uint8_t b) { return tgx::textstat_is_unit(b, flags); }); };
    if (stats) std::fill(stats, stats + S * tgx::kTextstatN, 0);  // the launcher's pre-set
    std::vector<uint64_t> summary(n_chunks), carry(n_chunks);
    textstat_walk_host(text, offs, S, [&](uint64_t c0, uint32_t n_in, uint64_t starts, const uint64_t*) {
        summary[c0 / tgx::kTextstatChunk] = tgx::textstat_summary(starts, units_of(c0, n_in));
    });
    uint64_t acc = 0;  // the exclusive scan under the segmented sum
    for (uint64_t k = 0; k < n_chunks; k++) {
        carry[k] = acc;
        acc = tgx::TextstatCarryOp()(acc, summary[k]);
    }
    textstat_walk_host(text, offs, S, [&](uint64_t c0, uint32_t n_in, uint64_t starts, const uint64_t* row) {
        if (line_start)
            for (uint32_t l = 0; l < n_in; l++) line_start[c0 + l] = (uint8_t)((starts >> l) & 1ull);
        if (!stats) return;
        const uint64_t units = units_of(c0, n_in);
        uint64_t ends = 0, longs = 0, len[tgx::kTextstatChunk] = {};
        for (uint32_t l = 0; l < n_in; l++) {
            const bool is_nl = text[c0 + l] == '\n';
            if (!is_nl && c0 + l + 1 != offs[row[l] + 1]) continue;
            ends |= 1ull << l;
            len[l] = tgx::textstat_line_len(starts, units, l, is_nl, carry[c0 / tgx::kTextstatChunk]);
            if (len[l] > line_limit) longs |= 1ull << l;
        }
        uint64_t ballots[tgx::kTextstatN] = {};
        ballots[tgx::kTsChars] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_char);
        ballots[tgx::kTsNewlines] = textstat_mask_host(text, c0, n_in, [](uint8_t b) { return b == '\n'; });
        ballots[tgx::kTsLines] = ends;
        ballots[tgx::kTsLongLines] = longs;
        ballots[tgx::kTsAlpha] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_alpha);
        ballots[tgx::kTsDigit] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_digit);
        ballots[tgx::kTsSpace] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_space);
        ballots[tgx::kTsNonAscii] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_non_ascii);
        ballots[tgx::kTsControl] = textstat_mask_host(text, c0, n_in, tgx::textstat_is_control);
        for (uint32_t a = 0; a < n_in;) {  // the stretch [a, b] of one row
            uint32_t b = a;
            while (b + 1 < n_in && row[b + 1] == row[a]) b++;
            const uint64_t i = row[a], stretch = tgx::textstat_span(a, b);
            const bool inside = tgx::textstat_row_inside(offs, i, c0);
            if (c0 + a == offs[i]) stats[tgx::kTsBytes * S + i] = (int64_t)(offs[i + 1] - offs[i]);
            uint64_t longest = 0;
            for (uint32_t l = a; l <= b; l++) longest = std::max(longest, len[l]);
            int64_t& max_line = stats[tgx::kTsMaxLine * S + i];
            if (inside)
                max_line = (int64_t)longest;
            else if (tgx::textstat_adds(longest))
                max_line = std::max(max_line, (int64_t)longest);
            for (uint32_t k = 0; k < tgx::kTextstatN; k++) {
                if (k == tgx::kTsBytes || k == tgx::kTsMaxLine) continue;
                const uint64_t v = tgx::textstat_popc(ballots[k] & stretch);
                if (inside)
                    stats[k * S + i] = (int64_t)v;
                else if (tgx::textstat_adds(v))
                    stats[k * S + i] += (int64_t)v;
            }
            a = b + 1;
        }
    });
}

}  // namespace

tgx_status tgx_text_stats_host(const uint8_t* text, const uint64_t* offs, uint64_t n_rows, uint64_t line_limit, uint32_t flags, int64_t* stats,
                               uint8_t* line_start) {
    const char* who = "tgx_text_stats_host";
    tgx_status st = textstat_check_source_host(who, text, offs, n_rows);
    if (st != TGX_OK) return st;
    if ((st = layout_check_flags(who, flags, tgx::kTextstatChars)) != TGX_OK) return st;
    if (!stats && !line_start) return fail(TGX_ERR_INVALID, "%s: stats and line_start are both NULL", who);
    if (n_rows == 0) return TGX_OK;
    textstat_host(text, offs, n_rows, line_limit, flags, stats, line_start);
    return TGX_OK;
}

tgx_status tgx_lines_host(const uint8_t* text, const uint64_t* offs, uint64_t n_rows, uint64_t* out_offs, uint64_t cap, uint64_t* n_lines) {
    const char* who = "tgx_lines_host";
    if (n_lines) *n_lines = 0;
    const tgx_status st = textstat_check_source_host(who, text, offs, n_rows);
    if (st != TGX_OK) return st;
    if (!n_lines) return fail(TGX_ERR_INVALID, "%s: n_lines is NULL", who);
    const uint64_t N = offs[n_rows];
    std::vector<uint8_t> marks(N);
    if (n_rows && N) textstat_host(text, offs, n_rows, 0, 0, nullptr, marks.data());
    uint64_t n = 0;
    for (uint64_t p = 0; p < N; p++) n += marks[p];
    *n_lines = n;
    if (n > tgx::kTextstatMaxLines) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^32-1 lines or more", who);
    if (cap < n + 1) return fail(TGX_ERR_INVALID, "%s: %llu offsets, room for %llu", who, (unsigned long long)(n + 1), (unsigned long long)cap);
    if (!out_offs) return fail(TGX_ERR_INVALID, "%s: out_offs is NULL", who);
    uint64_t k = 0;
    for (uint64_t p = 0; p < N; p++)  // the compaction of the marked positions
        if (marks[p]) out_offs[k++] = p;
    out_offs[n] = N;
    return TGX_OK;
}

// ---- word statistics (include/tgx_words.h) -----------------------------------------------------

namespace {

// The twin of wordstat.hip's two kernels and the scan between them: the chunks of textstat_walk_host, the masks as words,
// the summaries, the scan as a fold, and the second kernel lane by lane with its store / add rule.  The source and the
// table (u64[2 * n_stop], wordstat.h) have been checked, S > 0; stats and marks may each be NULL.
void wordstat_host(const uint8_t* text, const uint64_t* offs, uint64_t S, uint64_t word_limit, uint32_t flags, const uint64_t* table, uint32_t n_stop,
                   int64_t* stats, uint8_t* marks) {
    const uint64_t N = offs[S], n_chunks = (N + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk;
    const bool fold = (flags & tgx::kWordstatFold) != 0;
    auto masks_of = [&](uint64_t c0, uint32_t n_in, uint64_t starts, const uint64_t* row) {
        tgx::WordMasks m = {};
        for (uint32_t l = 0; l < n_in; l++) {
            const uint8_t b = text[c0 + l];
            const uint64_t bit = 1ull << l;
            const bool space = tgx::textstat_is_space(b);
            if (space || c0 + l == offs[row[l]]) m.resets |= bit;
            if (!space && tgx::textstat_is_unit(b, (flags & tgx::kWordstatChars) ? tgx::kTextstatChars : 0u)) m.units |= bit;
            if (tgx::textstat_is_alpha(b)) m.alpha |= bit;
            if (tgx::wordstat_is_wide(b)) m.wide |= bit;
            if (!space) m.nonspace |= bit;
        }
        m.starts = starts;
        return m;
    };
    if (stats) std::fill(stats, stats + S * tgx::kWordstatN, 0);  // the launcher's pre-set
    std::vector<uint64_t> summary(n_chunks), carry(n_chunks);
    textstat_walk_host(text, offs, S, [&](uint64_t c0, uint32_t n_in, uint64_t starts, const uint64_t* row) {
        summary[c0 / tgx::kTextstatChunk] = tgx::wordstat_summary(masks_of(c0, n_in, starts, row));
    });
    uint64_t acc = 0;  // the exclusive scan under WordstatCarryOp
    for (uint64_t k = 0; k < n_chunks; k++) {
        carry[k] = acc;
        acc = tgx::WordstatCarryOp()(acc, summary[k]);
    }
    textstat_walk_host(text, offs, S, [&](uint64_t c0, uint32_t n_in, uint64_t starts, const uint64_t* row) {
        const tgx::WordMasks m = masks_of(c0, n_in, starts, row);
        const uint64_t cy = carry[c0 / tgx::kTextstatChunk];
        uint64_t ballots[tgx::kWordstatN] = {}, hits[tgx::kWordstatMaxStop] = {}, len[tgx::kTextstatChunk] = {};
        uint8_t mark[tgx::kTextstatChunk] = {};
        ballots[tgx::kWsWordUnits] = m.units;
        for (uint32_t l = 0; l < n_in; l++) {
            const uint64_t p = c0 + l, bit = 1ull << l, row_begin = offs[row[l]], row_end = offs[row[l] + 1];
            uint8_t prev = 0;
            const uint64_t tail = tgx::wordstat_tail_of(text, p, row_begin, fold, &prev);
            const bool nonspace = (m.nonspace >> l) & 1ull;
            const bool is_wend = nonspace && (p + 1 == row_end || tgx::textstat_is_space(text[p + 1]));
            const uint32_t nsb = tgx::wordstat_nsb(m, l, cy);
            const bool is_nl = text[p] == '\n', is_lend = is_nl || p + 1 == row_end;
            if (is_wend) {
                const tgx::WordSoFar w = tgx::wordstat_word(m, l, cy);
                len[l] = w.units;
                ballots[tgx::kWsWords] |= bit;
                if (w.units > word_limit) ballots[tgx::kWsLongWords] |= bit;
                if (w.alpha) ballots[tgx::kWsAlphaWords] |= bit;
                if (w.alpha || w.wide) ballots[tgx::kWsAlphaWideWords] |= bit;
                for (uint32_t k = 0; k < n_stop; k++)
                    if (tgx::wordstat_matches(tail, prev, table[tgx::kWordstatStopWords * k], table[tgx::kWordstatStopWords * k + 1])) {
                        hits[k] |= bit;
                        ballots[tgx::kWsStopWords] |= bit;
                    }
            }
            if (text[p] == '#') ballots[tgx::kWsHash] |= bit;
            if (tgx::wordstat_is_ellipsis(tail)) ballots[tgx::kWsEllipsis] |= bit;
            if (tgx::wordstat_is_bullet(tail, nsb)) ballots[tgx::kWsBulletLines] |= bit;
            if (is_lend) {
                ballots[tgx::kWsLines] |= bit;
                if (tgx::wordstat_ellipsis_line(tail, is_nl)) ballots[tgx::kWsEllipsisLines] |= bit;
                if (tgx::wordstat_punct_line(tail, is_nl)) ballots[tgx::kWsPunctLines] |= bit;
            }
            mark[l] = (uint8_t)((tgx::wordstat_is_word_start(tail) ? tgx::kWordMarkStart : 0u) | (is_wend ? tgx::kWordMarkEnd : 0u) |
                                ((ballots[tgx::kWsStopWords] & bit) ? tgx::kWordMarkStop : 0u) | ((ballots[tgx::kWsBulletLines] & bit) ? tgx::kWordMarkBullet : 0u));
        }
        if (marks) std::copy(mark, mark + n_in, marks + c0);
        if (!stats) return;
        for (uint32_t a = 0; a < n_in;) {  // the stretch [a, b] of one row
            uint32_t b = a;
            while (b + 1 < n_in && row[b + 1] == row[a]) b++;
            const uint64_t i = row[a], stretch = tgx::textstat_span(a, b);
            const bool inside = tgx::textstat_row_inside(offs, i, c0);
            uint64_t longest = 0, stop_mask = 0;
            for (uint32_t l = a; l <= b; l++) longest = std::max(longest, len[l]);
            for (uint32_t k = 0; k < n_stop; k++)
                if (hits[k] & stretch) stop_mask |= 1ull << k;
            int64_t& max_word = stats[tgx::kWsMaxWord * S + i];
            if (inside)
                max_word = (int64_t)longest;
            else if (tgx::textstat_adds(longest))
                max_word = std::max(max_word, (int64_t)longest);
            for (uint32_t k = 0; k < tgx::kWordstatN; k++) {
                if (k == tgx::kWsMaxWord || k == tgx::kWsStopMask) continue;
                const uint64_t v = tgx::textstat_popc(ballots[k] & stretch);
                if (inside)
                    stats[k * S + i] = (int64_t)v;
                else if (tgx::textstat_adds(v))
                    stats[k * S + i] += (int64_t)v;
            }
            if (inside)
                stats[tgx::kWsStopMask * S + i] = (int64_t)stop_mask;
            else if (tgx::textstat_adds(stop_mask))
                stats[tgx::kWsStopMask * S + i] |= (int64_t)stop_mask;
            a = b + 1;
        }
    });
}

}  // namespace

tgx_status tgx_word_stats_host(const uint8_t* text, const uint64_t* offs, uint64_t n_rows, uint64_t word_limit, const uint8_t* stop_bytes,
                               const uint64_t* stop_offs, uint32_t n_stop, uint32_t flags, int64_t* stats, uint8_t* marks) {
    const char* who = "tgx_word_stats_host";
    tgx_status st = textstat_check_source_host(who, text, offs, n_rows);
    if (st != TGX_OK) return st;
    if ((st = layout_check_flags(who, flags, tgx::kWordstatChars | tgx::kWordstatFold)) != TGX_OK) return st;
    std::vector<uint64_t> table(tgx::kWordstatStopWords * std::max<uint32_t>(std::min(n_stop, tgx::kWordstatMaxStop), 1u));
    if (const char* why = tgx::wordstat_pack_table(stop_bytes, stop_offs, n_stop, flags, table.data())) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    if (!stats && !marks) return fail(TGX_ERR_INVALID, "%s: stats and marks are both NULL", who);
    if (n_rows == 0) return TGX_OK;
    wordstat_host(text, offs, n_rows, word_limit, flags, table.data(), n_stop, stats, marks);
    return TGX_OK;
}

// ---- front end ----------------------------------------------------------------------

tgx_status tgx_front_host(const uint8_t* text, const uint64_t* offs, uint64_t n_samples, const uint8_t* special_bytes, const uint64_t* special_offs,
                          uint32_t n_specials, uint32_t flags, uint64_t* seg_offs, int32_t** seg_special, uint64_t* n_segments, uint8_t** out_text,
                          uint64_t** out_offs, uint64_t* n_encoded) {
    const char* who = "tgx_front_host";
    if (!seg_offs || !seg_special || !n_segments || !out_text || !out_offs || !n_encoded) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *seg_special = nullptr;
    *out_text = nullptr;
    *out_offs = nullptr;
    *n_segments = *n_encoded = 0;
    tgx_status st = layout_check_flags(who, flags, TGX_FRONT_CRLF);
    if (st == TGX_OK) st = check_packed_list(who, "offs", "offsets", offs, n_samples, true);
    if (st != TGX_OK) return st;
    FrontHostTables ht;
    if ((st = front_build_tables(who, special_bytes, special_offs, n_specials, &ht)) != TGX_OK) return st;
    const uint64_t S = n_samples, N = offs[S];
    if (N && !text) return fail(TGX_ERR_INVALID, "%s: text is NULL", who);
    const tgx::FrontTables tab = front_tables(ht, ht.first_mask.data(), ht.first_start.data(), ht.by_first.data(), ht.sp_offs.data(), ht.sp_bytes.data());
    const uint64_t tiles = (N + tgx::kFrontTile - 1) / tgx::kFrontTile, slots = (N + tgx::kFrontGroup - 1) / tgx::kFrontGroup;
    // mark: as the kernel, tile by tile and slot by slot
    std::vector<uint16_t> hit(slots), crlf(slots), keep(slots);
    std::vector<uint64_t> tile_base(tiles + 1, 0), row_lo(tiles), row_hi(tiles);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        row_lo[tile] = tgx::pack_find_row(offs, 0, 0, S - 1, t0);
        row_hi[tile] = tgx::pack_find_row(offs, 0, 0, S - 1, last);
        uint64_t count = 0;
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t n_in = N - p0 < tgx::kFrontGroup ? (uint32_t)(N - p0) : tgx::kFrontGroup;
            uint8_t v[tgx::kFrontGroup] = {};
            memcpy(v, text + p0, n_in);
            uint32_t cr = 0;
            const uint32_t h = tgx::front_mark_slot(tab, text, offs, row_lo[tile], row_hi[tile], p0, n_in, v,
                                                    p0 + tgx::kFrontGroup < N ? text[p0 + tgx::kFrontGroup] : 0, &cr);
            hit[p0 / tgx::kFrontGroup] = (uint16_t)h;
            crlf[p0 / tgx::kFrontGroup] = (uint16_t)cr;
            count += tgx::front_popc(h);
        }
        tile_base[tile + 1] = tile_base[tile] + count;
    }
    // candidates, resolve
    const uint64_t C = tile_base[tiles];
    std::vector<uint64_t> cand_pos(C), cand_end(C), pm(C), acc_end(C, 0), la(C), seg_sum(C + 1, 0);
    std::vector<uint32_t> cand_special(C), cand_sample(C), cand_segs(C + 1, 0);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        uint64_t at = tile_base[tile];
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t h = hit[p0 / tgx::kFrontGroup];
            if (h) tgx::front_write_slot(tab, text, offs, row_lo[tile], row_hi[tile], p0, h, at, cand_pos.data(), cand_end.data(), cand_special.data(), cand_sample.data());
            at += tgx::front_popc(h);
        }
    }
    for (uint64_t c = 0; c < C; c++) pm[c] = std::max(cand_end[c], c ? pm[c - 1] : 0);
    for (uint64_t c = 0; c < C; c++)
        if (tgx::front_is_head(cand_pos.data(), pm.data(), c)) tgx::front_resolve_run(cand_pos.data(), cand_end.data(), pm.data(), C, c, acc_end.data());
    for (uint64_t c = 0; c < C; c++) la[c] = std::max(acc_end[c], c ? la[c - 1] : 0);
    for (uint64_t c = 0; c < C; c++) {
        cand_segs[c] = tgx::front_cand_segs(cand_pos.data(), acc_end.data(), la.data(), cand_sample.data(), offs, c);
        seg_sum[c + 1] = seg_sum[c] + cand_segs[c];
    }
    // segments
    std::vector<uint64_t> first(S + 1);
    for (uint64_t i = 0; i <= S; i++) first[i] = tgx::front_first_cand(cand_pos.data(), C, offs[i]);
    seg_offs[0] = 0;
    for (uint64_t i = 0; i < S; i++) {
        uint64_t tail;
        seg_offs[i + 1] = seg_offs[i] + tgx::front_sample_segs(offs, first.data(), seg_sum.data(), la.data(), i, &tail);
    }
    const uint64_t K = seg_offs[S];
    std::vector<uint64_t> seg_begin(K), seg_end(K);
    int32_t* ss = static_cast<int32_t*>(malloc(sizeof(int32_t) * std::max<uint64_t>(1, K)));
    if (!ss) return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    for (uint64_t c = 0; c < C; c++) {
        if (!acc_end[c]) continue;
        const uint64_t i = cand_sample[c];
        uint64_t k = seg_offs[i] + (seg_sum[c] - seg_sum[first[i]]);
        if (cand_segs[c] == 2) {
            seg_begin[k] = tgx::front_cursor_before(la.data(), c, offs[i]);
            seg_end[k] = cand_pos[c];
            ss[k++] = -1;
        }
        seg_begin[k] = cand_pos[c];
        seg_end[k] = cand_end[c];
        ss[k] = (int32_t)cand_special[c];
    }
    for (uint64_t i = 0; i < S; i++) {
        uint64_t tail;
        tgx::front_sample_segs(offs, first.data(), seg_sum.data(), la.data(), i, &tail);
        if (tail < offs[i + 1]) {
            const uint64_t k = seg_offs[i + 1] - 1;
            seg_begin[k] = tail;
            seg_end[k] = offs[i + 1];
            ss[k] = -1;
        }
    }
    std::vector<uint64_t> enc_begin, enc_end;
    for (uint64_t k = 0; k < K; k++)
        if (ss[k] < 0) {
            enc_begin.push_back(seg_begin[k]);
            enc_end.push_back(seg_end[k]);
        }
    const uint64_t E = enc_begin.size();
    // keep, pack
    std::vector<uint32_t> enc_local(E);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        const uint64_t e_lo = tgx::front_first_enc(enc_end.data(), 0, E, t0), e_hi = tgx::front_first_enc(enc_end.data(), 0, E, last);
        uint32_t count = 0;
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t n_in = N - p0 < tgx::kFrontGroup ? (uint32_t)(N - p0) : tgx::kFrontGroup;
            uint32_t begins = 0;
            uint64_t first_begin = 0;
            const uint32_t kp = tgx::front_keep_slot(enc_begin.data(), enc_end.data(), E, e_lo, e_hi, p0, n_in, crlf[p0 / tgx::kFrontGroup],
                                                     (flags & TGX_FRONT_CRLF) != 0, &begins, &first_begin);
            keep[p0 / tgx::kFrontGroup] = (uint16_t)kp;
            if (begins) tgx::front_slot_begins(kp, begins, first_begin, count, enc_local.data());
            count += tgx::front_popc(kp);
        }
        tile_base[tile + 1] = tile_base[tile] + count;
    }
    const uint64_t total = tiles ? tile_base[tiles] : 0;
    uint64_t* oo = static_cast<uint64_t*>(malloc(sizeof(uint64_t) * (E + 1)));
    uint8_t* ot = static_cast<uint8_t*>(malloc((size_t)std::max<uint64_t>(1, total)));
    if (!oo || !ot) {
        free(ss);
        free(oo);
        free(ot);
        return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    }
    for (uint64_t e = 0; e < E; e++) oo[e] = tile_base[enc_begin[e] / tgx::kFrontTile] + enc_local[e];
    oo[E] = total;
    for (uint64_t s = 0, at = 0; s < slots; s++) {  // at: the tile's base and the kept bytes of its slots so far
        const uint32_t kp = keep[s];
        for (uint32_t q = 0; q < tgx::kFrontGroup; q++)
            if ((kp >> q) & 1u) ot[at++] = text[s * tgx::kFrontGroup + q];
    }
    *seg_special = ss;
    *n_segments = K;
    *out_text = ot;
    *out_offs = oo;
    *n_encoded = E;
    return TGX_OK;
}

// ---- Unicode normalisation --------------------------------------------------------

namespace tgx::host {

namespace {
// the normaliser's data of unicode_tables.h behind an activity table (norm.h: NormTables' order)
tgx::NormTables norm_tables_over(const uint16_t* stage1, const uint8_t* stage2) {
    return {stage1,     stage2,     kCccCp,     kCccVal,     kCanonCp,       kCanonOff, kCanonSeq, kCanonLen, kCompatCp, kCompatOff,
            kCompatSeq, kCompatLen, kPairFirst, kPairSecond, kPairComposite, kCccN,     kCanonN,   kCompatN,  kPairN};
}
}  // namespace

const tgx::NormTables& norm_tables_on_host() {
    static const tgx::NormTables tab = norm_tables_over(norm_host_tables().stage1.data(), norm_host_tables().stage2.data());
    return tab;
}

// The activity of every scalar value (include/tgx.h: tgx_corpus_normalize), from the data of unicode_tables.h and the
// stream machine itself: a scalar that has no decomposition and is no Hangul syllable goes through the machine unchanged.
const NormHostTables& norm_host_tables() {
    static const NormHostTables tables = [] {
        NormHostTables h;
        h.ccc_cp_bytes = sizeof(kCccCp);
        h.ccc_val_bytes = sizeof(kCccVal);
        h.canon_cp_bytes = sizeof(kCanonCp);
        h.canon_off_bytes = sizeof(kCanonOff);
        h.canon_len_bytes = sizeof(kCanonLen);
        h.canon_seq_bytes = sizeof(kCanonSeq);
        h.compat_cp_bytes = sizeof(kCompatCp);
        h.compat_off_bytes = sizeof(kCompatOff);
        h.compat_len_bytes = sizeof(kCompatLen);
        h.compat_seq_bytes = sizeof(kCompatSeq);
        h.pair_bytes = sizeof(kPairFirst);
        const tgx::NormTables tab = norm_tables_over(nullptr, nullptr);  // the machine needs no activity table for a scalar alone
        std::vector<uint8_t> act(0x110000, 0);
        auto changes_alone = [&](uint32_t cp, uint32_t form) {
            uint32_t wcp[tgx::kNormWindow];
            uint8_t wcc[tgx::kNormWindow], out[128], self[4];
            tgx::NormStream s = {wcp, wcc, 1, out}, id = {wcp, wcc, 1, self};
            tgx::norm_emit(id, cp);
            const tgx::NormDecomp d = tgx::norm_decompose(tab, cp, (form & 2u) != 0);
            for (uint32_t k = 0; k < d.n; k++) tgx::norm_feed(tab, s, tgx::norm_decomp_at(d, k), (form & 1u) != 0);  // (at most 18 scalars of 4 bytes)
            tgx::norm_finalize(tab, s, (form & 1u) != 0);
            tgx::norm_flush(s);
            return s.produced != id.produced || memcmp(out, self, (size_t)id.produced) != 0;
        };
        for (uint32_t form = 0; form < 4; form++) {
            const uint8_t bit = (uint8_t)(1u << form);
            for (uint32_t k = 0; k < kCccN; k++) act[kCccCp[k]] |= bit;
            const uint32_t* cps = (form & 2u) ? kCompatCp : kCanonCp;
            const uint32_t n = (form & 2u) ? kCompatN : kCanonN;
            for (uint32_t k = 0; k < n; k++)
                if (changes_alone(cps[k], form)) act[cps[k]] |= bit;
            for (uint32_t cp = tgx::norm_hangul::S_BASE; cp < tgx::norm_hangul::S_BASE + tgx::norm_hangul::S_COUNT; cp++)
                if (changes_alone(cp, form)) act[cp] |= bit;
            if (form & 1u) {
                for (uint32_t k = 0; k < kPairN; k++) act[kPairSecond[k]] |= bit;
                for (uint32_t cp = 0x1161; cp <= 0x1175; cp++) act[cp] |= bit;
                for (uint32_t cp = 0x11A8; cp <= 0x11C2; cp++) act[cp] |= bit;
            }
            for (uint32_t cp = 0; cp < 0x110000; cp++) h.n_active[form] += (act[cp] >> form) & 1u;
        }
        h.stage1.assign(tgx::kNormStage1, 0);
        h.stage2.assign(256, 0);  // block 0: all inert
        for (uint32_t b = 0; b < tgx::kNormStage1; b++) {
            const uint8_t* blk = act.data() + (size_t)b * 256;
            if (std::all_of(blk, blk + 256, [](uint8_t x) { return x == 0; })) continue;
            h.stage1[b] = (uint16_t)(h.stage2.size() / 256);
            h.stage2.insert(h.stage2.end(), blk, blk + 256);
        }
        return h;
    }();
    return tables;
}

tgx_status norm_overflow(const char* who, uint64_t row) {
    set_error_detail(row, 0, 0);
    return fail(TGX_ERR_UNSUPPORTED, "%s: row %llu needs a stream window of more than %u scalars (a starter and %u non-starters; UAX #15 Stream-Safe text has at most 30 non-starters in a row)",
                who, (unsigned long long)row, tgx::kNormWindow, tgx::kNormWindow - 1);
}

}  // namespace tgx::host

tgx_status tgx_normalize_host(uint32_t form, const uint8_t* text, const uint64_t* offs, uint64_t n_rows, uint8_t** out_text, uint64_t** out_offs,
                              uint64_t* n_pieces) {
    const char* who = "tgx_normalize_host";
    if (!out_text || !out_offs || !n_pieces) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out_text = nullptr;
    *out_offs = nullptr;
    *n_pieces = 0;
    if (form > 3) return fail(TGX_ERR_INVALID, "%s: form must be 0 (NFD), 1 (NFC), 2 (NFKD) or 3 (NFKC)", who);
    tgx_status st = check_packed_list(who, "offs", "offsets", offs, n_rows, true);
    if (st != TGX_OK) return st;
    const uint64_t S = n_rows, N = offs[S];
    if (N && !text) return fail(TGX_ERR_INVALID, "%s: text is NULL", who);
    const tgx::NormTables& tab = norm_tables_on_host();
    const uint64_t tiles = (N + tgx::kFrontTile - 1) / tgx::kFrontTile, slots = (N + tgx::kFrontGroup - 1) / tgx::kFrontGroup;
    // mark: as the kernel, tile by tile and slot by slot
    std::vector<uint32_t> mask(slots), slot_pre(slots);
    std::vector<uint64_t> tile_base(tiles + 1, 0), tile_place(tiles + 1, 0), row_lo(tiles), row_hi(tiles);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        row_lo[tile] = tgx::pack_find_row(offs, 0, 0, S - 1, t0);
        row_hi[tile] = tgx::pack_find_row(offs, 0, 0, S - 1, last);
        uint64_t count = 0;
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t n_in = N - p0 < tgx::kFrontGroup ? (uint32_t)(N - p0) : tgx::kFrontGroup;
            uint8_t v[tgx::kFrontGroup] = {};
            memcpy(v, text + p0, n_in);
            const uint32_t m = tgx::norm_mark_slot(tab, form, text, offs, row_lo[tile], row_hi[tile], p0, n_in, v,
                                                   p0 + tgx::kFrontGroup < N ? text[p0 + tgx::kFrontGroup] : 0);
            mask[p0 / tgx::kFrontGroup] = m;
            count += tgx::front_popc(m >> 16);
        }
        tile_base[tile + 1] = tile_base[tile] + count;
    }
    const uint64_t P = tile_base[tiles];
    uint64_t* oo = static_cast<uint64_t*>(malloc(sizeof(uint64_t) * (S + 1)));
    if (!oo) return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    if (P == 0) {  // nothing to rewrite: a copy
        uint8_t* ot = static_cast<uint8_t*>(malloc((size_t)std::max<uint64_t>(1, N)));
        if (!ot) {
            free(oo);
            return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
        }
        if (N) memcpy(ot, text, (size_t)N);
        memcpy(oo, offs, sizeof(uint64_t) * (S + 1));
        *out_text = ot;
        *out_offs = oo;
        return TGX_OK;
    }
    // pieces
    std::vector<uint64_t> piece_begin(P), piece_row(P), piece_sum(P + 1, 0);
    for (uint64_t tile = 0; tile < tiles; tile++) {
        uint64_t at = tile_base[tile];
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t heads = mask[p0 / tgx::kFrontGroup] >> 16;
            if (heads) tgx::norm_write_pieces(offs, row_lo[tile], row_hi[tile], p0, heads, at, piece_begin.data(), piece_row.data());
            at += tgx::front_popc(heads);
        }
    }
    // length
    uint32_t wcp[tgx::kNormWindow];
    uint8_t wcc[tgx::kNormWindow];
    uint64_t overflow_row = tgx::kNormNoRow;
    for (uint64_t k = 0; k < P; k++) {
        tgx::NormStream s = {wcp, wcc, 1, nullptr};
        tgx::norm_run_piece(tab, form, text, piece_begin[k], offs[piece_row[k] + 1], s);
        piece_sum[k + 1] = piece_sum[k] + s.produced;
        if (s.overflow) overflow_row = std::min(overflow_row, piece_row[k]);
    }
    if (overflow_row != tgx::kNormNoRow) {
        free(oo);
        return norm_overflow(who, overflow_row);
    }
    // places
    for (uint64_t tile = 0; tile < tiles; tile++) {
        const uint64_t t0 = tile * tgx::kFrontTile, last = tgx::tile_last(t0, tgx::kFrontTile, N);
        uint32_t copied = 0, heads = 0;
        for (uint64_t p0 = t0; p0 <= last; p0 += tgx::kFrontGroup) {
            const uint32_t n_in = N - p0 < tgx::kFrontGroup ? (uint32_t)(N - p0) : tgx::kFrontGroup, m = mask[p0 / tgx::kFrontGroup];
            slot_pre[p0 / tgx::kFrontGroup] = copied | heads << 16;
            copied += tgx::front_popc(tgx::norm_verbatim(m, n_in));
            heads += tgx::front_popc(m >> 16);
        }
        tile_place[tile + 1] = tile_place[tile] + tgx::norm_tile_bytes(tile_base.data(), piece_sum.data(), tile, copied);
    }
    const tgx::NormPlaces pl = {mask.data(), slot_pre.data(), tile_base.data(), piece_sum.data(), tile_place.data()};
    const uint64_t total = tile_place[tiles];
    for (uint64_t r = 0; r <= S; r++) oo[r] = offs[r] < N ? tgx::norm_place(pl, offs[r]) : total;
    // write
    uint8_t* ot = static_cast<uint8_t*>(malloc((size_t)std::max<uint64_t>(1, total)));
    if (!ot) {
        free(oo);
        return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    }
    for (uint64_t p0 = 0; p0 < N; p0 += tgx::kFrontGroup) {
        const uint32_t n_in = N - p0 < tgx::kFrontGroup ? (uint32_t)(N - p0) : tgx::kFrontGroup;
        uint8_t v[tgx::kFrontGroup] = {};
        memcpy(v, text + p0, n_in);
        tgx::norm_copy_slot(pl, p0, n_in, v, ot);
    }
    for (uint64_t k = 0; k < P; k++) {
        tgx::NormStream s = {wcp, wcc, 1, ot + tgx::norm_place(pl, piece_begin[k])};
        tgx::norm_run_piece(tab, form, text, piece_begin[k], offs[piece_row[k] + 1], s);
    }
    *out_text = ot;
    *out_offs = oo;
    *n_pieces = P;
    return TGX_OK;
}

// ---- decode -----------------------------------------------------------------------

tgx_status tgx_decode_rows_host(const uint8_t* vocab_bytes, const uint64_t* vocab_offs, uint32_t vocab_size, const uint8_t* special_bytes,
                                const uint64_t* special_offs, uint32_t n_specials, const void* ids, uint32_t id_kind, const uint64_t* id_offs,
                                uint64_t n_rows, uint64_t row_len, const uint8_t* mask, const int32_t* lengths, uint32_t skip_id, int include_special,
                                uint8_t** out_text, uint64_t* out_offs, uint64_t* n_replaced, uint64_t* bad_sample, uint64_t* bad_id) {
    const char* who = "tgx_decode_rows_host";
    if (!vocab_offs || !out_text || !out_offs) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out_text = nullptr;
    if (id_kind > tgx::kDecodeI64) return fail(TGX_ERR_INVALID, "%s: id_kind %u", who, id_kind);
    if (id_offs && id_kind != tgx::kDecodeU32) return fail(TGX_ERR_INVALID, "%s: the offsets form takes u32 ids", who);
    tgx_status st = decode_check_specials(who, vocab_size, special_bytes, special_offs, n_specials);
    if (st != TGX_OK) return st;
    if (id_offs && (st = layout_check_host(who, static_cast<const uint32_t*>(ids), id_offs, n_rows)) != TGX_OK) return st;
    if (!id_offs && n_rows && row_len && n_rows > 0xFFFFFFFFFFFFFFFFull / 16 / row_len) return fail(TGX_ERR_UNSUPPORTED, "%s: too many elements", who);
    const uint64_t S = n_rows, N = id_offs ? id_offs[S] : n_rows * row_len;
    if (N && !ids) return fail(TGX_ERR_INVALID, "%s: ids is NULL", who);
    std::vector<uint8_t> len;
    std::vector<tgx::DecodeSlot> slots;
    if ((st = decode_build_tables(who, vocab_bytes, vocab_offs, vocab_size, &len, &slots)) != TGX_OK) return st;
    static const uint64_t kNoOffs[1] = {0};
    tgx::DecodeTables tab = {};
    tab.tok_len = len.data();
    tab.slots = slots.data();
    tab.bytes = vocab_bytes;
    tab.offs = vocab_offs;
    tab.sp_bytes = special_bytes;
    tab.sp_offs = n_specials ? special_offs : kNoOffs;
    tab.vocab_size = vocab_size;
    tab.n_specials = n_specials;
    tab.include_special = include_special ? 1 : 0;
    tgx::DecodeSrc src = {};
    src.ids = ids;
    src.offs = id_offs;
    src.mask = id_offs ? nullptr : mask;
    src.lengths = id_offs ? nullptr : lengths;
    src.n_rows = S;
    src.row_len = row_len;
    src.n = N;
    src.kind = id_kind;
    src.skip_id = id_offs ? TGX_NO_ID : skip_id;
    if (n_replaced) *n_replaced = 0;
    for (uint64_t i = 0; i <= S; i++) out_offs[i] = 0;
    // as the device: the elements' meta words, the two scans, ...
    std::vector<uint64_t> B(N + 1), X(N + 1);
    uint64_t bad = ~0ull, n_live_specials = 0;
    for (uint64_t j = 0, b = 0, x = 0; j <= N; j++) {
        B[j] = b;
        X[j] = x;
        if (j == N) break;
        const int64_t v = tgx::decode_elem(src, j);
        if (!tgx::decode_live(src, j, v)) continue;
        bool oob;
        const uint32_t meta = tgx::decode_meta(tab, v, &oob);
        if (oob && j < bad) bad = j;
        b += meta & ~tgx::kDecodeSpecial;
        x += meta >> 31;
        n_live_specials += meta >> 31;
    }
    if (bad != ~0ull) {
        const uint64_t row = id_offs ? (uint64_t)(std::upper_bound(id_offs, id_offs + S + 1, bad) - id_offs) - 1 : bad / row_len;
        return decode_oob(id_kind, tgx::decode_elem(src, bad), row, bad_sample, bad_id);
    }
    const uint64_t T = B[N], G = (T + tgx::kDecodeGroup - 1) / tgx::kDecodeGroup;
    uint8_t* raw = static_cast<uint8_t*>(aligned_alloc(16, (size_t)G * tgx::kDecodeGroup + 16));
    if (!raw) return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    if (T == 0) {
        *out_text = raw;
        return TGX_OK;
    }
    memset(raw, 0xA5, (size_t)G * tgx::kDecodeGroup + 16);  // (what lies behind the text may be anything)
    std::vector<uint32_t> flags(G), codes(G + 1, 0);
    // ... the fill kernel's tiles and thread slots, ...
    tgx::tiled_fill_host(
        T, T, tgx::kDecodeTile, tgx::kDecodeGroup, tgx::kDecodeBack, [&](uint64_t b) { return tgx::pack_find_row(B.data(), 0, 0, N - 1, b); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            uint8_t v[tgx::kDecodeGroup] = {};
            flags[e0 / tgx::kDecodeGroup] = tgx::decode_group(tab, src, B.data(), n_live_specials ? X.data() : nullptr, lo, hi, e0, n_in, v);
            memcpy(raw + e0, v, n_in);
            return true;
        });
    // ... the rows' raw starts, which start runs, ...
    for (uint64_t i = 0; i <= S; i++) {
        const uint64_t r = B[i < S ? tgx::decode_row_first(src, i) : N];
        out_offs[i] = r;
        if (r < T) flags[r / tgx::kDecodeGroup] |= 1u << (uint32_t)(r % tgx::kDecodeGroup);
    }
    // ... the UTF-8 rule per slot, ...
    uint64_t replaced = 0;
    for (uint64_t g = 0; g < G; g++) {
        codes[g] = tgx::decode_utf8_slot(raw, flags.data(), T, g);
        replaced += tgx::decode_code_replaced(codes[g]);
    }
    if (n_replaced) *n_replaced = replaced;
    if (replaced == 0) {
        *out_text = raw;
        return TGX_OK;
    }
    // ... and, after a replacement, the slots' positions and the second copy
    std::vector<uint64_t> gpos(G + 1);
    for (uint64_t g = 0, at = 0; g <= G; g++) {
        gpos[g] = at;
        at += tgx::decode_code_bytes(codes[g], tgx::kDecodeGroup);
    }
    uint8_t* text = static_cast<uint8_t*>(malloc((size_t)std::max<uint64_t>(1, gpos[G])));
    if (!text) {
        free(raw);
        return fail(TGX_ERR_INVALID, "%s: out of host memory", who);
    }
    for (uint64_t g = 0; g < G; g++) tgx::decode_expand_slot(raw, T, g, codes[g], text, gpos[g]);
    for (uint64_t i = 0; i <= S; i++) out_offs[i] = tgx::decode_final_pos(gpos.data(), codes.data(), out_offs[i], T);
    free(raw);
    *out_text = text;
    return TGX_OK;
}

// ---- spans ------------------------------------------------------------------------

namespace {

template <class T>
void spans_host_write(const tgx::LayoutSeq& seq, const uint64_t* offs, uint64_t n_rows, uint64_t n, const uint64_t* P, const uint32_t* vals,
                      uint32_t row_len, uint32_t flags, T* out) {
    if (row_len) {  // as the kernel: one pair per slot
        for (uint64_t e = 0; e < n_rows * (uint64_t)row_len; e++) {
            tgx::SpanPair s = {0, 0};
            if (n) s = tgx::span_pad_at(seq, offs, P, vals, row_len, flags, e);
            out[2 * e] = (T)s.start;
            out[2 * e + 1] = (T)s.end;
        }
        return;
    }
    // as the kernel: the tiled fill over the stream's elements
    tgx::tiled_fill_host(
        n, n, tgx::kSpanTile, tgx::kSpanGroup, 0, [&](uint64_t j) { return tgx::pack_find_row(offs, 0, 0, n_rows - 1, j); },
        [&](uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in) {
            tgx::SpanPair v[tgx::kSpanGroup] = {};
            tgx::span_group(offs, P, vals, lo, hi, e0, n_in, v);
            for (uint32_t k = 0; k < n_in; k++) {
                out[2 * (e0 + k)] = (T)v[k].start;
                out[2 * (e0 + k) + 1] = (T)v[k].end;
            }
            return true;
        });
}

// as the kernel: one pair per slot
template <class T>
void window_spans_host_write(const tgx::LayoutSeq& seq, const uint64_t* offs, const uint64_t* wo, uint64_t n_rows, uint64_t n, uint64_t n_windows,
                             const uint64_t* P, const uint32_t* vals, uint32_t row_len, uint32_t stride, uint32_t flags, T* out) {
    for (uint64_t e = 0; e < n_windows * (uint64_t)row_len; e++) {
        tgx::SpanPair s = {0, 0};
        if (n) s = tgx::span_window_at(seq, offs, wo, n_rows, P, vals, row_len, stride, flags, e);
        out[2 * e] = (T)s.start;
        out[2 * e + 1] = (T)s.end;
    }
}

// The meta pass and the scan of the span writers, and the int32 check of the rows' totals: vals[0 .. T] and P[0 .. T].
tgx_status span_host_sums(const char* who, const uint8_t* vocab_bytes, const uint64_t* vocab_offs, uint32_t vocab_size, const uint8_t* special_bytes,
                          const uint64_t* special_offs, uint32_t n_specials, const uint32_t* ids, const uint64_t* offs, uint64_t S, bool chars,
                          bool i64, std::vector<uint32_t>* vals_out, std::vector<uint64_t>* P_out) {
    const uint64_t T = offs[S];
    std::vector<uint16_t> words;
    const tgx_status st = span_build_words(who, vocab_bytes, vocab_offs, vocab_size, &words);
    if (st != TGX_OK) return st;
    std::vector<uint64_t> sp_words;
    span_special_words(special_bytes, special_offs, n_specials, chars, &sp_words);
    tgx::SpanTables tab = {};
    tab.words = words.data();
    tab.sp_words = sp_words.data();
    tab.vocab_size = vocab_size;
    tab.n_specials = n_specials;
    std::vector<uint32_t>& vals = *vals_out;
    std::vector<uint64_t>& P = *P_out;
    vals.assign((size_t)T + 1, 0);
    P.assign((size_t)T + 1, 0);
    for (uint64_t j = 0; j < T; j++) {
        bool oob;
        vals[j] = tgx::span_val(tab, ids[j], chars, &oob);
        if (oob) {
            const uint64_t row = (uint64_t)(std::upper_bound(offs, offs + S + 1, j) - offs) - 1;
            return decode_oob(tgx::kDecodeU32, ids[j], row, nullptr, nullptr);
        }
        P[j + 1] = P[j] + (vals[j] & ~tgx::kSpanValCont);
    }
    if (!i64) {
        uint64_t row_max = 0;
        for (uint64_t i = 0; i < S; i++) row_max = std::max(row_max, tgx::span_row_total(P.data(), offs, i));
        if (row_max >= 0x80000000ull) return span_too_long(who, row_max, chars);
    }
    return TGX_OK;
}

}  // namespace

tgx_status tgx_spans_host(const uint8_t* vocab_bytes, const uint64_t* vocab_offs, uint32_t vocab_size, const uint8_t* special_bytes,
                          const uint64_t* special_offs, uint32_t n_specials, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows,
                          uint32_t row_len, uint32_t bos_id, uint32_t eos_id, uint32_t flags, void* out) {
    const char* who = "tgx_spans_host";
    if (!vocab_offs) return fail(TGX_ERR_INVALID, "%s: vocab_offs is NULL", who);
    const bool padded = row_len != 0, chars = (flags & TGX_SPAN_CHARS) != 0, i64 = (flags & TGX_LAYOUT_I64) != 0;
    tgx_status st = span_check_args(who, vocab_size, special_bytes, special_offs, n_specials, padded, row_len, bos_id, eos_id, flags);
    if (st == TGX_OK) st = layout_check_host(who, ids, offs, n_rows);
    if (st != TGX_OK) return st;
    const uint64_t S = n_rows, T = offs[S];
    const uint64_t n_pairs = padded ? S * (uint64_t)row_len : (S ? T : 0);
    if (n_pairs == 0) return TGX_OK;
    if (!out) return fail(TGX_ERR_INVALID, "%s: out is NULL", who);
    std::vector<uint32_t> vals;
    std::vector<uint64_t> P;
    if ((st = span_host_sums(who, vocab_bytes, vocab_offs, vocab_size, special_bytes, special_offs, n_specials, ids, offs, S, chars, i64, &vals,
                             &P)) != TGX_OK)
        return st;
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, 0);
    const uint32_t* v = chars ? vals.data() : nullptr;
    if (i64)
        spans_host_write(seq, offs, S, T, P.data(), v, row_len, flags, static_cast<int64_t*>(out));
    else
        spans_host_write(seq, offs, S, T, P.data(), v, row_len, flags, static_cast<int32_t*>(out));
    return TGX_OK;
}

tgx_status tgx_window_spans_host(const uint8_t* vocab_bytes, const uint64_t* vocab_offs, uint32_t vocab_size, const uint8_t* special_bytes,
                                 const uint64_t* special_offs, uint32_t n_specials, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows,
                                 uint32_t row_len, uint32_t stride, uint32_t bos_id, uint32_t eos_id, uint32_t flags, uint64_t n_windows, void* out,
                                 uint64_t* n_windows_out) {
    const char* who = "tgx_window_spans_host";
    if (!vocab_offs || !n_windows_out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    if (row_len == 0) return fail(TGX_ERR_INVALID, "%s: row_len 0 (needs >= 1)", who);
    const bool chars = (flags & TGX_SPAN_CHARS) != 0, i64 = (flags & TGX_LAYOUT_I64) != 0;
    tgx_status st = span_check_args(who, vocab_size, special_bytes, special_offs, n_specials, true, row_len, bos_id, eos_id, flags);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, 0);
    if (st == TGX_OK) st = window_check_args(who, row_len, stride, seq.extra);
    if (st == TGX_OK) st = layout_check_host(who, ids, offs, n_rows);
    if (st != TGX_OK) return st;
    const uint64_t S = n_rows, T = offs[S];
    std::vector<uint64_t> wo;
    uint64_t max_row = 0;
    windows_host_offsets(offs, S, row_len - seq.extra, row_len - seq.extra - stride, &wo, &max_row);
    const uint64_t W = wo[S];
    if ((st = window_check_totals(who, max_row, W, nullptr)) != TGX_OK) return st;
    *n_windows_out = W;
    if (!out) return TGX_OK;
    if ((st = window_check_totals(who, max_row, W, &n_windows)) != TGX_OK || W == 0) return st;
    std::vector<uint32_t> vals;
    std::vector<uint64_t> P;
    if ((st = span_host_sums(who, vocab_bytes, vocab_offs, vocab_size, special_bytes, special_offs, n_specials, ids, offs, S, chars, i64, &vals,
                             &P)) != TGX_OK)
        return st;
    const uint32_t* v = chars ? vals.data() : nullptr;
    if (i64)
        window_spans_host_write(seq, offs, wo.data(), S, T, W, P.data(), v, row_len, stride, flags, static_cast<int64_t*>(out));
    else
        window_spans_host_write(seq, offs, wo.data(), S, T, W, P.data(), v, row_len, stride, flags, static_cast<int32_t*>(out));
    return TGX_OK;
}

// ---- lattice statistics -------------------------------------------------------------

namespace {

// the vocabulary as a byte trie of its own: child (node, byte) by hash, a later duplicate token overrides an earlier one
struct StatsTrie {
    std::unordered_map<uint64_t, uint32_t> next;  // node << 8 | byte -> node
    std::vector<double> score;                    // per node
    std::vector<uint8_t> terminal;
};

// log(exp(a) + exp(b)) for a, b finite or -inf (lattice_walk.h: log_add)
double stats_log_add_host(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo == -HUGE_VAL) return hi;
    return hi + log1p(exp(lo - hi));
}

}  // namespace

tgx_status tgx_lattice_stats_host(const uint8_t* vocab_bytes, const uint64_t* vocab_offs, const double* scores, uint32_t vocab_size,
                                  const uint8_t* text, const uint64_t* offs, uint64_t n_samples, double alpha, double* logz, double* escore,
                                  double* etokens, uint64_t* n_no_path) {
    const char* who = "tgx_lattice_stats_host";
    // alpha and the scores as sample_check (lattice_pass.cpp) takes them, with its statuses
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(TGX_ERR_INVALID, "alpha must be finite and >= 0 (got %g)", alpha);
    if (vocab_size && !scores) return fail(TGX_ERR_INVALID, "%s: scores is NULL", who);
    tgx_status st = check_packed_list(who, "vocabulary offsets", "vocabulary offsets", vocab_offs, vocab_size, false);
    if (st == TGX_OK) st = check_packed_list(who, "offs", "offsets", offs, n_samples, true);
    if (st != TGX_OK) return st;
    for (uint32_t i = 0; i < vocab_size; i++)
        if (!std::isfinite(scores[i])) return fail(TGX_ERR_UNSUPPORTED, "sampling needs every score to be finite");
    for (uint32_t i = 0; i < vocab_size; i++)
        if (!std::isfinite(alpha * scores[i])) return fail(TGX_ERR_INVALID, "alpha * score overflows (alpha %g)", alpha);
    const uint64_t S = n_samples, N = offs[S];
    if (N && !text) return fail(TGX_ERR_INVALID, "%s: text is NULL", who);
    if (vocab_size && vocab_offs[vocab_size] > vocab_offs[0] && !vocab_bytes) return fail(TGX_ERR_INVALID, "%s: vocab_bytes is NULL", who);

    StatsTrie trie;
    trie.score.assign(1, 0.0);
    trie.terminal.assign(1, 0);
    for (uint32_t i = 0; i < vocab_size; i++) {
        const uint64_t len = vocab_offs[i + 1] - vocab_offs[i];
        if (len > TGX_MAX_TOKEN_LEN)
            return fail(TGX_ERR_UNSUPPORTED, "%s: token of %llu bytes exceeds TGX_MAX_TOKEN_LEN (%d)", who, (unsigned long long)len, TGX_MAX_TOKEN_LEN);
        if (len == 0) continue;  // matches nothing
        uint32_t node = 0;
        for (uint64_t k = 0; k < len; k++) {
            const uint64_t key = ((uint64_t)node << 8) | vocab_bytes[vocab_offs[i] + k];
            auto it = trie.next.find(key);
            if (it == trie.next.end()) {
                it = trie.next.emplace(key, (uint32_t)trie.score.size()).first;
                trie.score.push_back(0.0);
                trie.terminal.push_back(0);
            }
            node = it->second;
        }
        trie.terminal[node] = 1;
        trie.score[node] = scores[i];
    }

    // as stats_kernel: A[p] by log_add over the matches ending at p in ascending order of their start, and with every
    // log_add the normalised expectations m[p], t[p] move towards the new term's by its share exp(x - A')
    uint64_t bad = 0;
    std::vector<double> A, M, T;
    for (uint64_t i = 0; i < S; i++) {
        const uint64_t beg = offs[i], n = offs[i + 1] - beg;
        A.assign(n + 1, -HUGE_VAL);
        M.assign(n + 1, 0.0);
        T.assign(n + 1, 0.0);
        A[0] = 0.0;
        for (uint64_t q = 0; q < n; q++) {
            if (A[q] == -HUGE_VAL) continue;
            uint32_t node = 0;
            for (uint64_t d = 0; d < TGX_MAX_TOKEN_LEN && q + d < n; d++) {
                const auto it = trie.next.find(((uint64_t)node << 8) | text[beg + q + d]);
                if (it == trie.next.end()) break;
                node = it->second;
                if (!trie.terminal[node]) continue;
                const uint64_t p = q + d + 1;
                const double s = trie.score[node];
                const double x = A[q] + alpha * s;
                const double nw = stats_log_add_host(A[p], x);
                const double pi = exp(x - nw);
                M[p] = M[p] + pi * ((M[q] + s) - M[p]);
                T[p] = T[p] + pi * ((T[q] + 1.0) - T[p]);
                A[p] = nw;
            }
        }
        const bool reached = A[n] != -HUGE_VAL;
        if (!reached) bad++;
        if (logz) logz[i] = A[n];
        if (escore) escore[i] = reached ? M[n] : NAN;
        if (etokens) etokens[i] = reached ? T[n] : NAN;
    }
    if (n_no_path) *n_no_path = bad;
    return TGX_OK;
}
