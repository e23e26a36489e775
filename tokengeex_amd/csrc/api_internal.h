// What the device-side host code (tgx_api.cpp, encode_pass.cpp, estep_pass.cpp, lattice_pass.cpp, result_ops.cpp, corpus_ops.cpp) and host_twins.cpp share, free of HIP
// types: the thread-local error state, and the argument checks that the *_host twins (host_twins.cpp) share with the
// device entry points.  Shared helpers live in tgx::host; what needs HIP types is in device_internal.h.  prune_host.cpp,
// frontback.cpp and unicode_norm.cpp take tgx_set_error from here.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/tgx.h"

// records the message tgx_last_error() returns (thread-local); tgx_api.cpp
tgx_status tgx_set_error(tgx_status st, const char* msg);

namespace tgx {
struct DecodeSlot;   // decode.h
struct FrontTables;  // front.h
struct NormTables;   // norm.h
}

namespace tgx::host {

// ---- thread-local error state ------------------------------------------------
inline thread_local std::string g_err_msg;
inline thread_local uint64_t g_err_sample = 0, g_err_pos = 0, g_err_len = 0;

inline tgx_status fail(tgx_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err_msg = buf;
    return st;
}
// what tgx_last_error_detail() returns
inline void set_error_detail(uint64_t sample, uint64_t pos, uint64_t len) {
    g_err_sample = sample;
    g_err_pos = pos;
    g_err_len = len;
}

// ---- argument checks of the *_host twins and of their device entry points (host_twins.cpp) ------------------------
tgx_status layout_check_ids(const char* who, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id);
tgx_status layout_check_flags(const char* who, uint32_t flags, uint32_t allowed);
tgx_status layout_check_row_len(const char* who, uint32_t row_len, uint32_t extra);
// the windowed layout: row_len >= extra + 1 and stride < row_len - extra; then the longest row and the windows against
// 2^31, and the windows against what the caller sized its buffers for (sized_for, NULL when nothing is written)
tgx_status window_check_args(const char* who, uint32_t row_len, uint32_t stride, uint32_t extra);
tgx_status window_check_totals(const char* who, uint64_t max_row, uint64_t n_windows, const uint64_t* sized_for);
// ids and offsets of n_rows rows in host memory
tgx_status layout_check_host(const char* who, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows);
tgx_status assemble_check(const char* who, const uint64_t* seg_offs, const int32_t* seg_special, uint64_t n_samples, uint32_t vocab_size,
                          uint32_t n_specials, bool have_segs, uint64_t n_rows, uint64_t* n_segs);
// fill-in-the-middle: the rates in [0, 1] and three pairwise distinct sentinels, none of them TGX_NO_ID; the output's
// vocabulary size for an input of vocab_size
tgx_status fim_check(const char* who, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id, double rate, double spm_rate);
uint32_t fim_vocab_size(uint32_t vocab_size, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id);
// row selection: TGX_ERR_INVALID naming output row k and its index `value`, which is not a row of n_src; every index of
// host rows against n_src (the smallest offending k is named)
tgx_status select_index_error(const char* who, uint64_t k, int64_t value, uint64_t n_src);
tgx_status select_check_rows(const char* who, const int64_t* rows, uint64_t n_select, uint64_t n_src);
// ids and offsets in host memory as a result's: layout_check_host, vocab_size <= 0xFFFFFFFE and every id below it
tgx_status result_check_host(const char* who, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t vocab_size);
tgx_status decode_build_tables(const char* who, const uint8_t* bytes, const uint64_t* offs, uint32_t V, std::vector<uint8_t>* len,
                               std::vector<tgx::DecodeSlot>* slots);
tgx_status decode_check_specials(const char* who, uint32_t vocab_size, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials);
// TGX_ERR_TOKEN_ID_OOB for element x (of a tgx::DecodeSrc::kind) of row `row`, with its error detail
tgx_status decode_oob(uint32_t kind, int64_t x, uint64_t row, uint64_t* bad_sample, uint64_t* bad_id);
tgx_status span_build_words(const char* who, const uint8_t* bytes, const uint64_t* offs, uint32_t V, std::vector<uint16_t>* words);
void span_special_words(const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials, bool chars, std::vector<uint64_t>* words);
tgx_status span_check_args(const char* who, uint32_t vocab_size, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials,
                           bool padded, uint32_t row_len, uint32_t bos_id, uint32_t eos_id, uint32_t flags);
tgx_status span_too_long(const char* who, uint64_t row_max, bool chars);
// the special tokens as the front kernels read them (front.h: FrontTables)
struct FrontHostTables {
    std::vector<uint32_t> first_mask, first_start, by_first, sp_offs;
    std::vector<uint8_t> sp_bytes, firsts;  // firsts: the distinct first bytes, ascending
    uint32_t max_len = 0;                   // the longest special
};
tgx::FrontTables front_tables(const FrontHostTables& t, const uint32_t* first_mask, const uint32_t* first_start, const uint32_t* by_first,
                              const uint32_t* sp_offs, const uint8_t* sp_bytes);
tgx_status front_build_tables(const char* who, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials, FrontHostTables* t);
// the normaliser's tables over host memory (norm.h: NormTables; the data of unicode_tables.h and the two-stage activity
// table made from it), built once per process; sizes in bytes of what tgx_corpus_normalize uploads once per device
struct NormHostTables {
    std::vector<uint16_t> stage1;
    std::vector<uint8_t> stage2;
    uint64_t n_active[4] = {0, 0, 0, 0};  // active scalar values per form
    size_t ccc_cp_bytes = 0, ccc_val_bytes = 0, canon_cp_bytes = 0, canon_off_bytes = 0, canon_len_bytes = 0, canon_seq_bytes = 0, compat_cp_bytes = 0,
           compat_off_bytes = 0, compat_len_bytes = 0, compat_seq_bytes = 0, pair_bytes = 0;
};
const NormHostTables& norm_host_tables();
const tgx::NormTables& norm_tables_on_host();
// TGX_ERR_UNSUPPORTED for a row whose stream window overflows, with its error detail
tgx_status norm_overflow(const char* who, uint64_t row);

}  // namespace tgx::host
