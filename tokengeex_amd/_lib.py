"""ctypes binding of the C ABI declared in include/tgx.h (tokengeex_amd/libtgx.so).

The extension is mandatory: importing this module raises if libtgx.so is missing
or does not export a declared symbol, and every compute call raises
TokenGeeXError when no gfx950 device is usable.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtgx.so")

# tgx_status (include/tgx.h)
OK, ERR_IO, ERR_JSON, ERR_TOKEN_ID_OOB, ERR_NO_PATH, ERR_DEVICE, ERR_Z_NOT_NORMAL, ERR_INVALID, \
    ERR_UNSUPPORTED = range(9)
MAX_TOKEN_LEN = 64
MAX_NBEST = 16  # TGX_MAX_NBEST
ESTEP_SNIPPET_LEN = 81920
NO_ID = 0xFFFFFFFF  # TGX_NO_ID: no bos / eos
LAYOUT_PAD_LEFT, LAYOUT_TRUNC_LEFT, LAYOUT_I64 = 1, 2, 4  # TGX_LAYOUT_*
FRONT_CRLF = 1  # TGX_FRONT_CRLF
SPAN_CHARS = 8  # TGX_SPAN_CHARS
SELECT_ROWS_DEVICE = 1  # TGX_SELECT_ROWS_DEVICE

# every exported symbol of include/tgx.h: name -> (restype, argtypes)
_vp, _u64, _u32, _i, _d = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
_pvp, _pu64 = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
SYMBOLS = {
    "tgx_last_error": (C.c_char_p, []),
    "tgx_last_error_detail": (None, [_pu64, _pu64, _pu64]),
    "tgx_abi_version": (_i, []),
    "tgx_device_count": (_i, []),
    "tgx_model_create": (_i, [_vp, _vp, _vp, _u32, _i, _pvp]),
    "tgx_model_create_ex": (_i, [_vp, _vp, _vp, _u32, _i, _u32, _pvp]),
    "tgx_model_create_derived": (_i, [_vp, _vp, _u32, _vp, _u32, _pvp]),
    "tgx_model_destroy": (None, [_vp]),
    "tgx_model_vocab_size": (_u32, [_vp]),
    "tgx_model_max_token_len": (_u32, [_vp]),
    "tgx_model_trie_bytes": (_u64, [_vp]),
    "tgx_model_device": (_i, [_vp]),
    "tgx_common_prefix_search": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _pu64]),
    "tgx_flat_trie_build": (_i, [_vp, _vp, _vp, _u32, _pvp]),
    "tgx_flat_trie_free": (None, [_vp]),
    "tgx_flat_trie_search": (_u64, [_vp, _vp, _u64, _vp, _vp, _u64]),
    "tgx_flat_trie_search8": (_u64, [_vp, _vp, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint32), _pu64,
                                     C.POINTER(C.c_double)]),
    "tgx_flat_trie_stats": (None, [_vp, _pu64, _pu64, C.POINTER(C.c_uint32)]),
    "tgx_flat_trie_copy": (None, [_vp, _vp, _vp, _vp]),
    "tgx_tok_hash_selftest": (_i, [_vp, _vp, _u32, C.POINTER(C.c_uint32), _pu64]),
    "tgx_dropout_u01_host": (_d, [_u64, _u64, _u64, _u32]),
    "tgx_encode_batch": (_i, [_vp, _vp, _vp, _u64, _d, _u64, _pvp]),
    "tgx_encode_batch_host": (_i, [_vp, _vp, _vp, _u64, _d, _u64, _vp, _u64, _vp, _pu64]),
    "tgx_encode_batch_multi": (_i, [_vp, _u32, _vp, _vp, _u64, _d, _u64, _vp, _u64, _vp, _pu64]),
    "tgx_result_num_samples": (_u64, [_vp]),
    "tgx_result_num_tokens": (_u64, [_vp]),
    "tgx_result_ids": (_vp, [_vp]),
    "tgx_result_offsets": (_vp, [_vp]),
    "tgx_result_copy_ids": (_i, [_vp, _vp, _u64]),
    "tgx_result_copy_offsets": (_i, [_vp, _vp, _u64]),
    "tgx_result_ids_device": (_vp, [_vp]),
    "tgx_result_offsets_device": (_vp, [_vp]),
    "tgx_result_free": (None, [_vp]),
    "tgx_corpus_upload": (_i, [_i, _vp, _vp, _u64, _pvp]),
    "tgx_corpus_free": (None, [_vp]),
    "tgx_corpus_num_samples": (_u64, [_vp]),
    "tgx_corpus_num_bytes": (_u64, [_vp]),
    "tgx_encode_corpus": (_i, [_vp, _vp, _d, _u64, _pvp]),
    "tgx_count_tokens": (_i, [_vp, _vp, _vp]),
    "tgx_count_pairs": (_i, [_vp, _vp, _pvp, _pvp, _pu64]),
    "tgx_count_pairs_top": (_i, [_vp, _vp, _u64, _pvp, _pvp, _pu64, _pu64]),
    "tgx_estep": (_i, [_vp, _vp, _u64, _d, _u64, _vp, C.POINTER(C.c_double)]),
    "tgx_split_specials": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _pvp, _pvp, _pvp, _pu64]),
    "tgx_pack_segments": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _vp, _vp, _pu64]),
    "tgx_normalize_segments": (_i, [_u32, _vp, _vp, _vp, _u64, _pvp, _pvp]),
    "tgx_unidata_version": (C.c_char_p, []),
    "tgx_assemble_ids": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _vp]),
    "tgx_decode_batch": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u64, _i, _pvp, _vp, _pu64, _pu64]),
    "tgx_utf8_lossy": (_u64, [_vp, _u64, _vp]),
    "tgx_substring_df": (_i, [_i, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _d, _u64, _pvp, _pvp, _pvp, _pu64, _pu64, _pu64]),
    "tgx_substring_df_top": (_i, [_i, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _d, _u64, _u64, _pvp, _pvp, _pvp, _pu64, _pu64, _pu64,
                                  _pu64, C.POINTER(C.c_uint32)]),
    "tgx_generate_u01": (_d, [_u64, _u64, _u64]),
    "tgx_free": (None, [_vp]),
    "tgx_pool_trim": (None, [_i]),
    "tgx_pool_filled_bytes": (_u64, []),
    "tgx_host_alloc": (_vp, [_u64]),
    "tgx_host_free": (None, [_vp]),
    "tgx_digamma": (_d, [_d]),
    "tgx_prune_m_step": (_i, [_vp, _vp, _u32, _vp, _vp, C.POINTER(C.c_uint32)]),
    "tgx_prune_alternatives": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _pvp]),
    "tgx_model_prune_alternatives": (_i, [_vp, _vp, _vp, _pvp]),
    "tgx_prune_select": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u32, _vp, C.POINTER(C.c_uint32)]),
    "tgx_last_kernel_times": (_i, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_last_algorithmic_bytes": (_u64, [_vp]),
    "tgx_last_encode_waves_per_cu": (_u32, [_vp]),
    "tgx_last_encode_redo_samples": (_u64, [_vp]),
    "tgx_model_score_values": (_u32, [_vp]),
    "tgx_last_encode_hot_values": (_u32, [_vp]),
    "tgx_last_encode_lean_items": (_u32, [_vp]),
    "tgx_last_encode_ids_in_place": (_i, [_vp]),
    "tgx_last_encode_top_table": (_i, [_vp]),
    "tgx_last_encode_long_samples": (_u64, [_vp]),
    "tgx_last_estep_pieces": (_u64, [_vp]),
    "tgx_last_estep_redo": (_u64, [_vp]),
    "tgx_last_encode_corun_cus": (_u32, [_vp]),
    "tgx_encode_corun_timeouts": (_u32, [_vp]),
    "tgx_sample_u01": (_d, [_u64, _u64, _u64, _u32]),
    "tgx_encode_batch_sample": (_i, [_vp, _vp, _vp, _u64, _d, _u64, _vp, _pvp]),
    "tgx_encode_corpus_sample": (_i, [_vp, _vp, _d, _u64, _vp, _pvp]),
    "tgx_lattice_stats_corpus": (_i, [_vp, _vp, _d, _vp, _vp, _vp, _pu64]),
    "tgx_lattice_stats_batch": (_i, [_vp, _vp, _vp, _u64, _d, _vp, _vp, _vp, _pu64]),
    "tgx_lattice_stats_host": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _d, _vp, _vp, _vp, _pu64]),
    "tgx_encode_batch_nbest": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _pvp]),
    "tgx_encode_corpus_nbest": (_i, [_vp, _vp, _u32, _vp, _vp, _pvp]),
    "tgx_result_device": (_i, [_vp]),
    "tgx_result_layout_info": (_i, [_vp, _u32, _u32, _pu64, _pu64]),
    "tgx_result_pad_device": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _pu64]),
    "tgx_result_pack_device": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _pu64]),
    "tgx_layout_pad_host": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _pu64]),
    "tgx_layout_pack_host": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _pu64]),
    "tgx_assemble_result": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _pvp]),
    "tgx_result_vocab_size": (_u32, [_vp]),
    "tgx_assemble_host": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _vp, _u64, _vp]),
    "tgx_decode_result": (_i, [_vp, _vp, _vp, _vp, _u32, _i, _vp, _pvp, _pu64, _pu64]),
    "tgx_decode_padded": (_i, [_vp, _vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _i, _vp, _pvp, _pu64, _pu64]),
    "tgx_text_num_rows": (_u64, [_vp]),
    "tgx_text_num_bytes": (_u64, [_vp]),
    "tgx_text_num_replaced": (_u64, [_vp]),
    "tgx_text_device": (_i, [_vp]),
    "tgx_text_copy_bytes": (_i, [_vp, _vp, _u64]),
    "tgx_text_copy_offsets": (_i, [_vp, _vp, _u64]),
    "tgx_text_bytes_device": (_vp, [_vp]),
    "tgx_text_offsets_device": (_vp, [_vp]),
    "tgx_text_free": (None, [_vp]),
    "tgx_corpus_from_text": (_i, [_vp, _pvp]),
    "tgx_decode_rows_host": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _u32, _i, _pvp, _vp, _pu64,
                                  _pu64, _pu64]),
    "tgx_result_spans_device": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    "tgx_result_pad_spans_device": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "tgx_spans_host": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _vp]),
    "tgx_result_window_info": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _pu64]),
    "tgx_result_window_pad_device": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "tgx_result_window_spans_device": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp]),
    "tgx_layout_windows_host": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _pu64]),
    "tgx_window_spans_host": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _u64, _vp, _pu64]),
    "tgx_corpus_split_specials": (_i, [_vp, _vp, _vp, _u32, _u32, _pvp, _pvp]),
    "tgx_plan_num_samples": (_u64, [_vp]),
    "tgx_plan_num_segments": (_u64, [_vp]),
    "tgx_plan_num_encoded": (_u64, [_vp]),
    "tgx_plan_device": (_i, [_vp]),
    "tgx_plan_copy": (_i, [_vp, _vp, _u64, _vp, _u64]),
    "tgx_plan_free": (None, [_vp]),
    "tgx_assemble_result_plan": (_i, [_vp, _vp, _vp, _u32, _pvp]),
    "tgx_front_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_corpus_copy_text": (_i, [_vp, _vp, _u64]),
    "tgx_corpus_copy_offsets": (_i, [_vp, _vp, _u64]),
    "tgx_front_host": (_i, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _pvp, _pu64, _pvp, _pvp, _pu64]),
    "tgx_corpus_normalize": (_i, [_vp, _u32, _pvp, _pu64]),
    "tgx_normalize_host": (_i, [_u32, _vp, _vp, _u64, _pvp, _pvp, _pu64]),
    "tgx_norm_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_fim_u01": (_d, [_u64, _u64, _u64]),
    "tgx_result_fim": (_i, [_vp, _u32, _u32, _u32, _d, _d, _u64, _u64, _vp, _vp, _vp, _pu64, _pvp]),
    "tgx_fim_host": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _d, _d, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _pu64]),
    "tgx_result_from_ids": (_i, [_i, _vp, _vp, _u64, _u32, _pvp]),
    "tgx_fim_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_select_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_result_select": (_i, [_vp, _vp, _u64, _u32, _vp, _pvp]),
    "tgx_result_lengths_device": (_i, [_vp, _vp, _vp]),
    "tgx_corpus_select": (_i, [_vp, _vp, _u64, _u32, _vp, _pvp]),
    "tgx_shuffle_key": (_u64, [_u64, _u64]),
    "tgx_shuffled_rows_device": (_i, [_i, _u64, _u64, _vp, _vp]),
    "tgx_shuffled_rows_host": (_i, [_u64, _u64, _vp]),
    "tgx_select_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "tgx_select_text_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "tgx_corpus_first_equal_device": (_i, [_vp, _u32, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tgx_result_first_equal_device": (_i, [_vp, _u32, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tgx_row_hash": (_u64, [_vp, _u64, _u64]),
    "tgx_corpus_row_hashes_device": (_i, [_vp, _u64, _vp, _vp]),
    "tgx_result_row_hashes_device": (_i, [_vp, _u64, _vp, _vp]),
    "tgx_first_equal_host": (_i, [_vp, _u32, _vp, _u64, _u32, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "tgx_dedup_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_dedup_last_rounds": (_u32, []),
    "tgx_result_minhash_device": (_i, [_vp, _u32, _u32, _u64, _u32, _vp, _vp]),
    "tgx_corpus_minhash_device": (_i, [_vp, _u32, _u32, _u64, _u32, _vp, _vp]),
    "tgx_minhash_value": (_u32, [_u64, _u32, _u64]),
    "tgx_minhash_bands_device": (_i, [_i, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp]),
    "tgx_minhash_near_first_device": (_i, [_i, _vp, _u64, _u32, _vp, _u32, _u32, _vp, _vp, C.POINTER(C.c_uint64)]),
    "tgx_minhash_host": (_i, [_vp, _u32, _vp, _u64, _u32, _u32, _u64, _vp]),
    "tgx_minhash_bands_host": (_i, [_vp, _u64, _u32, _u32, _u64, _vp, _vp]),
    "tgx_minhash_near_first_host": (_i, [_vp, _u64, _u32, _vp, _u32, _u32, _vp, C.POINTER(C.c_uint64)]),
    "tgx_minhash_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_gram_key": (_u64, [_vp, _u64, _u64]),
    "tgx_result_gramset_create": (_i, [_vp, _u32, _u64, _u32, _vp, _vp]),
    "tgx_corpus_gramset_create": (_i, [_vp, _u32, _u64, _u32, _vp, _vp]),
    "tgx_gramset_create_from_keys": (_i, [_i, _vp, _u64, _u32, _u32, _u64, _vp]),
    "tgx_gramset_size": (_u64, [_vp]),
    "tgx_gramset_info": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "tgx_gramset_keys": (_i, [_vp, _vp]),
    "tgx_gramset_free": (None, [_vp]),
    "tgx_result_gram_hits_device": (_i, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "tgx_corpus_gram_hits_device": (_i, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "tgx_gram_keys_host": (_i, [_vp, _u32, _vp, _u64, _u32, _u64, _vp, C.POINTER(C.c_uint64)]),
    "tgx_gram_hits_host": (_i, [_vp, _u32, _vp, _u64, _u32, _u64, _vp, _u64, _vp, _vp]),
    "tgx_gram_contains_host": (_i, [_vp, _u64, _vp, _u64, _vp]),
    "tgx_gram_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_corpus_text_stats_device": (_i, [_vp, _u64, _u32, _vp, _vp, _vp]),
    "tgx_corpus_lines": (_i, [_vp, _u32, _vp, _vp]),
    "tgx_text_stats_host": (_i, [_vp, _vp, _u64, _u64, _u32, _vp, _vp]),
    "tgx_lines_host": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(C.c_uint64)]),
    "tgx_textstat_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
    "tgx_result_repeat_stats_device": (_i, [_vp, _u32, _u64, _u32, _vp, _vp, _vp]),
    "tgx_corpus_repeat_stats_device": (_i, [_vp, _u32, _u64, _u32, _vp, _vp, _vp]),
    "tgx_repeat_stats_host": (_i, [_vp, _u32, _vp, _u64, _u32, _u64, _vp, _vp]),
    "tgx_repeat_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
}

# every exported symbol of include/tgx_words.h, which adds to the ABI in a header of its own: bound and checked at import
# as the table above is
WORD_SYMBOLS = {
    "tgx_corpus_word_stats_device": (_i, [_vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "tgx_word_stats_host": (_i, [_vp, _vp, _u64, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    "tgx_wordstat_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
}

# every exported symbol of include/tgx_phrases.h, a header of its own in the same way: bound and checked at import too
PHRASE_SYMBOLS = {
    "tgx_phraseset_create": (_i, [_i, _vp, _vp, _u32, _u32, _u32, _vp]),
    "tgx_phraseset_info": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "tgx_phraseset_free": (None, [_vp]),
    "tgx_corpus_phrase_hits_device": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "tgx_result_phrase_hits_device": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "tgx_phrase_hits_host": (_i, [_vp, _u32, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "tgx_phrase_last_times": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i]),
}


class TokenGeeXError(Exception):
    """tokengeex.TokenGeeXError — bindings/python/src/lib.rs:9,33-37; carries the
    reference's Display string (src/lib.rs:238-249)."""

    def __init__(self, message: str, status: int = -1, sample: int | None = None,
                 pos: int | None = None, length: int | None = None):
        super().__init__(message)
        self.status, self.sample, self.pos, self.length = status, sample, pos, length


def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process.  A PyTorch-ROCm wheel carries its own libamdhip64.so (soname libamdhip64.so.7, the
    name libtgx.so asks for) and libhsa-runtime64.so.  When torch is imported first, libtgx.so binds to that copy and the
    two share devices, streams and pointers (bench.py, dist.py).  Imported the other way round, libtgx.so would bring
    in the system's copy, torch its own beside it, and the runtime that initialises second finds no GPU — and
    tokengeex_amd.tensors hands torch's streams and data_ptr()s to libtgx.so, which only works inside one runtime.  So
    torch's copy, if there is one, is loaded here ahead of libtgx.so, WITHOUT importing torch (find_spec only looks the
    package up).  TGX_HIP_RUNTIME=system keeps the system's runtime (then import torch first, or do not use
    tokengeex_amd.tensors)."""
    import sys
    if os.environ.get("TGX_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for root in (spec.submodule_search_locations or []) if spec else []:
        path = os.path.join(root, "lib", "libamdhip64.so")
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass  # libtgx.so then loads the system's runtime, as without torch
            return


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is mandatory (no CPU fallback). "
            "Build it with `python tokengeex_amd/build.py`.")
    _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SYMBOLS.items()) + list(WORD_SYMBOLS.items()) + list(PHRASE_SYMBOLS.items()):
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.tgx_abi_version() != 1:
        raise ImportError("libtgx.so ABI version mismatch")
    return lib


lib = _load()


def check(status: int) -> None:
    if status == OK:
        return
    msg = (lib.tgx_last_error() or b"").decode("utf-8", "replace")
    if status in (ERR_NO_PATH, ERR_Z_NOT_NORMAL):
        s, p, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.tgx_last_error_detail(C.byref(s), C.byref(p), C.byref(l))
        raise TokenGeeXError(msg, status, s.value, p.value, l.value)
    raise TokenGeeXError(msg, status)


class _PinnedBlock:
    """Owner of one tgx_host_alloc block; numpy views keep it alive through their base chain."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.addr = lib.tgx_host_alloc(self.nbytes)
        if not self.addr:
            raise TokenGeeXError(lib.tgx_last_error().decode("utf-8", "replace"))
        self.buf = (C.c_ubyte * max(1, self.nbytes)).from_address(self.addr)

    def __del__(self):
        addr, self.addr = getattr(self, "addr", None), None
        if addr:
            lib.tgx_host_free(addr)


def pinned_empty(shape, dtype) -> np.ndarray:
    """numpy array over page-locked host memory (tgx_host_alloc): uploads from it and downloads into it are
    DMA transfers at the PCIe link's rate."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    blk = _PinnedBlock(n * dt.itemsize)
    arr = np.frombuffer(blk.buf, dtype=dt, count=n).reshape(shape)
    blk.buf._tgx_owner = blk  # the array's base is blk.buf: the block lives as long as any view of it
    return arr


def pool_trim(device: int = -1) -> None:
    """Returns the library's pooled device buffers to the HIP runtime (all devices if negative)."""
    lib.tgx_pool_trim(device)


def pool_filled_bytes() -> int:
    """Bytes of the library's own device buffers that TGX_POOL_FILL has filled in this process (0 without the knob)."""
    return int(lib.tgx_pool_filled_bytes())


def device_count() -> int:
    return lib.tgx_device_count()


def ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Packed:
    """A list of byte strings kept in the ABI's batch format (flat bytes + offsets), with subsets taken without a
    Python loop: what the prune driver carries its vocabulary in between passes (500 000 tokens: a list
    comprehension plus pack() per model cost as much as the native trie build)."""

    __slots__ = ("flat", "offs")

    def __init__(self, flat: np.ndarray, offs: np.ndarray):
        self.flat, self.offs = flat, offs

    @classmethod
    def of(cls, items) -> "Packed":
        return items if isinstance(items, Packed) else cls(*pack(items))

    def __len__(self) -> int:
        return int(self.offs.shape[0]) - 1

    def take(self, idx) -> "Packed":
        idx = np.asarray(idx, dtype=np.int64)
        beg, end = self.offs[:-1][idx].astype(np.int64), self.offs[1:][idx].astype(np.int64)
        lens = end - beg
        offs = np.zeros(idx.shape[0] + 1, np.uint64)
        np.cumsum(lens, out=offs[1:])
        total = int(offs[-1])
        # byte j of the output comes from beg[i] + (j - offs[i]) of the token i it belongs to
        src = np.repeat(beg - offs[:-1].astype(np.int64), lens) + np.arange(total, dtype=np.int64)
        return Packed(self.flat[src] if total else np.zeros(0, np.uint8), offs)

    def tolist(self) -> list[bytes]:
        raw, o = self.flat.tobytes(), self.offs.tolist()
        return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def pack(items) -> tuple[np.ndarray, np.ndarray]:
    """list[bytes] (or a Packed) -> (uint8 flat, uint64 offsets[len+1]) — the ABI's batch format."""
    if isinstance(items, Packed):
        return items.flat, items.offs
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    if len(items):
        np.cumsum(np.fromiter((len(t) for t in items), dtype=np.uint64, count=len(items)), out=offs[1:])
    flat = np.frombuffer(b"".join(items), dtype=np.uint8)
    return flat, offs


def _take(ptr_, n, ctype, dtype):
    """Copies a malloc'd array of n elements out of the library and frees it."""
    if not ptr_ or n == 0:
        if ptr_:
            lib.tgx_free(ptr_)
        return np.zeros(0, dtype)
    a = np.ctypeslib.as_array(C.cast(ptr_, C.POINTER(ctype)), shape=(n,)).copy()
    lib.tgx_free(ptr_)
    return a


def split_specials_flat(flat: np.ndarray, offs: np.ndarray, specials: list[bytes]):
    """SpecialTokenSplitter over a packed batch -> (seg_offs u64[S+1], seg_begin, seg_end u64[M], seg_special i32[M])."""
    sflat, soffs = pack(specials)
    n = offs.shape[0] - 1
    seg_offs = np.zeros(n + 1, np.uint64)
    sb, se, ss, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    check(lib.tgx_split_specials(ptr(flat) if flat.size else None, ptr(offs), n, ptr(sflat) if sflat.size else None, ptr(soffs),
                                 len(specials), ptr(seg_offs), C.byref(sb), C.byref(se), C.byref(ss), C.byref(m)))
    k = m.value
    return seg_offs, _take(sb, k, C.c_uint64, np.uint64), _take(se, k, C.c_uint64, np.uint64), _take(ss, k, C.c_int32, np.int32)


def pack_segments(flat: np.ndarray, seg_begin: np.ndarray, seg_end: np.ndarray, seg_special, crlf: bool):
    """The non-special segments back to back, CRLF-normalised on the way if asked -> (flat, offs)."""
    n = seg_begin.shape[0]
    total = int((seg_end.astype(np.int64) - seg_begin.astype(np.int64)).sum()) if n else 0
    out = np.empty(max(total, 1), np.uint8)
    out_offs = np.zeros(n + 1, np.uint64)
    m = C.c_uint64()
    check(lib.tgx_pack_segments(ptr(flat) if flat.size else None, ptr(seg_begin), ptr(seg_end),
                                None if seg_special is None else ptr(seg_special), n, 1 if crlf else 0, ptr(out), ptr(out_offs),
                                C.byref(m)))
    out_offs = out_offs[: m.value + 1]
    return out[: int(out_offs[-1])], out_offs


NORMAL_FORMS = {"nfd": 0, "nfc": 1, "nfkd": 2, "nfkc": 3}


def normalize_flat(form: str, flat: np.ndarray, offs: np.ndarray):
    """UnicodeProcessor::preprocess over a packed batch (src/processor.rs:124-137) -> (flat, offs), native (csrc/unicode_norm.cpp)."""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.shape[0] - 1
    beg, end = np.ascontiguousarray(offs[:-1]), np.ascontiguousarray(offs[1:])
    ot, oo = C.c_void_p(), C.c_void_p()
    check(lib.tgx_normalize_segments(NORMAL_FORMS[form], ptr(flat) if flat.size else None, ptr(beg) if n else None, ptr(end) if n else None, n,
                                     C.byref(ot), C.byref(oo)))
    out_offs = _take(oo, n + 1, C.c_uint64, np.uint64)
    return _take(ot, int(out_offs[-1]), C.c_uint8, np.uint8), out_offs


def unidata_version() -> str:
    return lib.tgx_unidata_version().decode()


def assemble_ids(seg_offs: np.ndarray, seg_special: np.ndarray, ids: np.ndarray, id_offs: np.ndarray, vocab_size: int):
    n = seg_offs.shape[0] - 1
    n_special = int((seg_special >= 0).sum()) if seg_special.size else 0
    out = np.empty(max(1, ids.shape[0] + n_special), np.uint32)
    out_offs = np.zeros(n + 1, np.uint64)
    check(lib.tgx_assemble_ids(ptr(seg_offs), ptr(seg_special) if seg_special.size else None, n, ptr(ids) if ids.size else None,
                               ptr(id_offs), vocab_size, ptr(out), ptr(out_offs)))
    return out[: int(out_offs[-1])], out_offs


def assemble_host(seg_offs: np.ndarray, seg_special: np.ndarray, ids: np.ndarray, id_offs: np.ndarray | None, vocab_size: int,
                  n_specials: int, ids_cap: int | None = None):
    """Host twin of NativeModel.assemble (tgx_assemble_host: the kernels' index arithmetic, no device) over the encode
    result of the non-special segments (ids u32[T], id_offs u64[E+1] or None when no segment is encoded) and the split
    plan -> (ids u32[T'], offsets u64[S+1]) with special k as vocab_size + k.  ids_cap: room at the destination (default:
    what is needed)."""
    seg_offs = np.ascontiguousarray(seg_offs, dtype=np.uint64)
    seg_special = np.ascontiguousarray(seg_special, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    id_offs = None if id_offs is None else np.ascontiguousarray(id_offs, dtype=np.uint64)
    n = seg_offs.shape[0] - 1
    n_enc = 0 if id_offs is None else id_offs.shape[0] - 1
    cap = ids.shape[0] + int((seg_special >= 0).sum()) if ids_cap is None else int(ids_cap)
    out = np.empty(max(1, cap), np.uint32)
    out_offs = np.zeros(n + 1, np.uint64)
    check(lib.tgx_assemble_host(ptr(ids) if ids.size else None, ptr(id_offs), n_enc, ptr(seg_offs), ptr(seg_special) if seg_special.size else None,
                                n, _u32_arg(vocab_size, "vocab_size"), _u32_arg(n_specials, "n_specials"), ptr(out), cap, ptr(out_offs)))
    return out[: int(out_offs[-1])], out_offs


def fim_u01(seed: int, row: int, draw: int) -> float:
    """The uniform of the fill-in-the-middle decisions (tgx_fim_u01), in [0, 1)."""
    m = 2**64 - 1
    return lib.tgx_fim_u01(seed & m, row & m, draw & m)


def fim_host(ids: np.ndarray, offs: np.ndarray, vocab_size: int, prefix_id: int, suffix_id: int, middle_id: int, *, rate: float = 1.0,
             spm_rate: float = 0.5, seed: int = 0, first_row: int = 0, ids_cap: int | None = None):
    """Host twin of NativeResult.fim (tgx_fim_host: the kernels' index arithmetic, no device) over ids u32[T] and offsets
    u64[S+1] -> (ids u32[T'], offsets u64[S+1], vocab_size, mode u8[S], cuts u64[S, 2], n_applied).  ids_cap: room at
    the destination (default: what can be needed, T + 3·S)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.shape[0] - 1
    cap = ids.shape[0] + 3 * max(n, 0) if ids_cap is None else int(ids_cap)
    out = np.empty(max(1, cap), np.uint32)
    out_offs = np.zeros(max(n, 0) + 1, np.uint64)
    mode = np.zeros(max(n, 0), np.uint8)
    cuts = np.zeros((max(n, 0), 2), np.uint64)
    na = C.c_uint64()
    pre, suf, mid = (_u32_arg(v, "sentinel id") for v in (prefix_id, suffix_id, middle_id))
    m = 2**64 - 1
    check(lib.tgx_fim_host(ptr(ids) if ids.size else None, ptr(offs) if offs.size else None, max(n, 0), _u32_arg(vocab_size, "vocab_size"), pre, suf,
                           mid, float(rate), float(spm_rate), int(seed) & m, int(first_row) & m, ptr(out), cap, ptr(out_offs),
                           ptr(mode) if n > 0 else None, ptr(cuts) if n > 0 else None, C.byref(na)))
    return out[: int(out_offs[-1])], out_offs, max(int(vocab_size), 1 + max(pre, suf, mid)), mode, cuts, na.value


def fim_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last NativeResult.fim (tgx_fim_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_fim_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


def _is_device_tensor(rows) -> bool:
    """A CUDA torch tensor, recognised without importing torch."""
    return bool(getattr(rows, "is_cuda", False)) and hasattr(rows, "data_ptr")


def _host_rows(rows, n_src: int) -> np.ndarray:
    """Indices given as a list, any numpy integer array, or a boolean mask of length n_src (numpy, or a torch tensor on
    the host) -> contiguous int64 indices."""
    if hasattr(rows, "detach") and hasattr(rows, "numpy"):   # a torch tensor on the host
        rows = rows.detach().numpy()
    a = np.asarray(rows)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != n_src:
            raise ValueError(f"a boolean mask must have one entry per row ({n_src}), got shape {a.shape}")
        return np.flatnonzero(a).astype(np.int64)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"rows must be a one-dimensional array of integers or a boolean mask (got {a.dtype}, {a.ndim} dimensions)")
    if a.dtype == np.uint64 and a.size and int(a.max()) > 2**63 - 1:
        raise ValueError("an index does not fit int64")
    return np.ascontiguousarray(a, dtype=np.int64)


def _select_args(rows, n_src: int, device: int, stream: int):
    """-> (pointer or None, M, flags, stream, what keeps the pointer alive) for tgx_result_select / tgx_corpus_select"""
    if _is_device_tensor(rows):
        index = getattr(rows.device, "index", None)
        if index is not None and index != device:
            raise ValueError(f"rows is on {rows.device}, the source on device {device}")
        if "bool" in str(rows.dtype):
            if rows.dim() != 1 or rows.shape[0] != n_src:
                raise ValueError(f"a boolean mask must have one entry per row ({n_src}), got shape {tuple(rows.shape)}")
            rows = rows.nonzero().reshape(-1)
        if rows.dim() != 1:
            raise TypeError("rows must be one-dimensional")
        if "int64" not in str(rows.dtype):
            if "int" not in str(rows.dtype):
                raise TypeError(f"rows must hold integers or be a boolean mask (got {rows.dtype})")
            rows = rows.long()
        rows = rows.contiguous()
        if not stream:
            import sys
            stream = sys.modules["torch"].cuda.current_stream(rows.device).cuda_stream   # (the tensor's module is loaded)
        m = int(rows.shape[0])
        return (rows.data_ptr() or None) if m else None, m, SELECT_ROWS_DEVICE, stream, rows
    a = _host_rows(rows, n_src)
    return ptr(a) if a.size else None, int(a.size), 0, stream, a


def select_host(ids: np.ndarray, offs: np.ndarray, rows, cap: int | None = None):
    """Host twin of NativeResult.select (tgx_select_host: the kernel's index arithmetic, no device) over ids u32[T] and
    offsets u64[S+1] -> (ids u32[T'], offsets u64[M+1]).  cap: room at the destination (default: what is needed)."""
    return _select_twin(lib.tgx_select_host, np.uint32, ids, offs, rows, cap)


def select_text_host(flat: np.ndarray, offs: np.ndarray, rows, cap: int | None = None):
    """Host twin of NativeCorpus.select (tgx_select_text_host) over text bytes u8[N] and offsets u64[S+1] -> (bytes,
    offsets u64[M+1])."""
    return _select_twin(lib.tgx_select_text_host, np.uint8, flat, offs, rows, cap)


def _select_twin(fn, dtype, data, offs, rows, cap):
    data = np.ascontiguousarray(data, dtype=dtype)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    rows = _host_rows(rows, n)
    if cap is None:   # what is needed, for indices in range (the twin refuses the others before it writes)
        ok = rows[(rows >= 0) & (rows < n)]
        cap = int((offs[1:][ok].astype(np.int64) - offs[:-1][ok].astype(np.int64)).sum()) if ok.size else 0
    out = np.empty(max(1, int(cap)), dtype)
    out_offs = np.zeros(rows.size + 1, np.uint64)
    check(fn(ptr(data) if data.size else None, ptr(offs) if offs.size else None, n, ptr(rows) if rows.size else None, rows.size, ptr(out), int(cap),
             ptr(out_offs)))
    return out[: int(out_offs[-1])], out_offs


def shuffle_key(seed: int, g: int) -> int:
    """The key of row g under `seed` in the seeded permutation (tgx_shuffle_key), a 64-bit integer."""
    m = 2**64 - 1
    return lib.tgx_shuffle_key(int(seed) & m, int(g) & m)


def shuffled_rows_host(n: int, seed: int) -> np.ndarray:
    """The seeded permutation of 0 .. n-1 as int64[n] (tgx_shuffled_rows_host): the rows sorted by (shuffle_key, index)."""
    rows = np.empty(int(n), np.int64)
    check(lib.tgx_shuffled_rows_host(int(n), int(seed) & (2**64 - 1), ptr(rows) if n else None))
    return rows


def shuffled_rows_device(device: int, n: int, seed: int, rows_ptr: int, stream: int = 0) -> None:
    """The same permutation written by the device into caller-owned device memory (int64[n], a raw integer pointer;
    tgx_shuffled_rows_device), queued on `stream` as in NativeResult.pad_device."""
    check(lib.tgx_shuffled_rows_device(int(device), int(n), int(seed) & (2**64 - 1), stream or None, rows_ptr or None))


def select_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last NativeResult.select or NativeCorpus.select
    (tgx_select_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_select_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


def first_equal_host(data: np.ndarray, offs: np.ndarray, hash_bits: int = 64):
    """Host twin of NativeCorpus.first_equal / NativeResult.first_equal (tgx_first_equal_host: the device's rounds through
    the same header, no device) over data u8[N] or u32[T] and offsets u64[S+1] in elements -> (first int64[S], n_unique,
    n_rounds).  hash_bits: bits of the row hash that make the sort key (0: every row collides)."""
    data = np.ascontiguousarray(data)
    if data.dtype not in (np.uint8, np.uint32):
        raise TypeError(f"data must be uint8 or uint32 (got {data.dtype})")
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    first = np.empty(n, np.int64)
    nu, nr = C.c_uint64(), C.c_uint32()
    check(lib.tgx_first_equal_host(ptr(data) if data.size else None, data.dtype.itemsize, ptr(offs) if offs.size else None, n, int(hash_bits),
                                   ptr(first) if n else None, C.byref(nu), C.byref(nr)))
    return first, int(nu.value), int(nr.value)


def row_hash(data: bytes, seed: int = 0) -> int:
    """tgx_row_hash of a row's bytes under `seed`, a 64-bit integer (a row of ids: its little-endian u32 bytes)."""
    data = bytes(data)
    return lib.tgx_row_hash(data if data else None, len(data), int(seed) & (2**64 - 1))


def dedup_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last first_equal, summed over its rounds
    (tgx_dedup_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_dedup_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


def dedup_last_rounds() -> int:
    """Rounds of the calling thread's last first_equal (tgx_dedup_last_rounds)."""
    return int(lib.tgx_dedup_last_rounds())


def minhash_host(data: np.ndarray, offs: np.ndarray, width: int = 5, n_perm: int = 128, seed: int = 0) -> np.ndarray:
    """Host twin of NativeCorpus.minhash / NativeResult.minhash (tgx_minhash_host: the kernel's tiles, chunks and flush
    rule through the same header, no device) over data u8[N] or u32[T] and offsets u64[S+1] in elements -> sig u32[S, K]."""
    data = np.ascontiguousarray(data)
    if data.dtype not in (np.uint8, np.uint32):
        raise TypeError(f"data must be uint8 or uint32 (got {data.dtype})")
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    sig = np.empty((n, max(int(n_perm), 0)), np.uint32)
    check(lib.tgx_minhash_host(ptr(data) if data.size else None, data.dtype.itemsize, ptr(offs) if offs.size else None, n, int(width), int(n_perm),
                               int(seed) & (2**64 - 1), ptr(sig) if sig.size else None))
    return sig


def minhash_bands_host(sig: np.ndarray, bands: int, seed: int = 0):
    """Host twin of minhash_bands (tgx_minhash_bands_host) over sig u32[S, K] -> (keys u64[S, B], heads int64[S, B])."""
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    S, K = sig.shape
    keys = np.empty((S, max(int(bands), 0)), np.uint64)
    heads = np.empty((S, max(int(bands), 0)), np.int64)
    # (never NULL: both outputs are asked for, also when there is no row)
    keep = np.zeros(1, np.uint64), np.zeros(1, np.int64)
    check(lib.tgx_minhash_bands_host(ptr(sig) if sig.size else None, S, K, int(bands), int(seed) & (2**64 - 1), ptr(keys if keys.size else keep[0]),
                                     ptr(heads if heads.size else keep[1])))
    return keys, heads


def minhash_near_first_host(sig: np.ndarray, heads: np.ndarray, min_agree: int):
    """Host twin of the clustering (tgx_minhash_near_first_host) over sig u32[S, K] and heads int64[S, B] -> (first
    int64[S], n_clusters)."""
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    heads = np.ascontiguousarray(heads, dtype=np.int64)
    S, K = sig.shape
    first = np.empty(S, np.int64)
    nc = C.c_uint64()
    check(lib.tgx_minhash_near_first_host(ptr(sig) if sig.size else None, S, K, ptr(heads) if heads.size else None, heads.shape[1], int(min_agree),
                                          ptr(first) if S else None, C.byref(nc)))
    return first, int(nc.value)


def minhash_value(h: int, k: int, seed: int = 0) -> int:
    """v_k(h) of the MinHash permutations under `seed` (tgx_minhash_value): with it a signature is extended elsewhere."""
    return int(lib.tgx_minhash_value(int(h) & (2**64 - 1), int(k), int(seed) & (2**64 - 1)))


def minhash_bands(device: int, d_sig: int, n_rows: int, n_perm: int, bands: int, seed: int = 0, d_keys: int = 0, d_heads: int = 0, *,
                  stream: int = 0) -> None:
    """Band keys u64[S, B] and bucket heads int64[S, B] of signatures u32[S, K], all raw integer pointers to device memory
    on `device` (tgx_minhash_bands_device); either output may be 0."""
    check(lib.tgx_minhash_bands_device(int(device), d_sig or None, int(n_rows), int(n_perm), int(bands), int(seed) & (2**64 - 1), stream or None,
                                       d_keys or None, d_heads or None))


def minhash_near_first(device: int, d_sig: int, n_rows: int, n_perm: int, d_heads: int, bands: int, min_agree: int, d_first: int, *,
                       stream: int = 0) -> int:
    """first int64[S] of the near-duplicate clusters into device memory (tgx_minhash_near_first_device) -> n_clusters."""
    nc = C.c_uint64()
    check(lib.tgx_minhash_near_first_device(int(device), d_sig or None, int(n_rows), int(n_perm), d_heads or None, int(bands), int(min_agree),
                                            stream or None, d_first or None, C.byref(nc)))
    return int(nc.value)


def minhash_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last MinHash calls (tgx_minhash_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_minhash_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


def _gram_source(data: np.ndarray, offs: np.ndarray):
    data = np.ascontiguousarray(data)
    if data.dtype not in (np.uint8, np.uint32):
        raise TypeError(f"data must be uint8 or uint32 (got {data.dtype})")
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    return data, offs, max(offs.shape[0] - 1, 0)


def gram_key(data: bytes, seed: int = 0) -> int:
    """The key of a gram from its bytes under `seed` (tgx_gram_key; a gram of ids: their little-endian u32 bytes)."""
    data = bytes(data)
    return int(lib.tgx_gram_key(data if data else None, len(data), int(seed) & (2**64 - 1)))


def gram_keys_host(data: np.ndarray, offs: np.ndarray, width: int, seed: int = 0) -> np.ndarray:
    """Host twin of a gram set's creation (tgx_gram_keys_host: the kernel's walk through the same header, no device) over
    data u8[N] or u32[T] and offsets u64[S+1] in elements -> the ascending distinct keys u64[n_keys]."""
    data, offs, n = _gram_source(data, offs)
    keys = np.empty(max(data.size, 1), np.uint64)
    nk = C.c_uint64()
    check(lib.tgx_gram_keys_host(ptr(data) if data.size else None, data.dtype.itemsize, ptr(offs) if offs.size else None, n, int(width),
                                 int(seed) & (2**64 - 1), ptr(keys), C.byref(nk)))
    return keys[:int(nk.value)].copy()


def gram_hits_host(data: np.ndarray, offs: np.ndarray, width: int, seed: int, keys: np.ndarray):
    """Host twin of gram_hits (tgx_gram_hits_host: the directory, the kernel's chunks and its store / add rule, no device)
    against keys u64[n] in any order -> (count int64[S], mask uint8[n_elems])."""
    data, offs, n = _gram_source(data, offs)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    count = np.full(n, -7, np.int64)
    mask = np.full(data.size, 7, np.uint8)
    keep = np.zeros(1, np.int64), np.zeros(1, np.uint8)   # (never NULL: both outputs are asked for)
    check(lib.tgx_gram_hits_host(ptr(data) if data.size else None, data.dtype.itemsize, ptr(offs) if offs.size else None, n, int(width),
                                 int(seed) & (2**64 - 1), ptr(keys) if keys.size else None, keys.size, ptr(count if n else keep[0]),
                                 ptr(mask if mask.size else keep[1])))
    return count, mask


def gram_contains_host(keys: np.ndarray, probes: np.ndarray) -> np.ndarray:
    """Membership of every probe key in the set of `keys` (any order, duplicates allowed) through the directory and
    bucket search that the kernel uses (tgx_gram_contains_host) -> bool[n_probes]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    out = np.full(probes.size, 7, np.uint8)
    check(lib.tgx_gram_contains_host(ptr(keys) if keys.size else None, keys.size, ptr(probes) if probes.size else None, probes.size,
                                     ptr(out) if out.size else None))
    return out.astype(bool)


def gram_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last gram-set and gram-hits calls (tgx_gram_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_gram_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


# ---- per-row text statistics and the line view (include/tgx.h; csrc/textstat.hip, csrc/textstat.h) ----
TEXTSTAT_N = 11
TEXTSTAT_CHARS = 1
TEXTSTAT_NAMES = ("bytes", "chars", "newlines", "lines", "max_line", "long_lines", "alpha", "digit", "space", "non_ascii", "control")


def textstat_flags(unit: str) -> int:
    """unit "char" or "byte" -> the flags of tgx_corpus_text_stats_device."""
    if unit not in ("char", "byte"):
        raise ValueError(f"unit must be 'char' or 'byte' (got {unit!r})")
    return TEXTSTAT_CHARS if unit == "char" else 0


def text_stats_host(text: np.ndarray, offs: np.ndarray, line_limit: int = 1000, unit: str = "char"):
    """Host twin of NativeCorpus.text_stats (tgx_text_stats_host: the kernel's chunks, summaries, carry and store / add
    rule through the same header, no device) over text u8[N] and offsets u64[S+1] -> (stats int64[11, S], line_start
    uint8[N])."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    stats = np.full((TEXTSTAT_N, n), -7, np.int64)
    marks = np.full(text.size, 7, np.uint8)
    keep = np.zeros(1, np.int64), np.zeros(1, np.uint8)   # (never NULL: both outputs are asked for)
    check(lib.tgx_text_stats_host(ptr(text) if text.size else None, ptr(offs) if offs.size else None, n, int(line_limit), textstat_flags(unit),
                                  ptr(stats if n else keep[0]), ptr(marks if marks.size else keep[1])))
    return stats, marks


def lines_host(text: np.ndarray, offs: np.ndarray) -> np.ndarray:
    """Host twin of NativeCorpus.lines (tgx_lines_host) -> the offsets u64[n_lines + 1] of the line view."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    out = np.full(text.size + 1, 7, np.uint64)
    nl = C.c_uint64()
    check(lib.tgx_lines_host(ptr(text) if text.size else None, ptr(offs) if offs.size else None, n, ptr(out), out.size, C.byref(nl)))
    return out[:int(nl.value) + 1].copy()


def textstat_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last text_stats or lines call (tgx_textstat_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_textstat_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


# ---- per-row word statistics (include/tgx_words.h; csrc/wordstat.hip, csrc/wordstat.h) ----
WORDSTAT_N = 14
WORDSTAT_CHARS, WORDSTAT_FOLD = 1, 2
WORDSTAT_NAMES = ("words", "word_units", "max_word", "long_words", "alpha_words", "alpha_wide_words", "hash", "ellipsis", "lines", "bullet_lines",
                  "ellipsis_lines", "punct_lines", "stop_words", "stop_mask")
WORD_MARK_START, WORD_MARK_END, WORD_MARK_STOP, WORD_MARK_BULLET = 1, 2, 4, 8
GOPHER_STOP_WORDS = (b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with")


def wordstat_flags(unit: str, fold_case: bool) -> int:
    """unit "char" or "byte", and whether the text's A-Z are lowered for the stop words -> the flags of
    tgx_corpus_word_stats_device."""
    return (WORDSTAT_CHARS if textstat_flags(unit) else 0) | (WORDSTAT_FOLD if fold_case else 0)


def _stop_table(stop_words):
    """words as bytes or str (UTF-8) -> (flat u8, offs u64, n) of the ABI; the library checks them"""
    words = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in (stop_words or ())]
    flat, offs = pack(words)
    return flat, offs, len(words)


def word_stats_host(text: np.ndarray, offs: np.ndarray, word_limit: int = 20, stop_words=GOPHER_STOP_WORDS, unit: str = "char",
                    fold_case: bool = True):
    """Host twin of NativeCorpus.word_stats (tgx_word_stats_host: the kernel's chunks, masks, summaries, carry and store /
    add rule through the same header, no device) over text u8[N] and offsets u64[S+1] -> (stats int64[14, S], marks
    uint8[N])."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(offs.shape[0] - 1, 0)
    sflat, soffs, n_stop = _stop_table(stop_words)
    stats = np.full((WORDSTAT_N, n), -7, np.int64)
    marks = np.full(text.size, 7, np.uint8)
    keep = np.zeros(1, np.int64), np.zeros(1, np.uint8)   # (never NULL: both outputs are asked for)
    check(lib.tgx_word_stats_host(ptr(text) if text.size else None, ptr(offs) if offs.size else None, n, int(word_limit),
                                  ptr(sflat) if sflat.size else None, ptr(soffs), n_stop, wordstat_flags(unit, fold_case),
                                  ptr(stats if n else keep[0]), ptr(marks if marks.size else keep[1])))
    return stats, marks


def wordstat_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last word_stats call (tgx_wordstat_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_wordstat_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


# ---- repeated n-grams within a row (include/tgx.h; csrc/repeat.hip, csrc/repeat.h) ----
REPEAT_N = 6
REPEAT_MASK_REPEAT = 1
REPEAT_MASK_MULTI = 2
REPEAT_NAMES = ("grams", "repeated", "multi", "top", "covered", "covered_all")
GRAM_MAX_BYTES = 64


def repeat_check_width(width: int, elem_bytes: int) -> int:
    """width must be in 1 .. 64 / elem_bytes, as the device calls check it -> int(width)."""
    width = int(width)
    if width < 1 or width * elem_bytes > GRAM_MAX_BYTES:
        raise ValueError(f"width {width} of {elem_bytes}-byte elements is not in 1 .. {GRAM_MAX_BYTES // elem_bytes}")
    return width


def repeat_stats_host(data: np.ndarray, offs: np.ndarray, width: int, seed: int = 0):
    """Host twin of repeat_stats (tgx_repeat_stats_host: the row keys, a stable sort, the run rule and the kernel's chunks,
    coverage window and store / add rule through the same header, no device) over data u8[N] or u32[T] and offsets
    u64[S+1] in elements -> (stats int64[6, S], mask uint8[n_elems])."""
    data, offs, n = _gram_source(data, offs)
    stats = np.full((REPEAT_N, n), -7, np.int64)
    mask = np.full(data.size, 7, np.uint8)
    keep = np.zeros(1, np.int64), np.zeros(1, np.uint8)   # (never NULL: both outputs are asked for)
    check(lib.tgx_repeat_stats_host(ptr(data) if data.size else None, data.dtype.itemsize, ptr(offs) if offs.size else None, n, int(width),
                                    int(seed) & (2**64 - 1), ptr(stats if n else keep[0]), ptr(mask if mask.size else keep[1])))
    return stats, mask


def repeat_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last repeat_stats call (tgx_repeat_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_repeat_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


class NativeGramSet:
    """Owns a tgx_gramset: the distinct keys of a source's n-grams in HBM with their bucket directory (csrc/gram.hip).
    Read-only after creation.  Made by NativeResult.gram_set, NativeCorpus.gram_set or from_keys."""

    KINDS = {1: "bytes", 4: "ids"}

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_gramset_free(self._h)
            self._h = None

    @classmethod
    def from_keys(cls, keys, width: int, kind: str, seed: int = 0, device: int = 0) -> "NativeGramSet":
        """A set on `device` from host keys u64[n] in any order, duplicates allowed (tgx_gramset_create_from_keys): the
        union of several sets' keys(), or keys made elsewhere with gram_key.  kind: "bytes" or "ids", with width and seed
        what a probe hashes its grams with."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        eb = {v: k for k, v in cls.KINDS.items()}[kind]
        h = C.c_void_p()
        check(lib.tgx_gramset_create_from_keys(int(device), ptr(keys) if keys.size else None, keys.size, int(width), eb, int(seed) & (2**64 - 1),
                                               C.byref(h)))
        return cls(h)

    def _info(self):
        w, eb, seed, dev, bits = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_int(), C.c_uint32()
        check(lib.tgx_gramset_info(self._h, C.byref(w), C.byref(eb), C.byref(seed), C.byref(dev), C.byref(bits)))
        return w.value, eb.value, seed.value, dev.value, bits.value

    @property
    def size(self) -> int:
        return int(lib.tgx_gramset_size(self._h))

    @property
    def width(self) -> int:
        return self._info()[0]

    @property
    def kind(self) -> str:
        return self.KINDS[self._info()[1]]

    @property
    def seed(self) -> int:
        return self._info()[2]

    @property
    def device(self) -> int:
        return self._info()[3]

    @property
    def dir_bits(self) -> int:
        return self._info()[4]

    def keys(self) -> np.ndarray:
        """The set's keys, ascending, copied to the host (tgx_gramset_keys)."""
        out = np.empty(self.size, np.uint64)
        check(lib.tgx_gramset_keys(self._h, ptr(out) if out.size else None))
        return out


# ---- literal phrase matching (include/tgx_phrases.h; csrc/phrase.hip, csrc/phrase.h) ----
PHRASE_FOLD_CASE, PHRASE_WHOLE_WORD = 1, 2
PHRASE_MAX_LEN, PHRASE_MAX_BYTES = 255, 256
PHRASE_KINDS = {1: "bytes", 4: "ids"}


def phrase_flags(fold_case: bool, whole_word: bool) -> int:
    """-> the flags of tgx_phraseset_create."""
    return (PHRASE_FOLD_CASE if fold_case else 0) | (PHRASE_WHOLE_WORD if whole_word else 0)


def _phrase_table(phrases, kind: str):
    """phrases as list[bytes | str] (a str as UTF-8) for kind "bytes", list[list[int]] for kind "ids" -> (flat u8 or u32,
    offs u64 in elements, n, elem_bytes) of the ABI; the library checks the lengths"""
    if kind not in ("bytes", "ids"):
        raise ValueError(f"kind must be 'bytes' or 'ids' (got {kind!r})")
    if kind == "bytes":
        items = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in phrases]
        flat, offs = pack(items)
        return np.ascontiguousarray(flat), offs, len(items), 1
    items = [np.asarray(w, dtype=np.int64).reshape(-1) for w in phrases]
    for w in items:
        if w.size and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF):
            raise ValueError("an id of a phrase is not in 0 .. 2^32-1")
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        np.cumsum(np.fromiter((w.size for w in items), dtype=np.uint64, count=len(items)), out=offs[1:])
    flat = np.concatenate(items).astype(np.uint32) if items else np.zeros(0, np.uint32)
    return np.ascontiguousarray(flat), offs, len(items), 4


def phrase_hits_host(data: np.ndarray, offs: np.ndarray, phrases, fold_case: bool = False, whole_word: bool = False):
    """Host twin of phrase_hits (tgx_phrase_hits_host: the same table, the kernel's chunks, filter, walk and store / add
    rule through the same header, no device) over data u8[N] or u32[T] and offsets u64[S+1] in elements ->
    (count int64[S], longest uint8[n_elems], per_phrase int64[P])."""
    data, offs, n = _gram_source(data, offs)
    pflat, poffs, n_phr, eb = _phrase_table(phrases, PHRASE_KINDS[data.dtype.itemsize])
    count = np.full(n, -7, np.int64)
    longest = np.full(data.size, 7, np.uint8)
    per = np.full(n_phr, -7, np.int64)
    keep = np.zeros(1, np.int64), np.zeros(1, np.uint8), np.zeros(1, np.int64)   # (never NULL: all outputs are asked for)
    check(lib.tgx_phrase_hits_host(ptr(data) if data.size else None, eb, ptr(offs) if offs.size else None, n, ptr(pflat) if pflat.size else None,
                                   ptr(poffs), n_phr, phrase_flags(fold_case, whole_word), ptr(count if n else keep[0]),
                                   ptr(longest if longest.size else keep[1]), ptr(per if n_phr else keep[2])))
    return count, longest, per


def phrase_last_times() -> dict[str, float]:
    """Device time in ms of each stage of the calling thread's last phrase_hits call (tgx_phrase_last_times)."""
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    n = lib.tgx_phrase_last_times(names, ms, 8)
    return {names[i].decode(): float(ms[i]) for i in range(n)}


class NativePhraseSet:
    """Owns a tgx_phraseset: the trie of a list of literal phrases in HBM with its first-level filter (csrc/phrase.hip).
    Read-only after creation: calls and threads share it."""

    def __init__(self, phrases, kind: str = "bytes", fold_case: bool = False, whole_word: bool = False, device: int = 0):
        pflat, poffs, n_phr, eb = _phrase_table(phrases, kind)
        h = C.c_void_p()
        check(lib.tgx_phraseset_create(int(device), ptr(pflat) if pflat.size else None, ptr(poffs), n_phr, eb, phrase_flags(fold_case, whole_word),
                                       C.byref(h)))
        self._h = h

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_phraseset_free(self._h)
            self._h = None

    def info(self) -> dict:
        """The fields of tgx_phraseset_info."""
        n, d, eb, fl, ml, dev, tb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int(), C.c_uint64()
        check(lib.tgx_phraseset_info(self._h, C.byref(n), C.byref(d), C.byref(eb), C.byref(fl), C.byref(ml), C.byref(dev), C.byref(tb)))
        return {"size": n.value, "distinct": d.value, "elem_bytes": eb.value, "flags": fl.value, "max_len": ml.value, "device": dev.value,
                "table_bytes": tb.value}

    size = property(lambda self: self.info()["size"])
    distinct = property(lambda self: self.info()["distinct"])
    kind = property(lambda self: PHRASE_KINDS[self.info()["elem_bytes"]])
    fold_case = property(lambda self: bool(self.info()["flags"] & PHRASE_FOLD_CASE))
    whole_word = property(lambda self: bool(self.info()["flags"] & PHRASE_WHOLE_WORD))
    max_len = property(lambda self: self.info()["max_len"])
    device = property(lambda self: self.info()["device"])
    table_bytes = property(lambda self: self.info()["table_bytes"])


def front_host(flat: np.ndarray, offs: np.ndarray, specials: list[bytes], crlf: bool):
    """Host twin of NativeCorpus.split_specials (tgx_front_host: the kernels' index arithmetic, no device) over a packed
    batch (offs from 0) -> (seg_offs u64[S+1], seg_special i32[K], segments' flat, segments' offsets u64[E+1]): the plan of
    split_specials_flat and what pack_segments packs."""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    sflat, soffs = pack(specials)
    n = offs.shape[0] - 1
    seg_offs = np.zeros(n + 1, np.uint64)
    ss, ot, oo, k, e = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    check(lib.tgx_front_host(ptr(flat) if flat.size else None, ptr(offs), n, ptr(sflat) if sflat.size else None, ptr(soffs), len(specials),
                             FRONT_CRLF if crlf else 0, ptr(seg_offs), C.byref(ss), C.byref(k), C.byref(ot), C.byref(oo), C.byref(e)))
    out_offs = _take(oo, e.value + 1, C.c_uint64, np.uint64)
    return seg_offs, _take(ss, k.value, C.c_int32, np.int32), _take(ot, int(out_offs[-1]), C.c_uint8, np.uint8), out_offs


def front_last_times() -> dict[str, float]:
    """Device milliseconds per stage of this thread's last NativeCorpus.split_specials (tgx_front_last_times)."""
    names, ms = (C.c_char_p * 8)(), (C.c_float * 8)()
    n = lib.tgx_front_last_times(names, ms, 8)
    return {names[k].decode(): float(ms[k]) for k in range(n)}


def _check_norm(status: int) -> None:
    """check(), with the row of a window overflow (ERR_UNSUPPORTED: tgx_last_error_detail's sample) on the exception."""
    if status == ERR_UNSUPPORTED:
        msg = (lib.tgx_last_error() or b"").decode("utf-8", "replace")
        s, p, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.tgx_last_error_detail(C.byref(s), C.byref(p), C.byref(l))
        raise TokenGeeXError(msg, status, s.value)
    check(status)


def normalize_host_twin(form: str, flat: np.ndarray, offs: np.ndarray):
    """Host twin of NativeCorpus.normalize (tgx_normalize_host: the kernels' decoder, stream machine and index arithmetic,
    no device) over a packed batch (offs from 0) -> (flat, offsets u64[S+1], the number of pieces): normalize_flat's
    bytes.  A row whose stream window overflows raises ERR_UNSUPPORTED with the lowest such row as .sample."""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.shape[0] - 1
    ot, oo, k = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _check_norm(lib.tgx_normalize_host(NORMAL_FORMS[form], ptr(flat) if flat.size else None, ptr(offs), n, C.byref(ot), C.byref(oo), C.byref(k)))
    out_offs = _take(oo, n + 1, C.c_uint64, np.uint64)
    return _take(ot, int(out_offs[-1]), C.c_uint8, np.uint8), out_offs, k.value


def norm_last_times() -> dict[str, float]:
    """Device milliseconds per stage of this thread's last NativeCorpus.normalize (tgx_norm_last_times)."""
    names, ms = (C.c_char_p * 8)(), (C.c_float * 8)()
    n = lib.tgx_norm_last_times(names, ms, 8)
    return {names[k].decode(): float(ms[k]) for k in range(n)}


def decode_batch_flat(vocab_flat, vocab_offs, vocab_size: int, special_flat, special_offs, n_specials: int,
                      ids: np.ndarray, id_offs: np.ndarray, include_special: bool):
    """decode_batch over packed ids -> (utf-8 bytes, offsets u64[S+1])."""
    n = id_offs.shape[0] - 1
    out_offs = np.zeros(n + 1, np.uint64)
    txt, bs, bi = C.c_void_p(), C.c_uint64(), C.c_uint64()
    st = lib.tgx_decode_batch(ptr(vocab_flat) if vocab_flat.size else None, ptr(vocab_offs), vocab_size,
                              ptr(special_flat) if special_flat.size else None, ptr(special_offs), n_specials,
                              ptr(ids) if ids.size else None, ptr(id_offs), n, 1 if include_special else 0, C.byref(txt),
                              ptr(out_offs), C.byref(bs), C.byref(bi))
    if st != OK:
        msg = (lib.tgx_last_error() or b"").decode("utf-8", "replace")
        raise TokenGeeXError(msg, st, bs.value, bi.value, None)
    return _take(txt, int(out_offs[-1]), C.c_uint8, np.uint8), out_offs


def _raise_decode(st: int, bad_sample: int, bad_id: int):
    msg = (lib.tgx_last_error() or b"").decode("utf-8", "replace")
    if st == ERR_TOKEN_ID_OOB:
        raise TokenGeeXError(msg, st, bad_sample, bad_id, None)
    raise TokenGeeXError(msg, st)


_DECODE_KINDS = {np.dtype(np.uint32): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2}  # id_kind of tgx_decode_rows_host


def decode_rows_host(vocab_flat, vocab_offs, vocab_size: int, special_flat, special_offs, n_specials: int, ids: np.ndarray,
                     id_offs: np.ndarray | None = None, *, mask: np.ndarray | None = None, lengths: np.ndarray | None = None,
                     skip_id: int | None = None, include_special: bool = True):
    """Host twin of NativeModel.decode_result / decode_padded (tgx_decode_rows_host: the kernels' index arithmetic, no
    device).  Offsets form: ids u32[N] with id_offs u64[S+1].  Padded form (id_offs None): ids [S, L] int32 or int64 with
    mask u8/bool [S, L], lengths i32[S] and skip_id, each optional -> (utf-8 bytes, offsets u64[S+1], n_replaced)."""
    vocab_flat = np.ascontiguousarray(vocab_flat, dtype=np.uint8)
    vocab_offs = np.ascontiguousarray(vocab_offs, dtype=np.uint64)
    special_flat = np.ascontiguousarray(special_flat, dtype=np.uint8)
    special_offs = np.ascontiguousarray(special_offs, dtype=np.uint64)
    if id_offs is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        id_offs = np.ascontiguousarray(id_offs, dtype=np.uint64)
        n, L = id_offs.shape[0] - 1, 0
    else:
        ids = np.ascontiguousarray(ids)
        if ids.ndim != 2 or ids.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise ValueError("the padded form takes a 2-d int32 or int64 array")
        n, L = ids.shape
        if mask is not None:
            mask = np.ascontiguousarray(mask).astype(np.uint8, copy=False)
            if mask.shape != ids.shape:
                raise ValueError("mask and ids differ in shape")
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.int32)
            if lengths.shape != (n,):
                raise ValueError("lengths must have one entry per row")
    out_offs = np.zeros(n + 1, np.uint64)
    txt, nr, bs, bi = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    st = lib.tgx_decode_rows_host(ptr(vocab_flat) if vocab_flat.size else None, ptr(vocab_offs), _u32_arg(vocab_size, "vocab_size"),
                                  ptr(special_flat) if special_flat.size else None, ptr(special_offs), _u32_arg(n_specials, "n_specials"),
                                  ptr(ids) if ids.size else None, _DECODE_KINDS[ids.dtype], None if id_offs is None else ptr(id_offs), n, L,
                                  None if mask is None or not mask.size else ptr(mask), None if lengths is None or not n else ptr(lengths),
                                  _id_or_none(skip_id), 1 if include_special else 0, C.byref(txt), ptr(out_offs), C.byref(nr), C.byref(bs),
                                  C.byref(bi))
    if st != OK:
        _raise_decode(st, bs.value, bi.value)
    return _take(txt, int(out_offs[-1]), C.c_uint8, np.uint8), out_offs, nr.value


def span_flags(unit: str = "byte", dtype=np.int32, padding_side: str = "right", truncation_side: str = "right") -> int:
    """The flags of a spans call: layout_flags with TGX_SPAN_CHARS for unit "char"."""
    if unit not in ("byte", "char"):
        raise ValueError(f"unit must be 'byte' or 'char' (got {unit!r})")
    return layout_flags(padding_side, truncation_side, dtype) | (SPAN_CHARS if unit == "char" else 0)


def spans_host(vocab_flat, vocab_offs, vocab_size: int, special_flat, special_offs, n_specials: int, ids: np.ndarray, offs: np.ndarray, *,
               unit: str = "byte", dtype=np.int32, row_len: int | None = None, bos_id: int | None = None, eos_id: int | None = None,
               padding_side: str = "right", truncation_side: str = "right", out: np.ndarray | None = None) -> np.ndarray:
    """Host twin of NativeModel.result_spans / result_pad_spans (tgx_spans_host: the kernels' index arithmetic, no device)
    over ids u32[T] and offsets u64[S+1] -> [T, 2] of dtype, or [S, row_len, 2] aligned with layout_pad_host's input_ids
    (bos, eos and padding get (0, 0)).  unit "byte": the token's bytes in its row's text; "char": its code points.  The
    byte unit reads only special_offs, so special_flat may be empty whatever they declare.  out: a C-contiguous array of
    that shape and dtype to write into."""
    vocab_flat = np.ascontiguousarray(vocab_flat, dtype=np.uint8)
    vocab_offs = np.ascontiguousarray(vocab_offs, dtype=np.uint64)
    special_flat = np.ascontiguousarray(special_flat, dtype=np.uint8)
    special_offs = np.ascontiguousarray(special_offs, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.shape[0] - 1
    if row_len is None:
        L, flags = 0, span_flags(unit, dtype)
        shape = (int(offs[-1]) if n else 0, 2)
    else:
        L, flags = _u32_arg(row_len, "row_len"), span_flags(unit, dtype, padding_side, truncation_side)
        if L < 1:
            raise TokenGeeXError("row_len must be at least 1", ERR_INVALID)
        shape = (n, L, 2)
    if out is None:
        out = np.empty(shape, np.dtype(dtype))
    elif out.shape != shape or out.dtype != np.dtype(dtype) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {np.dtype(dtype)} array of shape {shape}")
    st = lib.tgx_spans_host(ptr(vocab_flat) if vocab_flat.size else None, ptr(vocab_offs), _u32_arg(vocab_size, "vocab_size"),
                            ptr(special_flat) if special_flat.size else None, ptr(special_offs), _u32_arg(n_specials, "n_specials"),
                            ptr(ids) if ids.size else None, ptr(offs), n, L, _id_or_none(bos_id), _id_or_none(eos_id), flags,
                            ptr(out) if out.size else None)
    if st == ERR_TOKEN_ID_OOB:  # the row and the id, as the decode twins name them
        bs, bi, _ = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.tgx_last_error_detail(C.byref(bs), C.byref(bi), C.byref(_))
        _raise_decode(st, bs.value, bi.value)
    check(st)
    return out


def substring_df(flat: np.ndarray, part_begin: np.ndarray, part_end: np.ndarray, part_sample: np.ndarray,
                 max_token_length: int, insert_probability: float = 1.0, seed: int = 0, device: int = 0, with_collisions: bool = False,
                 part_origin=None):
    """Document frequencies of char-aligned substrings on the device -> (pos u64[D], len u32[D], df u32[D], n_windows
    [, entries that met a foreign run in a discarded attempt]).  part_origin: where every part's sample begins in `flat`
    (None: the part is its own sample) — the keep rule hashes the occurrence's offset in its sample."""
    flat = np.ascontiguousarray(flat, np.uint8)
    pb, pe = np.ascontiguousarray(part_begin, np.uint64), np.ascontiguousarray(part_end, np.uint64)
    ps = np.ascontiguousarray(part_sample, np.uint32)
    po = None if part_origin is None else np.ascontiguousarray(part_origin, np.uint64)
    pos, ln, df, n, nw, nc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib.tgx_substring_df(device, ptr(flat) if flat.size else None, flat.size, ptr(pb), ptr(pe), ptr(ps), None if po is None else ptr(po), pb.shape[0],
                               max_token_length, float(insert_probability), seed & (2**64 - 1), C.byref(pos), C.byref(ln),
                               C.byref(df), C.byref(n), C.byref(nw), C.byref(nc)))
    k = n.value
    out = (_take(pos, k, C.c_uint64, np.uint64), _take(ln, k, C.c_uint32, np.uint32), _take(df, k, C.c_uint32, np.uint32), nw.value)
    return out + (nc.value,) if with_collisions else out


def substring_df_top(flat: np.ndarray, part_begin: np.ndarray, part_end: np.ndarray, part_sample: np.ndarray,
                     max_token_length: int, top_k: int, insert_probability: float = 1.0, seed: int = 0, device: int = 0, part_origin=None):
    """The top_k most frequent substrings only (descending frequency; 0 = all)
    -> (pos, len, df, n_windows, n_distinct, cutoff_df): whatever was cut off occurs in at most cutoff_df samples."""
    flat = np.ascontiguousarray(flat, np.uint8)
    pb, pe = np.ascontiguousarray(part_begin, np.uint64), np.ascontiguousarray(part_end, np.uint64)
    ps = np.ascontiguousarray(part_sample, np.uint32)
    po = None if part_origin is None else np.ascontiguousarray(part_origin, np.uint64)
    pos, ln, df, n, nw, nc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    nd, cut = C.c_uint64(), C.c_uint32()
    check(lib.tgx_substring_df_top(device, ptr(flat) if flat.size else None, flat.size, ptr(pb), ptr(pe), ptr(ps), None if po is None else ptr(po), pb.shape[0],
                                   max_token_length, float(insert_probability), seed & (2**64 - 1), int(top_k), C.byref(pos),
                                   C.byref(ln), C.byref(df), C.byref(n), C.byref(nw), C.byref(nc), C.byref(nd), C.byref(cut)))
    k = n.value
    return (_take(pos, k, C.c_uint64, np.uint64), _take(ln, k, C.c_uint32, np.uint32), _take(df, k, C.c_uint32, np.uint32),
            nw.value, nd.value, cut.value)


def generate_u01(seed: int, sample: int, window_hash: int) -> float:
    return lib.tgx_generate_u01(seed & (2**64 - 1), sample, window_hash & (2**64 - 1))


def utf8_lossy(data: bytes) -> bytes:
    """String::from_utf8_lossy (the library's own implementation; tests compare it with Python's)."""
    src = np.frombuffer(data, np.uint8)
    out = np.empty(max(1, 3 * len(data)), np.uint8)
    n = lib.tgx_utf8_lossy(ptr(src) if len(data) else None, len(data), ptr(out))
    return out[:n].tobytes()


def _u32_arg(v, name: str) -> int:
    v = int(v)
    if not 0 <= v <= 0xFFFFFFFF:
        raise TokenGeeXError(f"{name} {v} is not a u32", ERR_INVALID)
    return v


def _id_or_none(v) -> int:
    return NO_ID if v is None else _u32_arg(v, "token id")


def layout_flags(padding_side: str = "right", truncation_side: str = "right", dtype=np.int32) -> int:
    """TGX_LAYOUT_* flags of a padded / packed layout; dtype: int32 or int64 (numpy)."""
    for side in (padding_side, truncation_side):
        if side not in ("left", "right"):
            raise ValueError(f"side must be 'left' or 'right' (got {side!r})")
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError(f"dtype must be int32 or int64 (got {dt})")
    return ((LAYOUT_PAD_LEFT if padding_side == "left" else 0) | (LAYOUT_TRUNC_LEFT if truncation_side == "left" else 0)
            | (LAYOUT_I64 if dt == np.dtype(np.int64) else 0))


def layout_pad_host(ids: np.ndarray, offs: np.ndarray, row_len: int, pad_id: int, *, bos_id: int | None = None,
                    eos_id: int | None = None, padding_side: str = "right", truncation_side: str = "right", dtype=np.int32) -> dict:
    """Host twin of NativeResult.pad_device (tgx_layout_pad_host: the same row mapping, no device) over ids u32[T] and
    offsets u64[S+1] -> {"input_ids": [S, row_len] of dtype, "attention_mask": u8 [S, row_len], "lengths": i32[S],
    "n_truncated": int}."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n, L = offs.shape[0] - 1, _u32_arg(row_len, "row_len")
    out = np.empty((n, L), np.dtype(dtype))
    mask = np.empty((n, L), np.uint8)
    lengths = np.empty(n, np.int32)
    nt = C.c_uint64()
    check(lib.tgx_layout_pad_host(ptr(ids) if ids.size else None, ptr(offs), n, L, _u32_arg(pad_id, "pad_id"), _id_or_none(bos_id), _id_or_none(eos_id),
                                  layout_flags(padding_side, truncation_side, dtype), ptr(out) if out.size else None,
                                  ptr(mask) if mask.size else None, ptr(lengths) if n else None, C.byref(nt)))
    return {"input_ids": out, "attention_mask": mask, "lengths": lengths, "n_truncated": nt.value}


def layout_pack_host(ids: np.ndarray, offs: np.ndarray, block_len: int, pad_id: int, *, bos_id: int | None = None,
                     eos_id: int | None = None, dtype=np.int32) -> dict:
    """Host twin of NativeResult.pack_device (tgx_layout_pack_host) -> {"input_ids": [B, block_len] of dtype, "doc_ids" and
    "positions": i32 [B, block_len]}."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n, L = offs.shape[0] - 1, _u32_arg(block_len, "block_len")
    a = (_id_or_none(bos_id) != NO_ID) + (_id_or_none(eos_id) != NO_ID)
    n_stream = int(offs[-1]) + n * a
    nb = -(-n_stream // L) if L else 0
    out = np.empty((nb, L), np.dtype(dtype))
    doc = np.empty((nb, L), np.int32)
    pos = np.empty((nb, L), np.int32)
    got = C.c_uint64()
    check(lib.tgx_layout_pack_host(ptr(ids) if ids.size else None, ptr(offs), n, L, _u32_arg(pad_id, "pad_id"), _id_or_none(bos_id), _id_or_none(eos_id),
                                   layout_flags(dtype=dtype), ptr(out) if out.size else None, ptr(doc) if doc.size else None,
                                   ptr(pos) if pos.size else None, C.byref(got)))
    assert got.value == nb, (got.value, nb)
    return {"input_ids": out, "doc_ids": doc, "positions": pos}


def layout_windows_host(ids: np.ndarray, offs: np.ndarray, row_len: int, stride: int, pad_id: int, *, bos_id: int | None = None,
                        eos_id: int | None = None, padding_side: str = "right", truncation_side: str = "right", dtype=np.int32,
                        n_windows: int | None = None) -> dict:
    """Host twin of NativeResult.window_pad_device (tgx_layout_windows_host: the same window mapping, no device) over ids
    u32[T] and offsets u64[S+1] -> {"input_ids": [W, row_len] of dtype, "attention_mask": u8 [W, row_len], "lengths",
    "overflow_to_sample_mapping" and "window_first": i32[W]}: every row as windows of row_len elements that repeat `stride`
    tokens of the window before.  n_windows: what the destinations are sized for (None: the twin is asked for W first)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n, L = offs.shape[0] - 1, _u32_arg(row_len, "row_len")
    args = (ptr(ids) if ids.size else None, ptr(offs), n, L, _u32_arg(stride, "stride"), _u32_arg(pad_id, "pad_id"), _id_or_none(bos_id),
            _id_or_none(eos_id), layout_flags(padding_side, truncation_side, dtype))
    got = C.c_uint64()
    if n_windows is None:
        check(lib.tgx_layout_windows_host(*args, 0, None, None, None, None, None, C.byref(got)))
        n_windows = got.value
    W = int(n_windows)
    out = np.empty((W, L), np.dtype(dtype))
    mask = np.empty((W, L), np.uint8)
    lengths, row, first = (np.empty(W, np.int32) for _ in range(3))
    keep = np.empty(1, np.dtype(dtype))   # a destination even when W = 0: NULL asks for W alone
    check(lib.tgx_layout_windows_host(*args, W, ptr(out) if out.size else ptr(keep), ptr(mask) if mask.size else None,
                                      ptr(lengths) if W else None, ptr(row) if W else None, ptr(first) if W else None, C.byref(got)))
    assert got.value == W, (got.value, W)
    return {"input_ids": out, "attention_mask": mask, "lengths": lengths, "overflow_to_sample_mapping": row, "window_first": first}


def window_spans_host(vocab_flat, vocab_offs, vocab_size: int, special_flat, special_offs, n_specials: int, ids: np.ndarray, offs: np.ndarray, *,
                      row_len: int, stride: int, unit: str = "byte", dtype=np.int32, bos_id: int | None = None, eos_id: int | None = None,
                      padding_side: str = "right", truncation_side: str = "right", n_windows: int | None = None) -> np.ndarray:
    """Host twin of NativeResult.window_spans_device (tgx_window_spans_host) -> [W, row_len, 2] of dtype, aligned element for
    element with layout_windows_host's input_ids: a kept token's span in its whole row's text, (0, 0) elsewhere."""
    vocab_flat = np.ascontiguousarray(vocab_flat, dtype=np.uint8)
    vocab_offs = np.ascontiguousarray(vocab_offs, dtype=np.uint64)
    special_flat = np.ascontiguousarray(special_flat, dtype=np.uint8)
    special_offs = np.ascontiguousarray(special_offs, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n, L = offs.shape[0] - 1, _u32_arg(row_len, "row_len")
    args = (ptr(vocab_flat) if vocab_flat.size else None, ptr(vocab_offs), _u32_arg(vocab_size, "vocab_size"),
            ptr(special_flat) if special_flat.size else None, ptr(special_offs), _u32_arg(n_specials, "n_specials"),
            ptr(ids) if ids.size else None, ptr(offs), n, L, _u32_arg(stride, "stride"), _id_or_none(bos_id), _id_or_none(eos_id),
            span_flags(unit, dtype, padding_side, truncation_side))
    got = C.c_uint64()
    if n_windows is None:
        check(lib.tgx_window_spans_host(*args, 0, None, C.byref(got)))
        n_windows = got.value
    W = int(n_windows)
    out = np.empty((W, L, 2), np.dtype(dtype))
    keep = np.empty(1, np.dtype(dtype))
    st = lib.tgx_window_spans_host(*args, W, ptr(out) if out.size else ptr(keep), C.byref(got))
    if st == ERR_TOKEN_ID_OOB:  # the row and the id, as the decode twins name them
        bs, bi, _ = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.tgx_last_error_detail(C.byref(bs), C.byref(bi), C.byref(_))
        _raise_decode(st, bs.value, bi.value)
    check(st)
    assert got.value == W, (got.value, W)
    return out


class LatticeStats:
    """Per-sample statistics of the Unigram lattice under P(x) ∝ exp(alpha · Σ score) (include/tgx.h: lattice statistics):
    logz, expected_score (raw scores), expected_tokens and n_bytes, f64 / u64 arrays in input order.  A sample whose
    end no path reaches has logz = -inf and NaN in the other two (no_path); n_no_path counts them."""

    def __init__(self, logz, expected_score, expected_tokens, n_bytes, alpha: float, n_no_path: int | None = None):
        self.logz = np.asarray(logz, np.float64)
        self.expected_score = np.asarray(expected_score, np.float64)
        self.expected_tokens = np.asarray(expected_tokens, np.float64)
        self.n_bytes = np.asarray(n_bytes, np.uint64)
        self.alpha = float(alpha)
        self.n_no_path = int(np.count_nonzero(np.isneginf(self.logz))) if n_no_path is None else int(n_no_path)

    def __len__(self) -> int:
        return self.logz.shape[0]

    @property
    def no_path(self) -> np.ndarray:
        return np.isneginf(self.logz)

    @property
    def entropy(self) -> np.ndarray:
        """Entropy of the segmentation distribution in nats: logz − alpha · expected_score (NaN where no_path)."""
        with np.errstate(invalid="ignore"):
            return self.logz - self.alpha * self.expected_score

    @property
    def bits_per_byte(self) -> np.ndarray:
        """−logz / (n_bytes · ln 2): at alpha = 1 the text's cost under the unigram LM (NaN for an empty sample)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return -self.logz / (self.n_bytes.astype(np.float64) * np.log(2.0))


def lattice_stats_host(tokens: list[bytes], scores, flat: np.ndarray, offs: np.ndarray, alpha: float = 1.0) -> LatticeStats:
    """The host twin of NativeModel.lattice_stats_flat (tgx_lattice_stats_host): plain f64, no device, no model."""
    vflat, voffs = pack(tokens)
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.shape[0] - 1
    out = np.zeros((3, max(n, 1)), np.float64)
    bad = C.c_uint64(0)
    check(lib.tgx_lattice_stats_host(ptr(vflat) if vflat.size else None, ptr(voffs), ptr(scores) if scores.size else None, len(tokens),
                                     ptr(flat) if flat.size else None, ptr(offs), n, float(alpha), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                     C.byref(bad)))
    return LatticeStats(out[0, :n].copy(), out[1, :n].copy(), out[2, :n].copy(), np.diff(offs), alpha, bad.value)


class NativeResult:
    """Owns a tgx_result (ids + offsets of one encode pass)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_result_free(self._h)
            self._h = None

    @property
    def num_tokens(self) -> int:
        return lib.tgx_result_num_tokens(self._h)

    @property
    def num_samples(self) -> int:
        return lib.tgx_result_num_samples(self._h)

    @property
    def vocab_size(self) -> int:
        """Every id of the result is below it: the model's vocabulary, plus the special tokens for an assembled result."""
        return lib.tgx_result_vocab_size(self._h)

    def offsets(self) -> np.ndarray:
        out = np.empty(self.num_samples + 1, np.uint64)
        check(lib.tgx_result_copy_offsets(self._h, ptr(out), out.size))
        return out

    def ids(self) -> np.ndarray:
        t = self.num_tokens
        if t == 0:
            return np.zeros(0, np.uint32)
        out = np.empty(t, np.uint32)   # the device copy lands in the array itself
        check(lib.tgx_result_copy_ids(self._h, ptr(out), t))
        return out

    def ids_into(self, out: np.ndarray) -> int:
        """Copies the ids into caller memory (uint32, at least num_tokens long); -> number of ids."""
        t = self.num_tokens
        assert out.dtype == np.uint32 and out.flags.c_contiguous and out.size >= t
        if t:
            check(lib.tgx_result_copy_ids(self._h, ptr(out), t))
        return t

    def ids_device_ptr(self) -> int:
        return lib.tgx_result_ids_device(self._h) or 0

    @property
    def device(self) -> int:
        return lib.tgx_result_device(self._h)

    # -- layouts for a model (include/tgx.h: tgx_result_pad_device / tgx_result_pack_device; csrc/layout.hip) --
    def layout_info(self, bos_id: int | None = None, eos_id: int | None = None) -> tuple[int, int]:
        """-> (max_row_len = longest row + A, n_stream = T + S·A), A = how many of bos / eos are given: what sizes the
        destinations of pad_device / pack_device.  The longest row is reduced on the device (one word comes back)."""
        mx, ns = C.c_uint64(), C.c_uint64()
        check(lib.tgx_result_layout_info(self._h, _id_or_none(bos_id), _id_or_none(eos_id), C.byref(mx), C.byref(ns)))
        return mx.value, ns.value

    def pad_device(self, row_len: int, pad_id: int, ids_ptr: int, *, mask_ptr: int = 0, lengths_ptr: int = 0,
                   bos_id: int | None = None, eos_id: int | None = None, flags: int = 0, stream: int = 0) -> int:
        """The rows padded / truncated to row_len, written by the device into caller-owned device memory given as raw
        integer pointers (ids: i32 or, with LAYOUT_I64, i64 [S·row_len]; mask u8[S·row_len]; lengths i32[S]; 0 = not
        wanted), queued on `stream` (a hipStream_t as an integer; 0: a stream of the library, which is ordered after everything
        queued earlier on the device's null stream — 0 is that stream's own handle, torch's default stream).  Returns when
        the stream has reached its end -> number of truncated rows."""
        nt = C.c_uint64()
        check(lib.tgx_result_pad_device(self._h, _u32_arg(row_len, "row_len"), _u32_arg(pad_id, "pad_id"), _id_or_none(bos_id), _id_or_none(eos_id),
                                        int(flags), stream or None, ids_ptr or None, mask_ptr or None, lengths_ptr or None, C.byref(nt)))
        return nt.value

    def pack_device(self, block_len: int, pad_id: int, ids_ptr: int, *, doc_ptr: int = 0, pos_ptr: int = 0,
                    bos_id: int | None = None, eos_id: int | None = None, flags: int = 0, stream: int = 0) -> int:
        """The rows' sequences back to back, cut into blocks of block_len (ids i32 / i64, doc and pos i32, each
        [n_blocks·block_len] with n_blocks = ceil(layout_info()[1] / block_len)); as pad_device -> n_blocks."""
        nb = C.c_uint64()
        check(lib.tgx_result_pack_device(self._h, _u32_arg(block_len, "block_len"), _u32_arg(pad_id, "pad_id"), _id_or_none(bos_id), _id_or_none(eos_id),
                                         int(flags), stream or None, ids_ptr or None, doc_ptr or None, pos_ptr or None, C.byref(nb)))
        return nb.value

    # -- overflow windows (include/tgx.h: tgx_result_window_pad_device / tgx_result_window_spans_device) --
    def window_info(self, row_len: int, stride: int = 0, *, bos_id: int | None = None, eos_id: int | None = None, flags: int = 0) -> int:
        """-> W, the windows of row_len elements (stride tokens repeated from one to the next) that the rows give: what
        sizes the destinations of window_pad_device / window_spans_device.  Counted and scanned on the device; one word
        comes back."""
        w = C.c_uint64()
        check(lib.tgx_result_window_info(self._h, _u32_arg(row_len, "row_len"), _u32_arg(stride, "stride"), _id_or_none(bos_id),
                                         _id_or_none(eos_id), _u32_arg(flags, "flags"), C.byref(w)))
        return w.value

    def window_pad_device(self, row_len: int, stride: int, pad_id: int, n_windows: int, ids_ptr: int, *, mask_ptr: int = 0,
                          lengths_ptr: int = 0, window_row_ptr: int = 0, window_first_ptr: int = 0, bos_id: int | None = None,
                          eos_id: int | None = None, flags: int = 0, stream: int = 0) -> None:
        """Every row as overlapping windows, written by the device into caller-owned device memory given as raw integer
        pointers (ids: i32 or, with LAYOUT_I64, i64 [W·row_len]; mask u8[W·row_len]; lengths, window_row — the row a window
        came from — and window_first — the index of its first kept token in that row — i32[W]; 0 = not wanted), as
        pad_device.  n_windows is the W of window_info the destinations are sized for: the call counts again and raises
        (ERR_INVALID) without writing when it finds another number."""
        check(lib.tgx_result_window_pad_device(self._h, _u32_arg(row_len, "row_len"), _u32_arg(stride, "stride"), _u32_arg(pad_id, "pad_id"),
                                               _id_or_none(bos_id), _id_or_none(eos_id), int(flags), stream or None, int(n_windows),
                                               ids_ptr or None, mask_ptr or None, lengths_ptr or None, window_row_ptr or None,
                                               window_first_ptr or None))

    def window_spans_device(self, model: "NativeModel", special_flat, special_offs, row_len: int, stride: int, n_windows: int,
                            spans_ptr: int, *, bos_id: int | None = None, eos_id: int | None = None, flags: int = 0, stream: int = 0) -> None:
        """The offsets mapping of window_pad_device's ids: [W, row_len, 2] int32 (int64 with LAYOUT_I64), a kept token's span
        in its whole row's text (SPAN_CHARS: in code points), (0, 0) on bos, eos and padding; model and specials as in
        NativeModel.result_spans."""
        sf, so, n = model._specials(special_flat, special_offs)
        check(lib.tgx_result_window_spans_device(model._h, self._h, ptr(sf) if sf.size else None, ptr(so), n, _u32_arg(row_len, "row_len"),
                                                 _u32_arg(stride, "stride"), _id_or_none(bos_id), _id_or_none(eos_id), _u32_arg(flags, "flags"),
                                                 stream or None, int(n_windows), spans_ptr or None))

    # -- fill-in-the-middle (include/tgx.h: tgx_result_fim; csrc/fim.hip) --
    @classmethod
    def from_ids(cls, ids: np.ndarray, offs: np.ndarray, vocab_size: int, device: int = 0) -> "NativeResult":
        """A result on `device` from host arrays (ids u32[T], offsets u64[S+1] from 0, every id below vocab_size): ids that
        were tokenised elsewhere, for fim, the layouts and decode_result."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.tgx_result_from_ids(int(device), ptr(ids) if ids.size else None, ptr(offs) if offs.size else None, max(offs.shape[0] - 1, 0),
                                      _u32_arg(vocab_size, "vocab_size"), C.byref(h)))
        return cls(h)

    def fim(self, prefix_id: int, suffix_id: int, middle_id: int, *, rate: float = 1.0, spm_rate: float = 0.5, seed: int = 0,
            first_row: int = 0, return_info: bool = False, stream: int = 0):
        """The rows rearranged for fill-in-the-middle on the device -> a new NativeResult (this one is only read): a row
        is rearranged with probability `rate` into PRE prefix SUF suffix MID middle (PSM) or, with probability spm_rate
        of those, PRE SUF suffix MID prefix middle (SPM), at two cuts drawn per row from (seed, first_row + row).
        return_info=True -> (NativeResult, mode u8[S]: 0 copied / 1 PSM / 2 SPM, cuts u64[S, 2]).  stream as in
        pad_device."""
        n = self.num_samples
        mode = np.zeros(n, np.uint8) if return_info else None
        cuts = np.zeros((n, 2), np.uint64) if return_info else None
        h = C.c_void_p()
        m = 2**64 - 1
        check(lib.tgx_result_fim(self._h, _u32_arg(prefix_id, "sentinel id"), _u32_arg(suffix_id, "sentinel id"), _u32_arg(middle_id, "sentinel id"),
                                 float(rate), float(spm_rate), int(seed) & m, int(first_row) & m, stream or None,
                                 ptr(mode) if return_info and n else None, ptr(cuts) if return_info and n else None, None, C.byref(h)))
        res = NativeResult(h)
        return (res, mode, cuts) if return_info else res

    # -- rows selected and reordered (include/tgx.h: tgx_result_select; csrc/select.hip) --
    def select(self, rows, *, stream: int = 0) -> "NativeResult":
        """A new result whose row k is row rows[k] of this one (any order, any subset, repeats allowed), moved on the
        device; this result is only read.  rows: a list or numpy integer array (uploaded), a boolean mask of length
        num_samples (its nonzero indices), or a CUDA torch tensor on the result's device (read in place, in the order of
        torch.cuda.current_stream unless a stream is given).  An index outside [0, num_samples) raises ERR_INVALID
        naming the first such k."""
        p, m, flags, stream, keep = _select_args(rows, self.num_samples, self.device, stream)
        h = C.c_void_p()
        check(lib.tgx_result_select(self._h, p, m, flags, stream or None, C.byref(h)))
        del keep
        return NativeResult(h)

    def lengths_device(self, ptr_: int, stream: int = 0) -> None:
        """The rows' lengths as int64[num_samples] written by the device into caller-owned device memory (a raw integer
        pointer; tgx_result_lengths_device), queued on `stream` as in pad_device."""
        check(lib.tgx_result_lengths_device(self._h, stream or None, ptr_ or None))

    # -- exact row deduplication (include/tgx.h: tgx_result_first_equal_device; csrc/dedup.hip) --
    def first_equal(self, d_first: int, *, stream: int = 0) -> int:
        """first[k] = the first row with row k's ids, as int64[S] into caller-owned device memory (a raw integer pointer;
        tgx_result_first_equal_device), queued on `stream` as in pad_device -> the number of distinct rows."""
        nu = C.c_uint64()
        check(lib.tgx_result_first_equal_device(self._h, 0, stream or None, d_first or None, C.byref(nu)))
        return int(nu.value)

    def row_hashes(self, d_hashes: int, seed: int = 0, *, stream: int = 0) -> None:
        """tgx_row_hash of every row's ids under `seed`, as u64[S] into caller-owned device memory
        (tgx_result_row_hashes_device)."""
        check(lib.tgx_result_row_hashes_device(self._h, int(seed) & (2**64 - 1), stream or None, d_hashes or None))

    # -- near-duplicate rows (include/tgx.h: tgx_result_minhash_device; csrc/minhash.hip) --
    def minhash(self, d_sig: int, width: int = 5, n_perm: int = 128, seed: int = 0, *, stream: int = 0) -> None:
        """The MinHash signature of every row's token n-grams of `width` ids, as u32[S, n_perm] into caller-owned device
        memory (a raw integer pointer; tgx_result_minhash_device), queued on `stream` as in pad_device."""
        check(lib.tgx_result_minhash_device(self._h, int(width), int(n_perm), int(seed) & (2**64 - 1), 0, stream or None, d_sig or None))

    # -- shared n-grams (include/tgx.h: tgx_result_gramset_create, tgx_result_gram_hits_device; csrc/gram.hip) --
    def gram_set(self, width: int, seed: int = 0, *, stream: int = 0) -> NativeGramSet:
        """The set of the keys of every n-gram of `width` ids of the rows (tgx_result_gramset_create), queued on `stream`
        as in pad_device.  This result is only read."""
        h = C.c_void_p()
        check(lib.tgx_result_gramset_create(self._h, int(width), int(seed) & (2**64 - 1), 0, stream or None, C.byref(h)))
        return NativeGramSet(h)

    def repeat_stats(self, width: int, seed: int = 0, d_stats: int = 0, d_mask: int = 0, *, stream: int = 0) -> None:
        """Per row the repetition statistics of its n-grams of `width` ids, as int64[6, S], and per id whether a repeat
        (bit 0) or a member of a class of two or more (bit 1) begins there, as u8[T], into caller-owned device memory
        (either may be 0; tgx_result_repeat_stats_device)."""
        check(lib.tgx_result_repeat_stats_device(self._h, int(width), int(seed) & (2**64 - 1), 0, stream or None, d_stats or None, d_mask or None))

    def gram_hits(self, grams: NativeGramSet, d_count: int = 0, d_mask: int = 0, *, stream: int = 0) -> None:
        """Per row the n-grams whose key is in `grams`, as int64[S], and per id whether the n-gram that begins there is
        one, as u8[T], into caller-owned device memory (raw integer pointers, either may be 0;
        tgx_result_gram_hits_device)."""
        check(lib.tgx_result_gram_hits_device(self._h, grams._h, 0, stream or None, d_count or None, d_mask or None))

    def phrase_hits(self, phrases: "NativePhraseSet", d_count: int = 0, d_longest: int = 0, d_per_phrase: int = 0, *, stream: int = 0) -> None:
        """Per row the occurrences of the phrases of `phrases`, as int64[S], per id the longest occurrence that begins
        there, as u8[T], and per phrase its occurrences, as int64[P], into caller-owned device memory (raw integer
        pointers, any may be 0, not all; tgx_result_phrase_hits_device)."""
        check(lib.tgx_result_phrase_hits_device(self._h, phrases._h, 0, stream or None, d_count or None, d_longest or None, d_per_phrase or None))

    def pad_host(self, row_len: int, pad_id: int, **kw) -> dict:
        """layout_pad_host over the ids and offsets copied to the host."""
        return layout_pad_host(self.ids(), self.offsets(), row_len, pad_id, **kw)

    def pack_host(self, block_len: int, pad_id: int, **kw) -> dict:
        """layout_pack_host over the ids and offsets copied to the host."""
        return layout_pack_host(self.ids(), self.offsets(), block_len, pad_id, **kw)


class NativeText:
    """Owns a tgx_text: the UTF-8 bytes and u64 offsets[S+1] of S decoded rows, resident in HBM (csrc/decode.hip)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_text_free(self._h)
            self._h = None

    @property
    def num_rows(self) -> int:
        return lib.tgx_text_num_rows(self._h)

    @property
    def num_bytes(self) -> int:
        return lib.tgx_text_num_bytes(self._h)

    @property
    def num_replaced(self) -> int:
        """Replacement characters String::from_utf8_lossy wrote."""
        return lib.tgx_text_num_replaced(self._h)

    @property
    def device(self) -> int:
        return lib.tgx_text_device(self._h)

    def bytes(self) -> np.ndarray:
        n = self.num_bytes
        out = np.empty(n, np.uint8)
        if n:
            check(lib.tgx_text_copy_bytes(self._h, ptr(out), n))
        return out

    def offsets(self) -> np.ndarray:
        out = np.empty(self.num_rows + 1, np.uint64)
        check(lib.tgx_text_copy_offsets(self._h, ptr(out), out.size))
        return out

    @property
    def bytes_ptr(self) -> int:
        return lib.tgx_text_bytes_device(self._h) or 0

    @property
    def offsets_ptr(self) -> int:
        return lib.tgx_text_offsets_device(self._h) or 0

    def to_corpus(self) -> "NativeCorpus":
        """A resident corpus over the rows (tgx_corpus_from_text: a device-to-device copy; the text stays valid)."""
        h = C.c_void_p()
        check(lib.tgx_corpus_from_text(self._h, C.byref(h)))
        c = NativeCorpus.__new__(NativeCorpus)
        c._h = h
        c.device = self.device
        return c


class NativePlan:
    """Owns a tgx_plan: the split plan of a resident corpus (seg_offs u64[S+1], seg_special i32[K]) in HBM (csrc/front.hip)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_plan_free(self._h)
            self._h = None

    @property
    def num_samples(self) -> int:
        return lib.tgx_plan_num_samples(self._h)

    @property
    def num_segments(self) -> int:
        return lib.tgx_plan_num_segments(self._h)

    @property
    def num_encoded(self) -> int:
        return lib.tgx_plan_num_encoded(self._h)

    @property
    def device(self) -> int:
        return lib.tgx_plan_device(self._h)

    def _copy(self):
        seg_offs = np.zeros(self.num_samples + 1, np.uint64)
        seg_special = np.zeros(self.num_segments, np.int32)
        check(lib.tgx_plan_copy(self._h, ptr(seg_offs), seg_offs.size, ptr(seg_special) if seg_special.size else None, seg_special.size))
        return seg_offs, seg_special

    def seg_offs(self) -> np.ndarray:
        return self._copy()[0]

    def seg_special(self) -> np.ndarray:
        return self._copy()[1]


class NativeCorpus:
    """Owns a tgx_corpus: a packed batch resident in HBM across passes."""

    def __init__(self, flat: np.ndarray, offs: np.ndarray, device: int = 0):
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.tgx_corpus_upload(device, ptr(flat) if flat.size else None, ptr(offs),
                                    offs.shape[0] - 1, C.byref(h)))
        self._h = h
        self.device = device

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_corpus_free(self._h)
            self._h = None

    @property
    def num_samples(self) -> int:
        return lib.tgx_corpus_num_samples(self._h)

    @property
    def num_bytes(self) -> int:
        return lib.tgx_corpus_num_bytes(self._h)

    def bytes(self) -> np.ndarray:
        """The corpus's text copied to the host (tgx_corpus_copy_text)."""
        n = self.num_bytes
        out = np.empty(n, np.uint8)
        if n:
            check(lib.tgx_corpus_copy_text(self._h, ptr(out), n))
        return out

    def offsets(self) -> np.ndarray:
        """The samples' offsets u64[S+1], from 0 (tgx_corpus_copy_offsets)."""
        out = np.empty(self.num_samples + 1, np.uint64)
        check(lib.tgx_corpus_copy_offsets(self._h, ptr(out), out.size))
        return out

    def split_specials(self, specials: list[bytes], crlf: bool) -> "tuple[NativeCorpus, NativePlan]":
        """The corpus split at special tokens on the device (tgx_corpus_split_specials, csrc/front.hip) -> (a resident corpus
        of the non-special segments, CRLF-normalised on the way if asked: what pack_segments packs; the plan of
        split_specials_flat, in HBM).  This corpus is only read."""
        sflat, soffs = pack(specials)
        hc, hp = C.c_void_p(), C.c_void_p()
        check(lib.tgx_corpus_split_specials(self._h, ptr(sflat) if sflat.size else None, ptr(soffs), len(specials), FRONT_CRLF if crlf else 0,
                                            C.byref(hc), C.byref(hp)))
        c = NativeCorpus.__new__(NativeCorpus)
        c._h = hc
        c.device = self.device
        return c, NativePlan(hp)

    def select(self, rows, *, stream: int = 0) -> "NativeCorpus":
        """A new resident corpus whose sample k is sample rows[k] of this one, moved on the device (tgx_corpus_select);
        rows as in NativeResult.select.  With the same rows, corpus and result stay aligned.  This corpus is only read."""
        p, m, flags, stream, keep = _select_args(rows, self.num_samples, self.device, stream)
        hc = C.c_void_p()
        check(lib.tgx_corpus_select(self._h, p, m, flags, stream or None, C.byref(hc)))
        del keep
        c = NativeCorpus.__new__(NativeCorpus)
        c._h = hc
        c.device = self.device
        return c

    def first_equal(self, d_first: int, *, stream: int = 0) -> int:
        """first[k] = the first sample with sample k's bytes, as int64[S] into caller-owned device memory (a raw integer
        pointer; tgx_corpus_first_equal_device), queued on `stream` -> the number of distinct samples.  With the same
        indices, corpus and result stay aligned.  This corpus is only read."""
        nu = C.c_uint64()
        check(lib.tgx_corpus_first_equal_device(self._h, 0, stream or None, d_first or None, C.byref(nu)))
        return int(nu.value)

    def row_hashes(self, d_hashes: int, seed: int = 0, *, stream: int = 0) -> None:
        """tgx_row_hash of every sample under `seed`, as u64[S] into caller-owned device memory
        (tgx_corpus_row_hashes_device)."""
        check(lib.tgx_corpus_row_hashes_device(self._h, int(seed) & (2**64 - 1), stream or None, d_hashes or None))

    def minhash(self, d_sig: int, width: int = 5, n_perm: int = 128, seed: int = 0, *, stream: int = 0) -> None:
        """The MinHash signature of every sample's byte shingles of `width` bytes, as u32[S, n_perm] into caller-owned
        device memory (tgx_corpus_minhash_device).  This corpus is only read."""
        check(lib.tgx_corpus_minhash_device(self._h, int(width), int(n_perm), int(seed) & (2**64 - 1), 0, stream or None, d_sig or None))

    def gram_set(self, width: int, seed: int = 0, *, stream: int = 0) -> NativeGramSet:
        """The set of the keys of every n-gram of `width` bytes of the samples (tgx_corpus_gramset_create).  This corpus is
        only read."""
        h = C.c_void_p()
        check(lib.tgx_corpus_gramset_create(self._h, int(width), int(seed) & (2**64 - 1), 0, stream or None, C.byref(h)))
        return NativeGramSet(h)

    def gram_hits(self, grams: NativeGramSet, d_count: int = 0, d_mask: int = 0, *, stream: int = 0) -> None:
        """Per sample the n-grams whose key is in `grams`, as int64[S], and per byte whether the n-gram that begins there
        is one, as u8[N], into caller-owned device memory (either may be 0; tgx_corpus_gram_hits_device).  This corpus is
        only read."""
        check(lib.tgx_corpus_gram_hits_device(self._h, grams._h, 0, stream or None, d_count or None, d_mask or None))

    def phrase_hits(self, phrases: "NativePhraseSet", d_count: int = 0, d_longest: int = 0, d_per_phrase: int = 0, *, stream: int = 0) -> None:
        """Per sample the occurrences of the phrases of `phrases`, as int64[S], per byte the longest occurrence that
        begins there, as u8[N], and per phrase its occurrences, as int64[P], into caller-owned device memory (any may be
        0, not all; tgx_corpus_phrase_hits_device).  This corpus is only read."""
        check(lib.tgx_corpus_phrase_hits_device(self._h, phrases._h, 0, stream or None, d_count or None, d_longest or None, d_per_phrase or None))

    def repeat_stats(self, width: int, seed: int = 0, d_stats: int = 0, d_mask: int = 0, *, stream: int = 0) -> None:
        """Per sample the repetition statistics of its n-grams of `width` bytes, as int64[6, S], and per byte whether a
        repeat (bit 0) or a member of a class of two or more (bit 1) begins there, as u8[N], into caller-owned device
        memory (either may be 0; tgx_corpus_repeat_stats_device).  This corpus is only read."""
        check(lib.tgx_corpus_repeat_stats_device(self._h, int(width), int(seed) & (2**64 - 1), 0, stream or None, d_stats or None, d_mask or None))

    def text_stats(self, d_stats: int = 0, d_line_start: int = 0, line_limit: int = 1000, unit: str = "char", *, stream: int = 0) -> None:
        """Per sample the eleven statistics of include/tgx.h as int64[11, S] (TEXTSTAT_NAMES; lengths in `unit`, "char" or
        "byte"), and per byte whether a line begins there, as u8[N], into caller-owned device memory (either may be 0;
        tgx_corpus_text_stats_device).  This corpus is only read."""
        check(lib.tgx_corpus_text_stats_device(self._h, int(line_limit), textstat_flags(unit), stream or None, d_stats or None, d_line_start or None))

    def word_stats(self, d_stats: int = 0, d_marks: int = 0, word_limit: int = 20, stop_words=GOPHER_STOP_WORDS, unit: str = "char",
                   fold_case: bool = True, *, stream: int = 0) -> None:
        """Per sample the fourteen word statistics of include/tgx_words.h as int64[14, S] (WORDSTAT_NAMES; word lengths in
        `unit`, "char" or "byte"), and per byte its marks (WORD_MARK_*), as u8[N], into caller-owned device memory (either
        may be 0; tgx_corpus_word_stats_device).  stop_words: at most 63 words of 1 to 8 bytes.  This corpus is only read."""
        sflat, soffs, n_stop = _stop_table(stop_words)
        check(lib.tgx_corpus_word_stats_device(self._h, int(word_limit), ptr(sflat) if sflat.size else None, ptr(soffs), n_stop,
                                               wordstat_flags(unit, fold_case), stream or None, d_stats or None, d_marks or None))

    def lines(self, *, stream: int = 0) -> "NativeCorpus":
        """A new resident corpus whose samples are the lines of this one, in order, each with its '\\n' if it has one
        (tgx_corpus_lines).  This corpus is only read."""
        hc = C.c_void_p()
        check(lib.tgx_corpus_lines(self._h, 0, stream or None, C.byref(hc)))
        c = NativeCorpus.__new__(NativeCorpus)
        c._h = hc
        c.device = self.device
        return c

    def normalize(self, form: str) -> "NativeCorpus":
        """The corpus under a Unicode normalisation form ("nfd", "nfc", "nfkd", "nfkc") on the device (tgx_corpus_normalize,
        csrc/norm.hip) -> a resident corpus of the same rows with normalize_flat's bytes; .n_pieces says how many stretches
        were rewritten (0: a device-to-device copy).  This corpus is only read.  A row whose stream window overflows raises
        ERR_UNSUPPORTED with the lowest such row as .sample."""
        hc, k = C.c_void_p(), C.c_uint64()
        _check_norm(lib.tgx_corpus_normalize(self._h, NORMAL_FORMS[form], C.byref(hc), C.byref(k)))
        c = NativeCorpus.__new__(NativeCorpus)
        c._h = hc
        c.device = self.device
        c.n_pieces = k.value
        return c


class NativeModel:
    """Owns a tgx_model: Model::from(vocab) flattened into HBM (src/model.rs:16-30)."""

    def __init__(self, tokens: list[bytes], scores, device: int = 0, for_estep: bool = False):
        flat, offs = pack(tokens)
        self._scores = np.ascontiguousarray(scores, dtype=np.float64)
        if self._scores.shape[0] != len(tokens):
            raise ValueError("scores and tokens differ in length")
        h = C.c_void_p()
        check(lib.tgx_model_create_ex(ptr(flat) if flat.size else None, ptr(offs), ptr(self._scores),
                                      len(tokens), device, 1 if for_estep else 0, C.byref(h)))
        self._h = h
        self.device = device

    @classmethod
    def create_plain(cls, tokens: list[bytes], scores, device: int = 0) -> "NativeModel":
        """The same model through tgx_model_create, the entry point without flags."""
        flat, offs = pack(tokens)
        m = cls.__new__(cls)
        m._scores = np.ascontiguousarray(scores, dtype=np.float64)
        if m._scores.shape[0] != len(tokens):
            raise ValueError("scores and tokens differ in length")
        h = C.c_void_p()
        check(lib.tgx_model_create(ptr(flat) if flat.size else None, ptr(offs), ptr(m._scores), len(tokens), device, C.byref(h)))
        m._h, m.device = h, device
        return m

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_h", None):
            lib.tgx_model_destroy(self._h)
            self._h = None

    def derive(self, keep_ids, scores, for_estep: bool = False) -> "NativeModel":
        """A model for the subset `keep_ids` (ascending ids of this model's tokens) with new scores, on this model's
        tables (tgx_model_create_derived): what prune builds per EM sub-iteration, without rebuilding the tries.
        Raises TokenGeeXError (unsupported) when this vocabulary has duplicate tokens."""
        keep = np.ascontiguousarray(keep_ids, dtype=np.uint32)
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        if sc.shape[0] != keep.shape[0]:
            raise ValueError("scores and keep_ids differ in length")
        h = C.c_void_p()
        check(lib.tgx_model_create_derived(self._h, ptr(keep), keep.shape[0], ptr(sc), 1 if for_estep else 0, C.byref(h)))
        m = NativeModel.__new__(NativeModel)
        m._scores = sc
        m._h = h
        m.device = self.device
        return m

    @property
    def vocab_size(self) -> int:
        return lib.tgx_model_vocab_size(self._h)

    @property
    def max_token_len(self) -> int:
        return lib.tgx_model_max_token_len(self._h)

    @property
    def trie_bytes(self) -> int:
        return lib.tgx_model_trie_bytes(self._h)

    def encode_batch_flat(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0,
                          seed: int = 0) -> NativeResult:
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.tgx_encode_batch(self._h, ptr(flat) if flat.size else None, ptr(offs),
                                   offs.shape[0] - 1, float(dropout), seed & (2**64 - 1), C.byref(h)))
        return NativeResult(h)

    def encode_batch_host(self, flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0, seed: int = 0,
                          ids_out: np.ndarray | None = None):
        """Host buffers in, host buffers out, with upload / kernels / download of the batch's chunks overlapped
        (tgx_encode_batch_host) -> (ids uint32[T] — a view of ids_out when given —, offsets uint64[S+1])."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        if ids_out is None:
            ids_out = np.empty(max(1, int(offs[-1] - offs[0])), np.uint32)
        assert ids_out.dtype == np.uint32 and ids_out.flags.c_contiguous
        out_offs = np.zeros(n + 1, np.uint64)
        t = C.c_uint64()
        check(lib.tgx_encode_batch_host(self._h, ptr(flat) if flat.size else None, ptr(offs), n, float(dropout),
                                        seed & (2**64 - 1), ptr(ids_out), ids_out.size, ptr(out_offs), C.byref(t)))
        return ids_out[: t.value], out_offs

    @staticmethod
    def encode_batch_multi(models: "list[NativeModel]", flat: np.ndarray, offs: np.ndarray, dropout: float = 0.0, seed: int = 0):
        """One batch over several model handles — one per GPU — from this one process (tgx_encode_batch_multi): byte-balanced
        shards, a host thread per handle, ids and offsets packed in sample order -> (ids uint32[T], offsets uint64[S+1])."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        ids_out = np.empty(max(1, int(offs[-1] - offs[0])), np.uint32)
        out_offs = np.zeros(n + 1, np.uint64)
        handles = (C.c_void_p * len(models))(*[m._h for m in models])
        t = C.c_uint64()
        check(lib.tgx_encode_batch_multi(handles, len(models), ptr(flat) if flat.size else None, ptr(offs), n, float(dropout),
                                         seed & (2**64 - 1), ptr(ids_out), ids_out.size, ptr(out_offs), C.byref(t)))
        return ids_out[: t.value], out_offs

    def prune_alternatives(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """FlatTrie.prune_alternatives for this model's vocabulary, over the model's own table
        -> (always_keep u8[V], alt_offs u32[V+1], alt_ids u32[...]) — src/prune.rs:179-203."""
        V = self.vocab_size
        always_keep = np.zeros(V, np.uint8)
        alt_offs = np.zeros(V + 1, np.uint32)
        p = C.c_void_p()
        check(lib.tgx_model_prune_alternatives(self._h, ptr(always_keep), ptr(alt_offs), C.byref(p)))
        k = int(alt_offs[V])
        ids = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(max(k, 1),))[:k].copy()
        lib.tgx_free(p)
        return always_keep, alt_offs, ids

    def encode_corpus(self, corpus: NativeCorpus, dropout: float = 0.0, seed: int = 0) -> NativeResult:
        h = C.c_void_p()
        check(lib.tgx_encode_corpus(self._h, corpus._h, float(dropout), seed & (2**64 - 1), C.byref(h)))
        return NativeResult(h)

    def encode_batch_sample_flat(self, flat: np.ndarray, offs: np.ndarray, alpha: float, seed: int,
                                 return_logz: bool = False):
        """One segmentation per sample drawn from the lattice under temperature alpha (tgx_encode_batch_sample)
        -> NativeResult, or (NativeResult, logz f64[S]) with return_logz."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        logz = np.zeros(max(n, 1), np.float64) if return_logz else None
        h = C.c_void_p()
        check(lib.tgx_encode_batch_sample(self._h, ptr(flat) if flat.size else None, ptr(offs), n, float(alpha),
                                          seed & (2**64 - 1), ptr(logz) if return_logz else None, C.byref(h)))
        return (NativeResult(h), logz[:n]) if return_logz else NativeResult(h)

    def lattice_stats_flat(self, flat: np.ndarray, offs: np.ndarray, alpha: float = 1.0) -> LatticeStats:
        """log Z, expected score and expected token count of every sample's lattice under temperature alpha, by one
        forward sweep on the device (tgx_lattice_stats_batch).  No sample fails the call: see LatticeStats.no_path."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        out = np.zeros((3, max(n, 1)), np.float64)
        bad = C.c_uint64(0)
        if n <= 0:  # nothing to upload
            return LatticeStats(out[0, :0], out[1, :0], out[2, :0], np.zeros(0, np.uint64), alpha, 0)
        check(lib.tgx_lattice_stats_batch(self._h, ptr(flat) if flat.size else None, ptr(offs), n, float(alpha), ptr(out[0]), ptr(out[1]),
                                          ptr(out[2]), C.byref(bad)))
        return LatticeStats(out[0, :n].copy(), out[1, :n].copy(), out[2, :n].copy(), np.diff(offs), alpha, bad.value)

    def lattice_stats_corpus(self, corpus: NativeCorpus, alpha: float = 1.0) -> LatticeStats:
        """lattice_stats_flat over a resident corpus (tgx_lattice_stats_corpus)."""
        n = corpus.num_samples
        out = np.zeros((3, max(n, 1)), np.float64)
        bad = C.c_uint64(0)
        check(lib.tgx_lattice_stats_corpus(self._h, corpus._h, float(alpha), ptr(out[0]), ptr(out[1]), ptr(out[2]), C.byref(bad)))
        return LatticeStats(out[0, :n].copy(), out[1, :n].copy(), out[2, :n].copy(), np.diff(corpus.offsets()), alpha, bad.value)

    def assemble(self, segs: "NativeResult | None", seg_offs: np.ndarray, seg_special: np.ndarray, n_specials: int) -> NativeResult:
        """The sample-level result of a batch split at special tokens, put together on the device (tgx_assemble_result,
        csrc/assemble.hip): segs is the encode or sampling result over the non-special segments (None when every segment
        is special), seg_offs u64[S+1] / seg_special i32[K] the split plan of split_specials_flat.  Special k gets the id
        vocab_size + k.  segs stays valid and is the caller's to free."""
        seg_offs = np.ascontiguousarray(seg_offs, dtype=np.uint64)
        seg_special = np.ascontiguousarray(seg_special, dtype=np.int32)
        h = C.c_void_p()
        check(lib.tgx_assemble_result(self._h, None if segs is None else segs._h, ptr(seg_offs), ptr(seg_special) if seg_special.size else None,
                                      seg_offs.shape[0] - 1, _u32_arg(n_specials, "n_specials"), C.byref(h)))
        return NativeResult(h)

    def assemble_plan(self, segs: "NativeResult | None", plan: NativePlan, n_specials: int) -> NativeResult:
        """assemble with the plan of NativeCorpus.split_specials, read where it is in HBM (tgx_assemble_result_plan)."""
        h = C.c_void_p()
        check(lib.tgx_assemble_result_plan(self._h, None if segs is None else segs._h, plan._h, _u32_arg(n_specials, "n_specials"), C.byref(h)))
        return NativeResult(h)

    # -- decode on the device (include/tgx.h: tgx_decode_result / tgx_decode_padded; csrc/decode.hip) --
    @staticmethod
    def _specials(special_flat, special_offs):
        sf = np.ascontiguousarray(special_flat, dtype=np.uint8)
        so = np.ascontiguousarray(special_offs, dtype=np.uint64)
        return sf, so, so.shape[0] - 1

    def decode_result(self, result: NativeResult, special_flat, special_offs, include_special: bool, stream: int = 0) -> "NativeText":
        """The rows of a result on this model's device decoded to UTF-8 text in HBM: ids >= vocab_size are the special tokens
        (special_flat / special_offs: their bytes in the batch format), every run of base ids between them goes through
        String::from_utf8_lossy on its own.  Queued on `stream` (a hipStream_t as an integer; 0: the library's blocking
        stream); returns when the stream has reached its end.  The result is only read."""
        sf, so, n = self._specials(special_flat, special_offs)
        h, bs, bi = C.c_void_p(), C.c_uint64(), C.c_uint64()
        st = lib.tgx_decode_result(self._h, result._h, ptr(sf) if sf.size else None, ptr(so), n, 1 if include_special else 0,
                                   stream or None, C.byref(h), C.byref(bs), C.byref(bi))
        if st != OK:
            _raise_decode(st, bs.value, bi.value)
        return NativeText(h)

    def decode_padded(self, ids_ptr: int, n_rows: int, row_len: int, i64: bool, *, mask_ptr: int = 0, lengths_ptr: int = 0,
                      skip_id: int | None = None, special_flat=(), special_offs=(0,), include_special: bool = True,
                      stream: int = 0) -> "NativeText":
        """[n_rows, row_len] ids in device memory (int32, or int64 with i64; raw integer pointers) decoded as decode_result
        does.  An element is live iff its mask byte (u8 [n_rows, row_len]) is non-zero, its column is below its row's
        length (i32[n_rows]) and it differs from skip_id — each test only when given; other elements are absent."""
        sf, so, n = self._specials(special_flat, special_offs)
        h, bs, bi = C.c_void_p(), C.c_uint64(), C.c_uint64()
        st = lib.tgx_decode_padded(self._h, ids_ptr or None, int(n_rows), int(row_len), LAYOUT_I64 if i64 else 0, mask_ptr or None,
                                   lengths_ptr or None, _id_or_none(skip_id), ptr(sf) if sf.size else None, ptr(so), n,
                                   1 if include_special else 0, stream or None, C.byref(h), C.byref(bs), C.byref(bi))
        if st != OK:
            _raise_decode(st, bs.value, bi.value)
        return NativeText(h)

    # -- token spans on the device (include/tgx.h: tgx_result_spans_device / tgx_result_pad_spans_device; csrc/spans.hip) --
    def result_spans(self, result: NativeResult, special_flat, special_offs, spans_ptr: int, *, flags: int = 0, stream: int = 0) -> None:
        """The span of every token of a result on this model's device in its row's text, written by the device into
        caller-owned device memory given as a raw integer pointer: [num_tokens, 2] int32, or int64 with LAYOUT_I64 in flags;
        SPAN_CHARS counts code points instead of bytes (span_flags puts the flags together).  ids >= vocab_size are the
        special tokens, as in decode_result.  Queued on `stream` (0: the library's blocking stream); returns when the
        stream has reached its end.  The result is only read."""
        sf, so, n = self._specials(special_flat, special_offs)
        check(lib.tgx_result_spans_device(self._h, result._h, ptr(sf) if sf.size else None, ptr(so), n, _u32_arg(flags, "flags"),
                                          stream or None, spans_ptr or None))

    def result_pad_spans(self, result: NativeResult, special_flat, special_offs, row_len: int, spans_ptr: int, *, bos_id: int | None = None,
                         eos_id: int | None = None, flags: int = 0, stream: int = 0) -> None:
        """result_spans in the padded form: [num_samples, row_len, 2], aligned element for element with what
        NativeResult.pad_device writes for the same row_len, bos_id, eos_id and side flags; bos, eos and padding get
        (0, 0)."""
        sf, so, n = self._specials(special_flat, special_offs)
        check(lib.tgx_result_pad_spans_device(self._h, result._h, ptr(sf) if sf.size else None, ptr(so), n, _u32_arg(row_len, "row_len"),
                                              _id_or_none(bos_id), _id_or_none(eos_id), _u32_arg(flags, "flags"), stream or None,
                                              spans_ptr or None))

    def encode_corpus_sample(self, corpus: NativeCorpus, alpha: float, seed: int, return_logz: bool = False):
        """encode_batch_sample_flat over a resident corpus (tgx_encode_corpus_sample)."""
        n = corpus.num_samples
        logz = np.zeros(max(n, 1), np.float64) if return_logz else None
        h = C.c_void_p()
        check(lib.tgx_encode_corpus_sample(self._h, corpus._h, float(alpha), seed & (2**64 - 1),
                                           ptr(logz) if return_logz else None, C.byref(h)))
        return (NativeResult(h), logz[:n]) if return_logz else NativeResult(h)

    def encode_batch_nbest_flat(self, flat: np.ndarray, offs: np.ndarray, nbest: int):
        """The nbest highest-scoring segmentations of every sample (tgx_encode_batch_nbest) -> (NativeResult of S·nbest
        rows, row s·nbest + r the r-th best of sample s; scores f64[S·nbest], -inf past n_found; n_found u32[S])."""
        flat = np.ascontiguousarray(flat, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = offs.shape[0] - 1
        scores = np.empty(max(n * int(nbest), 1), np.float64)
        n_found = np.empty(max(n, 1), np.uint32)
        h = C.c_void_p()
        check(lib.tgx_encode_batch_nbest(self._h, ptr(flat) if flat.size else None, ptr(offs), n, int(nbest), ptr(scores),
                                         ptr(n_found), C.byref(h)))
        return NativeResult(h), scores[:n * int(nbest)], n_found[:n]

    def encode_corpus_nbest(self, corpus: NativeCorpus, nbest: int):
        """encode_batch_nbest_flat over a resident corpus (tgx_encode_corpus_nbest)."""
        n = corpus.num_samples
        scores = np.empty(max(n * int(nbest), 1), np.float64)
        n_found = np.empty(max(n, 1), np.uint32)
        h = C.c_void_p()
        check(lib.tgx_encode_corpus_nbest(self._h, corpus._h, int(nbest), ptr(scores), ptr(n_found), C.byref(h)))
        return NativeResult(h), scores[:n * int(nbest)], n_found[:n]

    def count_tokens(self, corpus: NativeCorpus, freq: np.ndarray | None = None) -> np.ndarray:
        if freq is None:
            freq = np.zeros(self.vocab_size, np.uint64)
        assert freq.dtype == np.uint64 and freq.shape[0] == self.vocab_size and freq.flags.c_contiguous
        check(lib.tgx_count_tokens(self._h, corpus._h, ptr(freq)))
        return freq

    def count_pairs(self, corpus: NativeCorpus) -> tuple[np.ndarray, np.ndarray]:
        keys, counts, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.tgx_count_pairs(self._h, corpus._h, C.byref(keys), C.byref(counts), C.byref(n)))
        k = n.value
        ka = np.ctypeslib.as_array(C.cast(keys, C.POINTER(C.c_uint64)), shape=(max(k, 1),))[:k].copy()
        ca = np.ctypeslib.as_array(C.cast(counts, C.POINTER(C.c_uint64)), shape=(max(k, 1),))[:k].copy()
        lib.tgx_free(keys)
        lib.tgx_free(counts)
        return ka, ca

    def count_pairs_top(self, corpus: NativeCorpus, max_pairs: int) -> tuple[np.ndarray, np.ndarray, int]:
        """The max_pairs most frequent pairs, by descending count then ascending key -> (keys, counts, n_total)."""
        keys, counts, n, tot = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(lib.tgx_count_pairs_top(self._h, corpus._h, int(max_pairs), C.byref(keys), C.byref(counts),
                                      C.byref(n), C.byref(tot)))
        k = n.value
        ka = np.ctypeslib.as_array(C.cast(keys, C.POINTER(C.c_uint64)), shape=(max(k, 1),))[:k].copy()
        ca = np.ctypeslib.as_array(C.cast(counts, C.POINTER(C.c_uint64)), shape=(max(k, 1),))[:k].copy()
        lib.tgx_free(keys)
        lib.tgx_free(counts)
        return ka, ca, tot.value

    def estep(self, corpus: NativeCorpus, snippet_len: int = ESTEP_SNIPPET_LEN, dropout: float = 0.0,
              seed: int = 0, expected: np.ndarray | None = None) -> tuple[np.ndarray, float]:
        if expected is None:
            expected = np.zeros(self.vocab_size, np.float64)
        assert expected.dtype == np.float64 and expected.shape[0] == self.vocab_size
        z = C.c_double()
        check(lib.tgx_estep(self._h, corpus._h, snippet_len, float(dropout), seed & (2**64 - 1),
                            ptr(expected), C.byref(z)))
        return expected, z.value

    def common_prefix_search(self, s: bytes) -> list[tuple[int, int]]:
        buf = np.frombuffer(s, dtype=np.uint8)
        cap = len(s) + 1
        ids, lens = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        cnt = C.c_uint64()
        check(lib.tgx_common_prefix_search(self._h, ptr(buf) if len(s) else None, len(s), ptr(ids),
                                           ptr(lens), cap, C.byref(cnt)))
        return [(int(ids[i]), int(lens[i])) for i in range(cnt.value)]

    def last_kernel_times(self) -> dict[str, float]:
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        n = lib.tgx_last_kernel_times(self._h, names, ms, 8)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    def last_algorithmic_bytes(self) -> int:
        return lib.tgx_last_algorithmic_bytes(self._h)

    def last_encode_waves_per_cu(self) -> int:
        return lib.tgx_last_encode_waves_per_cu(self._h)

    def last_encode_redo_samples(self) -> int:
        return lib.tgx_last_encode_redo_samples(self._h)

    def score_values(self) -> int:
        return lib.tgx_model_score_values(self._h)

    def last_encode_hot_values(self) -> int:
        return lib.tgx_last_encode_hot_values(self._h)

    def last_encode_lean_items(self) -> tuple[int, int]:
        """(encode5_kernel's, encode6_kernel's) lean items of the last rows5 encode pass: masks of 1 = lean relaxation step,
        2 = builtin broadcast, 4 = one-instruction score fetch; 0: the kernel as it was, or
        not launched (a self-check: results do not depend on it)."""
        v = lib.tgx_last_encode_lean_items(self._h)
        return v & 0xFF, (v >> 8) & 0xFF

    def last_encode_lean_step(self) -> bool:
        """Whether encode5_kernel relaxed with the lean step in the last pass (last_encode_lean_items)."""
        return bool(self.last_encode_lean_items()[0] & 1)

    def last_encode_ids_in_place(self) -> bool:
        """Whether the last encode pass wrote its ids in place: token counts from encode5_kernel's relaxation, no scratch
        of 4 bytes per text byte, no compact_kernel (a self-check: results do not depend on it)."""
        return bool(lib.tgx_last_encode_ids_in_place(self._h))

    def last_encode_top_table(self) -> bool:
        """Whether the last pass's encode5_kernel was a top-table build: a walk's first two trie levels from one table
        indexed by the first two text bytes, no copy of the root's records in LDS (a self-check: results do not depend
        on it)."""
        return bool(lib.tgx_last_encode_top_table(self._h))

    def last_encode_long_samples(self) -> int:
        return lib.tgx_last_encode_long_samples(self._h)

    def last_estep_pieces(self) -> int:
        return lib.tgx_last_estep_pieces(self._h)

    def last_estep_redo(self) -> int:
        return lib.tgx_last_estep_redo(self._h)

    def last_encode_corun_cus(self) -> int:
        return lib.tgx_last_encode_corun_cus(self._h)

    def encode_corun_timeouts(self) -> int:
        return lib.tgx_encode_corun_timeouts(self._h)


class FlatTrie:
    """Host-only build of the device trie layout (tgx_flat_trie_*), no GPU needed."""

    def __init__(self, tokens: list[bytes], scores):
        flat, offs = pack(tokens)
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        h = C.c_void_p()
        check(lib.tgx_flat_trie_build(ptr(flat) if flat.size else None, ptr(offs), ptr(sc), len(tokens),
                                      C.byref(h)))
        self._h = h
        self._flat, self._offs, self._sc = flat, offs, sc

    def common_prefix_search8(self, s: bytes, max_hot: int = 6600):
        """The search over the 8-byte label-checked records of encode5_kernel -> (matches, stats)."""
        buf = np.frombuffer(s, dtype=np.uint8)
        cap = len(s) + 1
        ids, lens = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        nh, nc, cov = C.c_uint32(), C.c_uint64(), C.c_double()
        k = lib.tgx_flat_trie_search8(self._h, ptr(self._flat) if self._flat.size else None, ptr(self._offs), ptr(self._sc),
                                      max_hot, ptr(buf) if len(s) else None, len(s), ptr(ids), ptr(lens), cap,
                                      C.byref(nh), C.byref(nc), C.byref(cov))
        if k == 2**64 - 1:
            raise TokenGeeXError("8-byte records need fewer than 2^23 slots")
        return [(int(ids[i]), int(lens[i])) for i in range(k)], {"n_hot": nh.value, "n_cold": nc.value, "hot_coverage": cov.value}

    def __del__(self):
        if getattr(self, "_h", None):
            lib.tgx_flat_trie_free(self._h)
            self._h = None

    def common_prefix_search(self, s: bytes) -> list[tuple[int, int]]:
        buf = np.frombuffer(s, dtype=np.uint8)
        cap = len(s) + 1
        ids, lens = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        k = lib.tgx_flat_trie_search(self._h, ptr(buf) if len(s) else None, len(s), ptr(ids), ptr(lens), cap)
        return [(int(ids[i]), int(lens[i])) for i in range(k)]

    def stats(self) -> dict:
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        lib.tgx_flat_trie_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"n_slots": a.value, "n_nodes": b.value, "max_token_len": c.value,
                "fill": b.value / max(1, a.value)}

    @property
    def max_token_len(self) -> int:
        return self.stats()["max_token_len"]

    def table(self):
        """-> (check, base_flags, tokid) uint32 arrays of n_slots entries."""
        n = self.stats()["n_slots"]
        check, base, tokid = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        lib.tgx_flat_trie_copy(self._h, ptr(check), ptr(base), ptr(tokid))
        return check, base, tokid


    # ---- host half of `prune` (src/prune.rs) ----
    def prune_alternatives(self, tokens: list[bytes], scores) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (always_keep u8[V], alt_offs u32[V+1], alt_ids u32[...]) — src/prune.rs:179-203."""
        flat, offs = pack(tokens)
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        V = len(tokens)
        always_keep = np.zeros(V, np.uint8)
        alt_offs = np.zeros(V + 1, np.uint32)
        p = C.c_void_p()
        check(lib.tgx_prune_alternatives(self._h, ptr(flat) if flat.size else None, ptr(offs), ptr(sc), V,
                                         ptr(always_keep), ptr(alt_offs), C.byref(p)))
        k = int(alt_offs[V])
        ids = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(max(k, 1),))[:k].copy()
        lib.tgx_free(p)
        return always_keep, alt_offs, ids


def tok_hash_selftest(tokens: list[bytes]) -> tuple[int, int]:
    """-> (seed, mismatches) of the bytes -> id table built for `tokens` (host only)."""
    flat, offs = pack(tokens)
    seed, bad = C.c_uint32(), C.c_uint64()
    check(lib.tgx_tok_hash_selftest(ptr(flat) if flat.size else None, ptr(offs), len(tokens), C.byref(seed), C.byref(bad)))
    return seed.value, bad.value


def digamma(x: float) -> float:
    return lib.tgx_digamma(x)


def prune_m_step(expected: np.ndarray, keep: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """run_m_step — src/prune.rs:124-170 -> (surviving ids, new scores)."""
    expected = np.ascontiguousarray(expected, dtype=np.float64)
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    V = expected.shape[0]
    idx, sc, n = np.zeros(max(V, 1), np.uint32), np.zeros(max(V, 1), np.float64), C.c_uint32()
    check(lib.tgx_prune_m_step(ptr(expected), ptr(keep), V, ptr(idx), ptr(sc), C.byref(n)))
    return idx[:n.value].copy(), sc[:n.value].copy()


def prune_select(freq, keep, always_keep, alt_offs, alt_ids, scores, n_samples: int,
                 pruned_size: int) -> np.ndarray:
    """Loss-based selection — src/prune.rs:246-318 -> ids of the pruned vocabulary, final order."""
    freq = np.ascontiguousarray(freq, dtype=np.uint64)
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    always_keep = np.ascontiguousarray(always_keep, dtype=np.uint8)
    alt_offs = np.ascontiguousarray(alt_offs, dtype=np.uint32)
    alt_ids = np.ascontiguousarray(alt_ids, dtype=np.uint32)
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    V = freq.shape[0]
    out, n = np.zeros(max(V, 1), np.uint32), C.c_uint32()
    check(lib.tgx_prune_select(ptr(freq), ptr(keep), ptr(always_keep), ptr(alt_offs),
                               ptr(alt_ids) if alt_ids.size else None, ptr(scores), V, n_samples,
                               pruned_size, ptr(out), C.byref(n)))
    return out[:n.value].copy()


def dropout_u01(seed: int, sample: int, pos: int, length: int) -> float:
    return lib.tgx_dropout_u01_host(seed, sample, pos, length)


def sample_u01(seed: int, sample: int, pos: int, length: int) -> float:
    return lib.tgx_sample_u01(seed, sample, pos, length)


def sample_u01_array(seed: int, sample: np.ndarray, pos: np.ndarray, length: np.ndarray) -> np.ndarray:
    """tgx_sample_u01 over arrays (numpy u64 arithmetic wraps as the C code does)."""
    with np.errstate(over="ignore"):
        x = (np.uint64(seed & (2**64 - 1)) ^ np.uint64(0xD6E8FEB86659FD93)
             ^ (np.asarray(sample, np.uint64) * np.uint64(0x9E3779B97F4A7C15))
             ^ (np.asarray(pos, np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
             ^ (np.asarray(length, np.uint64) * np.uint64(0x165667B19E3779F9)))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return np.minimum(u, np.nextafter(1.0, 0.0))
