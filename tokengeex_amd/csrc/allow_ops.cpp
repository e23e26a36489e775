// The C ABI's document-frequency pass under an allow automaton (include/tgx_allow.h: tgx_substring_df_allow,
// tgx_allow_last_times): the automaton's check, the table's build and upload, the masks and the chunks' counts around the
// launchers of allow.hip, and the stages' times.  The arguments' checks, the uploads, the scan and everything from the sort
// on are generate.h's, the functions tgx_substring_df_top runs too; like it the call works on the default stream and is
// synchronous.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tgx_allow.h"
#include "allow.h"
#include "api_internal.h"
#include "device_internal.h"
#include "generate.h"

using namespace tgx::host;
using namespace tgx::dev;

namespace {

const char* const kAllowStageNames[tgx::kGenerateStages] = {"allow_mask_kernel", "allow_scan", "allow_emit_kernel", "allow_sort", "allow_runs", "allow_top"};
thread_local float g_allow_ms[tgx::kGenerateStages] = {0, 0, 0, 0, 0, 0};

tgx_status allow_fail(tgx::GenerateScratch& scratch, tgx_status st, const char* msg) {
    (void)hipDeviceSynchronize();
    scratch.release();
    return fail(st, "%s", msg);
}

}  // namespace

int tgx_allow_last_times(const char** names, float* ms, int cap) { return stage_times(kAllowStageNames, g_allow_ms, tgx::kGenerateStages, names, ms, cap); }

tgx_status tgx_substring_df_allow(int device, const uint8_t* text, uint64_t n_bytes, const uint64_t* part_begin, const uint64_t* part_end,
                                  const uint32_t* part_sample, const uint64_t* part_origin, uint64_t n_parts, uint32_t max_token_length,
                                  double insert_probability, uint64_t seed, const tgx_dfa64* allow, uint64_t top_k, uint64_t** out_pos, uint32_t** out_len,
                                  uint32_t** out_df, uint64_t* n_out, uint64_t* n_windows, uint64_t* n_collisions, uint64_t* n_distinct, uint32_t* cutoff_df) {
    const char* who = "tgx_substring_df_allow";
    const tgx::GenerateArgs a{device,   text,  n_bytes, part_begin, part_end, part_sample, part_origin,  n_parts,    max_token_length, insert_probability,
                              seed,     top_k, out_pos, out_len,    out_df,   n_out,       n_windows,    n_collisions, n_distinct,     cutoff_df};
    bool empty = false;
    tgx_status st = tgx::substring_df_check(a, &empty);
    if (st != TGX_OK) return st;
    if (!allow) return fail(TGX_ERR_INVALID, "%s: allow is NULL", who);
    if (const char* why = tgx::dfa64_check(allow->n_states, allow->start, allow->next, allow->tag)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    if (empty) return TGX_OK;
    tgx::GenerateScratch scratch;
    tgx::GenerateInput in{};
    if ((st = tgx::substring_df_upload(a, scratch, &in)) != TGX_OK) return st;
    const uint64_t n_chunks = tgx::allow_chunks(n_bytes);
    std::vector<uint8_t> table(tgx::kFindTableBytes);
    tgx::find_build_table(allow->n_states, allow->next, allow->tag, table.data());
    uint8_t* d_table = (uint8_t*)scratch.alloc(tgx::kFindTableBytes);
    uint32_t* d_mask = (uint32_t*)scratch.alloc((size_t)n_bytes * 4);
    uint32_t* d_count = (uint32_t*)scratch.alloc((size_t)n_chunks * 4);
    uint64_t* d_offs = (uint64_t*)scratch.alloc((size_t)(n_chunks + 1) * 8);
    if (!d_table || !d_mask || !d_count || !d_offs) return allow_fail(scratch, TGX_ERR_DEVICE, "out of device memory (generate: allow)");
    if (hipMemcpy(d_table, table.data(), tgx::kFindTableBytes, hipMemcpyHostToDevice) != hipSuccess)
        return allow_fail(scratch, TGX_ERR_DEVICE, "tgx_substring_df_allow: upload of the table failed");
    tgx::AllowParams P{};
    P.text = in.text;
    P.n_bytes = n_bytes;
    P.part_begin = in.part_begin;
    P.part_end = in.part_end;
    P.part_origin = in.part_origin;
    P.part_sample = in.part_sample;
    P.n_parts = n_parts;
    P.blk_part = in.blk_part;
    P.max_len = max_token_length;
    P.start = allow->start;
    P.prob = insert_probability;
    P.seed = seed;
    P.table = d_table;
    P.mask = d_mask;
    P.chunk_count = d_count;
    P.chunk_offs = d_offs;
    float ms[tgx::kGenerateStages] = {0, 0, 0, 0, 0, 0};
    tgx::GenerateTimer timer(nullptr, ms);
    timer.begin(tgx::kGenStageCount);
    if (tgx::launch_allow_mask(P, nullptr) != hipSuccess) return allow_fail(scratch, TGX_ERR_DEVICE, "allow_mask_kernel launch failed");
    timer.end(tgx::kGenStageCount);
    uint64_t M = 0;
    timer.begin(tgx::kGenStageScan);
    if ((st = tgx::substring_df_offsets(scratch, d_count, d_offs, n_chunks, &M)) != TGX_OK) return st;
    timer.end(tgx::kGenStageScan);
    st = tgx::substring_df_tail(a, scratch, in, M, [&](uint64_t salt, uint64_t key_mask, uint64_t* keys, uint64_t* vals) {
        P.salt = salt;
        P.key_mask = key_mask;
        P.keys = keys;
        P.vals = vals;
        return tgx::launch_allow_emit(P, nullptr);
    }, &timer);
    if (st != TGX_OK) return st;
    if (hipDeviceSynchronize() != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: the device failed after the result was read", who);
    timer.read();
    std::copy(ms, ms + tgx::kGenerateStages, g_allow_ms);
    return TGX_OK;
}
