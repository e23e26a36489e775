// What a pass on a model's own streams (encode_pass.cpp, estep_pass.cpp, lattice_pass.cpp) and the counting passes of
// tgx_api.cpp share, beside device_internal.h: the knobs, the launch arithmetic and the phase stamps of encode and the
// E-step, and the scratch, all from tgx_api.cpp; the encode parameters, the tables, the encode pass under the caller's
// locks and the end of a pass, which the lattice and counting passes share with encode, from encode_pass.cpp.
// Everything is DEFINED once (as device_internal.h requires of what has state: knob(), debug_on() and debug_flags()
// read the environment once), except the one template.  result_ops.cpp and corpus_ops.cpp run on a caller's stream
// and do not include this.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "device_internal.h"
#include "kernels.h"

namespace tgx::dev {

// ---- knobs (tgx_api.cpp) ---------------------------------------------------------------
// TGX_DEBUG=1: every launch logged to stderr and waited for
bool debug_on();
// an environment switch among the library's kernels and geometries; NULL unless the process opted in (TGX_KNOBS=1)
const char* knob(const char* name);
// an integer knob that holds only inside [lo, hi]
void knob_int(const char* name, int lo, int hi, int* x);
// TGX_E5_HOT / TGX_E7_HOT: a smaller LDS copy than fits
uint32_t knob_cap_hot(const char* name, uint32_t n_hot);
// TGX_FLAGS (timing experiments; with TGX_DEBUG=1 only)
uint32_t debug_flags();

// ---- launch arithmetic (tgx_api.cpp) -----------------------------------------------------
// blocks of the trace kernels: four samples per block and round, eight blocks per CU
uint32_t trace_blocks(const tgx_model* m, uint64_t n_samples);
// fewer waves (of four rows) per block when the pass has fewer units than the chip has rows
int waves_for_units(int waves, uint64_t units, uint64_t n_blocks);
// consecutive units of the order that a row claims per atomic
uint32_t claim_chunk_for(uint64_t n_bytes, uint64_t units);

// Phase stamps of a kernel's waves (diagnosis; TGX_STAMPS=<which> with TGX_DEBUG=1): 64 bytes per wave, cleared, owned by
// the pass.  d == nullptr: not asked for, or not to be had.
struct Stamps {
    unsigned long long* d = nullptr;
    size_t n_waves = 0;
};
Stamps stamps_begin(tgx_model* m, Pass& pass, char which, size_t n_waves);
void stamps_report(tgx_model* m, const Stamps& st, int ppl, const char* what, const char* unit, std::initializer_list<const char*> phases);

// ---- what sampling, statistics, n-best and the counting passes share with encode (encode_pass.cpp) ------------
// the corpus's scratch: back-pointers, counts, status and (with_tmp) the right-aligned ids (tgx_api.cpp)
tgx_status ensure_scratch(tgx_corpus* c, bool with_tmp = true);
// what every encode and sampling kernel is told about the model, the corpus and its scratch
tgx::EncodeParams base_encode_params(const tgx_model* m, const tgx_corpus* c, uint64_t seed);
// the token hash table and the 8-byte records, built at the first pass that reads them; caller holds m->mu
tgx_status ensure_encode_tables(tgx_model* m);
// encode5_kernel's top table (top_table.h) from the trie8 records just written to m->d_trie8: whoever writes those calls this
tgx_status upload_top_table(tgx_model* m, const tgx::Trie8Rec* rec, size_t n_slots, uint32_t root_base);
// m->h_ctrl->err as a status: TGX_ERR_NO_PATH with its error detail, or an internal error
tgx_status check_no_path(tgx_model* m, const tgx_corpus* c);
// counts in c->d_counts and ids right-aligned in c->d_tmp -> r's offsets and ids (the compaction is queued, not waited for)
tgx_status compact_ids(tgx_model* m, tgx_corpus* c, tgx_result* r, const char* what);
// tgx_encode_corpus under the caller's locks (m->mu, c->mu): the counting passes start with it
tgx_status encode_corpus_locked(tgx_model* m, tgx_corpus* c, double dropout, uint64_t seed, tgx_result** out);

// the tgx_encode_batch* entry points: the batch uploaded, `run` over the corpus, the corpus freed
template <class Run>
tgx_status on_uploaded_batch(const tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, Run run) {
    tgx_corpus* c = nullptr;
    tgx_status st = tgx_corpus_upload(m->device, text, offs, n_samples, &c);
    if (st != TGX_OK) return st;
    st = run(c);
    tgx_corpus_free(c);
    return st;
}

}  // namespace tgx::dev
