// Whether an encode pass writes its ids in place, host side: the decision as a pure function, and the
// host twin of the arithmetic by which encode5_kernel's counting builds carry a position's token count through the
// relaxation (device_common.h: relax5_count_cand).
#pragma once
#include <stdint.h>

namespace tgx {

// The winner word of a counting build is count << 8 | step: 24 bits of count.  A sample has at most one token per byte,
// and no position's count exceeds the position, so samples shorter than this cannot overflow the field.
constexpr uint64_t kCountFieldSamples = 1ull << 24;

// What a pass knows when it decides (encode_pass.cpp: choose_encode5)
struct IdsInPlaceQuery {
    bool rows5;          // the pass runs encode5_kernel / encode6_kernel (8-byte records, ranked values)
    bool long_tokens;    // tokens of 17..32 bytes: the LONG build, trace32_kernel
    bool dropout;        // a dropout pass
    uint64_t n_long;     // samples that go to encode6_kernel (alone or beside encode5_kernel)
    bool build_counts;   // the chosen build of encode5_kernel counts tokens (kernels.h: encode5_counts)
    uint64_t max_len;    // bytes of the batch's longest sample
    bool switched_on;    // TGX_IDS_IN_PLACE is not 0
    bool diagnostics;    // timing-experiment flags or stamps are set: those kernels skip work the count relies on
};

// In place: encode5_kernel leaves every sample's token count, the counts are scanned into the result's offsets, and
// trace_kernel writes the ids where they belong — no `tmp`, no compact_kernel.  Every term must hold; otherwise the
// pass runs as it always did (trace into `tmp`, scan, compaction).
inline bool ids_in_place(const IdsInPlaceQuery& q) {
    return q.rows5 && !q.long_tokens && !q.dropout && q.n_long == 0 && q.build_counts && q.max_len < kCountFieldSamples &&
           q.switched_on && !q.diagnostics;
}

// One relaxation step's candidate word: the winner of step `u` (0..15) comes from the position whose final word is
// `from`, and offers that position's count plus one with `u` as the step.
inline uint32_t count_step_word(uint32_t from, uint32_t u) { return (from | 0xFFu) + (1u + u); }
inline uint32_t count_of_word(uint32_t word) { return word >> 8; }
constexpr uint32_t kCountNoStep = 0xFFu;  // device_common.h: kNoStep — a sample's first position: count 0

}  // namespace tgx
