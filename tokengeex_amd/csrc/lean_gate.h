// The gate of encode5_kernel's / encode6_kernel's lean relaxation step (device_common.h: relax5_lean_step), host side.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace tgx {

// The lean step marks "not reached" with negative values of magnitude >= 2^1023 instead of -inf alone.  A reached
// position's score is a sum of at most one score per byte of its sample, and a sample has fewer than 2^32 bytes (the
// kernels count its positions in 32 bits).  With every score's magnitude at most 2^960 such a sum stays below
// 2^960 * 2^32 = 2^992: 2^31 below the marked class, whatever the corpus — so the gate is a property of the model.
// The same bound keeps a score below half an ulp of a marked value (2^970), which is what keeps that class closed
// under the step's additions.  Anything else (a larger score, an infinity, a NaN) keeps the full step.
constexpr int kLeanScoreExponent = 960;  // a score passes iff |score| < 2^960
// tested on the bits: the biased exponent field is at most 1023 + 959 (infinities and NaNs have 2047)
inline bool lean_score_ok(double score) {
    uint64_t b;
    memcpy(&b, &score, 8);
    return (uint32_t)((b >> 52) & 0x7FFu) <= 1023u + (uint32_t)kLeanScoreExponent - 1u;
}
inline bool lean_scores_ok(const double* scores, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!lean_score_ok(scores[i])) return false;
    return true;
}

}  // namespace tgx
