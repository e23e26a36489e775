// Stand-alone driver of the lean relaxation step's gate (csrc/lean_gate.h) for a sanitizer build:
// tests/test_lean_gate_native.py compiles it under -fsanitize=address,undefined and runs it.  No device is opened.
//
// Besides the gate's verdicts at its edge, the program checks on the host the two facts the device step relies on, with
// the same f64 additions: a path's score cannot reach the marked class when every score passes, and a marked value
// stays marked when a passing score is added to it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../tokengeex_amd/csrc/lean_gate.h"

namespace {

int g_failed = 0;
void expect(bool ok, const char* what) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s\n", what);
}

uint32_t high_word(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return (uint32_t)(b >> 32);
}
double with_high_word(double v, uint32_t hi) {
    uint64_t b;
    memcpy(&b, &v, 8);
    b = (b & 0xFFFFFFFFull) | ((uint64_t)hi << 32);
    memcpy(&v, &b, 8);
    return v;
}
// the device's test (device_common.h: kLeanUnreachedHi) and reset (kLeanResetHi)
bool marked(double v) { return high_word(v) >= 0xFFE00000u; }

}  // namespace

int main() {
    const double edge = std::ldexp(1.0, tgx::kLeanScoreExponent);  // 2^960
    const double inf = std::numeric_limits<double>::infinity();
    // ---- verdicts
    expect(tgx::lean_score_ok(0.0) && tgx::lean_score_ok(-0.0), "zero passes");
    expect(tgx::lean_score_ok(-12.5) && tgx::lean_score_ok(3.0), "ordinary scores pass");
    expect(tgx::lean_score_ok(std::numeric_limits<double>::denorm_min()), "a denormal passes");
    expect(tgx::lean_score_ok(-std::nextafter(edge, 0.0)) && tgx::lean_score_ok(std::nextafter(edge, 0.0)), "just inside passes");
    expect(!tgx::lean_score_ok(-edge) && !tgx::lean_score_ok(edge), "2^960 does not pass");
    expect(!tgx::lean_score_ok(-std::numeric_limits<double>::max()), "-DBL_MAX does not pass");
    expect(!tgx::lean_score_ok(-inf) && !tgx::lean_score_ok(inf), "infinities do not pass");
    expect(!tgx::lean_score_ok(std::nan("")) && !tgx::lean_score_ok(-std::nan("")), "NaNs do not pass");
    {
        // heap blocks of exactly n elements: reading one score too many is a report
        for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)1000}) {
            std::unique_ptr<double[]> s(new double[n]);
            for (size_t i = 0; i < n; i++) s[i] = -(double)(i % 17) - 0.5;
            expect(tgx::lean_scores_ok(s.get(), n), "a vocabulary of ordinary scores passes");
            if (n) {
                s[n - 1] = -edge;
                expect(!tgx::lean_scores_ok(s.get(), n), "the last score alone fails the vocabulary");
                s[n - 1] = -1.0;
                s[0] = inf;
                expect(!tgx::lean_scores_ok(s.get(), n), "the first score alone fails the vocabulary");
            }
        }
        expect(tgx::lean_scores_ok(nullptr, 0), "an empty vocabulary passes");
    }
    // ---- a path of the longest sample (2^32 - 1 bytes, one token per byte) at the lowest passing score is not marked
    {
        const double low = -std::nextafter(edge, 0.0);
        const double total = low * 4294967295.0;  // the sum's magnitude is at most this product's (plus rounding far below it)
        expect(!marked(total) && total > -std::ldexp(1.0, 993), "the longest path at the lowest score stays below 2^993");
        expect(!marked(-total), "and a positive sum is never marked");
    }
    // ---- the marked class is closed under the step's additions
    {
        const double low = -std::nextafter(edge, 0.0), high = std::nextafter(edge, 0.0);
        const double reset_lo = with_high_word(0.0, 0xFFEFFFFFu), reset_hi = -std::numeric_limits<double>::max();
        expect(marked(reset_lo) && marked(reset_hi) && marked(-inf), "what a lane is reset to is marked, and so is -inf");
        expect(std::fabs(reset_lo) >= std::ldexp(1.0, 1023), "a reset value's magnitude is at least 2^1023");
        for (double v : {reset_lo, reset_hi, -inf}) {
            double x = v;
            for (int i = 0; i < 4096; i++) x = x + high;  // positive scores cannot lift it out
            expect(marked(x), "marked + passing positive scores stays marked");
            x = v;
            for (int i = 0; i < 4096; i++) x = x + low;
            expect(marked(x) && !(x != x), "marked + passing negative scores stays marked (and is no NaN)");
        }
        expect(!marked(-std::ldexp(1.0, 1022)) && !marked(0.0) && !marked(std::numeric_limits<double>::max()),
               "values of magnitude below 2^1023, and positive ones, are not marked");
    }
    if (g_failed) return 1;
    printf("lean gate: ok\n");
    return 0;
}
