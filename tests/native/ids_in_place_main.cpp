// Stand-alone driver of the host side of "ids in place" (csrc/ids_in_place.h) for a sanitizer build:
// tests/test_ids_in_place_native.py compiles it under -fsanitize=address,undefined and runs it.  No device is opened.
//
// It checks the decision function term by term and at the edge of the count field (2^24 - 1 and 2^24 bytes), and the
// packed-count arithmetic of one relaxation step (count << 8 | step, as encode5_kernel's counting builds carry it) in
// plain C++ against a direct count along random winner sequences.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>

#include "../../tokengeex_amd/csrc/ids_in_place.h"

namespace {

int g_failed = 0;
void expect(bool ok, const char* what) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s\n", what);
}

tgx::IdsInPlaceQuery all_true() {
    tgx::IdsInPlaceQuery q{};
    q.rows5 = true;
    q.long_tokens = false;
    q.dropout = false;
    q.n_long = 0;
    q.build_counts = true;
    q.max_len = 65536;
    q.switched_on = true;
    q.diagnostics = false;
    return q;
}

}  // namespace

int main() {
    // ---- the decision: every term alone turns it off
    expect(tgx::ids_in_place(all_true()), "every term holds: in place");
    { auto q = all_true(); q.rows5 = false; expect(!tgx::ids_in_place(q), "another encode path: not in place"); }
    { auto q = all_true(); q.long_tokens = true; expect(!tgx::ids_in_place(q), "long tokens: not in place"); }
    { auto q = all_true(); q.dropout = true; expect(!tgx::ids_in_place(q), "dropout: not in place"); }
    { auto q = all_true(); q.n_long = 1; expect(!tgx::ids_in_place(q), "one sample for encode6_kernel: not in place"); }
    { auto q = all_true(); q.n_long = ~0ull; expect(!tgx::ids_in_place(q), "every sample for encode6_kernel: not in place"); }
    { auto q = all_true(); q.build_counts = false; expect(!tgx::ids_in_place(q), "a build that does not count: not in place"); }
    { auto q = all_true(); q.switched_on = false; expect(!tgx::ids_in_place(q), "TGX_IDS_IN_PLACE=0: not in place"); }
    { auto q = all_true(); q.diagnostics = true; expect(!tgx::ids_in_place(q), "timing experiments: not in place"); }
    { auto q = all_true(); q.max_len = 0; expect(tgx::ids_in_place(q), "empty samples only: in place"); }
    // ---- the count field's width
    expect(tgx::kCountFieldSamples == (1ull << 24), "24 bits of count above the step byte");
    { auto q = all_true(); q.max_len = (1ull << 24) - 1; expect(tgx::ids_in_place(q), "a sample of 2^24 - 1 bytes: in place"); }
    { auto q = all_true(); q.max_len = 1ull << 24; expect(!tgx::ids_in_place(q), "a sample of 2^24 bytes: not in place"); }
    { auto q = all_true(); q.max_len = ~0ull; expect(!tgx::ids_in_place(q), "the longest length: not in place"); }
    {   // the largest count such a sample can have fits, with any step below it, and one more would not
        const uint32_t top = tgx::count_step_word((((1u << 24) - 2u) << 8) | 7u, 15u);
        expect(tgx::count_of_word(top) == (1u << 24) - 1u && (top & 0xFFu) == 15u, "count 2^24 - 1 is representable");
        const uint32_t over = tgx::count_step_word(top, 0u);
        expect(tgx::count_of_word(over) == 0u, "count 2^24 wraps: why the decision stops one short");
    }
    // ---- one step's arithmetic
    expect(tgx::count_of_word(tgx::kCountNoStep) == 0u, "a sample's first position has count 0");
    for (uint32_t u = 0; u < 16; u++) {
        const uint32_t w = tgx::count_step_word(tgx::kCountNoStep, u);
        expect(w == (0x100u | u), "the first token: count 1, step u");
        for (uint32_t from : {0xFFu, 0x100u, 0x10Fu, 0x12345u << 8 | 3u, 0xFFFFFEu << 8 | 0xFu}) {
            const uint32_t got = tgx::count_step_word(from, u);
            expect(got == (from & ~0xFFu) + (0x100u | u), "the (x | 0xFF) + 1 + u form equals (x & ~0xFF) + (0x100 | u)");
            expect(((got - 0u) & 15u) == u, "the step's low four bits are what the length is read from");
        }
    }
    // ---- random winner sequences: position p's winner is a token of 1..16 bytes that starts at p - len; its word comes
    // from the start position's final word by the step (p - len) & 15, as in the kernel; the direct count walks back.
    {
        std::mt19937_64 rng(20240611);
        for (int trial = 0; trial < 200; trial++) {
            const size_t n = 1 + (size_t)(rng() % (trial < 20 ? 40 : 5000));
            // heap blocks of exactly n + 1 elements: an access past a sample's end is a report
            std::unique_ptr<uint32_t[]> word(new uint32_t[n + 1]), len(new uint32_t[n + 1]), direct(new uint32_t[n + 1]);
            word[0] = tgx::kCountNoStep;
            len[0] = 0;
            direct[0] = 0;
            const uint32_t mode = (uint32_t)(rng() % 3);  // 0: any length, 1: single bytes (count = n), 2: 16-byte tokens where they fit
            for (size_t p = 1; p <= n; p++) {
                const uint32_t most = (uint32_t)(p < 16 ? p : 16);
                uint32_t l = mode == 1 ? 1u : mode == 2 ? most : 1u + (uint32_t)(rng() % most);
                const size_t from = p - l;
                len[p] = l;
                word[p] = tgx::count_step_word(word[from], (uint32_t)(from & 15u));
                direct[p] = direct[from] + 1u;
            }
            bool ok = true;
            for (size_t p = 1; p <= n; p++) {
                ok = ok && tgx::count_of_word(word[p]) == direct[p];
                // the length as every reader of the step takes it: ((l - step - 1) & 15) + 1 with l = p & 15
                ok = ok && ((((uint32_t)(p & 15u) - word[p] - 1u) & 15u) + 1u) == len[p];
                ok = ok && direct[p] <= p;
            }
            // and the walk the trace does from the end: as many hops as the end's count says
            uint32_t hops = 0;
            for (size_t p = n; p > 0; p -= len[p]) hops++;
            ok = ok && hops == tgx::count_of_word(word[n]);
            if (mode == 1) ok = ok && tgx::count_of_word(word[n]) == n;
            expect(ok, "packed counts equal the direct counts along a random winner sequence");
        }
    }
    if (g_failed) return 1;
    printf("ids in place: ok\n");
    return 0;
}
