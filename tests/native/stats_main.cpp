// Stand-alone driver of the lattice statistics twin (include/tgx.h: tgx_lattice_stats_host) for a sanitizer build:
// tests/test_stats_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (the vocabulary's bytes,
// V + 1 offsets and V scores; N text bytes and S + 1 offsets in; S doubles per output), so that reading or writing one
// element too many is a report.  Every output is NULL in turn, and all of them; a batch without samples; samples of 0
// bytes at the start, in the middle and at the end; a sample without a path; a token of TGX_MAX_TOKEN_LEN bytes that ends
// exactly at the end of the text.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tgx.h"

namespace {

template <class T>
std::unique_ptr<T[]> block(size_t n) {  // exactly n elements; n = 0: a block no element of which may be touched
    return std::unique_ptr<T[]>(new T[n]);
}
template <class T>
std::unique_ptr<T[]> block_of(const std::vector<T>& v) {
    std::unique_ptr<T[]> b = block<T>(v.size());
    if (!v.empty()) memcpy(b.get(), v.data(), v.size() * sizeof(T));
    return b;
}

int g_failed = 0;
void expect(bool ok, const char* what, uint64_t run, double a = 0, double b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (run %llu: %.17g, %.17g)\n", what, (unsigned long long)run, a, b);
}

struct Vocab {
    std::unique_ptr<uint8_t[]> bytes;
    std::unique_ptr<uint64_t[]> offs;
    std::unique_ptr<double[]> scores;
    uint32_t n;
};

Vocab make_vocab(const std::vector<std::string>& toks, const std::vector<double>& scores) {
    std::vector<uint8_t> b;
    std::vector<uint64_t> o(1, 0);
    for (const std::string& t : toks) {
        b.insert(b.end(), t.begin(), t.end());
        o.push_back(b.size());
    }
    return {block_of(b), block_of(o), block_of(scores), (uint32_t)toks.size()};
}

bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

void run(uint64_t id, const Vocab& v, const std::vector<std::string>& samples, double alpha, uint64_t want_bad) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> offs(1, 0);
    for (const std::string& s : samples) {
        text.insert(text.end(), s.begin(), s.end());
        offs.push_back(text.size());
    }
    const uint64_t S = samples.size();
    const std::unique_ptr<uint8_t[]> b_text = block_of(text);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    std::unique_ptr<double[]> z = block<double>(S), es = block<double>(S), et = block<double>(S);
    uint64_t bad = ~0ull;
    tgx_status st = tgx_lattice_stats_host(v.bytes.get(), v.offs.get(), v.scores.get(), v.n, b_text.get(), b_offs.get(), S, alpha, z.get(),
                                           es.get(), et.get(), &bad);
    expect(st == TGX_OK, "all outputs: status", id, st);
    expect(bad == want_bad, "n_no_path", id, (double)bad, (double)want_bad);
    for (uint64_t i = 0; i < S; i++) {
        if (samples[i].empty()) expect(z[i] == 0.0 && es[i] == 0.0 && et[i] == 0.0, "an empty sample gives 0, 0, 0", id, z[i], es[i]);
        expect(std::isinf(z[i]) ? (z[i] < 0 && std::isnan(es[i]) && std::isnan(et[i])) : (std::isfinite(es[i]) && et[i] >= 0.0),
               "-inf goes with NaN, NaN", id, z[i], es[i]);
    }
    // every output NULL in turn, the count too, and all at once: the others are what they were
    for (int drop = 0; drop < 5; drop++) {
        std::unique_ptr<double[]> z2 = block<double>(S), es2 = block<double>(S), et2 = block<double>(S);
        uint64_t bad2 = ~0ull;
        st = tgx_lattice_stats_host(v.bytes.get(), v.offs.get(), v.scores.get(), v.n, b_text.get(), b_offs.get(), S, alpha,
                                    (drop == 0 || drop == 4) ? nullptr : z2.get(), (drop == 1 || drop == 4) ? nullptr : es2.get(),
                                    (drop == 2 || drop == 4) ? nullptr : et2.get(), (drop == 3 || drop == 4) ? nullptr : &bad2);
        expect(st == TGX_OK, "an output is NULL: status", id, st, drop);
        for (uint64_t i = 0; i < S; i++) {
            if (drop != 0 && drop != 4) expect(same(z2[i], z[i]), "logz with another output NULL", id, z2[i], z[i]);
            if (drop != 1 && drop != 4) expect(same(es2[i], es[i]), "escore with another output NULL", id, es2[i], es[i]);
            if (drop != 2 && drop != 4) expect(same(et2[i], et[i]), "etokens with another output NULL", id, et2[i], et[i]);
        }
        if (drop != 3 && drop != 4) expect(bad2 == want_bad, "n_no_path with another output NULL", id, (double)bad2, (double)want_bad);
    }
}

}  // namespace

int main() {
    const std::string long_tok(TGX_MAX_TOKEN_LEN, 'q');
    const Vocab v = make_vocab({"a", "b", "c", "ab", "bc", "abc", "ca", "cab", long_tok, "ab", ""},
                               {-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2, -4.0, -0.9, -1.0});
    run(1, v, {"abcabca", "", "a", "cabcab"}, 1.0, 0);
    run(2, v, {"", "abx", "", "abc", "x", ""}, 0.3, 2);                    // two samples without a path
    run(3, v, {}, 1.0, 0);                                                // no samples: blocks of no element
    run(4, v, {"ab" + long_tok, long_tok, long_tok.substr(1) + "a"}, 2.0, 1);  // the longest token ends at the text's end
    run(5, v, {std::string(300, 'a') + "bc" + std::string(200, 'c')}, 0.0, 0);
    const Vocab none = make_vocab({}, {});
    run(6, none, {"", "a"}, 1.0, 1);                                      // an empty vocabulary

    // argument errors leave the outputs alone and report sampling's statuses
    std::unique_ptr<uint8_t[]> t = block<uint8_t>(1);
    t[0] = 'a';
    std::unique_ptr<uint64_t[]> o = block<uint64_t>(2);
    o[0] = 0;
    o[1] = 1;
    std::unique_ptr<double[]> z = block<double>(1);
    z[0] = 42.0;
    expect(tgx_lattice_stats_host(v.bytes.get(), v.offs.get(), v.scores.get(), v.n, t.get(), o.get(), 1, -1.0, z.get(), nullptr, nullptr, nullptr) ==
               TGX_ERR_INVALID, "negative alpha", 7);
    expect(tgx_lattice_stats_host(v.bytes.get(), v.offs.get(), v.scores.get(), v.n, t.get(), o.get(), 1, NAN, z.get(), nullptr, nullptr, nullptr) ==
               TGX_ERR_INVALID, "NaN alpha", 7);
    expect(tgx_lattice_stats_host(v.bytes.get(), v.offs.get(), v.scores.get(), v.n, t.get(), o.get(), 1, INFINITY, z.get(), nullptr, nullptr, nullptr) ==
               TGX_ERR_INVALID, "infinite alpha", 7);
    const Vocab inf_score = make_vocab({"a", "b"}, {-1.0, -INFINITY});
    expect(tgx_lattice_stats_host(inf_score.bytes.get(), inf_score.offs.get(), inf_score.scores.get(), inf_score.n, t.get(), o.get(), 1, 1.0, z.get(),
                                  nullptr, nullptr, nullptr) == TGX_ERR_UNSUPPORTED, "a non-finite score", 7);
    const Vocab huge = make_vocab({"a", "b"}, {-1.0, -1e308});
    expect(tgx_lattice_stats_host(huge.bytes.get(), huge.offs.get(), huge.scores.get(), huge.n, t.get(), o.get(), 1, 100.0, z.get(), nullptr, nullptr,
                                  nullptr) == TGX_ERR_INVALID, "alpha * score overflows", 7);
    expect(z[0] == 42.0, "a refused call writes nothing", 7, z[0]);

    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("stats twin: ok\n");
    return 0;
}
