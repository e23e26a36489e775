// Stand-alone driver of the phrase twin (include/tgx_phrases.h: tgx_phrase_hits_host) for a sanitizer build:
// tests/test_phrase_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx_phrases.h documents (the elements, S + 1
// offsets, the phrases' elements, P + 1 phrase offsets, S counts, n_elems bytes of `longest`, P per-phrase counts), so
// that reading or writing one element too many is a report: the byte after a row's last occurrence is never read when
// the row ends the block, nor the byte in front of the first row.  The shapes: rows of 0 .. 6 elements and rows that end
// one to three elements on either side of a chunk of 64 elements, of a tile of 256 and of two tiles, between runs of
// empty rows, over an alphabet of six bytes, with phrases of 1, 2, 3 and 9 elements, a duplicate, and for text the
// greatest length, 255; every flag combination for text.  Every answer is checked against the definition written out
// plainly, phrase by phrase and start by start.  The dword fold of csrc/phrase.h is checked against the byte fold.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tgx_phrases.h"
#define TGX_HOST_ONLY
#include "../../tokengeex_amd/csrc/phrase.h"

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
void expect(bool ok, const char* what, uint64_t run, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (run %llu: %llu, %llu)\n", what, (unsigned long long)run, (unsigned long long)a, (unsigned long long)b);
}

uint32_t fold(uint32_t b, bool on) { return on && b >= 'A' && b <= 'Z' ? b | 0x20 : b; }
bool word_byte(uint32_t b) { return (b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_' || b >= 0x80; }

template <class T>
void run(uint64_t run_id, const std::vector<uint64_t>& lens, const std::vector<std::vector<T>>& phrases, uint32_t flags) {
    static const T alphabet[6] = {(T)'a', (T)'B', (T)'b', (T)' ', (T)'A', (T)'_'};
    std::vector<uint64_t> offs(1, 0), p_offs(1, 0);
    std::vector<T> data, p_data;
    uint64_t x = 88172645463325252ull + run_id;
    for (uint64_t len : lens) {
        for (uint64_t t = 0; t < len; t++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            data.push_back(alphabet[x % 6]);
        }
        offs.push_back(data.size());
    }
    for (const auto& p : phrases) {
        p_data.insert(p_data.end(), p.begin(), p.end());
        p_offs.push_back(p_data.size());
    }
    // the longest phrase is planted where rows have the room, so that it occurs
    const std::vector<T>& longp = *std::max_element(phrases.begin(), phrases.end(), [](const auto& a, const auto& b) { return a.size() < b.size(); });
    for (uint64_t i = 0; i + 1 < offs.size(); i++)
        if (offs[i + 1] - offs[i] >= longp.size()) std::copy(longp.begin(), longp.end(), data.begin() + (offs[i + 1] - longp.size()));
    const uint64_t S = lens.size(), N = data.size(), P = phrases.size();
    const bool fc = flags & TGX_PHRASE_FOLD_CASE, ww = flags & TGX_PHRASE_WHOLE_WORD;
    // the definition, plainly
    std::vector<int64_t> want_count(S, 0), want_per(P, 0);
    std::vector<uint8_t> want_longest(N, 0);
    for (uint64_t p = 0; p < P; p++) {
        bool dup = false;  // credited to the lowest index among the phrases equal after folding
        for (uint64_t q = 0; q < p && !dup; q++) {
            dup = phrases[q].size() == phrases[p].size();
            for (size_t k = 0; dup && k < phrases[p].size(); k++) dup = fold(phrases[q][k], fc) == fold(phrases[p][k], fc);
        }
        if (dup) continue;
        const uint64_t L = phrases[p].size();
        for (uint64_t i = 0; i < S; i++)
            for (uint64_t e = offs[i]; e + L <= offs[i + 1]; e++) {
                bool hit = true;
                for (uint64_t k = 0; hit && k < L; k++) hit = fold(data[e + k], fc) == fold(phrases[p][k], fc);
                if (hit && ww) hit = (e == offs[i] || !word_byte(data[e - 1])) && (e + L == offs[i + 1] || !word_byte(data[e + L]));
                if (!hit) continue;
                want_count[i]++;
                want_per[p]++;
                want_longest[e] = std::max<uint8_t>(want_longest[e], (uint8_t)L);
            }
    }
    const auto b_data = block_of(data);
    const auto b_offs = block_of(offs);
    const auto b_pd = block_of(p_data);
    const auto b_po = block_of(p_offs);
    for (int outs = 1; outs < 8; outs++) {  // every combination of outputs but none
        auto count = block<int64_t>(S);
        auto longest = block<uint8_t>(N);
        auto per = block<int64_t>(P);
        std::fill(count.get(), count.get() + S, -7);
        std::fill(longest.get(), longest.get() + N, 7);
        std::fill(per.get(), per.get() + P, -7);
        const tgx_status st = tgx_phrase_hits_host(b_data.get(), sizeof(T), b_offs.get(), S, b_pd.get(), b_po.get(), (uint32_t)P, flags,
                                                   outs & 1 ? count.get() : nullptr, outs & 2 ? longest.get() : nullptr, outs & 4 ? per.get() : nullptr);
        expect(st == TGX_OK, "status", run_id, outs, (uint64_t)st);
        if (st != TGX_OK) continue;
        for (uint64_t i = 0; i < S; i++) expect(count[i] == (outs & 1 ? want_count[i] : -7), "count", run_id, outs, i);
        for (uint64_t e = 0; e < N; e++) expect(longest[e] == (outs & 2 ? want_longest[e] : 7), "longest", run_id, outs, e);
        for (uint64_t p = 0; p < P; p++) expect(per[p] == (outs & 4 ? want_per[p] : -7), "per_phrase", run_id, outs, p);
    }
    uint64_t total = 0;
    for (int64_t c : want_count) total += (uint64_t)c;
    expect(total > 0 || N < 200 || ww, "the run has an occurrence", run_id);
}

template <class T>
std::vector<T> word(const char* s) {
    std::vector<T> v;
    for (; *s; s++) v.push_back((T)(uint8_t)*s);
    return v;
}

template <class T>
void runs(uint64_t base, uint32_t flags, size_t max_len) {
    std::vector<std::vector<T>> phrases = {word<T>("a"), word<T>("ab"), word<T>("Ab "), word<T>("b a_bB ab"), word<T>("ab"), word<T>("AB"), word<T>(" ")};
    std::vector<T> longp;
    for (size_t k = 0; k < max_len; k++) longp.push_back((T)("abB _"[k % 5]));
    phrases.push_back(longp);
    uint64_t id = base;
    run<T>(id++, {0, 0, 1, 2, 3, 4, 5, 6, 0, 0, 3, 2, 1, 0}, phrases, flags);
    for (uint64_t edge : {64u, 256u, 512u})
        for (int d = -3; d <= 3; d++) run<T>(id++, {0, 5, edge - 5 + d, 0, 0, 7, edge + 9 - d, 1, 0}, phrases, flags);
    run<T>(id++, {3, 5 * 256 + 37, 0, 2, 300}, phrases, flags);
    run<T>(id++, {}, phrases, flags);
    run<T>(id++, {0, 0, 0}, phrases, flags);
}

}  // namespace

int main() {
    for (uint32_t b = 0; b < 256; b++)
        for (int at = 0; at < 4; at++)
            for (int on = 0; on < 2; on++) {
                const uint32_t others = 0x5A41807Fu & ~(0xFFu << (8 * at)), x = others | b << (8 * at);
                uint32_t want = 0;
                for (int j = 0; j < 4; j++) want |= fold((x >> (8 * j)) & 0xFF, on) << (8 * j);
                expect(tgx::phrase_fold4(x, on) == want && tgx::phrase_fold(b, on) == fold(b, on), "fold4", b, at, on);
                expect(tgx::phrase_word_byte(b) == word_byte(b), "word_byte", b);
            }
    for (uint32_t flags = 0; flags < 4; flags++) runs<uint8_t>(1000 * (flags + 1), flags, 255);
    runs<uint32_t>(9000, 0, 64);
    // the documented errors
    const uint8_t text[3] = {'a', 'b', 'c'};
    const uint64_t offs[2] = {0, 3}, po[2] = {0, 1}, po_empty[2] = {0, 0};
    int64_t count[1];
    expect(tgx_phrase_hits_host(text, 1, offs, 1, text, po, 1, 0, nullptr, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
    expect(tgx_phrase_hits_host(text, 2, offs, 1, text, po, 1, 0, count, nullptr, nullptr) == TGX_ERR_INVALID, "elem_bytes", 0);
    expect(tgx_phrase_hits_host(text, 1, offs, 1, text, po, 1, 4, count, nullptr, nullptr) == TGX_ERR_INVALID, "unknown flag", 0);
    expect(tgx_phrase_hits_host(text, 1, offs, 1, text, po_empty, 1, 0, count, nullptr, nullptr) == TGX_ERR_INVALID, "empty phrase", 0);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("phrase twin: ok\n");
    return 0;
}
