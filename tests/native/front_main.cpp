// Stand-alone driver of the front end's host twin (include/tgx.h: tgx_front_host) for a sanitizer build:
// tests/test_front_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (N text bytes, S + 1
// offsets, the special tokens' bytes and n + 1 offsets, S + 1 seg_offs), so that reading or writing one element too many
// is a report; what comes back (K seg_special, E + 1 offsets, the packed bytes) is read to its documented end.  The
// twin is checked against a plain sequential splitter written here.  The shapes put sample ends, special tokens and
// "\r\n" pairs at the ends of the 4096-byte tiles and 16-byte thread slots, and a text that ends exactly with a tile.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tgx.h"

namespace {

template <class T>
std::unique_ptr<T[]> block_of(const std::vector<T>& v) {  // exactly v.size() elements
    std::unique_ptr<T[]> b(new T[v.size()]);
    if (!v.empty()) memcpy(b.get(), v.data(), v.size() * sizeof(T));
    return b;
}

int g_failed = 0;
void expect(bool ok, const char* what, int run, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (run %d, %llu, %llu)\n", what, run, (unsigned long long)a, (unsigned long long)b);
}

struct Want {
    std::vector<uint64_t> seg_offs, out_offs;
    std::vector<int32_t> seg_special;
    std::string out;
};

// the rule, sample by sample and byte by byte (src/tokenizer.rs:299-347, src/processor.rs:46-54)
Want reference(const std::vector<std::string>& samples, const std::vector<std::string>& specials, bool crlf) {
    Want w;
    w.seg_offs.push_back(0);
    w.out_offs.push_back(0);
    auto emit = [&](const std::string& seg) {
        for (size_t p = 0; p < seg.size(); p++)
            if (!(crlf && seg[p] == '\r' && p + 1 < seg.size() && seg[p + 1] == '\n')) w.out.push_back(seg[p]);
        w.out_offs.push_back(w.out.size());
        w.seg_special.push_back(-1);
    };
    for (const std::string& s : samples) {
        size_t cursor = 0;
        for (size_t p = 0; p < s.size();) {
            int hit = -1;
            for (size_t k = 0; k < specials.size() && hit < 0; k++)
                if (s.compare(p, specials[k].size(), specials[k]) == 0 && p + specials[k].size() <= s.size()) hit = (int)k;
            if (hit < 0) {
                p++;
                continue;
            }
            if (p > cursor) emit(s.substr(cursor, p - cursor));
            w.seg_special.push_back(hit);
            p += specials[hit].size();
            cursor = p;
        }
        if (cursor < s.size()) emit(s.substr(cursor));
        w.seg_offs.push_back(w.seg_special.size());
    }
    return w;
}

std::string filler(size_t n, unsigned salt) {
    std::string s(n, 'a');
    for (size_t i = 0; i < n; i++) s[i] = (char)('a' + (i * 7 + salt) % 23);
    return s;
}

int g_runs = 0;
void run(const std::vector<std::string>& samples, const std::vector<std::string>& specials) {
    std::vector<uint8_t> text, sp;
    std::vector<uint64_t> offs(1, 0), sp_offs(1, 0);
    for (const std::string& s : samples) {
        text.insert(text.end(), s.begin(), s.end());
        offs.push_back(text.size());
    }
    for (const std::string& s : specials) {
        sp.insert(sp.end(), s.begin(), s.end());
        sp_offs.push_back(sp.size());
    }
    const std::unique_ptr<uint8_t[]> b_text = block_of(text), b_sp = block_of(sp);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs), b_sp_offs = block_of(sp_offs);
    const uint64_t S = samples.size();
    for (uint32_t flags = 0; flags < 2; flags++) {
        const int id = g_runs++;
        const Want w = reference(samples, specials, flags != 0);
        std::unique_ptr<uint64_t[]> seg_offs(new uint64_t[S + 1]);
        int32_t* ss = nullptr;
        uint8_t* out = nullptr;
        uint64_t *out_offs = nullptr, K = ~0ull, E = ~0ull;
        const tgx_status st = tgx_front_host(b_text.get(), b_offs.get(), S, b_sp.get(), b_sp_offs.get(), (uint32_t)specials.size(), flags,
                                             seg_offs.get(), &ss, &K, &out, &out_offs, &E);
        expect(st == TGX_OK, "status", id, st);
        if (st != TGX_OK) continue;
        expect(K == w.seg_special.size() && E + 1 == w.out_offs.size(), "counts", id, K, E);
        if (K == w.seg_special.size() && E + 1 == w.out_offs.size()) {
            expect(memcmp(seg_offs.get(), w.seg_offs.data(), (S + 1) * 8) == 0, "seg_offs", id);
            expect(K == 0 || memcmp(ss, w.seg_special.data(), K * 4) == 0, "seg_special", id);
            expect(memcmp(out_offs, w.out_offs.data(), (E + 1) * 8) == 0, "out_offs", id);
            expect(out_offs[E] == w.out.size() && (w.out.empty() || memcmp(out, w.out.data(), w.out.size()) == 0), "packed bytes", id);
        }
        free(ss);
        free(out);
        free(out_offs);
    }
}

}  // namespace

int main() {
    const std::string SP = "<|special|>";
    const size_t T = 4096, M = SP.size();
    for (size_t o = T - M; o <= T + 1; o++) run({filler(o, 1) + SP + filler(40, 3)}, {SP});
    run({filler(T - M, 2) + SP}, {SP});                          // the text ends with a tile, and with a special
    run({filler(T - 1, 2) + "\r"}, {SP});                        // ... and with a '\r'
    run({filler(T - 1, 2) + "\r", "\n" + filler(15, 1)}, {SP});  // '\r' and '\n' of two samples, at a tile's end
    run({filler(15, 0) + "\r\n" + filler(14, 0) + "\r\r\n\n\r"}, {"\n\r"});
    run({filler(T - 1, 4) + "\r\n" + filler(20, 5), filler(T - 2, 6) + "\r\n\r\n"}, {"<s>"});
    for (size_t j = 1; j < M; j++) run({filler(T - j, 7) + SP.substr(0, j), SP.substr(j) + "cd"}, {SP});
    run({"x<abx"}, {"<a", "<ab"});
    run({"x<abx"}, {"<ab", "<a"});
    run({"ababababa", "ababa", "", "aaaaa", "aaaaaa", ""}, {"aba", "aa", "ba"});
    run({std::string(3 * T + 1, 'a')}, {"aa"});
    run({"b" + std::string(2 * T + 5, 'a'), std::string(7, 'a')}, {"aaa", "a"});
    run({"", "", "x<s>y", "", "", "", "<s>", "z", ""}, {"<s>"});
    run({"", "", ""}, {"<s>"});
    run({}, {"<s>"});
    run({"<s><s></s><s>", "</s></s>"}, {"<s>", "</s>"});
    run({filler(5000, 1) + "\r\n", "", "\r\nab\r", "\n", filler(33, 2)}, {});
    run({"ab\r\n<x>cd", "\r\n<x>", "\r\r\n<x>\r\n"}, {"\n<x>"});
    run({"a<\r\n>b\r\n<\r\n>", "<\r\n", ">"}, {"<\r\n>"});
    run({"\xfe\x80<s>\xc3", "\xc3<s>\xa9\xf0\x9f", "\x80\x80"}, {"<s>", "\xc3\xa9"});
    {
        std::string body;
        for (size_t k = 0; body.size() < 70000; k++) body += filler(64 - M, (unsigned)k) + SP;
        run({body.substr(0, 70000)}, {SP});
    }
    // arguments that are refused before anything is touched
    const uint64_t zero = 0, offs2[2] = {0, 0};
    uint64_t seg_offs[2], K = 0, E = 0, *oo = nullptr;
    int32_t* ss = nullptr;
    uint8_t* ot = nullptr;
    tgx_status st = tgx_front_host(nullptr, offs2, 1, nullptr, &zero, 0, 4, seg_offs, &ss, &K, &ot, &oo, &E);
    expect(st == TGX_ERR_INVALID, "unknown flags", -1, st);
    const uint8_t sp1[3] = {'<', 's', '>'};
    const uint64_t empty_special[3] = {0, 3, 3};
    st = tgx_front_host(nullptr, offs2, 1, sp1, empty_special, 2, 0, seg_offs, &ss, &K, &ot, &oo, &E);
    expect(st == TGX_ERR_INVALID, "empty special", -1, st);
    st = tgx_front_host(nullptr, offs2, 1, sp1, empty_special, 1, 0, seg_offs, nullptr, &K, &ot, &oo, &E);
    expect(st == TGX_ERR_INVALID, "NULL output", -1, st);
    std::vector<uint64_t> many(4098);
    for (size_t k = 0; k < many.size(); k++) many[k] = k;
    const std::unique_ptr<uint8_t[]> many_bytes(new uint8_t[4097]);
    memset(many_bytes.get(), 'x', 4097);
    st = tgx_front_host(nullptr, offs2, 1, many_bytes.get(), many.data(), 4097, 0, seg_offs, &ss, &K, &ot, &oo, &E);
    expect(st == TGX_ERR_UNSUPPORTED, "too many special tokens", -1, st);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("front twin: ok (%d runs)\n", g_runs);
    return 0;
}
