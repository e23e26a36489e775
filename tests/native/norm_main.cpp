// Stand-alone driver of the normalisation's host twin (include/tgx.h: tgx_normalize_host) for a sanitizer build:
// tests/test_norm_native.py compiles it with csrc/host_twins.cpp and csrc/unicode_norm.cpp under
// -fsanitize=address,undefined and runs it.  No device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (N text bytes, S + 1
// offsets), so that reading one byte past the text (a decoder that looks for a continuation byte behind a row's end, a
// slot's look-ahead) is a report; what comes back (S + 1 offsets, the bytes) is read to its documented end and compared
// with tgx_normalize_segments over the same rows.  The rows put heads, active scalars, row ends and cut sequences at the
// ends of the 4096-byte tiles and 16-byte thread slots, with empty rows between them and a piece that ends the text.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tgx.h"
#include "../../tokengeex_amd/csrc/api_internal.h"  // the error detail the twin leaves (tgx_last_error_detail is tgx_api.cpp's)

// csrc/unicode_norm.cpp records its messages here (csrc/tgx_api.cpp is not part of this program)
static std::string g_message;
tgx_status tgx_set_error(tgx_status st, const char* msg) {
    g_message = msg ? msg : "";
    return st;
}

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

std::string filler(size_t n, size_t salt) {
    std::string s(n, 'a');
    for (size_t i = 0; i < n; i++) s[i] = (char)('a' + (i * 7 + salt) % 23);
    return s;
}

struct Batch {
    std::vector<std::string> rows;
    size_t n = 0;
    void add(std::initializer_list<std::string> more) {
        for (const std::string& r : more) {
            rows.push_back(r);
            n += r.size();
        }
    }
    // ASCII after which the next byte stands k bytes in front of a multiple of mod
    std::string pad(size_t mod, size_t k) const { return filler((mod * 2 - k % mod - n % mod) % mod, n); }
};

int g_runs = 0;
// status of the twin; on TGX_OK the result is compared with tgx_normalize_segments
tgx_status run(const std::vector<std::string>& rows, uint64_t* pieces = nullptr) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> offs(1, 0);
    for (const std::string& r : rows) {
        text.insert(text.end(), r.begin(), r.end());
        offs.push_back(text.size());
    }
    const std::unique_ptr<uint8_t[]> b_text = block_of(text);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    const uint64_t S = rows.size();
    tgx_status last = TGX_OK;
    for (uint32_t form = 0; form < 4; form++) {
        const int id = g_runs++;
        uint8_t *got = nullptr, *want = nullptr;
        uint64_t *got_offs = nullptr, *want_offs = nullptr, P = ~0ull;
        last = tgx_normalize_host(form, b_text.get(), b_offs.get(), S, &got, &got_offs, &P);
        if (pieces) *pieces = P;
        if (last != TGX_OK) {
            expect(!got && !got_offs, "nothing is returned with an error", id);
            continue;
        }
        const tgx_status st = tgx_normalize_segments(form, b_text.get(), b_offs.get(), b_offs.get() + 1, S, &want, &want_offs);
        expect(st == TGX_OK, "tgx_normalize_segments", id, st);
        if (st == TGX_OK) {
            expect(memcmp(got_offs, want_offs, (S + 1) * 8) == 0, "offsets", id);
            expect(got_offs[S] == want_offs[S] && (want_offs[S] == 0 || memcmp(got, want, want_offs[S]) == 0), "bytes", id, got_offs[S], want_offs[S]);
        }
        free(got);
        free(got_offs);
        free(want);
        free(want_offs);
    }
    return last;
}

}  // namespace

int main() {
    const std::string acute = "\xcc\x81", jamo_v = "\xe1\x85\xa1", wide_a = "\xef\xbc\xa1", ga = "\xea\xb0\x80", stem = "\xf0\x9d\x85\xa5";
    Batch b;
    for (size_t mod : {(size_t)16, (size_t)4096}) {
        b.add({b.pad(mod, 1) + "e" + acute + "xyz", ""});
        b.add({b.pad(mod, 2) + "a" + acute + "b"});
        b.add({"", b.pad(mod, 4) + ga + jamo_v + "z"});
        b.add({b.pad(mod, 5) + ga + jamo_v + jamo_v});
        b.add({b.pad(mod, 2) + "q" + stem + "r", "", ""});
        b.add({b.pad(mod, 1) + wide_a + "k", b.pad(mod, 2) + "\xc3\x85" + "A\xcc\x8a"});
        b.add({b.pad(mod, 1) + "e", acute + "abc", ""});
        b.add({b.pad(mod, 2) + "e\xcc", "\x81" "abc"});
        b.add({b.pad(mod, 2) + ga.substr(0, 2), ga.substr(2) + jamo_v, ""});
        b.add({b.pad(mod, 3) + "\xe4\xb8\xad" + acute + "\xff" + acute + "o" + "\xcc\x81\xcc\x96\xcc\xa3"});
        b.add({b.pad(mod, 2) + "\xc4\x81" + "\xcc\x81\xcc\xa8", "\xe0\xa7\x87\xe0\xa6\xbe", "\xe1\x84\x80\xe1\x85\xa1\xe1\x86\xa8"});
        b.add({b.pad(mod, 3) + "e" + acute, "", b.pad(mod, 0), jamo_v + "!"});
    }
    const std::vector<std::string> invalid = {"\xff\xfe" "a\xcc\x81", "\xe4\xb8", "abc\x80\x80" "def", "\xf5\x80\x80\x80", "\xed\xa0\x80x", "e\xcc\x81\xc0\xaf"};
    for (const std::string& raw : invalid) b.add({raw, b.pad(16, 2) + raw, b.pad(4096, 3) + raw});
    b.add({"", "", filler(40, 1) + "u\xcc\x88\xcc\x81"});  // a piece ends the text
    uint64_t pieces = 0;
    expect(run(b.rows, &pieces) == TGX_OK && pieces > 20, "the edge batch", -1, pieces);
    // the same bytes as one row, and cut into rows of 1, 2, 3, ... bytes: every sequence is cut somewhere
    std::string all;
    for (const std::string& r : b.rows) all += r;
    expect(run({all}) == TGX_OK, "one row", -1);
    {
        std::vector<std::string> cut;
        for (size_t at = 0, k = 1; at < all.size(); at += k, k = k % 7 + 1) cut.push_back(all.substr(at, k));
        expect(run(cut) == TGX_OK, "cut rows", -1);
    }
    // texts that end with a cut sequence, at a slot's and a tile's last byte
    for (size_t n : {(size_t)15, (size_t)16, (size_t)4095, (size_t)4096})
        for (const std::string& tail : {std::string("\xcc"), std::string("\xe1\x85"), std::string("\xf0\x9d\x85"), std::string("e") + acute, jamo_v}) {
            expect(run({filler(n - tail.size(), n) + tail}) == TGX_OK, "a text's last bytes", (int)n);
            expect(run({filler(n - tail.size(), n), tail}) == TGX_OK, "a text's last row", (int)n);
        }
    expect(run({}) == TGX_OK && run({"", "", ""}) == TGX_OK, "no rows, no bytes", -1);
    // the window: a starter and 31 non-starters; U+0316 (class 220) sorts in front of U+0301 (230)
    std::string marks;
    for (int k = 0; k < 31; k++) marks += k % 2 ? "\xcc\x96" : "\xcc\x81";
    expect(run({"ok", "e" + marks, "", "x" + marks + "y" + marks}, &pieces) == TGX_OK && pieces == 3, "31 marks", -1, pieces);
    {
        const std::vector<std::string> rows = {"ok", "", "e" + marks + acute, "e" + marks, "o" + marks + acute + "!"};
        std::vector<uint8_t> text;
        std::vector<uint64_t> offs(1, 0);
        for (const std::string& r : rows) {
            text.insert(text.end(), r.begin(), r.end());
            offs.push_back(text.size());
        }
        const std::unique_ptr<uint8_t[]> b_text = block_of(text);
        const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
        uint8_t* got = nullptr;
        uint64_t *got_offs = nullptr, P = 0;
        tgx::host::g_err_sample = ~0ull;
        const tgx_status st = tgx_normalize_host(1, b_text.get(), b_offs.get(), rows.size(), &got, &got_offs, &P);
        const uint64_t row = tgx::host::g_err_sample;
        expect(st == TGX_ERR_UNSUPPORTED && !got && !got_offs && row == 2, "32 marks are refused and the lower row is named", -1, st, row);
    }
    {
        std::string jamo = ga;
        for (int k = 0; k < 3000; k++) jamo += jamo_v;
        expect(run({jamo, "tail"}, &pieces) == TGX_OK && pieces == 1, "3000 active starters", -1, pieces);
    }
    // arguments that are refused before anything is touched
    const uint64_t offs2[2] = {0, 0};
    uint8_t* ot = nullptr;
    uint64_t *oo = nullptr, P = 0;
    expect(tgx_normalize_host(4, nullptr, offs2, 1, &ot, &oo, &P) == TGX_ERR_INVALID, "form 4", -1);
    expect(tgx_normalize_host(1, nullptr, offs2, 1, nullptr, &oo, &P) == TGX_ERR_INVALID, "NULL output", -1);
    const uint64_t down[3] = {0, 2, 1};
    expect(tgx_normalize_host(1, (const uint8_t*)"ab", down, 2, &ot, &oo, &P) == TGX_ERR_INVALID, "offsets that decrease", -1);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("norm twin: ok (%d runs)\n", g_runs);
    return 0;
}
