// Stand-alone driver of encode5_kernel's top table (csrc/top_table.h) and LDS layout (csrc/encode5_layout.h) for a sanitizer
// build: tests/test_top_table_native.py compiles it with csrc/trie_build.cpp under -fsanitize=address,undefined and runs it.
// No device is opened.
//
//   (a) For small random vocabularies — with missing single bytes, 1-byte tokens without children, the bytes 0x00 and
//       0xFF in either place, duplicate tokens — every one of the 65 536 entries against a brute-force walk of the
//       vocabulary itself: the 1-byte rank, the 2-byte rank, whether a longer token goes on through (b0, b1), and then
//       the record the entry must carry (the trie8 record of that node: label b1; else a label that cannot equal b1).
//   (b) The table survives the re-rank's arithmetic: both halves of sref remapped through a permutation are what the
//       table built from remapped records holds.
//   (c) encode5_max_hot of the TOP layout is exact for every (waves, ppl, budget): its answer fits, its answer + 1 does
//       not; the layout with the root copy still fits its own answer.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../tokengeex_amd/csrc/encode5_layout.h"
#include "../../tokengeex_amd/csrc/top_table.h"
#include "../../tokengeex_amd/csrc/trie_build.h"

namespace {

int g_failed = 0;
std::string g_where;
void expect(bool ok, const char* what) {
    if (ok) return;
    if (g_failed++ < 40) fprintf(stderr, "FAILED %s: %s\n", g_where.c_str(), what);
}

struct Vocab {
    std::vector<std::string> toks;
    std::vector<double> scores;
};

// every table the encode pass builds over a vocabulary, from heap blocks of exactly their size
struct Built {
    tgx::FlatTrie ft;
    tgx::Trie8 t8;
    std::vector<tgx::Trie8Rec> top;
};
void build(const Vocab& v, Built* b) {
    const uint32_t n = (uint32_t)v.toks.size();
    size_t total = 0;
    for (const std::string& t : v.toks) total += t.size();
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[total ? total : 1]);
    std::unique_ptr<uint64_t[]> offs(new uint64_t[n + 1]);
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        offs[i] = at;
        memcpy(bytes.get() + at, v.toks[i].data(), v.toks[i].size());
        at += v.toks[i].size();
    }
    offs[n] = at;
    tgx::build_flat_trie(bytes.get(), offs.get(), v.scores.data(), n, &b->ft);
    tgx::build_trie8(b->ft, offs.get(), v.scores.data(), &b->t8);
    // the records as a heap block of exactly n_slots: a slot index past the table is a report
    const size_t ns = b->t8.rec.size();
    std::unique_ptr<tgx::Trie8Rec[]> rec(new tgx::Trie8Rec[ns ? ns : 1]);
    if (ns) memcpy(rec.get(), b->t8.rec.data(), ns * sizeof(tgx::Trie8Rec));
    tgx::build_top_table(rec.get(), ns, b->t8.root_base, &b->top);
}

// the rank of the score value of the LAST token with these bytes (a later duplicate overwrites an earlier one), 0: no such token
uint32_t rank_of(const Vocab& v, const tgx::Trie8& t8, const std::string& s) {
    for (size_t i = v.toks.size(); i-- > 0;) {
        if (v.toks[i] != s) continue;
        uint64_t bits;
        memcpy(&bits, &v.scores[i], 8);
        for (uint32_t r = 1; r < t8.values.size(); r++)
            if (t8.values[r] == bits) return r;
        return 0xFFFFFFFFu;  // a token whose value has no rank: reported by the caller's comparison
    }
    return 0u;
}

void check_vocab(const Vocab& v, const char* name) {
    g_where = name;
    Built b;
    build(v, &b);
    expect(b.t8.ok, "build_trie8 succeeds");
    if (!b.t8.ok) return;
    expect(b.top.size() == tgx::kTopEntries, "65 536 entries");
    if (b.top.size() != tgx::kTopEntries) return;
    // brute force: which single bytes and pairs are tokens, which pairs are prefixes of anything (the node exists)
    std::vector<uint8_t> node2(65536, 0);
    for (const std::string& t : v.toks)
        if (t.size() >= 2) node2[(uint8_t)t[0] | ((uint32_t)(uint8_t)t[1] << 8)] = 1;
    const std::vector<tgx::Trie8Rec>& rec = b.t8.rec;
    for (uint32_t b0 = 0; b0 < 256; b0++) {
        const uint32_t rank1 = rank_of(v, b.t8, std::string(1, (char)b0));
        for (uint32_t b1 = 0; b1 < 256; b1++) {
            const tgx::Trie8Rec e = b.top[b0 | (b1 << 8)];
            char where[64];
            snprintf(where, sizeof where, "%s (%02x %02x)", name, b0, b1);
            g_where = where;
            expect((e.sref >> 16) == rank1, "upper half of sref = rank of the 1-byte token b0, for every b1");
            std::string two(1, (char)b0);
            two.push_back((char)b1);
            const uint32_t rank2 = rank_of(v, b.t8, two);
            if (node2[b0 | (b1 << 8)]) {
                expect((e.rec >> 24) == b1, "the node exists: the entry's label is b1");
                expect((e.sref & tgx::kTrie8RankMask) == rank2, "lower half of sref = rank of the 2-byte token");
                // the entry is the trie8 record a two-level walk arrives at
                const uint32_t s0 = b.t8.root_base ^ b0;
                expect(s0 < rec.size() && (rec[s0].rec >> 24) == b0, "the root has the child b0");
                if (s0 < rec.size()) {
                    const uint32_t s1 = ((rec[s0].rec ^ (b1 << 3)) & 0xFFFFFFu) >> 3;
                    expect(s1 < rec.size() && rec[s1].rec == e.rec, "rec = the node's own trie8 record");
                }
            } else {
                expect((e.rec >> 24) != b1, "no node: a label that cannot equal b1");
                expect((e.sref & tgx::kTrie8RankMask) == 0u && rank2 == 0u, "no node: no 2-byte rank");
            }
        }
    }
    // (b) the re-rank: perm over the ranks, applied to the records and to both halves of the table's second words
    g_where = name;
    const uint32_t nv = (uint32_t)b.t8.values.size() - 1u;
    std::vector<uint32_t> perm(nv + 1u);
    std::iota(perm.begin(), perm.end(), 0u);
    std::mt19937 rng(nv * 2654435761u + 17u);
    std::shuffle(perm.begin() + 1, perm.end(), rng);
    std::vector<tgx::Trie8Rec> rec2 = rec, top2, top3 = b.top;
    for (tgx::Trie8Rec& r : rec2) r.sref = perm[r.sref & tgx::kTrie8RankMask];
    tgx::build_top_table(rec2.data(), rec2.size(), b.t8.root_base, &top2);
    for (tgx::Trie8Rec& r : top3) r.sref = (perm[r.sref & 0xFFFFu] & 0xFFFFu) | (perm[r.sref >> 16] << 16);
    bool same = top2.size() == top3.size();
    for (size_t i = 0; same && i < top2.size(); i++) same = top2[i].rec == top3[i].rec && top2[i].sref == top3[i].sref;
    expect(same, "remapping both halves of sref = rebuilding from remapped records");
}

std::string rand_token(std::mt19937& rng, const std::vector<uint8_t>& alphabet, uint32_t max_len) {
    const uint32_t len = 1u + rng() % max_len;
    std::string s;
    for (uint32_t i = 0; i < len; i++) s.push_back((char)alphabet[rng() % alphabet.size()]);
    return s;
}

void vocab_cases() {
    std::mt19937 rng(20240611u);
    {   // single bytes missing: 2-byte tokens whose first byte is no token
        Vocab v{{"ab", "ac", "b", "bcd", "zz"}, {-1.0, -2.0, -1.5, -3.0, -0.5}};
        check_vocab(v, "missing single bytes");
    }
    {   // 1-byte tokens that have no children at all
        Vocab v{{"a", "b", "c", std::string(1, '\0'), std::string(1, '\xFF')}, {-1.0, -2.0, -3.0, -4.0, -5.0}};
        check_vocab(v, "1-byte tokens, no children");
    }
    {   // 0x00 and 0xFF in either place, as tokens and as prefixes only
        Vocab v;
        const char z = '\0', f = '\xFF';
        v.toks = {std::string{z}, std::string{z, z}, std::string{z, f}, std::string{f, z}, std::string{f, f}, std::string{f, f, f},
                  std::string{'a', z}, std::string{'a', f, 'q'}, std::string{z, 'a', z}, std::string{f}};
        for (size_t i = 0; i < v.toks.size(); i++) v.scores.push_back(-1.0 - 0.25 * (double)i);
        check_vocab(v, "0x00 and 0xFF");
    }
    {   // duplicates: the later one's score is the payload; duplicates of 1- and 2-byte tokens with shared and own values
        Vocab v{{"a", "ab", "a", "ab", "abc", "b", "b", "ab"}, {-1.0, -2.0, -3.0, -2.0, -1.0, -7.0, -8.0, -9.0}};
        check_vocab(v, "duplicates");
    }
    {   // one token only, two bytes
        Vocab v{{"xy"}, {-1.0}};
        check_vocab(v, "one 2-byte token");
    }
    for (int round = 0; round < 12; round++) {
        // small alphabets make dense tries, the full byte range sparse ones; some rounds leave out every single byte
        std::vector<uint8_t> alphabet;
        const uint32_t na = round % 3 == 0 ? 256u : 2u + rng() % 12u;
        for (uint32_t i = 0; i < na; i++) alphabet.push_back(na == 256u ? (uint8_t)i : (uint8_t)(rng() % 256u));
        if (round % 4 == 1) alphabet[0] = 0x00, alphabet[1] = 0xFF;
        Vocab v;
        const uint32_t n = 20u + rng() % 300u;
        const uint32_t n_scores = round % 2 ? 7u : n;  // shared values, or a value per token
        for (uint32_t i = 0; i < n; i++) {
            std::string t = rand_token(rng, alphabet, 1u + (uint32_t)round % 6u);
            if (round % 4 == 2 && t.size() == 1) t.push_back((char)alphabet[rng() % alphabet.size()]);  // no single bytes at all
            v.toks.push_back(t);
            v.scores.push_back(-1.0 - (double)(rng() % n_scores) / 8.0);
        }
        if (round % 5 == 0) {  // duplicates with other scores
            for (uint32_t i = 0; i < 10; i++) {
                v.toks.push_back(v.toks[rng() % n]);
                v.scores.push_back(-40.0 - (double)i);
            }
        }
        char name[32];
        snprintf(name, sizeof name, "random %d", round);
        check_vocab(v, name);
    }
}

void layout_cases() {
    g_where = "layout";
    const uint32_t cu = 160u * 1024u;
    for (int waves = 1; waves <= 16; waves++)
        for (int ppl = 1; ppl <= 4; ppl++)
            for (uint32_t budget : {cu, cu / 2u, cu / 3u, cu / 4u, cu / 8u, 84u * 1024u, 12345u}) {
                char where[64];
                snprintf(where, sizeof where, "layout waves %d ppl %d budget %u", waves, ppl, budget);
                g_where = where;
                const uint32_t n = tgx::encode5_max_hot(false, waves, ppl, budget, true);
                uint32_t list_off = 0, root_off = 0, idx_off = 0;
                if (n) {
                    const uint32_t lds = tgx::encode5_lds_layout(n, false, waves, ppl, &list_off, &root_off, &idx_off, true);
                    expect(lds <= budget, "the answer fits");
                    expect((idx_off & 511u) == 0u && idx_off >= 8u * (n + 1u) && root_off <= idx_off, "table below the 512-aligned index buffers");
                    expect(lds == idx_off + (uint32_t)waves * (uint32_t)ppl * tgx::kE5GroupBytes, "index buffers to the end");
                }
                expect(tgx::encode5_lds_layout(n + 1u, false, waves, ppl, nullptr, nullptr, nullptr, true) > budget, "the answer + 1 does not fit");
                // the layout with the root copy keeps its estimate: it fits, and holds at most 255 values fewer than TOP's exact answer + the copy's 256
                const uint32_t n_old = tgx::encode5_max_hot(false, waves, ppl, budget, false);
                if (n_old) expect(tgx::encode5_lds_layout(n_old, false, waves, ppl, nullptr, nullptr, nullptr, false) <= budget, "root-copy layout: its answer fits");
                expect(n_old <= n, "the TOP layout holds at least as many values");
                const uint32_t lds_old = tgx::encode5_lds_layout(100u, false, waves, ppl, nullptr, &root_off, &idx_off, false);
                expect(idx_off >= root_off + tgx::kE5RootBytes && lds_old > idx_off, "root-copy layout: 2 KiB of root records below the index buffers");
            }
    g_where = "layout, the issue's figures";
    expect(tgx::encode5_lds_layout(9652u, false, 13, 3, nullptr, nullptr, nullptr, false) == 159232u, "13 waves with the root copy: 159 232 bytes");
    expect(tgx::encode5_lds_layout(9652u, false, 14, 3, nullptr, nullptr, nullptr, false) == 165376u, "14 waves with the root copy: 165 376 bytes");
    expect(tgx::encode5_lds_layout(9652u, false, 14, 3, nullptr, nullptr, nullptr, true) == 163328u, "14 waves without: 163 328 bytes");
    expect(tgx::encode5_max_hot(false, 14, 3, cu, true) == 9727u, "14 waves x 3 positions: 9 727 values");
    expect(tgx::encode5_max_hot(false, 13, 3, cu, false) == 10112u, "13 waves x 3 positions with the root copy: as before");
    expect(tgx::encode5_max_hot(false, 16, 3, cu, false) == 7808u, "16 waves x 3 positions with the root copy: as before");
}

}  // namespace

int main() {
    vocab_cases();
    layout_cases();
    if (g_failed) {
        fprintf(stderr, "top table: %d checks failed\n", g_failed);
        return 1;
    }
    printf("top table: ok\n");
    return 0;
}
