// Stand-alone driver of the table derivation (csrc/trie_build.cpp: derive_flat_trie, gather_derived_vocab) for a sanitizer
// build: tests/test_derive_native.py writes the structural cases of tests/derived_cases.py to a file, compiles this program
// with csrc/trie_build.cpp and csrc/prune_host.cpp under -fsanitize=address,undefined and runs it.  No device is opened.
//
// Per case and per link of its chain (so a second and a third derivation from a derived table too), on EVERY suffix of
// every text:
//   (a) flat_common_prefix_search on the derived table = brute force over the child's tokens = the search on a table
//       built from the child's vocabulary;
//   (b) the same through build_trie8 + trie8_common_prefix_search over the derived table;
//   (c) the same through build_trie8t + trie8t_common_prefix_search over the derived table;
//   (d) build_tok_hash over the child's bytes maps every kept token to its new id and no dropped token to any;
//   (f) tgx_prune_alternatives_flat on the derived table = the one on the table built from the child's vocabulary.
// usage: derive_main FIXTURE
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../tokengeex_amd/csrc/api_internal.h"
#include "../../tokengeex_amd/csrc/trie_build.h"

// csrc/prune_host.cpp records its messages here (csrc/tgx_api.cpp is not part of this program)
static std::string g_message;
tgx_status tgx_set_error(tgx_status st, const char* msg) {
    g_message = msg ? msg : "";
    return st;
}

namespace {

int g_failed = 0;
std::string g_where;
void expect(bool ok, const char* what) {
    if (ok) return;
    if (g_failed++ < 40) fprintf(stderr, "FAILED %s: %s\n", g_where.c_str(), what);
}

struct Reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    void need(size_t n) {
        if (n > data.size() - at) {
            fprintf(stderr, "the fixture is truncated\n");
            exit(2);
        }
    }
    uint64_t u64() {
        need(8);
        uint64_t v;
        memcpy(&v, data.data() + at, 8);
        at += 8;
        return v;
    }
    template <class T>
    std::vector<T> array(uint64_t n) {
        need(n * sizeof(T));
        std::vector<T> v(n);
        if (n) memcpy(v.data(), data.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

// token bytes as heap blocks of exactly their size: reading past the last token's end is a report
struct Vocab {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offs;  // n + 1
    std::vector<double> scores;
    uint32_t size() const { return (uint32_t)offs.size() - 1; }
    std::string token(uint32_t i) const { return std::string((const char*)bytes.data() + offs[i], (size_t)(offs[i + 1] - offs[i])); }
};

Vocab read_packed(Reader& r) {
    Vocab v;
    const uint64_t n = r.u64();
    v.offs = r.array<uint64_t>(n + 1);
    v.bytes = r.array<uint8_t>(v.offs[n]);
    return v;
}

using Matches = std::vector<std::pair<uint32_t, uint32_t>>;  // (id, length), ascending length

Matches brute(const std::unordered_map<std::string, uint32_t>& ids, uint32_t longest, const uint8_t* s, uint64_t n) {
    Matches out;
    for (uint32_t len = 1; len <= longest && len <= n; len++) {
        auto it = ids.find(std::string((const char*)s, len));
        if (it != ids.end()) out.push_back({it->second, len});
    }
    return out;
}

template <class Search>
Matches collect(uint64_t n, Search search) {
    std::vector<uint32_t> ids(n + 1), lens(n + 1);
    const uint64_t k = search(ids.data(), lens.data(), n + 1);
    Matches out;
    for (uint64_t i = 0; i < k && i < n + 1; i++) out.push_back({ids[i], lens[i]});
    if (k > n + 1) out.push_back({0xFFFFFFFFu, 0});  // more matches than bytes: never equal to the brute force
    return out;
}

struct Alternatives {
    std::vector<uint8_t> always_keep;
    std::vector<uint32_t> alt_offs, alt_ids;
    bool operator==(const Alternatives& o) const { return always_keep == o.always_keep && alt_offs == o.alt_offs && alt_ids == o.alt_ids; }
};

Alternatives alternatives(const tgx::FlatTrie& ft, const Vocab& v) {
    Alternatives a;
    a.always_keep.assign(v.size() + 1, 0);
    a.alt_offs.assign(v.size() + 1, 0);
    uint32_t* ids = nullptr;
    const int st = tgx_prune_alternatives_flat(&ft, v.bytes.data(), v.offs.data(), v.scores.data(), v.size(), a.always_keep.data(),
                                               a.alt_offs.data(), &ids);
    expect(st == 0, "tgx_prune_alternatives_flat succeeds");
    if (st == 0) a.alt_ids.assign(ids, ids + a.alt_offs[v.size()]);
    free(ids);
    return a;
}

// the child of `parent` on `cur`, checked against its own vocabulary; cur becomes the derived table
void check_link(tgx::FlatTrie* cur, Vocab* parent, const std::vector<uint32_t>& keep, const std::vector<double>& scores, const Vocab& texts) {
    const uint32_t PV = parent->size(), n_keep = (uint32_t)keep.size();
    std::vector<uint32_t> new_id(PV, tgx::kNoToken);
    for (uint32_t i = 0; i < n_keep; i++) new_id[keep[i]] = i;
    Vocab child;
    child.scores = scores;
    const uint32_t longest = tgx::gather_derived_vocab(parent->bytes.data(), parent->offs.data(), keep.data(), n_keep, &child.bytes, &child.offs);
    expect(child.offs.size() == (size_t)n_keep + 1 && child.offs[0] == 0 && child.bytes.size() == child.offs[n_keep], "the child's bytes are packed from 0");
    std::unordered_map<std::string, uint32_t> ids;
    uint32_t want_longest = 0;
    for (uint32_t i = 0; i < n_keep; i++) {
        expect(child.token(i) == parent->token(keep[i]), "token i of the child is token keep[i] of the parent");
        if (child.offs[i + 1] > child.offs[i]) ids[child.token(i)] = i;
        want_longest = std::max<uint32_t>(want_longest, (uint32_t)(child.offs[i + 1] - child.offs[i]));
    }
    expect(longest == want_longest, "gather_derived_vocab returns the longest kept token's length");

    tgx::FlatTrie derived, scratch;
    tgx::derive_flat_trie(*cur, new_id, scores.data(), longest, &derived);
    tgx::build_flat_trie(child.bytes.data(), child.offs.data(), child.scores.data(), n_keep, &scratch);
    expect(derived.table.size() == cur->table.size() && derived.tokid.size() == cur->tokid.size(), "no slot is added or freed");
    expect(derived.max_token_len == longest && scratch.max_token_len == longest, "max_token_len is the longest kept token's");
    {   // terminal bit <=> tokid <=> a kept token, with its score; check, label and inner untouched
        uint64_t terminals = 0;
        bool consistent = true, shape = true;
        for (size_t t = 0; t < derived.table.size(); t++) {
            const bool term = (derived.table[t].base & tgx::kTerminalBit) != 0;
            consistent = consistent && term == (derived.tokid[t] != tgx::kNoToken);
            if (term) {
                terminals++;
                consistent = consistent && derived.tokid[t] < n_keep && memcmp(&derived.table[t].score_bits, &scores[derived.tokid[t]], 8) == 0;
            } else {
                consistent = consistent && derived.table[t].score_bits == 0;
            }
            shape = shape && derived.table[t].check == cur->table[t].check &&
                    (derived.table[t].base & ~tgx::kTerminalBit) == (cur->table[t].base & ~tgx::kTerminalBit);
        }
        expect(consistent, "terminal bit, tokid and score agree on every slot");
        expect(shape && derived.label == cur->label && derived.inner == cur->inner, "check, base, label and inner are the parent's");
        expect(terminals == ids.size(), "one terminal slot per kept non-empty token");
    }
    tgx::Trie8 t8;
    tgx::build_trie8(derived, child.offs.data(), child.scores.data(), &t8);
    expect(t8.ok, "build_trie8 over the derived table");
    tgx::Trie8T t8t;
    tgx::build_trie8t(derived, child.offs.data(), child.scores.data(), &t8t);
    expect(t8t.ok && t8t.n_tok == ids.size(), "build_trie8t over the derived table ranks the kept tokens");

    uint64_t n_suffixes = 0, n_matches = 0;
    for (uint32_t x = 0; x < texts.size(); x++) {
        // a heap block of exactly the text's size
        const uint64_t n = texts.offs[x + 1] - texts.offs[x];
        std::vector<uint8_t> text(texts.bytes.begin() + (long)texts.offs[x], texts.bytes.begin() + (long)texts.offs[x + 1]);
        for (uint64_t p = 0; p <= n; p++) {
            const uint8_t* s = text.data() + p;
            const uint64_t m = n - p;
            const Matches want = brute(ids, longest, s, m);
            n_suffixes++;
            n_matches += want.size();
            expect(collect(m, [&](uint32_t* i, uint32_t* l, uint64_t cap) { return tgx::flat_common_prefix_search(derived, s, m, i, l, cap); }) == want,
                   "(a) the derived table's matches are the brute force's");
            expect(collect(m, [&](uint32_t* i, uint32_t* l, uint64_t cap) { return tgx::flat_common_prefix_search(scratch, s, m, i, l, cap); }) == want,
                   "(a) the from-scratch table's matches are the brute force's");
            if (t8.ok)
                expect(collect(m, [&](uint32_t* i, uint32_t* l, uint64_t cap) { return tgx::trie8_common_prefix_search(t8, derived, s, m, i, l, cap); }) == want,
                       "(b) the 8-byte records' matches are the brute force's");
            if (t8t.ok)
                expect(collect(m, [&](uint32_t* i, uint32_t* l, uint64_t cap) { return tgx::trie8t_common_prefix_search(t8t, s, m, i, l, cap); }) == want,
                       "(c) the ranked records' matches are the brute force's");
        }
    }
    expect(n_keep < 2 || n_matches > n_suffixes / 2, "the texts exercise the vocabulary");

    if (longest <= 32) {  // (d) the bytes -> id table of the trace
        tgx::TokHashTable th;
        tgx::build_tok_hash(child.bytes.data(), child.offs.data(), n_keep, &th);
        expect(th.ok, "build_tok_hash over the child's bytes");
        const auto lookup = [&](const std::string& tok) -> uint32_t {
            uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            memcpy(w, tok.data(), tok.size());
            const uint64_t h = tgx::tok_hash64_long(w, (uint32_t)tok.size(), th.seed);
            uint32_t i = (uint32_t)h & th.mask;
            for (uint32_t probe = 0; probe <= th.mask; probe++) {  // the device loop of trace_kernel
                const tgx::TokHashEntry& e = th.slots[i];
                if (!e.used) return tgx::kNoToken;
                if (e.hash == h) return e.id;
                i = (i + 1) & th.mask;
            }
            return tgx::kNoToken;
        };
        bool kept_ok = true, dropped_ok = true;
        for (uint32_t i = 0; th.ok && i < PV; i++) {
            const std::string tok = parent->token(i);
            if (tok.empty() || tok.size() > 32) continue;
            if (new_id[i] != tgx::kNoToken) kept_ok = kept_ok && lookup(tok) == new_id[i];
            else dropped_ok = dropped_ok && lookup(tok) == tgx::kNoToken;
        }
        expect(kept_ok, "(d) every kept token hashes to its new id");
        expect(dropped_ok, "(d) no dropped token hashes to any id");
    }
    if (n_keep)  // (an empty vocabulary has no score array to hand over)
        expect(alternatives(derived, child) == alternatives(scratch, child), "(f) prune alternatives on the derived table are the from-scratch table's");

    *cur = std::move(derived);
    *parent = std::move(child);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FIXTURE\n", argv[0]);
        return 2;
    }
    Reader r;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            perror(argv[1]);
            return 2;
        }
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof(buf), f)) > 0) r.data.insert(r.data.end(), buf, buf + k);
        fclose(f);
    }
    const uint64_t n_cases = r.u64();
    uint64_t n_links_total = 0;
    for (uint64_t ci = 0; ci < n_cases; ci++) {
        const uint64_t name_len = r.u64();
        const std::vector<uint8_t> name = r.array<uint8_t>(name_len);
        Vocab parent = read_packed(r);
        parent.scores = r.array<double>(parent.size());
        const uint64_t n_links = r.u64();
        std::vector<std::vector<uint32_t>> keeps;
        std::vector<std::vector<double>> scores;
        for (uint64_t k = 0; k < n_links; k++) {
            const uint64_t n_keep = r.u64();
            keeps.push_back(r.array<uint32_t>(n_keep));
            scores.push_back(r.array<double>(n_keep));
        }
        const Vocab texts = read_packed(r);
        tgx::FlatTrie cur;
        tgx::build_flat_trie(parent.bytes.data(), parent.offs.data(), parent.scores.data(), parent.size(), &cur);
        for (uint64_t k = 0; k < n_links; k++) {
            g_where = std::string(name.begin(), name.end()) + " link " + std::to_string(k + 1);
            check_link(&cur, &parent, keeps[k], scores[k], texts);  // (e): link k + 1 derives from the derived table of link k
            n_links_total++;
        }
    }
    if (r.at != r.data.size()) {
        fprintf(stderr, "the fixture has %zu bytes left over\n", r.data.size() - r.at);
        return 2;
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("derive: ok (%llu cases, %llu derivations)\n", (unsigned long long)n_cases, (unsigned long long)n_links_total);
    return 0;
}
