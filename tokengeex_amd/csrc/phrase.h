// Literal phrase matching (include/tgx_phrases.h: tgx_phraseset_create, tgx_*_phrase_hits_device, tgx_phrase_hits_host):
// what a phrase and an occurrence are, the fold, the record format of the phrase trie with its builder, the first-level
// filter, the walk from one start position and the rule by which a row's occurrences reach its count.  The kernels of
// phrase.hip and the host twin in host_twins.cpp both go through these functions.
//
// The source has S rows, row i the elements data[offs[i] .. offs[i+1]) of eb bytes (u8 text bytes or u32 ids, little
// endian); the trie is over BYTES for both, an id phrase being 4 L bytes that is only ever entered at an element's first
// byte.  The elements of all rows are laid end to end on the tiling of gram.h: a wave takes a chunk of 64 consecutive
// elements, a block of four waves a tile of 256, and a block a run of consecutive tiles.
//
// The table is an XOR double-array of 8-byte label-checked records in the shape of Trie8TRec (trie_build.h):
//   rec = base | label << 24,  tok = index of the phrase that ends at this node + 1, or 0
// The child by byte c of a node is the record at slot (rec ^ c) & 0xFFFFFF, valid iff its label is c: one gather and one
// compare per step.  The argument of trie_build.h that nothing else can pass the check, restated for ALL 256 byte
// values (text here is arbitrary bytes, so 0x00, 0xFE and 0xFF are labels like any other):
//   - every node with children has a base of its own, so a slot t that passes the check for (base, c) has the owner
//     base t ^ c = base: it is that node's child by c and nobody else's;
//   - no base has the low byte 0xFF, and an unused slot t carries the label (t ^ 0xFF) & 0xFF: a probe (base, c) of it
//     would need c = (base ^ c ^ 0xFF) & 0xFF, i.e. a base whose low byte is 0xFF;
//   - block 0 (slots 0 .. 255) holds no node: all of it is unused slots.  A leaf points at kPhraseLeafBase = 0xFE there,
//     and its probe by c reads slot 0xFE ^ c, whose label is c ^ 1.  The root is a base only (root_base), it has no record;
//     the root of an empty set is a leaf.
// build_flat_trie is not used for the slot assignment: host_twins.cpp must link without trie_build.cpp (the native
// tests build it alone), and its assignment keeps 0xFE / 0xFF free as LABELS, which this table cannot.  The builder
// below is the table's only one, for the device set and for the twin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gram.h"
#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kPhraseFoldCase = 1u, kPhraseWholeWord = 2u;
constexpr uint32_t kPhraseMaxLen = 255;     // elements of a phrase
constexpr uint32_t kPhraseMaxBytes = 256;   // and its bytes
constexpr uint32_t kPhraseMaxSlots = 1u << 24;
constexpr uint32_t kPhraseLeafBase = 0xFEu;
constexpr uint32_t kPhraseFilterWords = 2048;  // 65 536 bits: bit b0 * 256 + b1
constexpr int kPhraseStages = 1;
// the staged text of a tile: kPhraseLead bytes in front (the last of them is the byte before the tile), the tile, and a
// halo of max_bytes (a phrase from the tile's last start, and under whole word the byte after it)
constexpr uint32_t kPhraseLead = 4;
constexpr uint32_t kPhraseStageBytes = kPhraseLead + kGramTile * 4 + kPhraseMaxBytes;

struct alignas(8) PhraseRec {
    uint32_t rec;  // base | label << 24
    uint32_t tok;  // phrase index + 1, 0: no phrase ends here
};
static_assert(sizeof(PhraseRec) == 8, "a step is one 8-byte gather");

__host__ __device__ inline uint32_t phrase_fold(uint32_t b, bool fold) { return fold && b - 0x41u < 26u ? b | 0x20u : b; }
// phrase_fold of four bytes at once (the kernel stages by dwords): a byte < 0x80 is in A-Z iff adding 0x3F carries into
// bit 7 and adding 0x25 does not; 0x7F + 0x3F < 0x100, so no carry leaves a byte
__host__ __device__ inline uint32_t phrase_fold4(uint32_t x, bool fold) {
    const uint32_t y = x & 0x7F7F7F7Fu;
    const uint32_t m = (y + 0x3F3F3F3Fu) & ~(y + 0x25252525u) & ~x & 0x80808080u;
    return fold ? x | (m >> 2) : x;
}
__host__ __device__ inline bool phrase_word_byte(uint32_t b) {
    return (b | 0x20u) - 0x61u < 26u || b - 0x30u < 10u || b == 0x5Fu || b >= 0x80u;
}
__host__ __device__ inline bool phrase_filter_pass(const uint32_t* filter, uint32_t b0, uint32_t b1) {
    const uint32_t bit = b0 * 256u + b1;
    return (filter[bit >> 5] >> (bit & 31u)) & 1u;
}

// The occurrences that begin at one start: `avail` bytes of the row are left from the start on (clipped to max_bytes + 1
// by the caller, which keeps `k + 1 == avail` meaning "the row ends here"), get(k) is the folded byte k of them.  Under
// `whole` the caller has checked the element before the start; the one after an occurrence is checked here.
// credit(p) sees the phrase of every occurrence.  -> their number and the longest one's length in elements
struct PhraseHit {
    uint32_t count, longest;
};
template <class Get, class Credit>
__host__ __device__ inline PhraseHit phrase_walk(const PhraseRec* __restrict__ table, uint32_t root_base, uint32_t elem_bytes, uint32_t avail,
                                                 uint32_t max_bytes, bool whole, Get get, Credit credit) {
    PhraseHit h = {0, 0};
    const uint32_t limit = avail < max_bytes ? avail : max_bytes;
    uint32_t node = root_base;
    for (uint32_t k = 0; k < limit; k++) {
        const uint32_t c = get(k);
        const PhraseRec r = table[(node ^ c) & 0xFFFFFFu];
        if ((r.rec >> 24) != c) break;
        node = r.rec;
        if (r.tok && (!whole || k + 1 == avail || !phrase_word_byte(get(k + 1)))) {
            h.count++;
            h.longest = (k + 1) / elem_bytes;
            credit(r.tok - 1);
        }
    }
    return h;
}

// ---- the builder (host) ----------------------------------------------------------------------------------------

struct PhraseTable {
    std::vector<PhraseRec> rec;    // n_slots, a multiple of 256
    std::vector<uint32_t> filter;  // kPhraseFilterWords
    uint32_t root_base = kPhraseLeafBase;
    uint32_t n_distinct = 0;
    uint32_t max_len = 0;  // elements of the longest phrase; 0 for an empty set
};

enum PhraseBuild { kPhraseOk = 0, kPhraseInvalid = 1, kPhraseUnsupported = 2 };

namespace phrase_detail {

struct Blocks {
    std::vector<uint64_t> free_bits, base_used;  // four words per block
    std::vector<uint16_t> n_free, fails;
    size_t first_open = 1;
    void add() {
        for (int q = 0; q < 4; q++) {
            free_bits.push_back(~0ull);
            base_used.push_back(0);
        }
        n_free.push_back(256);
        fails.push_back(0);
    }
    bool is_free(size_t blk, uint32_t s) const { return (free_bits[4 * blk + (s >> 6)] >> (s & 63)) & 1; }
    bool base_taken(size_t blk, uint32_t b) const { return (base_used[4 * blk + (b >> 6)] >> (b & 63)) & 1; }
    // a base for the children bytes c[0 .. n): every slot base ^ c free, the base's low byte below 0xFE and not yet a base
    uint32_t place(const uint8_t* c, uint32_t n) {
        while (first_open < n_free.size() && (n_free[first_open] == 0 || fails[first_open] > 16)) first_open++;
        for (size_t blk = first_open, tried = 0;; blk++) {
            if (blk == n_free.size() || tried == 8) {
                blk = n_free.size();
                add();
            }
            if (n_free[blk] < n) continue;
            tried++;
            for (uint32_t b0 = 0; b0 < 0xFE; b0++) {
                if (base_taken(blk, b0)) continue;
                bool fits = true;
                for (uint32_t j = 0; j < n && fits; j++) fits = is_free(blk, b0 ^ c[j]);
                if (!fits) continue;
                base_used[4 * blk + (b0 >> 6)] |= 1ull << (b0 & 63);
                for (uint32_t j = 0; j < n; j++) {
                    const uint32_t s = b0 ^ c[j];
                    free_bits[4 * blk + (s >> 6)] &= ~(1ull << (s & 63));
                }
                n_free[blk] -= (uint16_t)n;
                return (uint32_t)blk * 256u + b0;
            }
            fails[blk]++;
        }
    }
};

}  // namespace phrase_detail

// phrases: P phrases, phrase p the elements [offs[p], offs[p+1]) of eb bytes each.  -> kPhraseOk and *out, or the reason
// in *why.  Phrases equal after folding are one phrase under the lowest index among them.
inline PhraseBuild phrase_build_table(const void* phrases_, const uint64_t* offs, uint32_t P, uint32_t eb, uint32_t flags, PhraseTable* out,
                                      const char** why) {
    const uint8_t* phrases = static_cast<const uint8_t*>(phrases_);
    *why = nullptr;
    if (eb != 1 && eb != 4) return *why = "elem_bytes is neither 1 nor 4", kPhraseInvalid;
    if (flags & ~(kPhraseFoldCase | kPhraseWholeWord)) return *why = "unknown flags", kPhraseInvalid;
    if (flags && eb != 1) return *why = "the fold and whole-word flags need 1-byte elements", kPhraseInvalid;
    if (P && (!offs || !phrases)) return *why = "phrases or phrase_offs is NULL", kPhraseInvalid;
    for (uint32_t p = 0; p < P; p++) {
        if (offs[p + 1] < offs[p]) return *why = "phrase_offs not monotone", kPhraseInvalid;
        const uint64_t L = offs[p + 1] - offs[p];
        if (L < 1 || L > kPhraseMaxLen || L * eb > kPhraseMaxBytes) return *why = "a phrase is empty or longer than 255 elements or 256 bytes", kPhraseInvalid;
    }
    const bool fold = flags & kPhraseFoldCase;
    // folded copies, packed from 0 in bytes
    std::vector<uint64_t> at(P + 1, 0);
    for (uint32_t p = 0; p < P; p++) at[p + 1] = at[p] + (offs[p + 1] - offs[p]) * eb;
    std::vector<uint8_t> bytes(at[P]);
    for (uint32_t p = 0; p < P; p++)
        for (uint64_t k = 0; k < at[p + 1] - at[p]; k++) bytes[at[p] + k] = (uint8_t)phrase_fold(phrases[offs[p] * eb + k], fold);
    std::vector<uint32_t> order(P);
    for (uint32_t p = 0; p < P; p++) order[p] = p;
    auto cmp3 = [&](uint32_t a, uint32_t b) {
        const uint64_t la = at[a + 1] - at[a], lb = at[b + 1] - at[b];
        const int c = std::memcmp(bytes.data() + at[a], bytes.data() + at[b], (size_t)(la < lb ? la : lb));
        return c ? c : la < lb ? -1 : la > lb ? 1 : 0;
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const int c = cmp3(a, b);
        return c ? c < 0 : a < b;
    });
    std::vector<uint32_t> distinct;  // ascending bytes; of equal phrases the lowest index
    for (uint32_t k = 0; k < P; k++)
        if (k == 0 || cmp3(order[k - 1], order[k]) != 0) distinct.push_back(order[k]);
    const uint32_t D = (uint32_t)distinct.size();

    out->filter.assign(kPhraseFilterWords, 0);
    out->n_distinct = D;
    out->max_len = 0;
    out->root_base = kPhraseLeafBase;
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t p = distinct[d];
        const uint64_t nb = at[p + 1] - at[p];
        out->max_len = std::max<uint32_t>(out->max_len, (uint32_t)(nb / eb));
        const uint32_t b0 = bytes[at[p]];
        if (nb == 1)
            for (uint32_t w = 0; w < 8; w++) out->filter[b0 * 8 + w] = ~0u;
        else {
            const uint32_t bit = b0 * 256u + bytes[at[p] + 1];
            out->filter[bit >> 5] |= 1u << (bit & 31u);
        }
    }

    // a node is the range [lo, hi) of `distinct` that shares a prefix of `depth` bytes; its children are placed together
    struct Node {
        uint32_t lo, hi, depth, slot;  // slot: the node's own record (unused for the root)
    };
    phrase_detail::Blocks blocks;
    blocks.add();  // block 0: unused slots only
    blocks.n_free[0] = 0;
    struct Placed {
        uint32_t slot, rec, tok;
    };
    std::vector<Placed> placed;
    std::vector<Node> stack;
    if (D) stack.push_back({0, D, 0, 0});
    uint8_t cb[256];
    uint32_t clo[257];
    while (!stack.empty()) {
        const Node nd = stack.back();
        stack.pop_back();
        // the phrase that ends at this node, if any, is the range's first (the shortest sorts first)
        uint32_t lo = nd.lo, tok = 0;
        if (at[distinct[lo] + 1] - at[distinct[lo]] == nd.depth) {
            tok = distinct[lo] + 1;
            lo++;
        }
        uint32_t n = 0;
        for (uint32_t k = lo; k < nd.hi; k++) {
            const uint8_t c = bytes[at[distinct[k]] + nd.depth];
            if (n == 0 || cb[n - 1] != c) {
                cb[n] = c;
                clo[n] = k;
                n++;
            }
        }
        clo[n] = nd.hi;
        uint32_t base = kPhraseLeafBase;
        if (n) {
            base = blocks.place(cb, n);
            if ((uint64_t)blocks.n_free.size() * 256 > kPhraseMaxSlots) return *why = "the phrase table exceeds 2^24 slots", kPhraseUnsupported;
            for (uint32_t j = 0; j < n; j++) stack.push_back({clo[j], clo[j + 1], nd.depth + 1, base ^ cb[j]});
        }
        if (nd.depth == 0)
            out->root_base = base;
        else
            placed.push_back({nd.slot, base | (uint32_t)bytes[at[distinct[nd.lo]] + nd.depth - 1] << 24, tok});
    }
    const size_t n_slots = blocks.n_free.size() * 256;
    out->rec.resize(n_slots);
    for (size_t t = 0; t < n_slots; t++) out->rec[t] = PhraseRec{(uint32_t)((t ^ 0xFFu) & 0xFFu) << 24, 0};
    for (const Placed& q : placed) out->rec[q.slot] = PhraseRec{q.rec, q.tok};
    return kPhraseOk;
}

// The count rule is gram.h's, with the stretch's occurrences in place of its hits: gram_row_inside -> a plain store,
// otherwise an add of a non-zero sum onto the pre-set 0 (gram_adds).

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// phrase.hip.  All pointers are device memory.  count i64[S], longest u8[n_elems], per_phrase i64[n_phrases]: each may
// be NULL.  The pre-sets of count and per_phrase are queued here.
hipError_t launch_phrase_hits(const DedupRows& rows, const PhraseRec* table, const uint32_t* filter, uint32_t root_base, uint32_t max_len,
                              uint32_t flags, uint32_t n_phrases, int64_t* count, uint8_t* longest, int64_t* per_phrase, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
