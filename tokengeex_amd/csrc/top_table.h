// The top table of encode5_kernel's TOP builds (encode5.hip): levels 0 and 1 of a trie walk from ONE gather, indexed by the
// first two text bytes, in place of the root records every block copied into its LDS (2 KiB that now hold hot score values,
// or let a block run one more wave: DESIGN.md section R9).
//
// One Trie8Rec-shaped entry per pair (b0, b1), at index b0 | b1 << 8 — the low 16 bits of the little-endian text word:
//   rec   the trie8 record of the node reached by b0 b1, label b1 in its top byte, exactly as the walk's level 1 would have
//         gathered it (so level 1's label check and next-offset arithmetic are the ordinary ones); where the trie has no
//         such node, a record whose label cannot equal b1 (b1 ^ 0xFF) with base 0
//   sref  low 16 bits: the rank of the 2-byte token b0 b1 (0: none) — the record's own;
//         high 16 bits: the rank of the 1-byte token b0 (0: none), the same for all 256 values of b1
// 65 536 entries, 512 KiB in HBM / L2.  Pure host code over the model's trie8 records: built wherever those are written,
// and remapped with them when the score values are re-ranked (both halves of sref hold ranks).
#pragma once
#include <stdint.h>

#include <vector>

#include "trie_build.h"

namespace tgx {

constexpr uint32_t kTopEntries = 1u << 16;

// rec: the model's n_slots trie8 records; root_base: the slot of the root's child by byte c is root_base ^ c.
// A slot beyond the table reads as the zero record, as the kernels' buffer loads do.
inline void build_top_table(const Trie8Rec* rec, size_t n_slots, uint32_t root_base, std::vector<Trie8Rec>* out) {
    out->assign(kTopEntries, Trie8Rec{0u, 0u});
    auto at = [&](uint32_t slot) { return slot < n_slots ? rec[slot] : Trie8Rec{0u, 0u}; };
    for (uint32_t b0 = 0; b0 < 256u; b0++) {
        const Trie8Rec r0 = at(root_base ^ b0);
        const bool have0 = (r0.rec >> 24) == b0;
        const uint32_t rank1 = have0 ? (r0.sref & kTrie8RankMask) : 0u;
        for (uint32_t b1 = 0; b1 < 256u; b1++) {
            Trie8Rec e{(b1 ^ 0xFFu) << 24, rank1 << 16};
            if (have0) {
                const Trie8Rec r1 = at(((r0.rec ^ (b1 << 3)) & 0xFFFFFFu) >> 3);
                if ((r1.rec >> 24) == b1) e = Trie8Rec{r1.rec, (r1.sref & kTrie8RankMask) | (rank1 << 16)};
            }
            (*out)[b0 | (b1 << 8)] = e;
        }
    }
}

}  // namespace tgx
