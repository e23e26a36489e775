/* tgx_allow.h: the document-frequency pass of vocabulary generation with the allow pattern applied on the device, before
 * the count.  An addition to the C ABI of tgx.h in a header of its own, as tgx_find.h and tgx_hashed.h are; it includes
 * tgx_patterns64.h, whose automaton struct it reuses, and the ABI version stays 1.  Status codes, threading and last-error
 * reporting are tgx.h's.
 *
 * ---- filter first, count after (csrc/allow.hip, csrc/allow.h; the reference's src/generate.rs:78-120) -------------------
 * tgx_substring_df_top counts every char-aligned window of up to max_token_length bytes and leaves the allow regex to the
 * caller, so top_k and cutoff_df are spent on substrings the caller throws away.  Here the filter runs inside the pass:
 * only the windows an automaton accepts are hashed, sorted and counted.
 *
 * The automaton.  A tgx_dfa64, ANCHORED (the automaton of the pattern itself, patterns.compile_pattern(..., search=False,
 *   max_states=64)) and with a dead state.  Its checks are tgx_dfa64's: an automaton whose start state is tagged (it
 *   accepts the empty string) is TGX_ERR_INVALID, and so is allow == NULL.  tag[s] != 0 is "tagged".  The library finds
 *   the dead states (those from which no tagged state is reachable) itself.
 *
 * Semantics.  A window (part k, start p, length l) is a CANDIDATE under tgx_substring_df's rules: p is a character start
 *   inside the part, p + l <= part_end[k], l <= max_token_length, and the window ends on a character boundary or at the
 *   part's end.  It is ALLOWED iff the walk q = start, q = next[text[p + i]][q] for i = 0 .. l - 1 ends in a tagged state
 *   (no re-entry: the whole window matches).  An allowed candidate is KEPT iff insert_probability >= 1 or
 *   tgx_generate_u01(seed, sample, (p - origin) << 8 | l) < insert_probability: the draw is a counter hash of the
 *   occurrence, so filtering does not shift it.  The result is exactly tgx_substring_df_top's with the substrings that
 *   are not allowed taken out: the same (pos, len, df) for every allowed substring; *n_windows counts the kept windows;
 *   *n_distinct, the top_k selection and *cutoff_df are over allowed substrings only.
 *
 * tgx_substring_df_allow(device, text, n_bytes, part_begin, part_end, part_sample, part_origin, n_parts, max_token_length,
 *   insert_probability, seed, allow, top_k, out_pos, out_len, out_df, n_out, n_windows, n_collisions, n_distinct,
 *   cutoff_df): tgx_substring_df_top's arguments, checks, statuses, outputs (malloc'd, tgx_free) and collision handling
 *   (TGX_KNOBS=1 TGX_GENERATE_COLLIDE=bits forces collisions here too), plus the automaton.  top_k = 0 returns everything.
 *   The arguments are checked before a device is asked for.
 *   A lane per start byte walks the automaton over a register-held copy of its chunk's text until it dies and leaves a
 *   32-bit mask of its kept lengths (allow_mask_kernel); a second kernel hashes and writes the windows of the set bits
 *   (allow_emit_kernel), and everything from the sort on is tgx_substring_df_top's own code.  A collision retry repeats
 *   the second kernel alone.  Scratch beyond tgx_substring_df_top's: 4 bytes per text byte of masks, and the windows'
 *   32 bytes each are only paid for kept windows.
 *
 * Host twin, no device: tgx_allow_masks_host(text, n_bytes, part_begin, part_end, part_sample, part_origin, n_parts,
 *   max_token_length, insert_probability, seed, allow, mask, n_windows).  mask, u32[n_bytes]: bit l - 1 of mask[p] is
 *   set iff the window (p, l) is kept; *n_windows (may be NULL) is the number of set bits.  The checks are those of the
 *   device call.  It goes through the kernels' header (csrc/allow.h): the table, the limit, the rule that a window is
 *   settled by the byte after it, the draw.
 *
 * tgx_allow_last_times: device time per stage of the calling thread's last tgx_substring_df_allow, as tgx_find_last_times
 * (the names are listed without a call): allow_mask_kernel, allow_scan, allow_emit_kernel, allow_sort, allow_runs (heads,
 * run ids, counts and the collision check, with the host's read of the run count in between), allow_top.  After a
 * collision retry the last four are those of the last attempt. */
#ifndef TGX_ALLOW_H
#define TGX_ALLOW_H

#include "tgx_patterns64.h"

#ifdef __cplusplus
extern "C" {
#endif

tgx_status tgx_substring_df_allow(int device, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_begin, const uint64_t *part_end, const uint32_t *part_sample, const uint64_t *part_origin, uint64_t n_parts, uint32_t max_token_length, double insert_probability, uint64_t seed, const tgx_dfa64 *allow, uint64_t top_k, uint64_t **out_pos, uint32_t **out_len, uint32_t **out_df, uint64_t *n_out, uint64_t *n_windows, uint64_t *n_collisions, uint64_t *n_distinct, uint32_t *cutoff_df);
tgx_status tgx_allow_masks_host(const uint8_t *text, uint64_t n_bytes, const uint64_t *part_begin, const uint64_t *part_end, const uint32_t *part_sample, const uint64_t *part_origin, uint64_t n_parts, uint32_t max_token_length, double insert_probability, uint64_t seed, const tgx_dfa64 *allow, uint32_t *mask, uint64_t *n_windows);
int tgx_allow_last_times(const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif

#endif /* TGX_ALLOW_H */
