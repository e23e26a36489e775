// The words of a shingle of up to 64 bytes from device memory, for the kernels that hash one per lane (minhash.hip:
// every shingle position of a row; gram.hip: every valid gram).  minhash_hash_words of minhash.h takes what they load.
// For translation units with kernels only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

// The n_words <= 8 little-endian words of the n_bytes <= 64 text bytes from text + s on, through the aligned dwords
// that cover them: up to 3 bytes in front of text + s and up to 11 behind the shingle are read, inside the 256 zeroed
// bytes of slack that a corpus's text has on either side in its allocation.  What lies past n_bytes is masked off.
__device__ inline void minhash_load_text(const uint8_t* text, uint64_t s, uint32_t n_bytes, uint64_t (&w)[8]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(text + s);
    const uint32_t r = (uint32_t)(a & 3u), sh = 8 * r;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - r);
    uint32_t d0 = n_bytes ? p[0] : 0u;  // (an empty row reads nothing)
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        w[j] = 0;
        if (8 * j < n_bytes) {
            const uint32_t d1 = p[2 * j + 1], d2 = p[2 * j + 2];
            const uint32_t lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
            const uint64_t x = (uint64_t)lo | ((uint64_t)hi << 32);
            const uint32_t left = n_bytes - 8 * j;
            w[j] = left >= 8 ? x : x & ((1ull << (8 * left)) - 1);
            d0 = d2;
        }
    }
}
// the same of n <= 16 ids from ids + s on: dword loads inside the shingle only (an id buffer has no slack to over-read)
__device__ inline void minhash_load_ids(const uint32_t* ids, uint64_t s, uint32_t n, uint64_t (&w)[8]) {
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint64_t lo = 2 * j < n ? ids[s + 2 * j] : 0u, hi = 2 * j + 1 < n ? ids[s + 2 * j + 1] : 0u;
        w[j] = lo | (hi << 32);
    }
}

}  // namespace tgx
