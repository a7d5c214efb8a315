// mem_extend.hpp -- the scalar steps of a maximal-exact-match extension (sas_mems.hip:
// k_mem_verify) on 2-bit packed words, 32 chars a word, the first char in the top two bits.
//
// They are __host__ __device__ so that tests/cpp/mem_extend_check.cpp drives the very code the
// kernel runs (the precedent of csr_tile.hpp and layout.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The first of the leading c chars (c in [0, 32]) at which the packed words a and b differ, c
// if they agree on all of them: chars at and past c take no part, whatever they hold (the zero
// padding behind a text or a query is code 0 = 'A' and would otherwise extend a match)
__host__ __device__ __forceinline__ uint32_t mem_first_diff(uint64_t a, uint64_t b, uint32_t c) {
    const uint64_t x = a ^ b;
    uint64_t d = (x | (x >> 1)) & 0x5555555555555555ull;  // one bit per differing char
    if (c < 32) d &= c ? ~0ull << (64 - 2 * c) : 0ull;
    if (d == 0) return c;
    return (uint32_t)__builtin_clzll(d) >> 1;
}

// One step of an extension that has matched `len` chars and may match `bound` (len < bound): tw
// and qw hold the next 32 chars of either side.  Returns the new length; the extension goes on
// while it is below `bound` and grew by a whole word
__host__ __device__ __forceinline__ uint64_t mem_extend_step(uint64_t tw, uint64_t qw, uint64_t len, uint64_t bound,
                                                             bool* more) {
    const uint32_t c = bound - len < 32 ? (uint32_t)(bound - len) : 32u;
    const uint32_t f = mem_first_diff(tw, qw, c);
    *more = f == 32 && len + 32 < bound;
    return len + f;
}

// char p of a packed text
__host__ __device__ __forceinline__ uint32_t mem_text_char(const uint64_t* __restrict__ tw, uint64_t p) {
    return (uint32_t)(tw[p >> 5] >> (62 - 2 * (p & 31))) & 3u;
}
