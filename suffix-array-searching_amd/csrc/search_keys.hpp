// search_keys.hpp -- device helpers that more than one lookup family uses: the LLCP tie (PLAIN, STREE),
// the prefix-relative pivot blocks (PLAIN, INLINE), and the predicates on a {32-char key, SA} entry
// (SECTOR, INTERP, QUAD, INLINE, PREFIX).  No kernels here.
#pragma once
#include "search_args.hpp"

// LLCP tie: the first h chars of suffix p are known equal to q's; inl = the suffix's
// chars [h, h + 16) from its LLCP entry.  Same result as suffix_less_from(.., h, ..),
// which only runs when those 16 chars match and both strings go on.
template <int QW, class Q>
__device__ __forceinline__ bool llcp_tie_less(const uint64_t* __restrict__ tw, uint64_t n, uint64_t p,
                                              const Q& q, uint32_t h, uint32_t inl, uint32_t* lcp) {
    const uint64_t lenS = n - p;
    const uint32_t L = lenS < (uint64_t)q.m ? (uint32_t)lenS : q.m;
    if (h < L) {
        const uint32_t c = L - h < 16 ? L - h : 16;
        const uint32_t mk = ~0u << (32 - 2 * c);  // c >= 1
        const uint32_t av = inl & mk, bv = (uint32_t)(q.chars32(h) >> 32) & mk;
        if (av != bv) {
            *lcp = h + (uint32_t)(__clz(av ^ bv) >> 1);
            return av < bv;
        }
        if (h + 16 < L) return suffix_less_from<QW>(tw, n, p, q, h + 16, lcp);
    }
    *lcp = L;
    return lenS < (uint64_t)q.m;
}

// The rel blocks' LDS groups (common.hpp RelLayout) into a workgroup's LDS: 16-B copies
__device__ __forceinline__ void stage_rel(uint4* s, const uint8_t* __restrict__ rel, uint32_t bytes) {
    const uint4* src = reinterpret_cast<const uint4*>(rel);
    for (uint32_t w = threadIdx.x; w < bytes / 16; w += blockDim.x) s[w] = src[w];
}
// Node k's block at level it (the root of group g, hh levels): from LDS for the staged groups,
// else two (one) 16-B loads of one line, issued together (one request)
__device__ __forceinline__ void rel_block(const SearchArgs& a, const uint4* s, uint32_t g, uint32_t it, uint32_t k,
                                          uint32_t hh, uint4& b0, uint4& b1) {
    const uint64_t off = a.rel_lay.base[g] + ((uint64_t)(k - (1u << it)) << (hh == SAS_REL_GROUP ? 5 : 4));
    if (g < a.rel_lay.lds_groups) {
        const uint32_t w = (uint32_t)off >> 4;
        b0 = s[w];
        if (hh == SAS_REL_GROUP) b1 = s[w + 1];
    } else {
        const uint4* p = reinterpret_cast<const uint4*>(a.rel + off);
        b0 = p[0];
        if (hh == SAS_REL_GROUP) b1 = p[1];
    }
}
// Slot j (1..15) of a block: the pivot's chars [P, P + 8) (slot 0 = P)
__device__ __forceinline__ uint32_t rel_slot(const uint4& b0, const uint4& b1, uint32_t j) {
    const uint4 v = j >= 8 ? b1 : b0;
    const uint32_t cw = (j >> 1) & 3u;
    const uint32_t wv = cw == 0 ? v.x : cw == 1 ? v.y : cw == 2 ? v.z : v.w;
    return ((j & 1u) ? (wv >> 16) : wv) & 0xFFFFu;
}

// Lower bound = first rank x with suffix(x) >= q.  In the sector tree that
// predicate is read off the fused leaf entry (key = first 32 chars, sa):
//   key != K64(q)          ->  key > K64
//   key == K64, m <= 32    ->  n - sa >= m   (equal padded prefixes: the shorter
//                                             suffix is a proper prefix of q)
//   key == K64, m > 32     ->  exact compare from char 32 (text read)
// suffix(p) < q when the first 32 chars are known equal (m > 32).  The windows
// past char 32 are all needed when q occurs at p (every positive answer), so the
// text words are loaded in chunks of up to 4 windows before any compare: their
// latencies overlap instead of chaining load -> compare -> branch per window.
template <int QW>
__device__ __forceinline__ bool tail_less32(const uint64_t* __restrict__ tw, uint64_t n, uint64_t p,
                                            const QueryRegs<QW>& q) {
    const uint64_t lenS = n - p;
    const uint32_t L = lenS < (uint64_t)q.m ? (uint32_t)lenS : q.m;
    const uint64_t w0 = (p + 32) >> 5;
    const uint32_t sh = (uint32_t)(p & 31) << 1;
    for (uint32_t off = 32, wi = 0; off < L; off += 128, wi += 4) {
        uint64_t wd[5];
#pragma unroll
        for (int i = 0; i < 5; i++) wd[i] = (off + 32 * i <= L + 31) ? tw[w0 + wi + i] : 0ull;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t o = off + 32 * i;
            if (o >= L) break;
            const uint32_t c = L - o < 32 ? L - o : 32;
            const uint64_t mk = chars_mask(c);
            const uint64_t t = (sh ? ((wd[i] << sh) | (wd[i + 1] >> (64 - sh))) : wd[i]) & mk;
            const uint64_t b = q.chars32(o) & mk;
            if (t != b) return t < b;
        }
    }
    return lenS < (uint64_t)q.m;
}

// PREFETCH: load the tail's text words up front (tail_less32); measured faster for
// the per-lane sector kernel, slower for the 4-lane quad kernel (register spills).
// SHORT1: QW == 1 means m <= 32 (qw_for), so the text compare is dead code there;
// false for kernels that hold fewer query words in registers than the query has.
template <int QW, bool PREFETCH = false, bool SHORT1 = true, class Q = QueryRegs<QW>>
__device__ __forceinline__ bool sector_ge(uint64_t key, uint64_t p, uint64_t K64, const SearchArgs& a,
                                          const Q& q) {
    if (key != K64) return key > K64;
    if ((SHORT1 && QW == 1) || q.m <= 32) return (a.n - p) >= (uint64_t)q.m;
    if (PREFETCH) return !tail_less32<QW>(a.tw, a.n, p, q);
    uint32_t lcp;
    return !suffix_less_from<QW>(a.tw, a.n, p, q, 32, &lcp);
}

// UPPER predicate for occurrence ranges: the first min(m, len) chars of
// suffix(x) compare > q (x is past every suffix that starts with q).
//   m <= 32: key > Q3, Q3 = q's 32-char key padded with 3s instead of 0s
//   m >  32: key != K64 -> key > K64; else exact compare from char 32
template <int QW>
__device__ __forceinline__ bool sector_gt_prefix(uint64_t key, uint64_t p, uint64_t K64, uint64_t Q3,
                                                 const SearchArgs& a, const QueryRegs<QW>& q) {
    if (QW == 1 || q.m <= 32) return key > Q3;
    if (key != K64) return key > K64;
    uint32_t lcp;
    bool lt = suffix_less_from<QW>(a.tw, a.n, p, q, 32, &lcp);
    return !lt && lcp < q.m;
}

#define QUAD_NO_SA (~0ull)  // "SA value not read yet" (never a valid 40-bit SA)
