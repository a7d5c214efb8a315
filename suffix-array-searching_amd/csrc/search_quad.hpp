// search_quad.hpp -- the quad tree's leaves as QUAD, INLINE, QUAD_LLCP and PREFIX read them, and the
// staging of its top layers (QUAD, QUAD_LLCP).  No kernels here.
#pragma once
#include "search_keys.hpp"

// Levels far larger than the 256 MiB Infinity Cache (quad_nt_from.., the leaves when
// quad_leaf_nt) are read with non-temporal loads so they do not evict the upper layers
// from L2; the query stream and the positions likewise (SAS_QUAD_NT_IO).  Same-box
// A/B at n = 2^30 (tools/ab_nt.sh): absolute layout 0.760 -> 0.713 ms, relative
// 0.790 -> 0.734 ms; NT on a level that partly fits the Infinity Cache (the 554 MB
// relative leaf-parent layer, the 59 MB absolute one) made it slower.
#ifndef SAS_QUAD_NT_IO
#define SAS_QUAD_NT_IO 1
#endif
__device__ __forceinline__ uint4 quad_leaf_load(const SearchArgs& a, const uint4* p) {
    return a.quad_leaf_nt ? nt_load4(p) : *p;
}

// Leaf formats (KO = key-only, SAS_BUILD_QUAD_COMPACT):
//   fused: entry x = 16 B {key64, SA lo32, SA bits 32..39}, 4 per 64-B leaf
//   KO:    entry x = key64, 8 per 64-B leaf; SA values come from the SA array
// Per-lane reads of one entry (the tails of the 4x kernel, INLINE's probes):
template <bool KO>
__device__ __forceinline__ uint64_t quad_entry_key(const SearchArgs& a, uint64_t x) {
    if (KO) return reinterpret_cast<const uint64_t*>(a.quad_leaves)[x];
    const uint2 k = reinterpret_cast<const uint2*>(a.quad_leaves)[2 * x];
    return (uint64_t)k.x | ((uint64_t)k.y << 32);
}
template <bool KO, int W>
__device__ __forceinline__ uint64_t quad_entry_sa(const SearchArgs& a, uint64_t x) {
    if (KO) return SaView<W>{a.sa}[x];
    const uint2 s = reinterpret_cast<const uint2*>(a.quad_leaves)[2 * x + 1];
    return (uint64_t)s.x | ((uint64_t)(s.y & 0xFFu) << 32);
}

__device__ __forceinline__ void stage_quad_top(const SearchArgs& a, uint4* s_nodes) {
    for (uint32_t w = threadIdx.x; w < a.quad_lds_nodes * 4; w += blockDim.x) s_nodes[w] = a.quad_inner[w];
    __syncthreads();
}
