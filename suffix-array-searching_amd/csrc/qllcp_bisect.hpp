// The ALU-only bisect step of k_sa_quad_llcp's walk (search_quad_llcp.hip), on the host and on the
// device, so that tests/cpp/qllcp_bisect_check.cpp can drive the very code the kernel runs.
//
// The walk bisects [l, r) of the SA's ranks like binary_search (sas/sa_search.rs:98-112), but
// the group step has already bounded the answer to [L0, U]: a mid below L0 or at or past U is
// decided without a memory access.  rk_t is uint32_t for sa_n < 2^32, so l + r may not be
// formed: for sa_n in (2^31, 2^32) it wraps for every query near the SA's top, mid comes out
// small, l falls back to the bottom and the loop never ends.  l + ((r - l) >> 1) is the same
// value (l < r) and stays below r <= sa_n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One step for l < r: mid = floor((l + r) / 2); true = probe the entry at mid (L0 <= mid < U),
// false = decided here, with l = mid + 1 (mid < L0) or r = mid (mid >= U)
template <typename rk_t>
__host__ __device__ __forceinline__ bool qllcp_bisect_step(rk_t& l, rk_t& r, rk_t L0, rk_t U, rk_t& mid) {
    mid = l + ((r - l) >> 1);
    if (mid < L0) {
        l = mid + 1;
        return false;
    }
    if (mid >= U) {
        r = mid;
        return false;
    }
    return true;
}

// The walk's right bound U = 4 kU + FU cut to sa_n, formed in 64 bits: with sa_n = 2^32 - 1 the
// last leaf is kU = 2^30 - 1 and 4 kU + 4 = 2^32 would wrap to 0 in rk_t = uint32_t
template <typename rk_t>
__host__ __device__ __forceinline__ rk_t qllcp_right_bound(uint32_t kU, uint32_t fU, bool to_end, uint64_t sa_n) {
    const uint64_t u = 4 * (uint64_t)kU + fU;
    return (rk_t)(to_end || u > sa_n ? sa_n : u);
}
