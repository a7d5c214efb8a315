// build_lcp.hip -- what is computed from adjacent SA entries: the LCP array, the LLCP / RLCP
// entries of the binary search's intervals, and the check that an SA is one (sas_verify,
// SAS_BUILD_VERIFY).
#include "build_util.hpp"
#include "build_steps.hpp"

// ------------------------------------------------------------------ LCP
// Kernels below take the text length n (suffix lengths) and the number of SA
// entries sa_n separately: a shard index holds a rank range of the global SA.
template <int W>
__global__ void k_lcp(const uint64_t* __restrict__ tw, uint64_t n, SaView<W> sa, uint64_t sa_n,
                      uint32_t* __restrict__ lcp) {
    GRID_STRIDE(r, sa_n) {
        if (r == 0) { lcp[0] = 0; continue; }
        uint64_t a = sa[r - 1], b = sa[r];
        uint64_t L = n - (a > b ? a : b);  // min suffix length
        uint64_t l = 0;
        while (l < L) {
            uint64_t x = text_chars32(tw, a + l) ^ text_chars32(tw, b + l);
            if (x) { l += __clzll(x) >> 1; break; }
            l += 32;
        }
        l = l < L ? l : L;
        lcp[r] = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l;
    }
}

int build_lcp(sas_index* x) {
    const uint64_t sa_n = x->sa_n;
    DevBuf l;
    TRY(l.alloc(sa_n * 4, "lcp"));
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(k_lcp<W>, dim3(grid_for(sa_n)), dim3(256), 0, 0, x->text_w, x->n, SaView<W>{x->sa}, sa_n,
                           l.as<uint32_t>());
    });
    HIP_TRY(hipGetLastError());
    x->lcp = static_cast<uint32_t*>(l.release());
    return 0;
}

// ------------------------------------------------------------------ LLCP / RLCP
// The Manber-Myers accelerant behind SAS_ALGO_LLCP.  binary_search's loop over
// [0, sa_n) (sas/sa_search.rs:98-112) probes rank m in exactly one interval [l, r):
// the one whose mid (l + r) / 2 is m.  Entry m (16 B) holds, for that interval,
//   .x, .y  SA[m] (40 bits) | Llcp << 40 | Rlcp << 52 (12 bits each, capped at
//           SAS_LLCP_CAP): Llcp = lcp(SA[l-1], SA[m]) = min LCP[l..m],
//           Rlcp = lcp(SA[m], SA[r]) = min LCP[m+1..r], LCP[0] = LCP[sa_n] = 0
//           standing for the virtual bounds (no inference there);
//   .z      16 chars of suffix SA[m] from char Llcp,  .w  16 chars from char Rlcp
//           (2-bit packed, first char high, zero past the text end): the chars a
//           tie compares first, so a tie rarely reads text.
// Built bottom-up over the implicit tree, one launch per depth: min LCP[l..m] is the
// smaller of the left child's two values (LCP[m] when that child is empty), and
// likewise on the right; a min of capped values is the capped min.
// Depth of rank m's interval, or maxd + 1 when it is deeper than maxd.
__device__ __forceinline__ uint32_t bs_node(uint64_t sa_n, uint64_t m, uint32_t maxd, uint64_t* l, uint64_t* r) {
    uint64_t lo = 0, hi = sa_n;
    uint32_t d = 0;
    for (;;) {
        const uint64_t mid = (lo + hi) >> 1;
        if (mid == m) break;
        if (d == maxd) return maxd + 1;
        if (m < mid) hi = mid;
        else lo = mid + 1;
        d++;
    }
    *l = lo;
    *r = hi;
    return d;
}

template <int W>
__global__ void k_llcp_level(const uint64_t* __restrict__ tw, SaView<W> sa, const uint32_t* __restrict__ lcp,
                             uint64_t sa_n, uint32_t depth, uint4* __restrict__ e) {
    GRID_STRIDE(m, sa_n) {
        uint64_t l = 0, r = 0;
        if (bs_node(sa_n, m, depth, &l, &r) != depth) continue;
        auto lcp_at = [&](uint64_t i) -> uint64_t {
            return (i == 0 || i >= sa_n) ? 0ull : (lcp[i] < SAS_LLCP_CAP ? lcp[i] : SAS_LLCP_CAP);
        };
        auto child_min = [&](uint64_t c) -> uint64_t {
            const uint4 v = e[c];
            const uint64_t a = (v.y >> 8) & SAS_LLCP_CAP, b = v.y >> 20;
            return a < b ? a : b;
        };
        const uint64_t L = l < m ? child_min((l + m) >> 1) : lcp_at(m);
        const uint64_t R = m + 1 < r ? child_min((m + 1 + r) >> 1) : lcp_at(r);
        const uint64_t p = sa[m];
        const uint64_t lo = p | (L << 40) | (R << 52);
        // L, R <= n - p (an lcp never exceeds the suffix), so these reads stay inside
        // the padded text
        e[m] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)(text_chars32(tw, p + L) >> 32),
                          (uint32_t)(text_chars32(tw, p + R) >> 32));
    }
}

int build_llcp(sas_index* x) {
    const uint64_t sa_n = x->sa_n;
    DevBuf e;
    TRY(e.alloc(sa_n * 16, "llcp entries"));
    const uint32_t depths = 64 - __builtin_clzll(sa_n);  // binary_search iterations
    for (int d = (int)depths - 1; d >= 0; d--) {
        with_sa_w(x->sa_w, [&](auto Wc) {
            constexpr int W = decltype(Wc)::value;
            hipLaunchKernelGGL(k_llcp_level<W>, dim3(grid_for(sa_n)), dim3(256), 0, 0, x->text_w, SaView<W>{x->sa},
                               x->lcp, sa_n, (uint32_t)d, e.as<uint4>());
        });
    }
    HIP_TRY(hipGetLastError());
    x->llcp = e.as<uint4>();
    e.release();
    return 0;
}

// ------------------------------------------------------------------ verify
template <int W>
__global__ void k_verify_adj(const uint64_t* __restrict__ tw, uint64_t n, SaView<W> sa,
                             uint64_t sa_n, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ bad) {
    GRID_STRIDE(r, sa_n) {
        uint64_t b = sa[r];
        if (b >= n) { atomicOr(bad, 1u); continue; }
        if (bitmap) atomicOr(&bitmap[b >> 5], 1u << (b & 31));
        if (r == 0) continue;
        uint64_t a = sa[r - 1];
        if (a >= n) continue;
        uint64_t la = n - a, lb = n - b, L = la < lb ? la : lb, l = 0;
        bool lt;
        for (;;) {
            if (l >= L) { lt = la < lb; break; }
            uint64_t c = L - l < 32 ? L - l : 32;
            uint64_t mk = chars_mask((uint32_t)c);
            uint64_t x = text_chars32(tw, a + l) & mk, y = text_chars32(tw, b + l) & mk;
            if (x != y) { lt = x < y; break; }
            l += 32;
        }
        if (!lt) atomicOr(bad, 2u);  // sas/sa_search.rs:36-38 assert!(t[x..] < t[y..])
    }
}

__global__ void k_count_bits(const uint32_t* __restrict__ bitmap, uint64_t words, unsigned long long* cnt) {
    unsigned long long c = 0;
    GRID_STRIDE(w, words) c += __popc(bitmap[w]);
    if (c) atomicAdd(cnt, c);
}

// full = the SA must be a permutation of 0..n (false for a shard's rank range)
int verify_sa(const uint64_t* tw, uint64_t n, const uint8_t* sa, uint32_t w, uint64_t sa_n, bool full) {
    DevBuf bitmap, bad;
    uint64_t words = (n + 31) / 32;
    if (full) {
        TRY(bitmap.alloc(words * 4, "verify bitmap"));
        HIP_TRY(hipMemset(bitmap.p, 0, words * 4));
    }
    TRY(bad.alloc(16, "verify flags"));
    HIP_TRY(hipMemset(bad.p, 0, 16));
    if (w == 8)
        hipLaunchKernelGGL(k_verify_adj<8>, dim3(grid_for(sa_n)), dim3(256), 0, 0, tw, n, SaView<8>{sa}, sa_n,
                           full ? bitmap.as<uint32_t>() : nullptr, bad.as<uint32_t>());
    else if (w == 5)
        hipLaunchKernelGGL(k_verify_adj<5>, dim3(grid_for(sa_n)), dim3(256), 0, 0, tw, n, SaView<5>{sa}, sa_n,
                           full ? bitmap.as<uint32_t>() : nullptr, bad.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_verify_adj<4>, dim3(grid_for(sa_n)), dim3(256), 0, 0, tw, n, SaView<4>{sa}, sa_n,
                           full ? bitmap.as<uint32_t>() : nullptr, bad.as<uint32_t>());
    if (full)
        hipLaunchKernelGGL(k_count_bits, dim3(grid_for(words)), dim3(256), 0, 0, bitmap.as<uint32_t>(), words,
                           reinterpret_cast<unsigned long long*>(bad.as<uint32_t>() + 2));
    HIP_TRY(hipGetLastError());
    uint32_t h[4];
    HIP_TRY(hipMemcpy(h, bad.p, 16, hipMemcpyDeviceToHost));
    uint64_t seen = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    if (h[0] & 1) SAS_FAIL(EINVAL, "suffix array holds an entry >= n");
    if (h[0] & 2) SAS_FAIL(EINVAL, "suffix array not sorted: adjacent suffixes not strictly increasing");
    if (full && seen != n) SAS_FAIL(EINVAL, "suffix array is not a permutation of 0..n");
    return 0;
}

extern "C" int sas_verify(const sas_index* index) {
    if (!index) SAS_FAIL(EINVAL, "sas_verify: null index");
    if (index->tag_lines)
        SAS_FAIL(ENOTSUP, "sas_verify: a bucket-line index holds no SA array (verify at build: SAS_BUILD_VERIFY)");
    HIP_TRY(hipSetDevice(index->device));
    return verify_sa(index->text_w, index->n, index->sa, index->sa_w, index->sa_n, index->sa_n == index->n);
}
