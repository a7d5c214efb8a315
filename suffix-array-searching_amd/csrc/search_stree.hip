// search_stree.hip -- STREE / STREE_LLCP: k_sa_stree, k_sa_stree4x and their launcher.
#include "search_keys.hpp"

// ------------------------------------------------------------------ STREE
// 4-lane cooperative node reads (one request per 64-B node): lane
// j holds keys 4j..4j+3, the group sums its counts with DPP.
__device__ __forceinline__ uint32_t quad_cnt_lt(uint4 v, uint32_t K) {
    return quad_sum((v.x < K) + (v.y < K) + (v.z < K) + (v.w < K));
}
__device__ __forceinline__ uint32_t quad_cnt_eq(uint4 v, uint32_t K) {
    return quad_sum((v.x == K) + (v.y == K) + (v.z == K) + (v.w == K));
}

// Descend the internal layers for key K; returns the leaf node index (within
// the leaf layer).  sst/s_tree.rs:196-203 with unsigned keys.  LDS layers, then
// HBM layers (separate loops: ds_read / global_load, not FLAT).
__device__ __forceinline__ uint64_t stree_descend(const SearchArgs& a, const uint4* s_nodes, uint32_t K,
                                                  uint32_t sub) {
    uint64_t k = 0;
    const uint4* g = reinterpret_cast<const uint4*>(a.stree);
    uint32_t h = 0;
    for (; h < a.stree_lds_layers && h + 1 < a.stree_height; h++)
        k = k * (SAS_STREE_B + 1) + quad_cnt_lt(s_nodes[(a.stree_off[h] + k) * 4 + sub], K);
    for (; h + 1 < a.stree_height; h++) k = k * (SAS_STREE_B + 1) + quad_cnt_lt(g[(a.stree_off[h] + k) * 4 + sub], K);
    return k;
}

// The exact lower bound of q inside [r0, r1], the run of suffixes whose padded 16-char key
// is q's (the S-tree descent's result); returns its position.
// LT = false: binary search over [r0, r1] with mlr skipping from char 16 (SA + text reads).
// LT = true (SAS_ALGO_STREE_LLCP): the LLCP entries (Manber-Myers Llcp / Rlcp, SAS_BUILD_LLCP)
//   belong to the implicit binary-search tree over the whole SA, so the tail walks that tree
//   from its root: a mid outside the run is decided by the S-tree keys with no read (below r0:
//   < q; at or past r1: > q), a mid inside reads its 16-B entry and applies the LLCP rules of
//   k_sa_binary.  A bound outside the run has an lcp with q below 16 that no compare measured;
//   the first entry read after it supplies it: for a suffix a < the run (key16(a) < K) and b in
//   the run, lcp(a, b) = lcp(a, q), and symmetrically for the right bound (up to a text-end
//   suffix b shorter than 16 chars, where lcp(b, c) may fall below lcp(q, c)).  Taking the
//   entry's own Llcp / Rlcp for such a side makes that side tie (Llcp = llcp), so a probe
//   decided on it always compares (from its lcp, which b shares with q either way); a side
//   inside the run carries an exact lcp from an earlier compare or rule.  So every rule is
//   applied on an exact lcp and the result is binary_search's.
template <int QW, int W, bool LT, class Q>
__device__ __forceinline__ uint64_t stree_tail(const SearchArgs& a, const Q& q, uint32_t m, uint64_t r0,
                                               uint64_t r1, uint32_t* probes) {
    const SaView<W> sa{a.sa};
    const uint64_t n = a.n, sa_n = a.sa_n;
    if (!LT) {
        // exact lower bound inside [r0, r1]: chars [0, min(16, m)) match every suffix there
        const uint32_t h16 = m < 16 ? m : 16;
        uint64_t l = r0, r = r1;
        uint32_t llcp = h16, rlcp = h16;
        sa_val_t<W> pr = 0;
        bool have = false;
        while (l < r) {
            const uint64_t mid = (l + r) >> 1;
            const sa_val_t<W> p = (sa_val_t<W>)sa[mid];
            uint32_t lcp;
            const uint32_t h = llcp < rlcp ? llcp : rlcp;
            const bool lt = suffix_less_from<QW>(a.tw, n, p, q, h, &lcp);
            (*probes)++;
            if (lt) {
                l = mid + 1;
                llcp = lcp;
            } else {
                r = mid;
                rlcp = lcp;
                pr = p;
                have = true;
            }
        }
        if (l >= sa_n) return a.next_pos;
        return have ? (uint64_t)pr : (uint64_t)sa[l];
    }
    uint64_t l = 0, r = sa_n, pr = 0;
    uint32_t llcp = 0, rlcp = 0;
    bool have = false;
    for (;;) {
        // the walk to the next mid inside the run, ALU only: the lanes of a wave reach their
        // in-run mids at different depths, and one load per outer iteration keeps their
        // reads in lockstep (a load inside the walk would serialise their latencies)
        uint64_t mid = 0;
        while (l < r) {
            mid = (l + r) >> 1;
            if (mid < r0) l = mid + 1;       // key16 < K: < q, no read
            else if (mid >= r1) r = mid;     // key16 > K: > q, no read
            else break;
        }
        if (!(l < r)) break;
        const uint4 e = a.llcp[mid];
        const uint64_t p = (uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32);
        const uint32_t x = (e.y >> 8) & SAS_LLCP_CAP, y = e.y >> 20;
        if (l <= r0) llcp = x;  // the left bound SA[l - 1] lies before the run (or l = 0)
        if (r >= r1) rlcp = y;  // the right bound SA[r] lies past it (or r = sa_n)
        (*probes)++;
        bool lt;
        uint32_t lcp, hh = 0, inl = 0;
        bool decided = true;
        if (llcp >= rlcp) {
            if (x > llcp) { lt = true; lcp = llcp; }
            else if (x < llcp && x < SAS_LLCP_CAP) { lt = false; lcp = x; }
            else { decided = false; hh = x; inl = e.z; }
        } else {
            if (y > rlcp) { lt = false; lcp = rlcp; }
            else if (y < rlcp && y < SAS_LLCP_CAP) { lt = true; lcp = y; }
            else { decided = false; hh = y; inl = e.w; }
        }
        if (!decided) lt = llcp_tie_less<QW>(a.tw, n, p, q, hh, inl, &lcp);
        if (lt) {
            l = mid + 1;
            llcp = lcp;
        } else {
            r = mid;
            rlcp = lcp;
            pr = p;
            have = true;
        }
    }
    if (r >= sa_n) return a.next_pos;
    if (have) return pr;
    const uint4 e = a.llcp[r];  // r moved only past the run (or is r1 itself)
    return (uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32);
}

// One 4-lane group per query.  The S-tree descent and the leaf scans are
// cooperative; the exact tail search in [r0, r1] (SA + text reads) runs on all
// four lanes identically, so its loads coalesce to one request each.
template <int QW, int W>
__global__ __launch_bounds__(SAS_BIN_BLOCK, SAS_BIN_WAVES) void k_sa_stree(SearchArgs a) {
    __shared__ uint4 s_nodes[SAS_STREE_LDS_NODES * 4];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.stree);
        for (uint32_t w = threadIdx.x; w < a.stree_lds_nodes * 4; w += blockDim.x) s_nodes[w] = g[w];
        __syncthreads();
    }
    uint32_t bad = 0;
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    const uint4* g = reinterpret_cast<const uint4*>(a.stree);
    const uint64_t ol = a.stree_off[a.stree_height - 1];
    const uint64_t sa_n = a.sa_n;
    const uint64_t leaf_nodes = (sa_n + 15) / 16;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / QUAD_G;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / QUAD_G; i < a.nq; i += stride) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint32_t K = (uint32_t)(q.w[0] >> 32);  // padded 16-char key of q
        uint32_t probes = a.stree_height - 1;

        uint64_t k = stree_descend(a, s_nodes, K, sub);
        const uint4 lv = load4(g + (ol + k) * 4 + sub, a.stree_leaf_nt);
        const uint32_t c = quad_cnt_lt(lv, K), e = quad_cnt_eq(lv, K);
        probes++;
        uint64_t r0 = k * 16 + c;
        uint64_t r1 = r0 + e;
        if (c + e == 16) {  // the run of equal keys may continue in the next leaves
            uint64_t kk = k + 1;
            int steps = 0;
            for (; kk < leaf_nodes && steps < 4; kk++, steps++) {
                const uint32_t e2 = quad_cnt_eq(g[(ol + kk) * 4 + sub], K);
                probes++;
                r1 += e2;
                if (e2 < 16) break;
            }
            if (kk < leaf_nodes && steps == 4) {  // long run: lower_bound(K + 1)
                if (K == SAS_KEY_MAX) {
                    r1 = sa_n;
                } else {
                    uint64_t k2 = stree_descend(a, s_nodes, K + 1, sub);
                    probes += a.stree_height - 1;
                    r1 = k2 * 16 + quad_cnt_lt(g[(ol + k2) * 4 + sub], K + 1);
                    probes++;
                }
            }
        }
        if (r0 > sa_n) r0 = sa_n;
        if (r1 > sa_n) r1 = sa_n;
        const uint64_t pos = stree_tail<QW, W, false>(a, q, m, r0, r1, &probes);
        if (sub == 0) {
            a.out_pos[i] = pos;
            if (a.out_probes) a.out_probes[i] = probes;
        }
    }
    if (bad) atomicOr(a.bad, 1u);
}



// Long queries (QW > 1): one query per LANE, four queries per 4-lane group.
// The group walks the S-tree cooperatively for each of its four queries in turn
// (one request per 64-B node, the 16-char key taken from the owning lane), then
// every lane runs the exact tail search of its own query in parallel: the descent
// costs one request per node as in k_sa_stree, and the tail keeps the per-lane
// parallelism of a one-lane-per-query search (the text compares of long queries dominate).
template <int QW, int W, bool LT = false, bool EXQ = false>
__global__ __launch_bounds__(BIN_BLOCK(QW), BIN_WAVES(QW)) void k_sa_stree4x(SearchArgs a) {
    using QR = typename std::conditional<EXQ && (QW > 2), QueryRegsExact<QW>, QueryRegs<QW>>::type;
    __shared__ uint4 s_nodes[SAS_STREE_LDS_NODES * 4];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.stree);
        for (uint32_t w = threadIdx.x; w < a.stree_lds_nodes * 4; w += blockDim.x) s_nodes[w] = g[w];
        __syncthreads();
    }
    uint32_t bad = 0;
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    const int lane0 = (int)((threadIdx.x & 63) & ~3u);
    const uint4* g = reinterpret_cast<const uint4*>(a.stree);
    const uint64_t ol = a.stree_off[a.stree_height - 1];
    const uint64_t sa_n = a.sa_n;
    const uint64_t leaf_nodes = (sa_n + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // the loop runs while ANY query of the group is in range (group-uniform)
    for (uint64_t gi = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) - sub; gi < a.nq; gi += stride) {
        const uint64_t i = gi + sub;
        const bool mine = i < a.nq;
        const uint8_t* qb;
        uint32_t m = 0;
        QR q;
        if (mine) {
            query_ptr(a, i, &qb, &m);
            q.load(qb, m, &bad);
        } else {
            q.bytes = a.qbytes;
            q.m = 0;
            for (int j = 0; j < QW; j++) q.w[j] = 0;
        }
        const uint32_t Kmine = (uint32_t)(q.w[0] >> 32);  // padded 16-char key of this lane's query
        uint32_t probes = 0;
        uint64_t my_r0 = 0, my_r1 = 0;
        for (uint32_t j = 0; j < QUAD_G; j++) {
            if (gi + j >= a.nq) break;  // group-uniform
            const uint32_t K = (uint32_t)__shfl((int)Kmine, lane0 + (int)j, 64);
            uint32_t pr_j = a.stree_height - 1;
            const uint64_t k = stree_descend(a, s_nodes, K, sub);
            const uint4 lv = load4(g + (ol + k) * 4 + sub, a.stree_leaf_nt);
            const uint32_t c = quad_cnt_lt(lv, K), e = quad_cnt_eq(lv, K);
            pr_j++;
            uint64_t r0 = k * 16 + c, r1 = r0 + e;
            if (c + e == 16) {
                uint64_t kk = k + 1;
                int steps = 0;
                for (; kk < leaf_nodes && steps < 4; kk++, steps++) {
                    const uint32_t e2 = quad_cnt_eq(g[(ol + kk) * 4 + sub], K);
                    pr_j++;
                    r1 += e2;
                    if (e2 < 16) break;
                }
                if (kk < leaf_nodes && steps == 4) {
                    if (K == SAS_KEY_MAX) {
                        r1 = sa_n;
                    } else {
                        const uint64_t k2 = stree_descend(a, s_nodes, K + 1, sub);
                        pr_j += a.stree_height;
                        r1 = k2 * 16 + quad_cnt_lt(g[(ol + k2) * 4 + sub], K + 1);
                    }
                }
            }
            if (sub == j) {
                my_r0 = r0 > sa_n ? sa_n : r0;
                my_r1 = r1 > sa_n ? sa_n : r1;
                probes = pr_j;
            }
        }
        if (!mine) continue;
        // exact lower bound of this lane's query inside [r0, r1] (per lane)
        const uint64_t pos = stree_tail<QW, W, LT>(a, q, m, my_r0, my_r1, &probes);
        a.out_pos[i] = pos;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// STREE / STREE_LLCP
template <int W>
static void launch_stree_w(int num_cus, hipStream_t st, const SearchArgs& a, int algo, int qw) {
    const uint64_t cap = (uint64_t)num_cus * SAS_BIN_BPC;
    // m <= 32: the cooperative kernel (descent dominates; one lane per query, k_sa_stree4x, measured
    // no gain there); longer: one lane per query
    if (algo == SAS_ALGO_STREE && qw == 1)
        return launch(launch_ctx(a.nq * QUAD_G, SAS_BIN_BLOCK, cap, st), k_sa_stree<1, W>, a);
    const LaunchCtx c = launch_ctx(a.nq, BIN_BLOCK(qw), cap, st);
    with_qw_exq(qw, all_words_in_regs(a, qw), [&](auto Q, auto X) {
        constexpr int QW = decltype(Q)::value;
        constexpr bool EXQ = decltype(X)::value;
        // STREE_LLCP: the same descent, the LLCP tail (stree_tail) on one lane per query at every
        // m: the tail's walk to its in-run mids diverges between queries, which a 4-lane group
        // per query would pay 4 times over (m = 32: 1.77 ms cooperative)
        if (algo == SAS_ALGO_STREE) launch(c, k_sa_stree4x<QW, W, false, EXQ>, a);
        else launch(c, k_sa_stree4x<QW, W, true, EXQ>, a);
    });
}

void launch_stree(int num_cus, hipStream_t st, const SearchArgs& a, int algo, uint32_t sa_w, int qw) {
    if (sa_w == 5) launch_stree_w<5>(num_cus, st, a, algo, qw);
    else launch_stree_w<4>(num_cus, st, a, algo, qw);
}
