// search_quad_llcp.hip -- QUAD_LLCP past 32 chars: k_sa_quad_llcp and its launcher.
#include "search_quad.hpp"
#include "qllcp_bisect.hpp"

// quad_x0_finish for a query of m <= 32 chars on fused leaves: the 32-char key and the
// suffix length decide every entry (sector_ge's m <= 32 case), so no text is compared
__device__ __forceinline__ uint64_t quad_short_finish(const SearchArgs& a, uint64_t K64, uint32_t m, uint64_t x0,
                                                      bool known, bool eq0, uint64_t p0, uint32_t* probes) {
    const uint64_t sa_n = a.sa_n;
    auto pred = [&](uint64_t y, uint64_t* py) -> bool {
        const uint4 e = a.quad_leaves[y];
        const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32);
        *py = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
        if (key != K64) return key > K64;
        return a.n - *py >= (uint64_t)m;
    };
    if (x0 >= sa_n) return a.next_pos;
    bool ok;
    if (known) {
        ok = !eq0 || a.n - p0 >= (uint64_t)m;
    } else {
        ok = pred(x0, &p0);
        (*probes)++;
    }
    if (ok) return p0;
    // rare: exponential + binary search over x0+1 ..
    uint64_t lo = x0 + 1, hi = sa_n, step = 1, py;
    while (lo < sa_n) {
        hi = lo + step - 1;
        if (hi >= sa_n) { hi = sa_n; break; }
        (*probes)++;
        if (pred(hi, &py)) break;
        lo = hi + 1;
        step *= 2;
        hi = sa_n;
    }
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        (*probes)++;
        if (pred(mid, &py)) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= sa_n) return a.next_pos;
    (*probes)++;
    pred(lo, &py);
    return py;
}

// ------------------------------------------------------------------ QUAD_LLCP
// configs[2] as one kernel (SAS_ALGO_QUAD_LLCP): QUAD's descent over the fused 32-char keys,
// and where the routed leaf does not settle the query, Manber-Myers LLCP skipping
// (the SAS_BUILD_LLCP entries, as stree_tail<.., true>) inside the run of suffixes that share
// q's key.  Absolute layout (quad_fan 17: 16-char left-max separators), fused leaves.
//
// The descent routes on q's 16-char key K16, so leaf k holds the first suffix whose 16-char key
// is >= K16 (s0 = 4k + count(key16 < K16)), and every suffix before it has key16 < K16.  At
// every inner node the group also counts the separators <= K16: the first level where that
// count exceeds the < K16 one is where the path of K16 + 1 leaves q's path (a run of equal
// 16-char keys spans at most a few leaves, so the paths part near the leaves), and the
// suffixes past q's 16-char run are found by descending from there -- one or two requests
// instead of a second descent from the root.  From the leaves' 32-char keys:
//   L0 = 4k + count(key64 < K64): every suffix before L0 is < q;
//   U  = the first suffix whose key64 > K64 (leaf k, or the leaf of K16 + 1 when it holds a
//        key <= K64), else the end s1 of the 16-char run: every suffix from U on is > q.
// A query that the leaf settles (the common case on random text: U <= L0 + 1) costs QUAD's
// reads and at most one text compare (k_sa_quad4x's).  Otherwise the LLCP walk runs from the
// root of the entries' implicit binary-search tree: a mid below L0 goes right and one at or
// past U goes left with no read; a mid in [L0, U) reads its 16-B entry.  A bound that no read
// measured takes an lcp as stree_tail does -- the entry's own Llcp / Rlcp, which makes that
// side tie (so the probe compares from there) -- except a left bound inside leaf k, whose exact
// lcp with q the leaf's 32-char key gives (min(first differing char, suffix length)).  That
// substitution is sound because every mid read lies in q's 16-char run [s0, s1), and in q's
// 32-char run when both L0 and U are exact at 32 chars (kappa = 32): then a ties' compare
// starts at char kappa (a suffix shorter than kappa in the run is a proper prefix of q).
// Queries of <= 32 chars in a ragged batch finish as k_sa_quad4x's do (their 32-char key
// decides every entry).  out_probes: inner levels + leaves + entries + text compares read.
template <int QW, class Q>
__device__ __forceinline__ bool qllcp_tie_less(const SearchArgs& a, uint64_t p, const Q& q, uint32_t hh, uint32_t inl,
                                               uint32_t kappa, uint32_t* lcp) {
    const uint64_t lenS = a.n - p;
    if (lenS < kappa) {  // its padded key matched q's: a proper prefix of q (m > 32)
        *lcp = (uint32_t)lenS;
        return true;
    }
    uint32_t h = kappa;
    if (hh + 16 > kappa) {
        // llcp_tie_less: the entry's 16 chars after hh first (those below kappa compare equal)
        const uint32_t L = lenS < (uint64_t)q.m ? (uint32_t)lenS : q.m;
        if (hh < L) {
            const uint32_t c = L - hh < 16 ? L - hh : 16;
            const uint32_t mk = ~0u << (32 - 2 * c);
            const uint32_t av = inl & mk, bv = (uint32_t)(q.chars32(hh) >> 32) & mk;
            if (av != bv) {
                *lcp = hh + (uint32_t)(__clz(av ^ bv) >> 1);
                return av < bv;
            }
        }
        h = hh + 16;
    }
    return suffix_less_from<QW>(a.tw, a.n, p, q, h, lcp);
}

#define QLLCP_NONE 0xFFu

// k_sa_quad_llcp's workgroup size (two workgroups a CU): 768 -> 6 waves a SIMD, 80 VGPRs;
// 512 -> 4 waves, 128 VGPRs
#ifndef SAS_QLLCP_BLOCK
#define SAS_QLLCP_BLOCK 768
#endif
// ... for m > 64 (4 or 8 query words in registers)
#ifndef SAS_QLLCP_BLOCK_LONG
#define SAS_QLLCP_BLOCK_LONG 768
#endif
#define QLLCP_BLOCK(QW) ((QW) <= 2 ? SAS_QLLCP_BLOCK : SAS_QLLCP_BLOCK_LONG)
// descent on K16 recording where K16 + 1's path parts from it (level, node index one level down)
__device__ __forceinline__ uint32_t quad_descend_split(const SearchArgs& a, const uint4* s_nodes, uint32_t K16,
                                                       uint32_t sub, uint32_t* dlev, uint32_t* dnode) {
    uint32_t k = 0, dl = QLLCP_NONE, dn = 0;
    auto step = [&](uint4 v, uint32_t h) {
        const uint32_t lt = (v.x < K16) + (v.y < K16) + (v.z < K16) + (v.w < K16);
        const uint32_t le = (v.x <= K16) + (v.y <= K16) + (v.z <= K16) + (v.w <= K16);
        const uint32_t cc = quad_sum(lt | (le << 8));
        const uint32_t c = cc & 0xFFu, c2 = cc >> 8;
        if (dl == QLLCP_NONE && c2 > c) {
            dl = h;
            dn = k * SAS_QUAD_FAN + c2;
        }
        k = k * SAS_QUAD_FAN + c;
    };
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_LDS; h++)
        if (h < a.quad_lds_layers) step(s_nodes[((uint32_t)a.quad_off[h] + k) * 4 + sub], h);
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_INNER; h++) {
        if (h >= a.quad_lds_layers && h < a.quad_inner_layers) {
            const uint4* pv = a.quad_inner + (a.quad_off[h] + k) * 4 + sub;
            step(h >= a.quad_nt_from ? nt_load4(pv) : *pv, h);
        }
    }
    *dlev = dl;
    *dnode = dn;
    return k;
}

// K16 + 1's descent from node k of level h0 (separators <= K16 = < K16 + 1)
__device__ __forceinline__ uint32_t quad_descend_from(const SearchArgs& a, const uint4* s_nodes, uint32_t h0,
                                                      uint32_t k, uint32_t K16, uint32_t sub) {
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_LDS; h++) {
        if (h >= h0 && h < a.quad_lds_layers) {
            const uint4 v = s_nodes[((uint32_t)a.quad_off[h] + k) * 4 + sub];
            k = k * SAS_QUAD_FAN + quad_sum((v.x <= K16) + (v.y <= K16) + (v.z <= K16) + (v.w <= K16));
        }
    }
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_INNER; h++) {
        if (h >= h0 && h >= a.quad_lds_layers && h < a.quad_inner_layers) {
            const uint4* pv = a.quad_inner + (a.quad_off[h] + k) * 4 + sub;
            const uint4 v = h >= a.quad_nt_from ? nt_load4(pv) : *pv;
            k = k * SAS_QUAD_FAN + quad_sum((v.x <= K16) + (v.y <= K16) + (v.z <= K16) + (v.w <= K16));
        }
    }
    return k;
}

// the per-query state a lane keeps between the group steps, packed (k_sa_quad_llcp)
#define QL_C16(st) ((st) & 7u)           // leaf k's keys16 < K16
#define QL_C64(st) (((st) >> 3) & 7u)    // leaf k's keys64 < K64 (4: none >= K64 in it)
#define QL_FU(st) (((st) >> 6) & 7u)     // U = 4 kU + FU
#define QL_KNOWN (1u << 9)               // leaf k holds a key >= K64 (L0 exact at 32 chars)
#define QL_EQ0 (1u << 10)                // ... and it is K64
#define QL_UK (1u << 11)                 // U known
#define QL_X32 (1u << 12)                // U exact at 32 chars too: q's 32-char run
#define QL_LAM0 (1u << 13)               // entry L0 compared below q: L0 + 1, its lcp in lcp0
#define QL_END (1u << 14)                // q's 16-char run reaches the end: U = sa_n
#define QL_DLEV(st) ((st) >> 24)         // where K16 + 1's path parts from q's (QLLCP_NONE: not)
// leaf k's keys all below q's (L0 past it): read the next entry to settle q as k_sa_quad4x
// would (1), or go to the walk from L0 = 4k + 4 with kappa 16 (0), or read it only when just
// leaf k's last entry shares q's 16-char key (2).  On random text that is the usual shape of
// the case (one other suffix with q's 16-char key below q, a leaf boundary between them) and
// the next entry is q's; on repetitive text a 16-char run fills more of the leaf and the
// next entry is rarely L0 itself, so the read would mostly be wasted
#ifndef SAS_QLLCP_NEXT
#define SAS_QLLCP_NEXT 2
#endif

// k_sa_quad_llcp: the group step (descent, leaf, counts), the settle (k_sa_quad4x's reads: the
// first entry not below q's 32-char key and at most one compare), then for what that does not
// settle U (where the run leaves leaf k; cooperative) and the LLCP walk.  (Round 6 also
// measured it split in two kernels, the unsettled queries' state handed over in a list: the
// list's scattered query and result accesses cost more than the split saved)
// EXACT: launched only with m <= 32 QW (QueryRegsExact: no repacking from the bytes);
// R32: sa_n < 2^32, the walk's ranks in 32 bits
template <int QW, bool EXACT, bool R32>
__global__ __launch_bounds__(QLLCP_BLOCK(QW), QLLCP_BLOCK(QW) * 2 / 256) void k_sa_quad_llcp(SearchArgs a) {
    using QR = typename std::conditional<EXACT, QueryRegsExact<QW>, QueryRegsRepack<QW>>::type;
    __shared__ uint4 s_nodes[SAS_QUAD_LDS_NODES * 4];
    stage_quad_top(a, s_nodes);
    uint32_t bad = 0;
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    const int lane0 = (int)((threadIdx.x & 63) & ~3u);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
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
        const uint64_t Kmine = q.w[0];
        uint32_t probes = a.quad_inner_layers + 1;
        // this lane's query, from its group step: leaf k, the leaf kU of U, the packed counts and
        // flags (QL_*), leaf k's entries' lcps with q (8 bits each), K16 + 1's node below its
        // parting level, and the SA values at L0 and U when a leaf read delivered them
        uint32_t kq = 0, st = 0, lam = 0, dnode = 0;
        uint64_t p0 = QUAD_NO_SA;
        for (uint32_t j = 0; j < QUAD_G; j++) {
            if (gi + j >= a.nq) break;  // group-uniform
            const uint64_t K64 = __shfl((unsigned long long)Kmine, lane0 + (int)j, 64);
            const uint32_t K16 = (uint32_t)(K64 >> 32);
            uint32_t dl, dn;
            const uint32_t k = quad_descend_split(a, s_nodes, K16, sub, &dl, &dn);
            const uint4 e = quad_leaf_load(a, a.quad_leaves + 4 * (uint64_t)k + sub);
            const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32);
            const uint32_t cc = quad_sum((uint32_t)(e.y < K16) | ((uint32_t)(key < K64) << 8) |
                                         ((uint32_t)(key <= K64) << 16));
            const uint32_t c16 = cc & 0xFFu, c64 = (cc >> 8) & 0xFFu, le64 = cc >> 16;
            // this entry's lcp with q: min(first differing char of the 32-char keys, length)
            uint32_t d = key == K64 ? 32u : (uint32_t)__clzll(key ^ K64) >> 1;
            if (4 * (uint64_t)k + sub < a.sa_n) {
                const uint64_t len = a.n - ((uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32));
                if ((uint64_t)d > len) d = (uint32_t)len;
            }
            const uint32_t lamj = quad_sum(d << (8 * sub));  // disjoint bytes: the sum is the OR
            const uint32_t eq0 = (uint32_t)__shfl((int)(e.x == (uint32_t)K64 && e.y == K16), lane0 + (int)(c64 & 3), 64);
            const uint32_t z0 = (uint32_t)__shfl((int)e.z, lane0 + (int)(c64 & 3), 64);
            const uint32_t w0 = (uint32_t)__shfl((int)e.w, lane0 + (int)(c64 & 3), 64);
            if (sub == j) {
                kq = k;
                lam = lamj;
                dnode = dn;
                st = c16 | (c64 << 3) | (dl << 24);
                if (c64 < 4) {
                    st |= QL_KNOWN | QL_X32 | (eq0 ? QL_EQ0 : 0u);
                    p0 = (uint64_t)z0 | ((uint64_t)(w0 & 0xFFu) << 32);
                }
                if (le64 < 4) {  // leaf k holds the first key > K64
                    st |= QL_UK | (le64 << 6);
                } else if (K16 == 0xFFFFFFFFu) {  // q's 16-char run reaches the end
                    st = (st & ~QL_X32) | QL_UK | QL_END;
                }
            }
        }
        uint64_t pos = 0;
        bool done = !mine;
        uint32_t lcp0 = 0;
        if (mine && m <= 32) {
            // the 32-char key decides every entry: k_sa_quad4x's finish
            pos = quad_short_finish(a, Kmine, m, 4 * (uint64_t)kq + QL_C64(st), (st & QL_KNOWN) != 0,
                                    (st & QL_EQ0) != 0, p0, &probes);
            done = true;
        } else if (mine && 4 * (uint64_t)kq + QL_C64(st) >= a.sa_n) {
            pos = a.next_pos;
            done = true;
        } else if (mine) {
            if (!(st & QL_KNOWN) && (SAS_QLLCP_NEXT == 1 || (SAS_QLLCP_NEXT == 2 && QL_C16(st) == 3))) {
                // leaf k's keys are all below q's: the next entry, as k_sa_quad4x reads it (a
                // key still below q's leaves L0 inexact at 32 chars, the walk's kappa 16)
                const uint4 e = a.quad_leaves[4 * (uint64_t)kq + 4];
                const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32);
                probes++;
                if (key >= Kmine) {
                    st |= QL_KNOWN | ((st & QL_END) ? 0u : QL_X32) | (key == Kmine ? QL_EQ0 : 0u);
                    p0 = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
                }
            }
            if (st & QL_KNOWN) {
                // the first suffix not below q's 32-char key: > it, or one compare from char 32
                // (k_sa_quad4x's common case); below q, it is the walk's exact left bound
                if (!(st & QL_EQ0) || (probes++, !suffix_less_from<QW>(a.tw, a.n, p0, q, 32, &lcp0))) {
                    pos = p0;
                    done = true;
                } else {
                    st |= QL_LAM0;
                }
            }
        }
        uint32_t kU = kq;
        // U for the queries whose 32-char run leaves leaf k: the leaf of K16 + 1, from where its
        // path parts from q's (near the leaves: one or two requests)
        const bool needU = !done && !(st & QL_UK);
        const uint32_t nu = quad_mask(needU);  // group-uniform
        for (uint32_t j = 0; nu && j < QUAD_G; j++) {
            if (!(nu & (1u << j))) continue;
            const uint64_t K64 = __shfl((unsigned long long)Kmine, lane0 + (int)j, 64);
            const uint32_t K16 = (uint32_t)(K64 >> 32);
            const uint32_t dl = (uint32_t)__shfl((int)st, lane0 + (int)j, 64) >> 24;
            uint32_t ku = (uint32_t)__shfl((int)kq, lane0 + (int)j, 64);
            if (dl != QLLCP_NONE) {
                ku = quad_descend_from(a, s_nodes, dl + 1, (uint32_t)__shfl((int)dnode, lane0 + (int)j, 64), K16, sub);
                if (sub == j) probes += a.quad_inner_layers - dl;
            }
            const uint4 eU = quad_leaf_load(a, a.quad_leaves + 4 * (uint64_t)ku + sub);
            const uint64_t keyU = (uint64_t)eU.x | ((uint64_t)eU.y << 32);
            const uint32_t cu = quad_sum((uint32_t)(keyU <= K64) | ((uint32_t)(eU.y <= K16) << 8));
            const uint32_t le64U = cu & 0xFFu, le16U = cu >> 8;
            // a key <= K64 in the leaf: everything before it is too, and the next one is the
            // first key > K64; none: the 16-char run's end, exact at 16 chars
            const uint32_t f = le64U ? le64U : le16U;
            if (sub == j) {
                kU = ku;
                st = (st & ~(7u << 6)) | (f << 6) | QL_UK;
                if (!le64U) st &= ~QL_X32;
            }
        }
        if (!mine) continue;
        if (!done) {
            using rk_t = typename std::conditional<R32, uint32_t, uint64_t>::type;
            const rk_t sa_n = (rk_t)a.sa_n;
            // no wrap in 32 bits: this query passed 4 kq + C64 < sa_n above, so kb, s0 <= kb + C64
            // and L0 <= kb + C64 + 1 are at most sa_n; U is formed in 64 bits (qllcp_bisect.hpp)
            const rk_t kb = 4 * (rk_t)kq;
            const rk_t s0 = kb + QL_C16(st);
            const rk_t L0 = kb + QL_C64(st) + ((st & QL_LAM0) ? 1 : 0);
            const rk_t U = qllcp_right_bound<rk_t>(kU, QL_FU(st), (st & QL_END) != 0, a.sa_n);
            const uint32_t kappa = (st & QL_X32) ? 32u : 16u;
            rk_t l = 0, r = sa_n;
            uint64_t pr = QUAD_NO_SA;
            uint32_t llcp = 0, rlcp = 0;
            for (;;) {
                rk_t mid = 0;
                while (l < r)  // ALU only, as stree_tail
                    if (qllcp_bisect_step<rk_t>(l, r, L0, U, mid)) break;
                if (!(l < r)) break;
                const uint4 e = a.llcp[mid];
                const uint32_t x = (e.y >> 8) & SAS_LLCP_CAP, y = e.y >> 20;
                if (l <= s0) llcp = x;  // SA[l - 1] before q's 16-char run (or l = 0)
                else if (l <= L0)       // in leaf k, below q: exact
                    llcp = ((st & QL_LAM0) && l == L0) ? lcp0 : (lam >> (8 * (uint32_t)(l - 1 - kb))) & 0xFFu;
                if (r >= U) rlcp = y;   // SA[r] past q's run (or r = sa_n)
                probes++;
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
                const uint64_t p = (uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32);
                if (!decided) lt = qllcp_tie_less<QW, QR>(a, p, q, hh, inl, kappa, &lcp);
                if (lt) {
                    l = mid + 1;
                    llcp = lcp;
                } else {
                    r = mid;
                    rlcp = lcp;
                    pr = p;
                }
            }
            if (r >= sa_n) pos = a.next_pos;
            else if (pr != QUAD_NO_SA) pos = pr;
            else {
                const uint4 eu = a.llcp[r];
                pos = (uint64_t)eu.x | ((uint64_t)(eu.y & 0xFFu) << 32);
                probes++;
            }
        }
        a.out_pos[i] = pos;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// QUAD_LLCP past 32 chars.  Fused leaves, any SA width (the leaves and the LLCP entries carry
// 40-bit positions), with every query word in registers when the batch's longest query is known
// to fit them, else two words and the rest repacked from the bytes.  qw = 1 goes to QUAD
// (launch_search).
void launch_quad_llcp(int num_cus, hipStream_t st, const SearchArgs& a, int qw) {
    const bool exact = all_words_in_regs(a, qw);
    const bool r32 = a.sa_n < (1ull << 32);
    // the grid is sized by QLLCP_BLOCK(2) whatever the workgroup size (the kernels stride over
    // the batch): launch_ctx with the final block size would change the grid
    LaunchCtx c = launch_ctx(a.nq, QLLCP_BLOCK(2), (uint64_t)num_cus * 2, st);
    c.block = dim3((unsigned)(exact ? QLLCP_BLOCK(qw) : QLLCP_BLOCK(2)));
    auto go = [&](auto Q, auto X) {
        constexpr int QW = decltype(Q)::value;
        constexpr bool EXACT = decltype(X)::value;
        if (r32) launch(c, k_sa_quad_llcp<QW, EXACT, true>, a);
        else launch(c, k_sa_quad_llcp<QW, EXACT, false>, a);
    };
    if (!exact) return go(std::integral_constant<int, 2>{}, std::false_type{});
    with_qw(qw, [&](auto Q) {
        if constexpr (decltype(Q)::value >= 2) go(Q, std::true_type{});
    });
}
