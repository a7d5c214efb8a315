// search_prefix.hip -- PREFIX: k_sa_prefix, k_sa_prefix2 (the headline), their range kernels and launchers.
#include "search_quad.hpp"

// ------------------------------------------------------------------ PREFIX
// The reference's prefix table, live (fill_prefix_table / prefix_range,
// sas/sa_search.rs:59-95; p = 0 there, :31).  One lane per query: K = q's first p
// chars zero padded; every suffix whose p-char key is < K is < q and every one whose
// key is > K is > q (zero padding keeps key order = slice order), so
// the lower bound lies in [table[K], table[K+1]], found by a binary search over the
// quad leaf entries of that range with the sector predicate.  At p = ceil(log4 n) + 1
// a random lookup is two memory requests: the table pair, then one leaf entry.
#ifndef SAS_PREFIX_NT
#define SAS_PREFIX_NT 1  // non-temporal table / entry loads (-3%, tools/ab_prefix.py)
#endif
#ifndef SAS_PREFIX_SPLITQ
#define SAS_PREFIX_SPLITQ 1  // lane pairs split a 32-B query load (k_sa_prefix2; -4%)
#endif
#ifndef SAS_PREFIX_QPREFETCH
#define SAS_PREFIX_QPREFETCH 1  // load the next query while this one's entry is in flight (-1%)
#endif
#ifndef SAS_PREFIX_QWMAX
// most query words k_sa_prefix holds in registers: 8, or 4 with the later words of a longer
// query repacked from the bytes (QueryRegs repacks only at QW > 2: the static_assert above launch_table)
#define SAS_PREFIX_QWMAX 8
#endif
// k_sa_prefix2 on the headline shape (fixed 32-char queries, lane pairs): queries in flight
// per lane pair (round 6 A/B hook; 1 = one lookup at a time)
#ifndef SAS_PREFIX_ILP
#define SAS_PREFIX_ILP 1
#endif
template <int QW, bool KO, int W, int TW>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_prefix(SearchArgs a) {
    uint32_t bad = 0;
    const uint32_t sh = 64 - 2 * a.prefix_chars;
    const uint64_t sa_n = a.sa_n;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        if (!slot_live(a, i)) continue;
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        if (a.qwords) {  // packed fixed-length query: the key word itself
            q.bytes = nullptr;
            q.m = m;
            q.w[0] = a.qwords[i] & chars_mask(m);
        } else {
            q.load(qb, m, &bad);
        }
        const uint64_t K64 = q.w[0];
        const uint64_t K = pt_slot(a, K64 >> sh);
        uint64_t lo, hi = 0, pos = QUAD_NO_SA;
        const uint32_t* pt = reinterpret_cast<const uint32_t*>(a.prefix);
        const uint4* pt16 = reinterpret_cast<const uint4*>(a.prefix);
        bool have_hi = true;
        if (TW == 16) {
            // inline entry: the range's first suffix {key, rank, SA}; if it is >= q it is
            // the answer, and this was the only read
            const uint4 e0 = SAS_PREFIX_NT ? nt_load4(pt16 + K) : pt16[K];
            lo = e0.z;
            have_hi = false;
            if (lo >= sa_n) {
                pos = a.next_pos;
            } else if (sector_ge<QW>((uint64_t)e0.x | ((uint64_t)e0.y << 32), e0.w, K64, a, q)) {
                pos = e0.w;
            } else {
                hi = pt16[K + 1].z;
                have_hi = true;
            }
        } else if (TW == 5) {
            const SaView<5> v{a.prefix};
            lo = v[K];
            hi = v[K + 1];
        } else if (SAS_PREFIX_NT) {
            // two 4-B loads: the rank pair as one dword-aligned 8-B load measured the same
            lo = __builtin_nontemporal_load(pt + K);
            hi = __builtin_nontemporal_load(pt + K + 1);
        } else {
            lo = pt[K];
            hi = pt[K + 1];
        }
        const uint64_t lo0 = lo;
        uint64_t hi0 = hi;
        // binary_search over [table[K], table[K+1]) (sas/sa_search.rs:98-112); with inline
        // entries rank lo is already known to be < q.  A scan of short ranges with
        // independent loads measured slower (0.53 -> 0.60 ms at c1, 26.6 -> 39.4 ms at c3):
        // its key re-reads lengthen the dependent chain.
        if (pos == QUAD_NO_SA) {
            uint64_t pr = QUAD_NO_SA;
            if (TW == 16) lo++;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                uint64_t key, pp;
                if (KO) {
                    key = quad_entry_key<true>(a, mid);
                    pp = key == K64 ? quad_entry_sa<true, W>(a, mid) : QUAD_NO_SA;
                } else {
                    const uint4 e = SAS_PREFIX_NT ? nt_load4(a.quad_leaves + mid) : a.quad_leaves[mid];
                    key = (uint64_t)e.x | ((uint64_t)e.y << 32);
                    pp = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
                }
                if (sector_ge<QW>(key, pp, K64, a, q)) {
                    hi = mid;
                    pr = pp;  // SA at rank hi (QUAD_NO_SA: not read); lo ends at hi
                } else {
                    lo = mid + 1;
                }
            }
            if (lo >= sa_n) pos = a.next_pos;
            else if (pr != QUAD_NO_SA) pos = pr;
            else pos = quad_entry_sa<KO, W>(a, lo);
        }
        // out_probes = the reference's cnt (sas/sa_search.rs:86-112): 1 for the table, then
        // binary_search's iterations over [table[K], table[K+1]), which end at rank lo
        uint32_t probes = 1;
        if (a.out_probes) {
            if (!have_hi) hi0 = pt16[K + 1].z;
            for (uint64_t l2 = lo0, h2 = hi0; l2 < h2; probes++) {
                const uint64_t mid = (l2 + h2) >> 1;
                if (mid < lo) l2 = mid + 1;
                else h2 = mid;
            }
        }
        a.out_pos[i] = pos;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// SAS_BUILD_PREFIX_INLINE2 / _INLINE4: 16·G-byte entries, the first G suffixes (ranks
// r .. r + G - 1) of the range of q's p-char key.  A G-lane group reads the entry as one
// request (16 B per lane), each lane tests one suffix, and the group ballot takes the
// first that is >= q; only if all are < q does the search go on in [r + G, table[K+1]).
// HI40 (a part index of a text >= 2^32 chars): slot 1's rank word holds bits 32..39 of
// every slot's SA value, one byte per slot.
// k_sa_prefix2's lookup of query i once its table entry e (entry K) is in: the pair's slots
// tested, the rare bisection past them, the position (and the reference's cnt) stored
template <int QW, int G, bool HI40>
__device__ __forceinline__ void prefix2_finish(const SearchArgs& a, const uint4* pt, uint64_t i, uint64_t K,
                                               const uint4& e, const QueryRegs<QW>& q, uint64_t K64, uint32_t sub,
                                               int lane0) {
    const uint64_t sa_n = a.sa_n;
    const uint32_t hb = HI40 ? (uint32_t)__shfl((int)e.z, lane0 + 1, 64) : 0u;
    // two slots beside a >= 2^32-char text: bits 32..39 of the rank in slot 1's rank word
    const uint64_t r0 = (uint64_t)(uint32_t)__shfl((int)e.z, lane0, 64) |
                        (HI40 && G == 2 ? (uint64_t)((hb >> 16) & 0xFFu) << 32 : 0ull);
    const uint64_t rank = r0 + sub;
    const uint64_t pe = HI40 ? ((uint64_t)e.w | ((uint64_t)((hb >> (8 * sub)) & 0xFFu) << 32)) : (uint64_t)e.w;
    // rank sa_n stands for "past every suffix": it is the answer if reached
    const bool ok = rank >= sa_n || sector_ge<QW>((uint64_t)e.x | ((uint64_t)e.y << 32), pe, K64, a, q);
    const uint32_t grp = (uint32_t)(__ballot(ok) >> lane0) & ((1u << G) - 1u);
    const uint32_t j = grp ? (uint32_t)__builtin_ctz(grp) : 0u;
    const uint32_t pw = (uint32_t)__shfl((int)e.w, lane0 + (int)j, 64);
    uint64_t ans, pos;
    if (grp) {
        ans = r0 + j;
        pos = ans >= sa_n ? a.next_pos : (HI40 ? ((uint64_t)pw | ((uint64_t)((hb >> (8 * j)) & 0xFFu) << 32)) : pw);
    } else {
        uint64_t lo = r0 + G, hi = pt_rank<G, HI40>(pt, K + 1), pr = QUAD_NO_SA;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint4 f = SAS_PREFIX_NT ? nt_load4(a.quad_leaves + mid) : a.quad_leaves[mid];
            const uint64_t pp = (uint64_t)f.z | ((uint64_t)(f.w & 0xFFu) << 32);
            if (sector_ge<QW>((uint64_t)f.x | ((uint64_t)f.y << 32), pp, K64, a, q)) {
                hi = mid;
                pr = pp;
            } else {
                lo = mid + 1;
            }
        }
        ans = lo;
        if (lo >= sa_n) pos = a.next_pos;
        else if (pr != QUAD_NO_SA) pos = pr;
        else pos = quad_entry_sa<false, 4>(a, lo);
    }
    if (sub == 0) {
        a.out_pos[i] = pos;  // a non-temporal store here gave nothing
        if (a.out_probes) {  // the reference's cnt over [table[K], table[K+1])
            uint32_t probes = 1;
            for (uint64_t l2 = r0, h2 = pt_rank<G, HI40>(pt, K + 1); l2 < h2; probes++) {
                const uint64_t mid = (l2 + h2) >> 1;
                if (mid < ans) l2 = mid + 1;
                else h2 = mid;
            }
            a.out_probes[i] = probes;
        }
    }
}

template <int QW, int G, bool HI40 = false>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_prefix2(SearchArgs a) {
    uint32_t bad = 0;
    const uint32_t sh = 64 - 2 * a.prefix_chars;
    const uint32_t sub = threadIdx.x & (G - 1);
    const int lane0 = (int)((threadIdx.x & 63) & ~(uint32_t)(G - 1));
    const uint4* pt = reinterpret_cast<const uint4*>(a.prefix);
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / G;
    // fixed 32-char queries at 16-B aligned addresses: the pair splits each query load
    const bool split = SAS_PREFIX_SPLITQ && G == 2 && QW == 1 && a.qoff == nullptr && a.qwords == nullptr &&
                       a.m_fixed == 32 && a.bcounts == nullptr &&
                       (((uintptr_t)a.qbytes) & 15) == 0;
    auto qload = [&](uint64_t k) -> uint4 {
        const uint4* p = reinterpret_cast<const uint4*>(a.qbytes + k * 32) + sub;
        return SAS_QUAD_NT_IO ? nt_load4(p) : *p;
    };
    const uint64_t i0 = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / G;
    if (SAS_PREFIX_ILP > 1 && split) {
        // two queries per lane pair in flight: i and i + stride, both table entries requested
        // before either is tested (the next two queries' loads overlap the lookups)
        auto pack_q = [&](const uint4& v, uint64_t k, QueryRegs<QW>& q) {
            bad |= (v.x | v.y | v.z | v.w) & 0xFCFCFCFCu;
            const uint32_t part = (pack4(v.x) << 24) | (pack4(v.y) << 16) | (pack4(v.z) << 8) | pack4(v.w);
            const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)part, 0xB1, 0xF, 0xF, false);
            q.bytes = a.qbytes + k * 32;
            q.m = 32;
            q.w[0] = sub ? (((uint64_t)other << 32) | part) : (((uint64_t)part << 32) | other);
        };
        const uint4 z = make_uint4(0, 0, 0, 0);
        uint4 va = i0 < a.nq ? qload(i0) : z, vb = i0 + stride < a.nq ? qload(i0 + stride) : z;
        for (uint64_t i = i0; i < a.nq; i += 2 * stride) {
            const uint64_t i2 = i + stride;
            const bool two = i2 < a.nq;  // group-uniform
            const uint4 ua = va, ub = vb;
            if (i + 2 * stride < a.nq) va = qload(i + 2 * stride);
            if (i2 + 2 * stride < a.nq) vb = qload(i2 + 2 * stride);
            QueryRegs<QW> qa, qb2;
            pack_q(ua, i, qa);
            pack_q(ub, i2, qb2);
            const uint64_t Ka = pt_slot(a, qa.w[0] >> sh), Kb = pt_slot(a, qb2.w[0] >> sh);
            const uint4 ea = SAS_PREFIX_NT ? nt_load4(pt + G * Ka + sub) : pt[G * Ka + sub];
            uint4 eb = z;
            if (two) eb = SAS_PREFIX_NT ? nt_load4(pt + G * Kb + sub) : pt[G * Kb + sub];
            prefix2_finish<QW, G, HI40>(a, pt, i, Ka, ea, qa, qa.w[0], sub, lane0);
            if (two) prefix2_finish<QW, G, HI40>(a, pt, i2, Kb, eb, qb2, qb2.w[0], sub, lane0);
        }
        if (bad) atomicOr(a.bad, 1u);
        return;
    }
    uint4 vnext = make_uint4(0, 0, 0, 0);
    if (SAS_PREFIX_QPREFETCH && split && i0 < a.nq) vnext = qload(i0);
    for (uint64_t i = i0; i < a.nq; i += stride) {
        if (!slot_live(a, i)) continue;  // group-uniform: the G lanes share i
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        if (a.qwords) {  // packed: the key word itself (both lanes, one 8-B request)
            q.bytes = nullptr;
            q.m = m;
            q.w[0] = a.qwords[i] & chars_mask(m);
        } else if (split) {
            // the pair splits the 32-B query: lane j packs bytes 16j..16j+15 to 32 bits,
            // then the halves are swapped within the pair (DPP quad_perm [1,0,3,2])
            uint4 v;
            if (SAS_PREFIX_QPREFETCH) {  // the next query's load overlaps this lookup
                v = vnext;
                if (i + stride < a.nq) vnext = qload(i + stride);
            } else {
                v = qload(i);
            }
            bad |= (v.x | v.y | v.z | v.w) & 0xFCFCFCFCu;
            const uint32_t part = (pack4(v.x) << 24) | (pack4(v.y) << 16) | (pack4(v.z) << 8) | pack4(v.w);
            const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)part, 0xB1, 0xF, 0xF, false);
            q.bytes = qb;
            q.m = m;
            q.w[0] = sub ? (((uint64_t)other << 32) | part) : (((uint64_t)part << 32) | other);
        } else {
            q.load(qb, m, &bad);  // every lane of the group: the same addresses, one request
        }
        const uint64_t K64 = q.w[0];
        const uint64_t K = pt_slot(a, K64 >> sh);
        const uint4 e = SAS_PREFIX_NT ? nt_load4(pt + G * K + sub) : pt[G * K + sub];
        prefix2_finish<QW, G, HI40>(a, pt, i, K, e, q, K64, sub, lane0);
    }
    if (bad) atomicOr(a.bad, 1u);
}

// Occurrence ranges from the prefix table (any entry format; Search::search_prefix,
// sas/util.rs:36-46): lo = the lower bound, bisected in [table[K], table[K+1]]; hi = the
// first suffix whose first min(m, len) chars are > q, bisected in the range of the
// routing key (q padded with 3s for m <= 32, its own key above), with the predicates of
// k_sa_quad_range over the quad leaves' entries.
template <int QW, bool KO, int W>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_prefix_range(SearchArgs a, uint64_t* out_hi) {
    uint32_t bad = 0;
    const uint32_t sh = 64 - 2 * a.prefix_chars;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        // both bisections advance in lock step: two independent entry reads in flight per lane
        uint64_t lo, l1, hi, h1;
        prefix_range(a, K64 >> sh, &lo, &l1);
        prefix_range(a, (q.m <= 32 ? Q3 : K64) >> sh, &hi, &h1);
        while (lo < l1 || hi < h1) {
            const bool g0 = lo < l1, g1 = hi < h1;
            const uint64_t m0 = (lo + l1) >> 1, m1 = (hi + h1) >> 1;
            const uint64_t k0 = g0 ? quad_entry_key<KO>(a, m0) : 0;
            const uint64_t k1 = g1 ? quad_entry_key<KO>(a, m1) : 0;
            const uint64_t p0 = (g0 && k0 == K64) ? quad_entry_sa<KO, W>(a, m0) : QUAD_NO_SA;
            const uint64_t p1 = (g1 && q.m > 32 && k1 == K64) ? quad_entry_sa<KO, W>(a, m1) : QUAD_NO_SA;
            if (g0) {
                if (sector_ge<QW>(k0, p0, K64, a, q)) l1 = m0;
                else lo = m0 + 1;
            }
            if (g1) {
                if (sector_gt_prefix<QW>(k1, p1, K64, Q3, a, q)) h1 = m1;
                else hi = m1 + 1;
            }
        }
        if (hi < lo) hi = lo;
        a.out_pos[i] = a.rank_lo + lo;
        out_hi[i] = a.rank_lo + hi;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// Occurrence ranges on a G-slot inline prefix table (SAS_BUILD_PREFIX_INLINE2 / _INLINE4):
// the G lanes of a query read its entry (the first G suffixes of the range of its p-char
// key) as one request and test both bounds' predicates on every slot: lo = the first slot
// >= q, hi = the first slot whose first min(m, len) chars are > q (m >= p: the suffixes
// starting with q all lie in the key's range).  A bound not inside the entry is bisected
// in [r + G, table[K + 1]) (hi, for m < p: in the range of the 3-padded key), both in
// lock step as k_sa_prefix_range does; every lane of the group runs the same loop (same
// addresses: one request per probe).
template <int QW, int G, bool HI40 = false>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_prefix2_range(SearchArgs a, uint64_t* out_hi) {
    uint32_t bad = 0;
    const uint32_t sh = 64 - 2 * a.prefix_chars;
    const uint64_t sa_n = a.sa_n;
    const uint32_t sub = threadIdx.x & (G - 1);
    const int lane0 = (int)((threadIdx.x & 63) & ~(uint32_t)(G - 1));
    const uint4* pt = reinterpret_cast<const uint4*>(a.prefix);
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / G;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / G; i < a.nq; i += stride) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);  // every lane of the group: the same addresses, one request
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        const uint64_t K = pt_slot(a, K64 >> sh);
        const uint4 e = pt[G * K + sub];
        const uint32_t hb = HI40 ? (uint32_t)__shfl((int)e.z, lane0 + 1, 64) : 0u;
        const uint64_t r0 = (uint64_t)(uint32_t)__shfl((int)e.z, lane0, 64) |
                            (HI40 && G == 2 ? (uint64_t)((hb >> 16) & 0xFFu) << 32 : 0ull);
        const uint64_t rank = r0 + sub;
        const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32);
        const uint64_t pe = HI40 ? ((uint64_t)e.w | ((uint64_t)((hb >> (8 * sub)) & 0xFFu) << 32)) : (uint64_t)e.w;
        // rank sa_n stands for "past every suffix": both bounds are reached there
        const bool past = rank >= sa_n;
        const bool ge = past || sector_ge<QW>(key, pe, K64, a, q);
        const bool whole = m >= a.prefix_chars;  // hi inside the key's range too
        const bool gt = past || (whole && sector_gt_prefix<QW>(key, pe, K64, Q3, a, q));
        const uint32_t mask = (1u << G) - 1u;
        const uint32_t gge = (uint32_t)(__ballot(ge) >> lane0) & mask;
        const uint32_t ggt = (uint32_t)(__ballot(gt) >> lane0) & mask;
        uint64_t lo, l1, hi, h1;
        if (gge) {
            lo = l1 = r0 + (uint32_t)__builtin_ctz(gge);
        } else {
            lo = r0 + G;
            l1 = pt_rank<G, HI40>(pt, K + 1);
        }
        if (whole) {
            if (ggt) {
                hi = h1 = r0 + (uint32_t)__builtin_ctz(ggt);
            } else {
                hi = r0 + G;
                h1 = gge ? pt_rank<G, HI40>(pt, K + 1) : l1;
            }
        } else {
            prefix_range(a, Q3 >> sh, &hi, &h1);
        }
        while (lo < l1 || hi < h1) {
            const bool g0 = lo < l1, g1 = hi < h1;
            const uint64_t m0 = (lo + l1) >> 1, m1 = (hi + h1) >> 1;
            const uint64_t k0 = g0 ? quad_entry_key<false>(a, m0) : 0;
            const uint64_t k1 = g1 ? quad_entry_key<false>(a, m1) : 0;
            const uint64_t p0 = (g0 && k0 == K64) ? quad_entry_sa<false, 4>(a, m0) : QUAD_NO_SA;
            const uint64_t p1 = (g1 && q.m > 32 && k1 == K64) ? quad_entry_sa<false, 4>(a, m1) : QUAD_NO_SA;
            if (g0) {
                if (sector_ge<QW>(k0, p0, K64, a, q)) l1 = m0;
                else lo = m0 + 1;
            }
            if (g1) {
                if (sector_gt_prefix<QW>(k1, p1, K64, Q3, a, q)) h1 = m1;
                else hi = m1 + 1;
            }
        }
        if (hi < lo) hi = lo;
        if (sub == 0) {
            a.out_pos[i] = a.rank_lo + lo;
            out_hi[i] = a.rank_lo + hi;
        }
    }
    if (bad) atomicOr(a.bad, 1u);
}

// PREFIX.  QueryRegs<QW>::word returns 0 past the register words for QW <= 2 (such kernels only
// ever see queries that fit them), so a k_sa_prefix clamped below 4 words would mis-compare long
// queries
static_assert(SAS_PREFIX_QWMAX > 2, "SAS_PREFIX_QWMAX: 4 or 8 (QueryRegs repacks later words only for QW > 2)");

// a table of TW-byte entries (4, 5; 16: one inline slot), one lane per query
template <bool KO, int W, int TW>
static void launch_table(const LaunchCtx& c, const SearchArgs& a, int qw) {
    with_qw(qw, [&](auto Q) {
        constexpr int QW = decltype(Q)::value < SAS_PREFIX_QWMAX ? decltype(Q)::value : SAS_PREFIX_QWMAX;
        launch(c, k_sa_prefix<QW, KO, W, TW>, a);
    });
}

// G inline slots per entry, G lanes per query
template <int G>
static void launch_slots(const LaunchCtx& c, const SearchArgs& a, int qw) {
    with_qw(qw, [&](auto Q) {
        if (a.prefix_hi40) launch(c, k_sa_prefix2<decltype(Q)::value, G, true>, a);
        else launch(c, k_sa_prefix2<decltype(Q)::value, G, false>, a);
    });
}

template <bool KO, int W>
static void launch_prefix_leaves(const LaunchCtx& c, const SearchArgs& a, int qw) {
    if (a.prefix_w == 5) launch_table<KO, W, 5>(c, a, qw);
    else if (a.prefix_w == 16 && !KO) launch_table<KO, W, 16>(c, a, qw);
    else if (a.prefix_w == 32 && !KO) launch_slots<2>(c, a, qw);
    else if (a.prefix_w == 64 && !KO) launch_slots<4>(c, a, qw);
    else launch_table<KO, W, 4>(c, a, qw);
}

void launch_prefix(const LaunchCtx& c, const SearchArgs& a, bool ko, uint32_t sa_w, int qw) {
    with_leaves(ko, sa_w, [&](auto KO, auto W) {
        launch_prefix_leaves<decltype(KO)::value, decltype(W)::value>(c, a, qw);
    });
}

template <int G>
static void launch_slots_range(const LaunchCtx& c, const SearchArgs& a, int qw, uint64_t* dhi) {
    with_qw(qw, [&](auto Q) {
        if (a.prefix_hi40) launch(c, k_sa_prefix2_range<decltype(Q)::value, G, true>, a, dhi);
        else launch(c, k_sa_prefix2_range<decltype(Q)::value, G, false>, a, dhi);
    });
}

void launch_prefix_range(const LaunchCtx& c, const SearchArgs& a, bool inline_slots, bool ko, uint32_t sa_w,
                                int qw, uint64_t* dhi) {
    if (inline_slots)
        return a.prefix_w == 32 ? launch_slots_range<2>(c, a, qw, dhi) : launch_slots_range<4>(c, a, qw, dhi);
    with_leaves(ko, sa_w, [&](auto KO, auto W) {
        with_qw(qw, [&](auto Q) {
            launch(c, k_sa_prefix_range<decltype(Q)::value, decltype(KO)::value, decltype(W)::value>, a, dhi);
        });
    });
}
