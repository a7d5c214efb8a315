// search_quad.hip -- QUAD (k_sa_quad, k_sa_quad4x, k_sa_quad_range) and INLINE (k_sa_inline), and their
// launchers.
#include "search_quad.hpp"

// ------------------------------------------------------------------ QUAD
// A 4-lane group per query.  Every node is 64 B and the group loads it with one
// 16-B load per lane, which the memory system serves as ONE request (a per-lane
// 32-B node costs two): tools/treebench measured 19-22 ps per DRAM-level 64-B
// group load vs 26.5 ps for a per-lane 32-B node.  Inner nodes: 16 left-max
// 16-char separators, 17-ary; lane j counts its 4, the group sums by shuffles.
// Leaves: 4 entries {key64, SA}, lane j evaluates entry j, a group ballot picks
// the first entry >= q.  All branches are group-uniform.
// m <= 32 queries at an 8-B aligned address with m % 8 == 0 (the headline shape):
// lane j of the group loads bytes 8j..8j+7 (one contiguous 32-B request per query
// instead of two 16-B halves per lane) and packs them to 16 bits; the group ORs the
// four parts with DPP quad_perm moves.
__device__ __forceinline__ uint64_t quad_key32(const uint8_t* __restrict__ qb, uint32_t m, uint32_t sub,
                                               uint32_t* bad) {
    uint32_t part = 0;
    if (8 * sub < m) {
        uint2 v;
        if (SAS_QUAD_NT_IO) {  // the query stream is read once: keep it out of L2
            const uint64_t w = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(qb + 8 * sub));
            v = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
        } else {
            v = *reinterpret_cast<const uint2*>(qb + 8 * sub);
        }
        *bad |= (v.x | v.y) & 0xFCFCFCFCu;
        part = (pack4(v.x) << 8) | pack4(v.y);
    }
    // chars 8j..8j+7 -> bits 63-16j .. 48-16j
    uint32_t hi = (sub < 2) ? (part << (16 - 16 * sub)) : 0u;
    uint32_t lo = (sub >= 2) ? (part << (16 - 16 * (sub - 2))) : 0u;
    hi |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xF, 0xF, false);
    lo |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xF, 0xF, false);
    hi |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0x4E, 0xF, 0xF, false);
    lo |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0x4E, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}

// Evaluate leaf L for the bound's predicate (UPPER = false: suffix(x) >= q;
// UPPER = true: the first min(m, len) chars of suffix(x) are > q, sector_gt_prefix).
// Returns the first qualifying entry of the leaf (EPL if none; entries x >= sa_n
// never qualify) and *p = its SA value, group-uniform (KO: QUAD_NO_SA when the
// predicate did not need it).  Fused leaves: lane j holds entry j; KO leaves: lane j
// holds entries 2j, 2j+1 and reads an SA value only for an entry whose key ties q's.
template <int QW, bool UPPER, bool KO, int W>
__device__ __forceinline__ uint32_t quad_leaf(const SearchArgs& a, const QueryRegs<QW>& q, uint64_t K64, uint64_t Q3,
                                              uint64_t L, uint32_t sub, uint64_t* p) {
    const int lane0 = (int)((threadIdx.x & 63) & ~3u);
    const uint4 e = quad_leaf_load(a, a.quad_leaves + 4 * L + sub);
    // short-circuit: padding entries (x >= sa_n) carry all-ones keys/SA and must never
    // reach the predicate (its m > 32 text compare would read past the text)
    auto pred = [&](uint64_t key, uint64_t pp) -> bool {
        return UPPER ? sector_gt_prefix<QW>(key, pp, K64, Q3, a, q) : sector_ge<QW>(key, pp, K64, a, q);
    };
    if (!KO) {
        const uint64_t x = 4 * L + sub;
        const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32);
        const uint64_t pp = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
        const uint32_t mk = quad_mask(x < a.sa_n && pred(key, pp));
        const uint32_t f = mk ? (uint32_t)__builtin_ctz(mk) : 4u;
        *p = __shfl((unsigned long long)pp, lane0 + (int)(f & 3), 64);
        return f;
    }
    const uint64_t x0 = 8 * L + 2 * sub;
    const uint64_t k0 = (uint64_t)e.x | ((uint64_t)e.y << 32), k1 = (uint64_t)e.z | ((uint64_t)e.w << 32);
    // the SA value matters only on a tie with q's 32-char key (UPPER with m <= 32: never)
    const bool tie_ok = !(UPPER && q.m <= 32);
    uint64_t p0 = QUAD_NO_SA, p1 = QUAD_NO_SA;
    if (tie_ok && k0 == K64 && x0 < a.sa_n) p0 = quad_entry_sa<true, W>(a, x0);
    if (tie_ok && k1 == K64 && x0 + 1 < a.sa_n) p1 = quad_entry_sa<true, W>(a, x0 + 1);
    const bool t0 = x0 < a.sa_n && pred(k0, p0);
    const bool t1 = x0 + 1 < a.sa_n && pred(k1, p1);
    const uint32_t many = quad_mask(t0 || t1), m0 = quad_mask(t0);
    if (!many) {
        *p = QUAD_NO_SA;
        return 8;
    }
    const uint32_t j = (uint32_t)__builtin_ctz(many);
    const uint32_t s = ((m0 >> j) & 1u) ? 0u : 1u;  // entry 2j (t0) or 2j+1
    *p = __shfl((unsigned long long)(s ? p1 : p0), lane0 + (int)j, 64);
    return 2 * j + s;
}

// Inner-node descent of the 4-lane group to the leaf for routing key R (a padded
// 32-char key).  Absolute nodes (quad_fan 17): lane j counts its 4 of the 16 u32
// 16-char separators < R's first 16 chars.  Prefix-relative nodes (quad_fan 31,
// k_quad_rel_layer): lane 0's word 0 is the header {d, P}, broadcast to the group;
// if R's first d chars equal P, the child is the count of 16-bit separators below
// R's chars [d, d+8); if they are below P every entry of the subtree is >= R (child
// 0), if above, every entry is < R (the last child; a layer's last node, which may
// have fewer children, has d = 0, so it never answers "above").  Either way every
// entry before the chosen child is < R, the invariant the leaf search needs.
typedef short quad_short2 __attribute__((ext_vector_type(2)));
// sign bits (15, 31) of the saturating packed i16 difference w - tt: set where the
// 16-bit half of w is below tt's (both stored XOR 0x8000, so signed order = unsigned)
__device__ __forceinline__ uint32_t lt2_signs(uint32_t w, uint32_t tt) {
    const quad_short2 d = __builtin_elementwise_sub_sat(__builtin_bit_cast(quad_short2, w),
                                                        __builtin_bit_cast(quad_short2, tt));
    return __builtin_bit_cast(uint32_t, d);
}

// m0 = 0 on lane 0 of the group (its word 0 is the header), 0x80008000 elsewhere
__device__ __forceinline__ uint32_t quad_rel_child(uint4 v, uint64_t R, uint32_t m0) {
    const uint32_t hdr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.x, 0x00, 0xF, 0xF, false);
    const uint64_t full = R >> (48 - ((hdr >> 26) & 62u));  // R's chars [0, d + 8)
    const uint32_t Qd = (uint32_t)(full >> 16), P = hdr & 0x7FFFFFFu;
    const uint32_t T = (uint32_t)full & 0xFFFFu;
    const uint32_t tt = (T | (T << 16)) ^ 0x80008000u;
    uint32_t c = __builtin_popcount(lt2_signs(v.x, tt) & m0);
    c += __builtin_popcount(lt2_signs(v.y, tt) & 0x80008000u);
    c += __builtin_popcount(lt2_signs(v.z, tt) & 0x80008000u);
    c += __builtin_popcount(lt2_signs(v.w, tt) & 0x80008000u);
    c = quad_sum(c);
    return Qd == P ? c : (Qd < P ? 0u : SAS_QUAD_RFAN - 1);
}

__device__ __forceinline__ uint32_t quad_abs_child(uint4 v, uint32_t R16) {
    return quad_sum((v.x < R16) + (v.y < R16) + (v.z < R16) + (v.w < R16));
}

// Both loops are unrolled over the layer index so the per-layer offsets (kernel
// arguments) are loop-invariant scalar loads hoisted out of the query loop; the leaf
// index fits 32 bits (build_quad refuses more than 2^32 leaves).
template <bool REL>
__device__ __forceinline__ uint32_t quad_descend_t(const SearchArgs& a, const uint4* s_nodes, uint64_t R, uint32_t sub) {
    const uint32_t R16 = (uint32_t)(R >> 32);
    const uint32_t m0 = sub ? 0x80008000u : 0u;
    uint32_t k = 0;
    // LDS layers, then HBM layers: separate loops keep the loads ds_read / global_load
    // (a pointer select between the two address spaces compiles to FLAT loads)
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_LDS; h++) {
        if (h < a.quad_lds_layers) {
            const uint4 v = s_nodes[((uint32_t)a.quad_off[h] + k) * 4 + sub];
            k = REL ? k * SAS_QUAD_RFAN + quad_rel_child(v, R, m0) : k * SAS_QUAD_FAN + quad_abs_child(v, R16);
        }
    }
#pragma unroll
    for (uint32_t h = 0; h < SAS_QUAD_MAX_INNER; h++) {
        if (h >= a.quad_lds_layers && h < a.quad_inner_layers) {
            const uint4* pv = a.quad_inner + (a.quad_off[h] + k) * 4 + sub;
            const uint4 v = h >= a.quad_nt_from ? nt_load4(pv) : *pv;
            k = REL ? k * SAS_QUAD_RFAN + quad_rel_child(v, R, m0) : k * SAS_QUAD_FAN + quad_abs_child(v, R16);
        }
    }
    return k;
}

__device__ __forceinline__ uint64_t quad_descend(const SearchArgs& a, const uint4* s_nodes, uint64_t R, uint32_t sub) {
    return a.quad_fan == SAS_QUAD_RFAN ? quad_descend_t<true>(a, s_nodes, R, sub)
                                       : quad_descend_t<false>(a, s_nodes, R, sub);
}

// First local rank with the bound's predicate (monotone over ranks): descent on the
// 16-char routing key, the routed leaf, then (rare) an exponential + binary search
// over later leaves for a run of equal routing keys that crosses leaves.  Returns
// sa_n if no entry qualifies; *px = SA at the returned rank (group-uniform;
// QUAD_NO_SA if a KO leaf did not need it).
template <int QW, bool UPPER, bool KO, int W>
__device__ __forceinline__ uint64_t quad_bound(const SearchArgs& a, const uint4* s_nodes, const QueryRegs<QW>& q,
                                               uint64_t K64, uint64_t Q3, uint32_t sub, uint32_t* probes,
                                               uint64_t* px) {
    constexpr uint32_t EPL = KO ? 8 : 4;
    const uint64_t nl = a.quad_leaf_count;
    const uint64_t k = quad_descend(a, s_nodes, (UPPER && q.m <= 32) ? Q3 : K64, sub);
    *probes += a.quad_inner_layers + 1;
    // routed leaf k: every entry before it fails the predicate
    uint64_t pl;
    uint32_t f = quad_leaf<QW, UPPER, KO, W>(a, q, K64, Q3, k, sub, &pl);
    uint64_t L = k;
    if (f == EPL) {
        // leaf nl = virtual: past every entry
        uint64_t lo = k + 1, step = 1, hi = nl;
        while (lo < nl) {
            hi = lo + step - 1;
            if (hi >= nl) { hi = nl; break; }
            uint64_t pp;
            (*probes)++;
            if (quad_leaf<QW, UPPER, KO, W>(a, q, K64, Q3, hi, sub, &pp) < EPL) break;
            lo = hi + 1;
            step *= 2;
            hi = nl;
        }
        while (lo < hi) {
            uint64_t mid = (lo + hi) >> 1;
            uint64_t pp;
            (*probes)++;
            if (quad_leaf<QW, UPPER, KO, W>(a, q, K64, Q3, mid, sub, &pp) < EPL) hi = mid;
            else lo = mid + 1;
        }
        L = lo;
        if (L < nl) {
            f = quad_leaf<QW, UPPER, KO, W>(a, q, K64, Q3, L, sub, &pl);
            (*probes)++;
        }
    }
    if (f == EPL) return a.sa_n;
    *px = pl;
    return EPL * L + f;
}

template <int QW, bool KO, int W>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_quad(SearchArgs a) {
    __shared__ uint4 s_nodes[SAS_QUAD_LDS_NODES * 4];
    stage_quad_top(a, s_nodes);
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    uint32_t bad = 0;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / QUAD_G;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / QUAD_G; i < a.nq; i += stride) {
        if (!slot_live(a, i)) continue;  // group-uniform: the 4 lanes share i
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        if (QW == 1 && a.qoff == nullptr && (m & 7) == 0 && (((uintptr_t)qb) & 7) == 0) {
            q.bytes = qb;
            q.m = m;
            q.w[0] = quad_key32(qb, m, sub, &bad);
        } else {
            q.load(qb, m, &bad);
        }
        uint32_t probes = 0;
        uint64_t px = 0;
        const uint64_t x = quad_bound<QW, false, KO, W>(a, s_nodes, q, q.w[0], 0, sub, &probes, &px);
        if (KO && x < a.sa_n && px == QUAD_NO_SA) px = quad_entry_sa<true, W>(a, x);  // group-uniform address
        if (sub == 0) {
            const uint64_t res = (x >= a.sa_n) ? a.next_pos : px;
            if (SAS_QUAD_NT_IO) __builtin_nontemporal_store(res, a.out_pos + i);
            else a.out_pos[i] = res;
            if (a.out_probes) a.out_probes[i] = probes;
        }
    }
    if (bad) atomicOr(a.bad, 1u);
}

// query words the 4x kernel holds in registers (later words are repacked from the
// bytes): 2 measured ~2% faster than 4/8 (fewer spills) on ragged 8..256 queries
#ifndef SAS_QUAD4X_MAXREGS
#define SAS_QUAD4X_MAXREGS 2
#endif
// The per-lane finish of k_sa_quad4x: every entry before x0 is < q (the routed leaf's count
// of 32-char keys below q's); key0 / p0 = entry x0's key and SA value when the leaf read
// delivered them (known).  The predicate at x0 (a key tie: one text compare from char 32),
// and in the rare case it fails an exponential + binary search over the following entries.
// Returns the position.  No tail_less32 prefetch in the compares (sector_ge's PREFETCH): in
// the 4x tails it measured 4-6% slower (more spills).
template <int QW, bool KO, int W, class Q>
__device__ __forceinline__ uint64_t quad_x0_finish(const SearchArgs& a, const Q& q, uint64_t K64,
                                                   uint64_t x0, bool known, uint64_t key0, uint64_t p0,
                                                   uint32_t* probes) {
    const uint64_t sa_n = a.sa_n;
    bool ok = false;
    if (x0 < sa_n) {
        const uint64_t key = known ? key0 : quad_entry_key<KO>(a, x0);
        if (key != K64) {
            ok = key > K64;
        } else {
            if (p0 == QUAD_NO_SA) p0 = quad_entry_sa<KO, W>(a, x0);
            ok = sector_ge<QW, false, false, Q>(key, p0, K64, a, q);
        }
        if (!known) (*probes)++;
    }
    uint64_t x = x0;
    if (!ok && x0 < sa_n) {  // rare: exponential + binary search over x0+1 ..
        auto pred = [&](uint64_t y) -> bool {
            const uint64_t key = quad_entry_key<KO>(a, y);
            if (key != K64) return key > K64;
            return sector_ge<QW, false, false, Q>(key, quad_entry_sa<KO, W>(a, y), K64, a, q);
        };
        uint64_t lo = x0 + 1, hi = sa_n, step = 1;
        while (lo < sa_n) {
            hi = lo + step - 1;
            if (hi >= sa_n) { hi = sa_n; break; }
            (*probes)++;
            if (pred(hi)) break;
            lo = hi + 1;
            step *= 2;
            hi = sa_n;
        }
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            (*probes)++;
            if (pred(mid)) hi = mid;
            else lo = mid + 1;
        }
        x = lo;
        p0 = QUAD_NO_SA;
    }
    if (x >= sa_n) return a.next_pos;
    return (p0 != QUAD_NO_SA) ? p0 : quad_entry_sa<KO, W>(a, x);
}

// Long queries (QW > 1), as k_sa_stree4x: one query per LANE, four per 4-lane group.
// The group descends the quad tree and reads the routed leaf cooperatively for each
// of its four queries in turn (one request per 64-B node), which places each query
// at x0 = the first entry of that leaf whose 32-char key is >= its own (the entry's
// key and fused SA value travel to the owning lane by a shuffle).  Every entry
// before x0 is < q.  Then every lane finishes its own query: the predicate at x0
// (typically a key tie -> one text compare from char 32, the part that dominates for
// long queries), and in the rare case it fails an exponential + binary search over
// the following entries.
// RP: queries longer than QW register words (their later words repacked from the bytes)
template <int QW, bool KO, int W, bool RP>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_quad4x(SearchArgs a) {
    using QR = typename std::conditional<RP, QueryRegsRepack<QW>, QueryRegs<QW>>::type;
    constexpr uint32_t EPL = KO ? 8 : 4;
    __shared__ uint4 s_nodes[SAS_QUAD_LDS_NODES * 4];
    stage_quad_top(a, s_nodes);
    uint32_t bad = 0;
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    const int lane0 = (int)((threadIdx.x & 63) & ~3u);
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
        const uint64_t Kmine = q.w[0];  // padded 32-char key of this lane's query
        uint32_t probes = a.quad_inner_layers + 1;
        uint64_t x0 = 0, key0 = 0, p0 = QUAD_NO_SA;
        bool known = false;
        for (uint32_t j = 0; j < QUAD_G; j++) {
            if (gi + j >= a.nq) break;  // group-uniform
            const uint64_t K64 = __shfl((unsigned long long)Kmine, lane0 + (int)j, 64);
            const uint64_t k = quad_descend(a, s_nodes, K64, sub);
            const uint4 e = quad_leaf_load(a, a.quad_leaves + 4 * k + sub);
            uint64_t ksel, psel = QUAD_NO_SA;
            uint32_t c;
            if (KO) {
                const uint64_t ka = (uint64_t)e.x | ((uint64_t)e.y << 32), kb = (uint64_t)e.z | ((uint64_t)e.w << 32);
                c = quad_sum((ka < K64) + (kb < K64));
                ksel = (c & 1) ? kb : ka;
            } else {
                ksel = (uint64_t)e.x | ((uint64_t)e.y << 32);
                psel = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
                c = quad_sum(ksel < K64);
            }
            const int src = lane0 + (int)((KO ? c >> 1 : c) & 3);
            const uint64_t kc = __shfl((unsigned long long)ksel, src, 64);
            const uint64_t pc = KO ? QUAD_NO_SA : __shfl((unsigned long long)psel, src, 64);
            if (sub == j) {
                x0 = EPL * k + c;
                known = c < EPL;  // else x0 starts the next leaf: nothing read for it yet
                key0 = kc;
                p0 = known ? pc : QUAD_NO_SA;
            }
        }
        if (!mine) continue;
        const uint64_t pos = quad_x0_finish<QW, KO, W, QR>(a, q, Kmine, x0, known, key0, p0, &probes);
        a.out_pos[i] = pos;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// Occurrence ranges on the quad tree: global ranks [lo, hi) of the suffixes
// that start with q (out_pos = lo, out_hi = hi), as k_sa_sector_range.
template <int QW, bool KO, int W>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_quad_range(SearchArgs a, uint64_t* out_hi) {
    __shared__ uint4 s_nodes[SAS_QUAD_LDS_NODES * 4];
    stage_quad_top(a, s_nodes);
    const uint32_t sub = threadIdx.x & (QUAD_G - 1);
    uint32_t bad = 0;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / QUAD_G;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / QUAD_G; i < a.nq; i += stride) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        uint32_t probes = 0;
        uint64_t px = 0;
        const uint64_t lo = quad_bound<QW, false, KO, W>(a, s_nodes, q, K64, Q3, sub, &probes, &px);
        uint64_t hi = quad_bound<QW, true, KO, W>(a, s_nodes, q, K64, Q3, sub, &probes, &px);
        if (hi < lo) hi = lo;
        if (sub == 0) {
            a.out_pos[i] = a.rank_lo + lo;
            out_hi[i] = a.rank_lo + hi;
            if (a.out_probes) a.out_probes[i] = probes;
        }
    }
    if (bad) atomicOr(a.bad, 1u);
}

// ------------------------------------------------------------------ INLINE
// binary_search_batch<64>'s probes (sas/sa_search.rs:157-196: same mids, same
// ilog2(n)+1 lockstep iterations, same LDS top as PLAIN) but each probe reads the
// quad leaves' entry: the 32-char key decides unless it equals the query's (then
// the SA value -- in the fused entry, or from the SA array for KO leaves -- and the
// text from char 32), so a len-32 probe is one memory request instead of an SA
// word + two text words.
template <int QW, bool TOP, bool KO, int W>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_inline(SearchArgs a) {
    __shared__ uint4 s_rel[TOP ? SAS_REL_LDS_BYTES / 16 : 1];  // the rel blocks' LDS groups
    if (TOP) {
        stage_rel(s_rel, a.rel, a.rel_lay.lds_bytes);
        __syncthreads();
    }
    uint32_t bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        uint64_t l = 0, r = a.sa_n, pr = QUAD_NO_SA;
        uint32_t k = 1, probes = 0;
        // selects, not a branch on ge: the branch form made the compiler store l or pr through a
        // selected pointer into scratch (24 B a lane, round 5's make resource)
        auto take = [&](uint64_t mid, bool ge, uint64_t p) {
            probes++;
            r = ge ? mid : r;
            pr = ge ? p : pr;
            l = ge ? l : mid + 1;
        };
        uint32_t it = 0;
        if (TOP) {
            // the prefix-relative blocks, as PLAIN reads them; an 8-char tie reads the probe's
            // own entry (key != K64 decides key > K64, the sector predicate)
            for (uint32_t g = 0; g < a.rel_lay.groups; ++g) {
                const uint32_t hh = a.rel_lay.h[g];
                uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0;
                if (l < r) rel_block(a, s_rel, g, it, (uint32_t)k, hh, b0, b1);
                const uint32_t P = b0.x & 0x7FFFu;
                const uint32_t c0 = q.m > P ? q.m - P : 0u;
                const uint32_t c = c0 < 8 ? c0 : 8u;
                const uint32_t mk = c ? (0xFFFFu << (16 - 2 * c)) & 0xFFFFu : 0u;
                const uint32_t qk = (uint32_t)((K64 << (2 * P)) >> 48) & mk;
                for (uint32_t t = 0; t < hh; ++t, ++it) {
                    if (!(l < r)) continue;
                    const uint64_t mid = (l + r) >> 1;
                    const uint32_t key = rel_slot(b0, b1, (1u << t) | (k & ((1u << t) - 1u))) & mk;
                    bool ge;
                    uint64_t p = QUAD_NO_SA;
                    if (key != qk) {
                        ge = key > qk;
                    } else {
                        uint64_t ek;
                        if (KO) {
                            ek = quad_entry_key<true>(a, mid);
                            p = ek == K64 ? quad_entry_sa<true, W>(a, mid) : QUAD_NO_SA;
                        } else {
                            const uint4 e = a.quad_leaves[mid];
                            ek = (uint64_t)e.x | ((uint64_t)e.y << 32);
                            p = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
                        }
                        ge = sector_ge<QW>(ek, p, K64, a, q);
                    }
                    k = 2 * k + (ge ? 0u : 1u);
                    take(mid, ge, p);
                }
            }
        }
        for (; it < a.iters; ++it) {
            if (l < r) {
                const uint64_t mid = (l + r) >> 1;
                uint64_t key, p;
                if (KO) {
                    key = quad_entry_key<true>(a, mid);
                    p = key == K64 ? quad_entry_sa<true, W>(a, mid) : QUAD_NO_SA;
                } else {
                    const uint4 e = a.quad_leaves[mid];
                    key = (uint64_t)e.x | ((uint64_t)e.y << 32);
                    p = (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
                }
                take(mid, sector_ge<QW>(key, p, K64, a, q), p);
            }
        }
        // SA[r] not seen yet (a compact leaf's key, or a pivot decided by its first 16 chars)
        if (r >= a.sa_n) pr = a.next_pos;
        else if (pr == QUAD_NO_SA) pr = KO ? quad_entry_sa<true, W>(a, r) : quad_entry_sa<false, W>(a, r);
        a.out_pos[i] = pr;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// QUAD / INLINE
template <bool KO, int W>
static void launch_quad_leaves(const LaunchCtx& c, const SearchArgs& a, int algo, int qw, bool top) {
    if (algo == SAS_ALGO_QUAD) {
        // m <= 32: the cooperative kernel; longer: one lane per query (as STREE), two query
        // words in registers (m <= 64), later ones repacked from the bytes
        if (qw == 1) launch(c, k_sa_quad<1, KO, W>, a);
        else if (qw == 2) launch(c, k_sa_quad4x<2, KO, W, false>, a);
        else launch(c, k_sa_quad4x<SAS_QUAD4X_MAXREGS, KO, W, true>, a);
    } else if (top) {
        with_qw(qw, [&](auto Q) { launch(c, k_sa_inline<decltype(Q)::value, true, KO, W>, a); });
    } else {
        with_qw(qw, [&](auto Q) { launch(c, k_sa_inline<decltype(Q)::value, false, KO, W>, a); });
    }
}

void launch_quad(const LaunchCtx& c, const SearchArgs& a, int algo, bool ko, uint32_t sa_w, int qw, bool top) {
    with_leaves(ko, sa_w, [&](auto KO, auto W) {
        launch_quad_leaves<decltype(KO)::value, decltype(W)::value>(c, a, algo, qw, top);
    });
}

void launch_quad_range(const LaunchCtx& c, const SearchArgs& a, bool ko, uint32_t sa_w, int qw, uint64_t* dhi) {
    with_leaves(ko, sa_w, [&](auto KO, auto W) {
        with_qw(qw, [&](auto Q) {
            launch(c, k_sa_quad_range<decltype(Q)::value, decltype(KO)::value, decltype(W)::value>, a, dhi);
        });
    });
}
