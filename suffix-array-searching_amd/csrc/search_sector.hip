// search_sector.hip -- SECTOR (k_sa_sector, k_sa_sector_range) and INTERP (k_sa_interp): one lane per
// query on the sector predicate, and their launchers.
#include "search_keys.hpp"

// ------------------------------------------------------------------ SECTOR
// SA value of leaf entry j (0/1) from the leaf's second 16 B: low word + bits 32..39
__device__ __forceinline__ uint64_t sector_sa(uint4 sv, uint32_t j) {
    uint32_t lo = j ? sv.y : sv.x;
    return (uint64_t)lo | ((uint64_t)((sv.z >> (8 * j)) & 0xFF) << 32);
}

__device__ __forceinline__ void sector_entry(const uint4* __restrict__ leaves, uint64_t x, uint64_t* key, uint64_t* p) {
    const uint64_t* kk = reinterpret_cast<const uint64_t*>(leaves + 2 * (x >> 1));
    *key = kk[x & 1];
    *p = sector_sa(leaves[2 * (x >> 1) + 1], (uint32_t)(x & 1));
}

// First local rank x with pred(x) (pred monotone over ranks, false before the
// routed leaf), by descent on the 16-char key R16, the routed leaf, and an
// exponential + binary search on the leaf array for runs that cross leaves.
template <int QW, bool UPPER>
__device__ __forceinline__ uint64_t sector_bound(const SearchArgs& a, const uint4* s_nodes, const QueryRegs<QW>& q,
                                                 uint64_t K64, uint64_t Q3, uint32_t* probes, uint64_t* px) {
    const uint64_t sa_n = a.sa_n;
    const uint4* leaves = a.sec_leaves;
    const uint4* g = reinterpret_cast<const uint4*>(a.sec_inner);
    const uint32_t R16 = (uint32_t)(((UPPER && q.m <= 32) ? Q3 : K64) >> 32);
    auto pred = [&](uint64_t key, uint64_t p) -> bool {
        return UPPER ? sector_gt_prefix<QW>(key, p, K64, Q3, a, q) : sector_ge<QW, true>(key, p, K64, a, q);
    };
    uint64_t k = 0;
    auto count8 = [&](uint4 v0, uint4 v1) -> uint32_t {
        return (v0.x < R16) + (v0.y < R16) + (v0.z < R16) + (v0.w < R16) + (v1.x < R16) + (v1.y < R16) +
               (v1.z < R16) + (v1.w < R16);
    };
    // LDS layers, then HBM layers (separate loops: ds_read / global_load, not FLAT)
    uint32_t h = 0;
    for (; h < a.sec_lds_layers; h++) {
        const uint4* node = s_nodes + (a.sec_off[h] + k) * 2;
        k = k * SAS_SECTOR_FAN + count8(node[0], node[1]);
    }
    for (; h < a.sec_inner_layers; h++) {
        const uint4* node = g + (a.sec_off[h] + k) * 2;
        k = k * SAS_SECTOR_FAN + count8(node[0], node[1]);
    }
    *probes += a.sec_inner_layers;
    // leaf k: entries 2k, 2k+1 (everything before 2k fails pred)
    // (non-temporal loads here measured 8% slower: tools/ab_nt2.sh)
    uint4 kv = leaves[2 * k], sv = leaves[2 * k + 1];
    (*probes)++;
    uint64_t key0 = (uint64_t)kv.x | ((uint64_t)kv.y << 32), key1 = (uint64_t)kv.z | ((uint64_t)kv.w << 32);
    const uint64_t p0 = sector_sa(sv, 0), p1 = sector_sa(sv, 1);
    if (2 * k < sa_n && pred(key0, p0)) {
        *px = p0;
        return 2 * k;
    }
    if (2 * k + 1 < sa_n && pred(key1, p1)) {
        *px = p1;
        return 2 * k + 1;
    }
    // rare: a run of entries sharing the routing key continues to the right --
    // exponential search, then binary search, on the leaf array
    uint64_t lo = 2 * k + 2, step = 1, hi;
    if (lo >= sa_n) return sa_n;
    for (;;) {
        hi = lo + step - 1;
        if (hi >= sa_n) { hi = sa_n; break; }
        uint64_t kk, pp;
        sector_entry(leaves, hi, &kk, &pp);
        (*probes)++;
        if (pred(kk, pp)) break;
        lo = hi + 1;
        step *= 2;
    }
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        uint64_t kk, pp;
        sector_entry(leaves, mid, &kk, &pp);
        (*probes)++;
        if (pred(kk, pp)) hi = mid;
        else lo = mid + 1;
    }
    if (lo < sa_n) {
        uint64_t kk;
        sector_entry(leaves, lo, &kk, px);
    }
    return lo;
}

__device__ __forceinline__ void stage_sector_top(const SearchArgs& a, uint4* s_nodes) {
    const uint4* g = reinterpret_cast<const uint4*>(a.sec_inner);
    for (uint32_t w = threadIdx.x; w < a.sec_lds_nodes * 2; w += blockDim.x) s_nodes[w] = g[w];
    __syncthreads();
}

template <int QW>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_sector(SearchArgs a) {
    __shared__ uint4 s_nodes[SAS_SECTOR_LDS_NODES * 2];
    stage_sector_top(a, s_nodes);
    uint32_t bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        uint32_t probes = 0;
        uint64_t px = 0;
        uint64_t x = sector_bound<QW, false>(a, s_nodes, q, q.w[0], 0, &probes, &px);
        a.out_pos[i] = (x >= a.sa_n) ? a.next_pos : px;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// Occurrence ranges: global ranks [lo, hi) of the suffixes that start with q.
// out_pos = lo, out_hi = hi (both rank_lo-based).
template <int QW>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_sector_range(SearchArgs a, uint64_t* out_hi) {
    __shared__ uint4 s_nodes[SAS_SECTOR_LDS_NODES * 2];
    stage_sector_top(a, s_nodes);
    uint32_t bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        uint32_t probes = 0;
        uint64_t px = 0;
        uint64_t lo = sector_bound<QW, false>(a, s_nodes, q, K64, Q3, &probes, &px);
        uint64_t hi = sector_bound<QW, true>(a, s_nodes, q, K64, Q3, &probes, &px);
        if (hi < lo) hi = lo;
        a.out_pos[i] = a.rank_lo + lo;
        out_hi[i] = a.rank_lo + hi;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// ------------------------------------------------------------------ INTERP
// interpolation_search<16> (sas/sa_search.rs:376-421), one lane per query.  string_value<16>
// (sas/util.rs:76-117) of a suffix is the high half of its 32-char packed key; of the query,
// the high half of its first packed word (zero padded past m).  The mid is the
// reference's l + (r-l)(q_val - l_val + 1) / (r_val - l_val + 2) in wrapping u64 arithmetic
// (its release build), clamped to [l + (r-l)/16, l + 15(r-l)/16] (:406-409), so l <= mid < r
// and every probe is an exact compare: the result is binary_search's, the probe count the
// reference's cnt.  FUSED: a probe reads the fused quad leaf entry {key64, SA} (one 16-B
// request); otherwise SA[mid], then the text window (two dependent requests), as the
// reference does.  range: start from the prefix table's range of q's first p chars (cnt + 1,
// sas/sa_search.rs:86-89).
template <int QW, int W, bool FUSED>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_interp(SearchArgs a, uint32_t range) {
    uint32_t bad = 0;
    const SaView<W> sa{a.sa};
    const uint64_t sa_n = a.sa_n;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        uint64_t l = 0, r = sa_n;
        uint32_t cnt = 0;
        if (range) {
            prefix_range(a, K64 >> (64 - 2 * a.prefix_chars), &l, &r);
            cnt = 1;
        }
        auto probe = [&](uint64_t x, uint64_t* key) -> uint64_t {
            if (FUSED) {
                const uint4 e = nt_load4(a.quad_leaves + x);
                *key = (uint64_t)e.x | ((uint64_t)e.y << 32);
                return (uint64_t)e.z | ((uint64_t)(e.w & 0xFFu) << 32);
            }
            const uint64_t p = sa[x];
            *key = text_chars32(a.tw, p);
            return p;
        };
        uint64_t key = 0, l_val = 0, r_val = 1ull << 32, pr = QUAD_NO_SA;
        if (l < sa_n) {  // sa.suffix(l) (:378)
            (void)probe(l, &key);
            l_val = key >> 32;
        }
        if (r < sa_n) {  // sa.suffix(r) when r < len, else 4^K (:379-383)
            pr = probe(r, &key);
            r_val = key >> 32;
        }
        const uint64_t q_val = K64 >> 32;
        while (l < r) {
            cnt++;
            uint64_t mid = l + ((r - l) * (q_val - l_val + 1)) / (r_val - l_val + 2);
            const uint64_t low = l + (r - l) / 16, high = l + 15 * (r - l) / 16;
            mid = mid < low ? low : (mid > high ? high : mid);
            const uint64_t p = probe(mid, &key);
            if (sector_ge<QW>(key, p, K64, a, q)) {  // !(t < q)
                r = mid;
                r_val = key >> 32;
                pr = p;
            } else {
                l = mid + 1;
                l_val = key >> 32;
            }
        }
        a.out_pos[i] = l >= sa_n ? a.next_pos : pr;  // pr = SA[r] (read or moved), l == r
        if (a.out_probes) a.out_probes[i] = cnt;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// SECTOR: positions come from the fused leaves, no SA reads, one instance per QW
void launch_sector(const LaunchCtx& c, const SearchArgs& a, int qw) {
    with_qw(qw, [&](auto Q) { launch(c, k_sa_sector<decltype(Q)::value>, a); });
}

void launch_sector_range(const LaunchCtx& c, const SearchArgs& a, int qw, uint64_t* dhi) {
    with_qw(qw, [&](auto Q) { launch(c, k_sa_sector_range<decltype(Q)::value>, a, dhi); });
}

// INTERP
template <int W, bool FUSED>
static void launch_interp_w(const LaunchCtx& c, const SearchArgs& a, int qw, uint32_t range) {
    with_qw(qw, [&](auto Q) { launch(c, k_sa_interp<decltype(Q)::value, W, FUSED>, a, range); });
}

// fused quad leaves (W = 4 instantiation, no SA reads) or SA + text at any width
void launch_interp(const LaunchCtx& c, const SearchArgs& a, bool fused, uint32_t sa_w, int qw, uint32_t range) {
    if (fused) launch_interp_w<4, true>(c, a, qw, range);
    else if (sa_w == 8) launch_interp_w<8, false>(c, a, qw, range);
    else if (sa_w == 5) launch_interp_w<5, false>(c, a, qw, range);
    else launch_interp_w<4, false>(c, a, qw, range);
}
