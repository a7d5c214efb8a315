// search_tagged.hip -- TAGGED, on entries (k_sa_tagged*) and on bucket lines (k_sa_tagged_lines*), and
// their launchers.
#include "search_keys.hpp"

// ------------------------------------------------------------------ TAGGED
// SAS_BUILD_TAGGED (the configs[3] path): entries e[r] = {SA[r] 40 bits |
// chars [p, p+12) of that suffix << 40} in rank order, and the bucket table of the
// reference's prefix_range (sas/sa_search.rs:86-95) with p live: {first rank 40 bits |
// count 24 bits} per p-char key.  Every entry of q's bucket shares q's (zero-padded) first p
// chars, so the entry's tag extends that to a (p+12)-char key: "tag < q's tag" proves
// suffix < q, "tag > q's tag" proves suffix > q, and only a tie needs the length (m <= p+12)
// or an exact compare from char p+12 (the sector predicate with L = p + 12).  A lookup is:
// the bucket word (one aligned 8-B read), the first SAS_TAG_WIN entries of the bucket as
// 16-B entry pairs (a bucket holds ~4 suffixes at n = 4^p), the text past char p+12 of the
// single candidate whose tag ties q's (a positive query's own suffix; read as 16-B word
// pairs, suffix_less_from_x2), and its position straight from the entry.  Larger buckets
// continue with a binary search over the rest.
#ifndef SAS_TAG_WIN
#define SAS_TAG_WIN 8
#endif
#ifndef SAS_TAG_WINS
#define SAS_TAG_WINS 1
#endif
#define TAG_M40 (SAS_SA40_MAX - 1)
// waves per SIMD the long-query (QW >= SAS_TAG_LB_QW) instances are built for
#ifndef SAS_TAG_LB
#define SAS_TAG_LB 5
#endif
#ifndef SAS_TAG_LB_QW
#define SAS_TAG_LB_QW 1
#endif
// threads per block of k_sa_tagged (one wave per SIMD per block: the grid is num_cus x
// SAS_TAG_LB blocks)
#ifndef SAS_TAG_BLOCK
#define SAS_TAG_BLOCK 256
#endif

// chars [p, p+12) of a packed 32-char key (p + 12 <= 32)
__device__ __forceinline__ uint32_t tag_of_key(uint64_t k64, uint32_t p) { return (uint32_t)((k64 << (2 * p)) >> 40); }

// suffix(e) >= q, for an entry of q's bucket
template <int QW, class Q>
__device__ __forceinline__ bool tag_ge(uint64_t e, uint32_t Q12, const SearchArgs& a, const Q& q) {
    const uint32_t T = (uint32_t)(e >> 40);
    if (T != Q12) return T > Q12;
    const uint64_t p = e & TAG_M40;
    const uint32_t L = a.tag_p + SAS_TAG_CHARS;
    if (q.m <= L) return (a.n - p) >= (uint64_t)q.m;  // equal padded keys: a shorter suffix is a prefix of q
    // one text word pair at a time: loading the first 2 pairs together was within noise, 3-4
    // cost 20-25% through register pressure (profiles/HISTORY.md)
    uint32_t lcp;
    return !suffix_less_from_x2<QW>(a.tw, a.n, p, q, L, &lcp);
}

// the first min(m, len) chars of suffix(e) are > q, for an entry of the bucket of q's routing
// key (Q3 = q padded with 3s when m <= p + 12, else q's own; as sector_gt_prefix)
template <int QW, class Q>
__device__ __forceinline__ bool tag_gt_prefix(uint64_t e, uint32_t Q12, uint32_t Q3t, const SearchArgs& a,
                                              const Q& q) {
    const uint32_t T = (uint32_t)(e >> 40);
    const uint32_t L = a.tag_p + SAS_TAG_CHARS;
    if (q.m <= L) return T > Q3t;
    if (T != Q12) return T > Q12;
    uint32_t lcp;
    const bool lt = suffix_less_from_x2<QW>(a.tw, a.n, e & TAG_M40, q, L, &lcp);
    return !lt && lcp < q.m;
}

// ranks [lo, hi) of p-char key x (a saturated count reads the next bucket word)
__device__ __forceinline__ void tag_bucket(const SearchArgs& a, uint64_t x, uint64_t* lo, uint64_t* hi) {
    const uint64_t t = __builtin_nontemporal_load(a.tag_table + x);
    *lo = t & TAG_M40;
    const uint64_t c = t >> 40;
    *hi = c == 0xFFFFFFull ? (a.tag_table[x + 1] & TAG_M40) : *lo + c;
}

// One lookup on the tagged index (q: QueryRegs or WaveQuery).
template <int QW, class Q>
__device__ __forceinline__ void tagged_lookup(const SearchArgs& a, const Q& q, uint64_t i) {
    const uint64_t* ent = reinterpret_cast<const uint64_t*>(a.sa);
    const uint64_t sa_n = a.sa_n;
    const uint32_t sh = 64 - 2 * a.tag_p;
    const uint64_t K64 = q.w[0];
    const uint32_t Q12 = tag_of_key(K64, a.tag_p);
    uint64_t lo, hi;
    tag_bucket(a, K64 >> sh, &lo, &hi);
    // the bucket's suffixes are ranks [lo, hi); rank hi (the next bucket's first suffix, > q)
    // is the answer when all of them are < q, and is read only then (by the bisection
    // below, which ends at hi).  The window holds the first nw entries, loaded as 16-B
    // aligned entry pairs: half the load instructions of 8-B loads, and fewer L1->L2
    // requests and TLB lookups, which bound this kernel (the entries carry 16 bytes of
    // padding, so the pair holding rank sa_n - 1 is readable)
    // SAS_TAG_WINS windows of SAS_TAG_WIN entries are scanned before the bisection: a wave
    // waits for its slowest lane, and a bucket past one window (~2% of lanes at 4 suffixes
    // per bucket, so most waves hold one) costs one more dependent read instead of
    // log2(count - SAS_TAG_WIN) of them
    uint64_t ans = 0, pos = 0, start = lo;
    bool done = false;
#pragma unroll 1
    for (int w = 0; w < SAS_TAG_WINS; w++) {
        const uint64_t wb = lo + (uint64_t)w * SAS_TAG_WIN;
        const uint64_t rest = hi - wb;
        const uint32_t nw = rest < SAS_TAG_WIN ? (uint32_t)rest : (uint32_t)SAS_TAG_WIN;
        uint64_t e[SAS_TAG_WIN];
        {
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            const uint32_t o = (uint32_t)(wb & 1);
            const u64x2* ep = reinterpret_cast<const u64x2*>(ent + (wb & ~1ull));
            uint64_t w2[SAS_TAG_WIN + 2];
#pragma unroll
            for (int j = 0; j < SAS_TAG_WIN / 2 + 1; j++) {
                const u64x2 v = (2u * j < o + nw) ? __builtin_nontemporal_load(ep + j) : u64x2{0ull, 0ull};
                w2[2 * j] = v.x;
                w2[2 * j + 1] = v.y;
            }
#pragma unroll
            for (int j = 0; j < SAS_TAG_WIN; j++) e[j] = (uint32_t)j < nw ? (o ? w2[j + 1] : w2[j]) : 0ull;
        }
        // first slot whose tag is >= q's: every slot before it is < q (tags are sorted
        // within a bucket)
        uint32_t j0 = nw;
#pragma unroll
        for (int j = SAS_TAG_WIN - 1; j >= 0; j--)
            if ((uint32_t)j < nw && (uint32_t)(e[j] >> 40) >= Q12) j0 = (uint32_t)j;
        uint64_t ej = e[0];
#pragma unroll
        for (int j = 1; j < SAS_TAG_WIN; j++) ej = (j0 == (uint32_t)j) ? e[j] : ej;
        if (j0 < nw) {
            const uint64_t r = wb + j0;
            // a text-slice query t[src .. src + m) and the tying entry of suffix src: that
            // suffix starts with q, so it is >= q without reading the text (the slice must
            // lie inside the text)
            const uint64_t src = query_source(q);
            const bool own = src != ~0ull && src + q.m <= a.n && (ej & TAG_M40) == src && (uint32_t)(ej >> 40) == Q12;
            if (own || tag_ge<QW>(ej, Q12, a, q)) {
                ans = r;
                pos = ej & TAG_M40;
                done = true;
            }
            start = r + 1;  // a tag tie whose suffix is < q
            break;
        }
        start = wb + nw;  // the whole window is < q
        if (start >= hi) break;
    }
    if (!done) {  // binary search over the rest of the bucket (rank hi if nothing qualifies)
        uint64_t l2 = start, h2 = hi, pr = QUAD_NO_SA;
        while (l2 < h2) {
            const uint64_t mid = (l2 + h2) >> 1;
            const uint64_t f = __builtin_nontemporal_load(ent + mid);
            if (tag_ge<QW>(f, Q12, a, q)) {
                h2 = mid;
                pr = f & TAG_M40;
            } else {
                l2 = mid + 1;
            }
        }
        ans = l2;
        pos = l2 >= sa_n ? a.next_pos : (pr != QUAD_NO_SA ? pr : (ent[l2] & TAG_M40));
    }
    a.out_pos[i] = pos;
    if (a.out_probes) {  // the reference's cnt: the table, then binary_search over [lo, hi)
        uint32_t probes = 1;
        for (uint64_t l2 = lo, h2 = hi; l2 < h2; probes++) {
            const uint64_t mid = (l2 + h2) >> 1;
            if (mid < ans) l2 = mid + 1;
            else h2 = mid;
        }
        a.out_probes[i] = probes;
    }
}

// byte offset and length of query i
__device__ __forceinline__ void query_span(const SearchArgs& a, uint64_t i, uint64_t* off, uint32_t* m) {
    if (a.qoff) {
        *off = a.qoff[i];
        *m = a.qlen[i];
    } else {
        *off = i * (uint64_t)a.m_fixed;
        *m = a.m_fixed;
    }
}

#ifndef SAS_TAG_WQ
#define SAS_TAG_WQ 1
#endif

template <int QW>
__global__ __launch_bounds__(SAS_TAG_BLOCK, (QW >= SAS_TAG_LB_QW ? SAS_TAG_LB : 8)) void k_sa_tagged(SearchArgs a) {
    uint32_t bad = 0;
#if SAS_TAG_WQ
    // wave-uniform loop over batches of 64 consecutive queries; the batch's bytes are staged
    // through LDS (wave_stage_queries) unless they are spread out
    __shared__ uint32_t wq[SAS_TAG_BLOCK / 64][2 * SAS_WQ_WORDS];
    uint32_t* L32 = wq[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t b0 = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x & ~63u); b0 < a.nq;
         b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = b0 + lane;
        const bool act = i < a.nq;
        uint64_t qo = 0;
        uint32_t m = 0;
        if (act) query_span(a, i, &qo, &m);
        uint64_t base;
        if (wave_stage_queries(a.qbytes, qo, m, act, L32, &base)) {
            if (act) {
                WaveQuery q;
                q.init(L32, (uint32_t)(qo - base), m);
                tagged_lookup<QW>(a, q, i);
            }
        } else if (act) {
            ByteQuery q;
            q.init(a.qbytes + qo, m);
            tagged_lookup<QW>(a, q, i);
        }
    }
#else
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        tagged_lookup<QW>(a, q, i);
    }
#endif
    if (bad) atomicOr(a.bad, 1u);
}

// SAS_QUERIES_ARE_SLICES: query i is the slice t[qoff[i] .. qoff[i] + qlen[i]) of the indexed
// text, read from the packed text (no query bytes), one lane per query.
template <int QW>
__global__ __launch_bounds__(SAS_TAG_BLOCK, SAS_TAG_LB) void k_sa_tagged_slices(SearchArgs a) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t qo;
        uint32_t m;
        query_span(a, i, &qo, &m);
        TextQuery q;
        q.init(a.tw, qo, m);
        tagged_lookup<QW>(a, q, i);
    }
}

// Occurrence ranges on the tagged index: lo = the lower bound in q's bucket, hi = the first
// suffix whose first min(m, len) chars are > q, in the bucket of the routing key; both
// bisections advance in lock step (two entry reads in flight).
template <int QW>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_tagged_range(SearchArgs a, uint64_t* out_hi) {
    uint32_t bad = 0;
    const uint64_t* ent = reinterpret_cast<const uint64_t*>(a.sa);
    const uint32_t sh = 64 - 2 * a.tag_p;
    const uint32_t L = a.tag_p + SAS_TAG_CHARS;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        const uint32_t Q12 = tag_of_key(K64, a.tag_p), Q3t = tag_of_key(Q3, a.tag_p);
        uint64_t lo, l1, hi, h1;
        tag_bucket(a, K64 >> sh, &lo, &l1);
        tag_bucket(a, (m <= L ? Q3 : K64) >> sh, &hi, &h1);
        while (lo < l1 || hi < h1) {
            const bool g0 = lo < l1, g1 = hi < h1;
            const uint64_t m0 = (lo + l1) >> 1, m1 = (hi + h1) >> 1;
            const uint64_t e0 = g0 ? __builtin_nontemporal_load(ent + m0) : 0;
            const uint64_t e1 = g1 ? __builtin_nontemporal_load(ent + m1) : 0;
            if (g0) {
                if (tag_ge<QW>(e0, Q12, a, q)) l1 = m0;
                else lo = m0 + 1;
            }
            if (g1) {
                if (tag_gt_prefix<QW>(e1, Q12, Q3t, a, q)) h1 = m1;
                else hi = m1 + 1;
            }
        }
        if (hi < lo) hi = lo;
        a.out_pos[i] = a.rank_lo + lo;
        out_hi[i] = a.rank_lo + hi;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// ------------------------------------------------------------------ TAGGED on bucket lines
// SAS_BUILD_TAG_LINES (build_tagged.hip, build_tag_lines): line b holds bucket b's header
// {overflow offset | count} and the 48-bit entries {SA | tag << sb} of ranks first .. first +
// 19 (common.hpp: u16 high halves, then u32 low halves), so the bucket word and the first
// window of the tagged lookup above are one 128-B request, and 20 slots keep 98% of the
// positive lookups at ~16 suffixes per bucket inside it.  An 8-lane group reads the lines of
// its 8 queries (one per lane) together, 16 B per lane (lane 0 the header and hi[0..3], lanes
// 1 and 2 hi[4..19], lanes 3..7 lo[0..19]); per line lanes 0-2 count the slots whose tag is
// below the query's, the group sums the counts, and the lanes holding that slot's halves
// hand them to the query's lane; the rest -- the tie's text compare, a larger bucket's
// overflow window -- is per lane.  Slots past the bucket's count hold the next buckets' first
// suffixes with the maximal tag, so "every suffix of the bucket is < q" finds its answer (the
// first suffix after the bucket, rank first + count) in the same line whenever count < 20
// (and at overflow index count - 20 otherwise).
#define TL_G 8
// waves per SIMD the line kernels are built for: the 8 line loads a lane keeps in flight take
// 32 VGPRs (at 5 waves the kernel spills)
#ifndef SAS_TL_LB
#define SAS_TL_LB 4
#endif
#ifndef SAS_TL_WIN
#define SAS_TL_WIN 8  // overflow entries a lane reads before bisecting the rest
#endif

// entry j of bucket b: line slot j (j < 20) or overflow entry j - 20
__device__ __forceinline__ uint64_t tl_entry(const SearchArgs& a, uint64_t b, uint64_t ovf, uint64_t j) {
    return j < SAS_TL_SLOTS ? tl_slot(a.tag_lines, b, (uint32_t)j)
                            : __builtin_nontemporal_load(a.tag_ovf + ovf + (j - SAS_TL_SLOTS));
}

// bucket b's suffix count from its header word (a saturated count reads the first-rank table)
__device__ __forceinline__ uint64_t tl_count(const SearchArgs& a, uint64_t b, uint64_t h0) {
    const uint64_t c = h0 >> 40;
    return c == 0xFFFFFFull ? a.tag_first[b + 1] - a.tag_first[b] : c;
}

// chars known equal to q's when an entry's tag ties with q's: the bucket's p and the tag's whole chars
__device__ __forceinline__ uint32_t tl_known(const SearchArgs& a) { return a.tag_p + (tl_tag_bits(a.tag_sb) >> 1); }

// text word pairs a bucket-line lookup loads together for its tie's compare: 5 pairs (80 B)
// cover chars [p + 12, 256) of any suffix, so no compare of a query of <= 256 chars waits for a
// second round trip (loaded lazily they are ~3 dependent round trips of the whole wave).  Same
// box, 2*10^7 ragged 8..256 at n = 2^34: 5 pairs 1.91 ms, 4 pairs 1.99, 3 pairs 2.05-2.07
// (gpurun_out A/B, profiles/r3/); 0: the lazy pair loop (suffix_less_from_x2).  The pairs come
// from the text copy in which they lie in one 128-B line (sas_index::text2).
#ifndef SAS_TL_PRE
#define SAS_TL_PRE 5
#endif

// suffix(e) >= q for an entry of q's bucket (Qt: q's tag), the tie's text compare preloading
// (PRE) or pair by pair (the rare bisection and the range kernel)
template <int QW, bool PRE, class Q>
__device__ __forceinline__ bool tl_ge(uint64_t e, uint32_t Qt, const SearchArgs& a, const Q& q) {
    const uint32_t T = (uint32_t)(e >> a.tag_sb);
    if (T != Qt) return T > Qt;
    const uint64_t p = e & tl_sa_mask(a.tag_sb);
    const uint32_t L = tl_known(a);
    if (q.m <= L) return (a.n - p) >= (uint64_t)q.m;
    const uint64_t src = query_source(q);  // a text-slice query's own suffix starts with q
    if (src != ~0ull && src + q.m <= a.n && p == src) return true;
    uint32_t lcp;
#if SAS_TL_PRE
    if (PRE) return !suffix_less_from_pre<SAS_TL_PRE>(a.tw, a.tw2, a.n, p, q, L, &lcp);
#endif
    return !suffix_less_from_x2<QW>(a.tw, a.n, p, q, L, &lcp);
}

// the first min(m, len) chars of suffix(e) are > q, for an entry of the bucket of q's routing
// key (Q3t: the tag of q padded with 3s; as tag_gt_prefix)
template <int QW, class Q>
__device__ __forceinline__ bool tl_gt_prefix(uint64_t e, uint32_t Qt, uint32_t Q3t, const SearchArgs& a, const Q& q) {
    const uint32_t T = (uint32_t)(e >> a.tag_sb);
    const uint32_t L = tl_known(a);
    if (q.m <= L) return T > Q3t;
    if (T != Qt) return T > Qt;
    uint32_t lcp;
    const bool lt = suffix_less_from_x2<QW>(a.tw, a.n, e & tl_sa_mask(a.tag_sb), q, L, &lcp);
    return !lt && lcp < q.m;
}

// The lookup after the line: f = the number of the bucket's first 20 suffixes whose tag is
// below q's (20: all of them), ef = slot f's entry when f < 20, h0 = the line's header word
// {overflow offset | count}.  Slots past the bucket's count carry the maximal tag, so f <=
// count when count < 20, and f == count finds the first suffix after the bucket.  The answer
// is entry j of the bucket for the first j in [0, count] whose suffix is >= q (j = count: the
// next bucket's first suffix).  A wave waits for its slowest lane at every step, so the loads
// of the lanes that need the overflow window are issued before the other lanes' text compares
// wait for theirs: one round trip serves both.
template <int QW, class Q>
__device__ __forceinline__ void tl_finish(const SearchArgs& a, const Q& q, uint64_t i, uint64_t b, uint64_t h0,
                                          uint32_t f, uint64_t ef, uint32_t Qt) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const uint32_t sb = a.tag_sb;
    const uint64_t cnt = tl_count(a, b, h0), ovf = h0 & TAG_M40;
    // the overflow window [20, cnt] (entry cnt is >= q whatever its tag), as 16-B aligned pairs
    const bool ovfl = f >= SAS_TL_SLOTS && cnt > SAS_TL_SLOTS;
    const uint64_t rest = ovfl ? cnt + 1 - SAS_TL_SLOTS : 0;
    const uint32_t nw = rest < SAS_TL_WIN ? (uint32_t)rest : (uint32_t)SAS_TL_WIN;
    const uint32_t o = (uint32_t)(ovf & 1);
    uint64_t w2[SAS_TL_WIN + 2];
    if (ovfl) {
        const u64x2* ep = reinterpret_cast<const u64x2*>(a.tag_ovf + (ovf & ~1ull));
#pragma unroll
        for (int k = 0; k < SAS_TL_WIN / 2 + 1; k++) {
            const u64x2 v = (2u * k < o + nw) ? __builtin_nontemporal_load(ep + k) : u64x2{0ull, 0ull};
            w2[2 * k] = v.x;
            w2[2 * k + 1] = v.y;
        }
    }
    uint64_t j = 0, e = 0, start = SAS_TL_SLOTS, cj = 0, ce = 0;
    bool done = false, cand = false;  // cand: entry ce (index cj) needs the compare
    if (f < SAS_TL_SLOTS) {
        if (f >= cnt) {  // the first suffix after the bucket
            j = f;
            e = ef;
            done = true;
        } else {
            cand = true;
            cj = f;
            ce = ef;
        }
        start = (uint64_t)f + 1;  // a tie whose suffix is < q: the search goes on
    } else if (cnt == SAS_TL_SLOTS) {  // every suffix of the bucket is < q: the next one's first
        j = cnt;
        e = tl_entry(a, b, ovf, cnt);
        done = true;
    } else if (ovfl) {
        uint64_t ew[SAS_TL_WIN];
#pragma unroll
        for (int k = 0; k < SAS_TL_WIN; k++) ew[k] = (uint32_t)k < nw ? (o ? w2[k + 1] : w2[k]) : 0ull;
        uint32_t k0 = nw;
#pragma unroll
        for (int k = SAS_TL_WIN - 1; k >= 0; k--)
            if ((uint32_t)k < nw && (SAS_TL_SLOTS + k == cnt || (uint32_t)(ew[k] >> sb) >= Qt)) k0 = (uint32_t)k;
        uint64_t ek0 = ew[0];
#pragma unroll
        for (int k = 1; k < SAS_TL_WIN; k++) ek0 = (k0 == (uint32_t)k) ? ew[k] : ek0;
        if (k0 < nw) {
            const uint64_t r = SAS_TL_SLOTS + k0;
            if (r == cnt) {
                j = r;
                e = ek0;
                done = true;
            } else {
                cand = true;
                cj = r;
                ce = ek0;
            }
            start = r + 1;
        } else {
            start = SAS_TL_SLOTS + nw;
        }
    }
    if (cand && tl_ge<QW, true>(ce, Qt, a, q)) {  // one compare site: a slot's or the window's
        j = cj;
        e = ce;
        done = true;
    }
    if (!done && start == cnt) {  // the first suffix after the bucket
        j = cnt;
        e = tl_entry(a, b, ovf, cnt);
        done = true;
    }
    if (!done) {  // binary search over [start, cnt): entry cnt is >= q
        uint64_t l2 = start, h2 = cnt, pe = 0;
        bool have = false;
        while (l2 < h2) {
            const uint64_t mid = (l2 + h2) >> 1;
            const uint64_t fm = tl_entry(a, b, ovf, mid);
            if (tl_ge<QW, false>(fm, Qt, a, q)) {
                h2 = mid;
                pe = fm;
                have = true;
            } else {
                l2 = mid + 1;
            }
        }
        j = l2;
        e = (have && l2 < cnt) ? pe : tl_entry(a, b, ovf, l2);
    }
    const uint64_t s = e & tl_sa_mask(sb);
    a.out_pos[i] = s == tl_sa_mask(sb) ? a.next_pos : s;
    if (a.out_probes) {  // the reference's cnt: the table, then binary_search over [first, first + cnt)
        uint32_t probes = 1;
        for (uint64_t l2 = 0, h2 = cnt; l2 < h2; probes++) {
            const uint64_t mid = (l2 + h2) >> 1;
            if (mid < j) l2 = mid + 1;
            else h2 = mid;
        }
        a.out_probes[i] = probes;
    }
}

// Exchanges inside an aligned group of 8 lanes without address registers: ds_swizzle in bit
// mode (lane' = ((lane & and) | or) ^ xor within each 32-lane half) and DPP quad_perm.
__device__ __forceinline__ uint32_t g8_swz(uint32_t v, int pattern_k) {
    switch (pattern_k) {  // broadcast from lane k of the group: and 0x18, or k
        case 0: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (0 << 5));
        case 1: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (1 << 5));
        case 2: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (2 << 5));
        case 3: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (3 << 5));
        case 4: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (4 << 5));
        case 5: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (5 << 5));
        case 6: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (6 << 5));
        default: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (7 << 5));
    }
}
// sum over the group of 8 (every lane gets it)
__device__ __forceinline__ uint32_t g8_sum(uint32_t c) {
    c += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0xB1, 0xF, 0xF, false);  // lane ^ 1
    c += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x4E, 0xF, 0xF, false);  // lane ^ 2
    return c + (uint32_t)__builtin_amdgcn_ds_swizzle((int)c, 0x1F | (4 << 10));    // lane ^ 4
}
__device__ __forceinline__ uint32_t sel4(const uint4& v, uint32_t k) {
    const uint32_t lo = (k & 1) ? v.y : v.x, hi = (k & 1) ? v.w : v.z;
    return (k & 2) ? hi : lo;
}

// The cooperative part: every lane of the wave calls it together (act: the lane holds query
// i).  Lane s of a group holds 16 B of each of the group's 8 lines (common.hpp); per line
// lanes 0-2 count the slots whose tag is below the line's query's (the tag halves are the
// high bits of the u16 fields: h < Qt << (sb - 32)), the group sums the counts into f, and the
// lanes holding hi[f] ((f + 4) / 8) and lo[f] (3 + f / 4) hand them, with the header word, to
// the query's lane.
template <int QW, class Q>
__device__ __forceinline__ void tl_lookup(const SearchArgs& a, const Q& q, bool act, uint64_t i) {
    const uint32_t lane = threadIdx.x & 63, sub = lane & (TL_G - 1), g0 = lane & ~(uint32_t)(TL_G - 1);
    const uint32_t sh = 64 - 2 * a.tag_p, hs = a.tag_sb - 32;
    const uint64_t K64 = act ? q.w[0] : 0ull;
    const uint64_t b = K64 >> sh;
    const uint32_t Qt = tl_tag_of_key(K64, a.tag_p, tl_tag_bits(a.tag_sb));
    const uint4* L4 = reinterpret_cast<const uint4*>(a.tag_lines);
    uint4 v[TL_G];
#pragma unroll
    for (int k = 0; k < TL_G; k++) {
        const uint64_t bk = ((uint64_t)g8_swz((uint32_t)(b >> 32), k) << 32) | g8_swz((uint32_t)b, k);
        v[k] = nt_load4(L4 + bk * 8 + sub);
    }
    // tag fields of this lane's 16 B: lane 0 the upper 8 B (hi[0..3]), lanes 1 and 2 all of it;
    // a field h counts when h < Qt << (sb - 32), two fields per packed saturating subtract
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 one = {1, 1};
    const bool lo_tags = sub == 1 || sub == 2, hi_tags = sub <= 2;
    uint64_t my_h0 = 0, my_ef = 0;
    uint32_t my_f = 0;
#pragma unroll
    for (int k = 0; k < TL_G; k++) {
        const uint32_t Qs = g8_swz(Qt, k) << hs;  // (h >> hs) < Qt  <=>  h < Qt << hs
        const uint32_t Qp = Qs | (Qs << 16);
        const u16x2 Qlo = __builtin_bit_cast(u16x2, lo_tags ? Qp : 0u), Qhi = __builtin_bit_cast(u16x2, hi_tags ? Qp : 0u);
        const u16x2 acc =
            __builtin_elementwise_min(__builtin_elementwise_sub_sat(Qlo, __builtin_bit_cast(u16x2, v[k].x)), one) +
            __builtin_elementwise_min(__builtin_elementwise_sub_sat(Qlo, __builtin_bit_cast(u16x2, v[k].y)), one) +
            __builtin_elementwise_min(__builtin_elementwise_sub_sat(Qhi, __builtin_bit_cast(u16x2, v[k].z)), one) +
            __builtin_elementwise_min(__builtin_elementwise_sub_sat(Qhi, __builtin_bit_cast(u16x2, v[k].w)), one);
        const uint32_t f = g8_sum((uint32_t)acc.x + acc.y);
        const uint32_t fe = (f + 4) & 7;
        const uint32_t hw = (sel4(v[k], fe >> 1) >> ((fe & 1) * 16)) & 0xFFFFu;
        const uint32_t mine = sub < 3 ? hw : sel4(v[k], f & 3);
        const uint32_t hl = (f + 4) >> 3, ll = 3 + (f >> 2);
        const uint32_t hiv = (uint32_t)__shfl((int)mine, (int)(g0 + (hl < 2 ? hl : 2u)), 64);
        const uint32_t lov = (uint32_t)__shfl((int)mine, (int)(g0 + (ll < 7 ? ll : 7u)), 64);
        const uint64_t h0 = ((uint64_t)g8_swz(v[k].y, 0) << 32) | g8_swz(v[k].x, 0);
        if (sub == (uint32_t)k) {
            my_h0 = h0;
            my_f = f;
            my_ef = ((uint64_t)hiv << 32) | lov;
        }
        __builtin_amdgcn_sched_barrier(0);  // one line at a time: interleaved, the 8 spill
    }
    if (act) tl_finish<QW>(a, q, i, b, my_h0, my_f, my_ef, Qt);
}

template <int QW>
__global__ __launch_bounds__(SAS_TAG_BLOCK, SAS_TL_LB) void k_sa_tagged_lines(SearchArgs a) {
    // wave-uniform loop over batches of 64 consecutive queries, staged as in k_sa_tagged
    __shared__ uint32_t wq[SAS_TAG_BLOCK / 64][2 * SAS_WQ_WORDS];
    uint32_t* L32 = wq[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t b0 = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x & ~63u); b0 < a.nq;
         b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = b0 + lane;
        const bool act = i < a.nq;
        uint64_t qo = 0;
        uint32_t m = 0;
        if (act) query_span(a, i, &qo, &m);
        uint64_t base;
        if (wave_stage_queries(a.qbytes, qo, m, act, L32, &base)) {
            WaveQuery q;
            q.init(L32, act ? (uint32_t)(qo - base) : 0u, act ? m : 0u);
            tl_lookup<QW>(a, q, act, i);
        } else {
            ByteQuery q;
            q.init(a.qbytes + qo, act ? m : 0u);
            tl_lookup<QW>(a, q, act, i);
        }
    }
}

// SAS_QUERIES_ARE_SLICES on bucket lines
template <int QW>
__global__ __launch_bounds__(SAS_TAG_BLOCK, SAS_TL_LB) void k_sa_tagged_lines_slices(SearchArgs a) {
    for (uint64_t b0 = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x & ~63u); b0 < a.nq;
         b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = b0 + (threadIdx.x & 63);
        const bool act = i < a.nq;
        uint64_t qo = 0;
        uint32_t m = 0;
        if (act) query_span(a, i, &qo, &m);
        TextQuery q;
        q.init(a.tw, qo, m);
        tl_lookup<QW>(a, q, act, i);
    }
}

// Measured and not kept (profiles/r3/defer/, same box, 2*10^7 ragged 8..256 at n = 2^34):
// * two passes: the lanes whose answer lies past the line's 20 slots (~2% of lanes, in most
//   waves) wrote their query index into a per-wave list and a second kernel ran them whole,
//   so no wave waited for the overflow window and its second compare: 1.67 against 1.48 ms
//   (one list counter for the grid, claimed by an atomic per wave: 3.3 ms);
// * the next batch's query offsets and lengths loaded a batch ahead: 1.478 against 1.462 ms.
// The kernel is bound by the rate of its random requests (0.84 of the ceiling), not by the
// round trips of a wave's slowest lane.

// Occurrence ranges on bucket lines: both bounds bisected in their buckets (entries by
// bucket index: slot or overflow), as k_sa_tagged_range does over rank-ordered entries.
template <int QW>
__global__ __launch_bounds__(SEARCH_BLOCK, 8) void k_sa_tagged_lines_range(SearchArgs a, uint64_t* out_hi) {
    uint32_t bad = 0;
    const uint32_t sh = 64 - 2 * a.tag_p, tb = tl_tag_bits(a.tag_sb);
    const uint32_t L = tl_known(a);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QueryRegs<QW> q;
        q.load(qb, m, &bad);
        const uint64_t K64 = q.w[0];
        const uint64_t Q3 = m >= 32 ? K64 : (K64 | (~0ull >> (2 * m)));
        const uint32_t Qt = tl_tag_of_key(K64, a.tag_p, tb), Q3t = tl_tag_of_key(Q3, a.tag_p, tb);
        const uint64_t b0 = K64 >> sh, b1 = (m <= L ? Q3 : K64) >> sh;
        const uint64_t h00 = a.tag_lines[b0 * 16], h10 = a.tag_lines[b1 * 16];
        const uint64_t o0 = h00 & TAG_M40, o1 = h10 & TAG_M40;
        uint64_t lo = 0, l1 = tl_count(a, b0, h00), hi = 0, h1 = tl_count(a, b1, h10);
        while (lo < l1 || hi < h1) {
            const bool g0 = lo < l1, g1 = hi < h1;
            const uint64_t m0 = (lo + l1) >> 1, m1 = (hi + h1) >> 1;
            const uint64_t e0 = g0 ? tl_entry(a, b0, o0, m0) : 0;
            const uint64_t e1 = g1 ? tl_entry(a, b1, o1, m1) : 0;
            if (g0) {
                if (tl_ge<QW, false>(e0, Qt, a, q)) l1 = m0;
                else lo = m0 + 1;
            }
            if (g1) {
                if (tl_gt_prefix<QW>(e1, Qt, Q3t, a, q)) h1 = m1;
                else hi = m1 + 1;
            }
        }
        uint64_t rlo = a.tag_first[b0] + lo, rhi = a.tag_first[b1] + hi;
        if (rhi < rlo) rhi = rlo;
        a.out_pos[i] = a.rank_lo + rlo;
        out_hi[i] = a.rank_lo + rhi;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// TAGGED, on entries or bucket lines (a.tag_lines).  slices: the queries are slices of the
// indexed text (SAS_QUERIES_ARE_SLICES)
void launch_tagged(int num_cus, hipStream_t st, const SearchArgs& a, int qw, bool slices) {
    const bool lines = a.tag_lines != nullptr;
    const uint64_t per_cu = lines ? SAS_TL_LB : (qw >= SAS_TAG_LB_QW ? SAS_TAG_LB : 8);
    const LaunchCtx c = launch_ctx(a.nq, SAS_TAG_BLOCK, (uint64_t)num_cus * per_cu, st);
    with_qw(qw, [&](auto Q) {
        constexpr int QW = decltype(Q)::value;
        if (lines && slices) launch(c, k_sa_tagged_lines_slices<QW>, a);
        else if (lines) launch(c, k_sa_tagged_lines<QW>, a);
        else if (slices) launch(c, k_sa_tagged_slices<QW>, a);
        else launch(c, k_sa_tagged<QW>, a);
    });
}

void launch_tagged_range(const LaunchCtx& c, const SearchArgs& a, int qw, uint64_t* dhi) {
    with_qw(qw, [&](auto Q) {
        constexpr int QW = decltype(Q)::value;
        if (a.tag_lines) launch(c, k_sa_tagged_lines_range<QW>, a, dhi);
        else launch(c, k_sa_tagged_range<QW>, a, dhi);
    });
}
