// sas_rescue.hip -- paired-end mapping with mate rescue (sas.h: sas_map_pairs_rescue,
// sas_map_pairs_rescue_fixed).  Steps 1..3 and the records are those of sas_map_pairs
// (pair_path.hpp declares them, sas_pairs.hip defines them); between them, for the pairs that the
// join left without a proper candidate:
//
//   3a. the anchors    every locus of an eligible pair (no proper candidate, at most max_anchors
//                      loci over both mates and strands) whose partner's length takes part is an
//                      anchor.  RsAnchors says so per locus; a scan of it over the P slots of the
//                      loci scratch and k_rescue_anchors compact the anchors' locus numbers.  Most
//                      pairs are proper, so the scan below must not stride over all loci.  The
//                      anchor count NA stays on the device, behind the scan;
//   3b. k_pair_rescue  output-centric over NA x CPA items, CPA = ceil((spread + 1) / RS_CHUNK)
//                      chunks of window ends per anchor, a constant of the call: item ->
//                      (anchor, chunk) is one division.  One lane per item runs Myers' search
//                      form (EdMyers, the column step of k_ed_verify) for the partner's other
//                      strand over the text columns [max(0, c0 - 1 - m_b - k_rescue), c1) of its
//                      chunk of ends [c0, c1]: an alignment of cost <= k_rescue that ends at e
//                      starts at or after e - m_b - k_rescue, so the free-start score over those
//                      columns, capped at k_rescue + 1, is D(e) for every end from c0 - 1 on,
//                      whichever chunk computes it (the exactness argument of k_ed_verify).  The
//                      column before c0 is there for the run heads: a head is a candidate end
//                      that is the window's first end or whose predecessor is no candidate, and
//                      the lane knows D(c0 - 1) from its lead-in, so a run that crosses a chunk
//                      edge is counted once, with no communication.  A lane stops once score -
//                      ends left > k_rescue, and no column >= n is read.  Each lane reduces its
//                      chunk to one key in the layout of the join's key and a head count, and
//                      combines them per pair with a 64-bit atomicMin and atomicAdd: integer min
//                      and add only, so the result does not depend on the order of arrival.
//                      On an index with a sequence layout (template bool LAY) the window is cut to
//                      the anchor's sequence and the lane runs rs_scan_chunk_lay, which resets
//                      at every segment's lo and skips the gap columns.
#include "pair_path.hpp"

#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#ifndef RS_CHUNK
#define RS_CHUNK SAS_RESCUE_CHUNK  // window ends per work item (DESIGN §5 has the sweep)
#endif
#define RS_BLOCK 256

// Locus l is an anchor: 1 or 0 (0 at and past L)
struct RsAnchors {
    const uint64_t* lkey;
    const uint64_t* meta;    // [0] = L
    const uint64_t* nloci;   // per batch query
    const uint64_t* pcnt;    // per pair: proper candidates
    const uint64_t* qoff;    // the batch's lengths (MmQueries::len)
    const uint32_t* qlen;
    uint32_t m;
    uint64_t nq;             // reads: batch query r is read r, nq + r its reverse complement
    uint32_t ebits, k_rescue;
    uint64_t max_anchors;
    __device__ __host__ uint64_t operator()(uint64_t l) const {
        if (l >= meta[0]) return 0;
        const uint64_t b = lkey[l] >> ebits;
        const bool s = b >= nq;
        const uint64_t r = s ? b - nq : b, i = r >> 1;
        if (r >= nq || pcnt[i]) return 0;
        const uint64_t anchors = nloci[2 * i] + nloci[2 * i + 1] + nloci[nq + 2 * i] + nloci[nq + 2 * i + 1];
        if (anchors > max_anchors) return 0;
        const uint64_t bb = s ? (r ^ 1ull) : nq + (r ^ 1ull);  // the partner on the other strand
        const uint32_t mb = qoff ? qlen[bb] : m;
        return mb > k_rescue && mb <= SAS_ED_MAX_M ? 1ull : 0ull;
    }
};

// aidx[rank] = the locus of anchor `rank`; ascan: the exclusive scan of RsAnchors over P + 1 slots
__global__ void k_rescue_anchors(RsAnchors a, const uint64_t* __restrict__ ascan, uint64_t P,
                                 uint64_t* __restrict__ aidx) {
    GRID_STRIDE(l, P) {
        if (a(l)) aidx[ascan[l]] = l;
    }
}

struct RsArgs {
    const uint64_t* tw;
    uint64_t n;
    const uint64_t* lkey;
    const uint8_t* ldist;
    const uint64_t* aidx;
    const uint64_t* na;     // the anchor count, on the device
    MmQueries B;            // the batch
    uint64_t nq;            // reads
    uint32_t ebits, k_rescue, min_frag, max_frag;
    uint32_t cpa;           // chunks per anchor
    uint64_t* rmin;         // per pair: the least key (MAP_NONE before)
    uint64_t* rcnt;         // per pair: candidate runs (0 before)
    LayoutView lay;         // LAY: the index's sequence layout
};

// The ends [c0, c1] (0 <= c0 <= c1 <= n) of the window [lo, hi] of one anchor, `first` its first
// end.  rev: the anchor is the reverse mate, so the ends scanned are e_x; base: the key's sum of
// the anchor's distance, o, and e_x of a forward anchor
template <int NW>
__device__ __forceinline__ void rs_scan_chunk(const RsArgs& a, const uint8_t* __restrict__ qb, uint32_t m, int64_t c0,
                                              int64_t c1, int64_t first, int64_t lo, int64_t hi, bool rev,
                                              uint64_t base, uint64_t* best_out, uint32_t* heads_out) {
    const int64_t kr = (int64_t)a.k_rescue;
    int64_t w0 = c0 - 1 - (int64_t)m - kr;                          // the columns [w0, c1), c1 <= n
    if (w0 < 0) w0 = 0;
    uint64_t best = MAP_NONE;
    uint32_t heads = 0;
    EdMyers<NW> my;
    my.init(qb, m);
    int64_t score = m;
    bool prev = false;                                              // D(w0) from nothing is m > k_rescue
    for (int64_t col = w0; col < c1; col += 32) {
        uint64_t tx = text_chars32(a.tw, (uint64_t)col);            // col < c1 <= n
        const int64_t cend = col + 32 < c1 ? col + 32 : c1;
        for (int64_t c = col; c < cend; c++, tx <<= 2) {
            score += my.column(tx);
            const int64_t e = c + 1;                                // the score is D of end c + 1
            const bool cand = score <= kr;
            if (cand && e >= c0) {
                const uint64_t key = base + ((uint64_t)score << PR_SUM_SHIFT) +
                                     (rev ? ((uint64_t)e << PR_EX_SHIFT) + (uint64_t)(hi - e) : (uint64_t)(e - lo));
                best = key < best ? key : best;
                heads += !prev || e == first ? 1u : 0u;
            }
            prev = cand;
            if (score - (c1 - e) > kr) {                            // out of reach for every later end
                col = c1;
                break;
            }
        }
    }
    *best_out = best;
    *heads_out = heads;
}

// rs_scan_chunk on an index with a sequence layout: the columns [w0, c1) can cross several segment
// edges.  The lane finds the first segment that ends behind w0 once and keeps its [slo, shi); it
// resets (EdMyers::reset, score = m) before the first column of each segment, so the score is
// D_L of sas.h; at a gap column it reports no candidate (prev = false) and jumps to the next
// segment's lo, or to the chunk's end when no segment starts before c1, so a gap of any length
// costs one step.  A reset does not clear prev: the end at a segment's lo belongs to the segment
// before it when the two are adjacent.  The early exit fires only when the current segment
// reaches the chunk's end (behind a reset the score starts again at m), and in a gap when no
// segment starts before c1.  w0 inside a segment needs no more than before: the lead-in argument
template <int NW>
__device__ __forceinline__ void rs_scan_chunk_lay(const RsArgs& a, const uint8_t* __restrict__ qb, uint32_t m,
                                                  int64_t c0, int64_t c1, int64_t first, int64_t lo, int64_t hi,
                                                  bool rev, uint64_t base, uint64_t* best_out, uint32_t* heads_out) {
    const int64_t kr = (int64_t)a.k_rescue, none = INT64_MAX;
    int64_t w0 = c0 - 1 - (int64_t)m - kr;                          // the columns [w0, c1), c1 <= n
    if (w0 < 0) w0 = 0;
    uint64_t g = 0, gh = a.lay.nseg;
    while (g < gh) {                                                // the segments with hi <= w0 lie before
        const uint64_t mid = (g + gh) >> 1;
        if ((int64_t)a.lay.seg_hi[mid] <= w0) g = mid + 1;
        else gh = mid;
    }
    int64_t slo = g < a.lay.nseg ? (int64_t)a.lay.seg_lo[g] : none, shi = g < a.lay.nseg ? (int64_t)a.lay.seg_hi[g] : none;
    uint64_t best = MAP_NONE;
    uint32_t heads = 0;
    EdMyers<NW> my;
    my.init(qb, m);
    int64_t score = m;
    bool prev = false;
    for (int64_t col = w0; col < c1; col += 32) {
        uint64_t tx = text_chars32(a.tw, (uint64_t)col);            // col < c1 <= n
        const int64_t cend = col + 32 < c1 ? col + 32 : c1;
        for (int64_t c = col; c < cend; c++, tx <<= 2) {
            if (c >= shi) {                                         // the next segment (they are not empty)
                g++;
                slo = g < a.lay.nseg ? (int64_t)a.lay.seg_lo[g] : none;
                shi = g < a.lay.nseg ? (int64_t)a.lay.seg_hi[g] : none;
            }
            if (c < slo) {                                          // a gap column: its end has no D_L
                prev = false;
                col = (slo < c1 ? slo : c1) - 32;                   // go on at the next segment's lo, or stop:
                break;                                              // the outer step adds the 32 and reloads tx
            }
            if (c == slo) {
                my.reset();
                score = m;
            }
            score += my.column(tx);
            const int64_t e = c + 1;
            const bool cand = score <= kr;
            if (cand && e >= c0) {
                const uint64_t key = base + ((uint64_t)score << PR_SUM_SHIFT) +
                                     (rev ? ((uint64_t)e << PR_EX_SHIFT) + (uint64_t)(hi - e) : (uint64_t)(e - lo));
                best = key < best ? key : best;
                heads += !prev || e == first ? 1u : 0u;
            }
            prev = cand;
            if (shi >= c1 && score - (c1 - e) > kr) {               // out of reach for every later end
                col = c1;
                break;
            }
        }
    }
    *best_out = best;
    *heads_out = heads;
}

// NW: 1, 2, 4 words of 64 rows for every read of the batch (fixed length), 0: by each partner's m.
// LAY: the index has a sequence layout; without one the instructions are those from before
template <int NW, bool LAY>
__global__ __launch_bounds__(RS_BLOCK) void k_pair_rescue(RsArgs a) {
    const uint64_t items = *a.na * (uint64_t)a.cpa;
    const uint64_t emask = (1ull << a.ebits) - 1ull;
    const int64_t spread = (int64_t)a.max_frag - (int64_t)a.min_frag, n = (int64_t)a.n;
    GRID_STRIDE(it, items) {
        const uint64_t ai = it / a.cpa;
        const int64_t ch = (int64_t)(it - ai * a.cpa);
        const uint64_t l = a.aidx[ai];
        const uint64_t lk = a.lkey[l], b = lk >> a.ebits;
        const int64_t ea = (int64_t)(lk & emask);
        const bool rev = b >= a.nq;
        const uint64_t r = rev ? b - a.nq : b, rb = r ^ 1ull;
        const uint64_t bb = rev ? rb : a.nq + rb;                   // the partner on the other strand
        const uint32_t ma = a.B.len(b), mb = a.B.len(bb);
        if (mb <= a.k_rescue || mb > SAS_ED_MAX_M) continue;        // no anchor: a guard for the word count
        // the window of the partner's ends, and this item's chunk of it
        const int64_t lo = rev ? ea + (int64_t)mb - (int64_t)a.max_frag : ea - (int64_t)ma + (int64_t)a.min_frag;
        const int64_t hi = lo + spread;
        int64_t first = lo > 0 ? lo : 0;
        int64_t c0 = lo + ch * (int64_t)RS_CHUNK, c1 = c0 + (int64_t)RS_CHUNK - 1;
        if (c1 > hi) c1 = hi;
        if (c1 > n) c1 = n;
        if (c0 < 0) c0 = 0;
        if (LAY) {  // the window is cut to the anchor's sequence, (seq_start[i], seq_start[i + 1]]
            const uint64_t sq = layout_seq_of_end(a.lay, (uint64_t)ea);
            if (sq == LAYOUT_NONE) continue;
            const int64_t s0 = (int64_t)a.lay.seq_start[sq] + 1, s1 = (int64_t)a.lay.seq_start[sq + 1];
            if (first < s0) first = s0;
            if (c0 < s0) c0 = s0;
            if (c1 > s1) c1 = s1;
        }
        if (c0 > c1) continue;
        const uint64_t o = (rev ? rb : r) & 1ull;                   // f - 2 i of the forward mate
        const uint64_t base = ((uint64_t)a.ldist[l] << PR_SUM_SHIFT) | (o << PR_O_SHIFT) |
                              (rev ? 0ull : (uint64_t)ea << PR_EX_SHIFT);
        const uint8_t* qb = a.B.qbytes + a.B.off(bb);
        uint64_t best = MAP_NONE;
        uint32_t heads = 0;
        if (LAY) {
            if (NW == 1 || (NW == 0 && mb <= 64))
                rs_scan_chunk_lay<1>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
            else if (NW == 2 || (NW == 0 && mb <= 128))
                rs_scan_chunk_lay<2>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
            else rs_scan_chunk_lay<4>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
        } else if (NW == 1 || (NW == 0 && mb <= 64)) rs_scan_chunk<1>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
        else if (NW == 2 || (NW == 0 && mb <= 128))
            rs_scan_chunk<2>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
        else rs_scan_chunk<4>(a, qb, mb, c0, c1, first, lo, hi, rev, base, &best, &heads);
        const uint64_t pair = r >> 1;
        if (best != MAP_NONE) atomicMin((unsigned long long*)&a.rmin[pair], (unsigned long long)best);
        if (heads) atomicAdd((unsigned long long*)&a.rcnt[pair], (unsigned long long)heads);
    }
}

// All arrays on the device; Q: the caller's 2 np reads
static int rescue_device(const sas_index* x, const MmQueries& Q, const PairCall& c, const PairOut& o, hipStream_t st,
                         uint32_t flags) {
    PairState ps;
    TRY(pair_join_batch(x, Q, c, st, flags, ps));
    const uint64_t nq = Q.nq, np = nq / 2, P = ps.ms.s.P;
    PoolBuf rslots, ascan, aidx;
    uint64_t* rmin = nullptr;
    uint64_t* rcnt = nullptr;
    if (c.max_anchors && P) {  // without a proposal there is no locus and no anchor
        hipMemPool_t pool;
        TRY(sas_scratch_pool(x, &pool));
        // the rescue's slots and the anchor scratch, sized from P: anchors <= loci <= P
        TRY(rslots.alloc(pool, 2 * np * 8, st));
        HIP_TRY(hipMemsetAsync(rslots.p, 0xFF, np * 8, st));
        HIP_TRY(hipMemsetAsync(rslots.as<uint64_t>() + np, 0, np * 8, st));
        rmin = rslots.as<uint64_t>();
        rcnt = rmin + np;
        TRY(ascan.alloc(pool, (P + 1) * 8, st));
        TRY(aidx.alloc(pool, P * 8, st));
        const MmQueries& B = ps.ms.B;
        RsAnchors an{};
        an.lkey = ps.lkey.as<uint64_t>();
        an.meta = ps.meta.as<uint64_t>();
        an.nloci = ps.ms.nloci;
        an.pcnt = ps.pslots.as<uint64_t>() + np;
        an.qoff = B.qoff;
        an.qlen = B.qlen;
        an.m = B.m;
        an.nq = nq;
        an.ebits = ps.ms.s.ebits;
        an.k_rescue = c.k_rescue;
        an.max_anchors = c.max_anchors;
        // 3a. the anchors
        TRY(pool_scan(pool, st, rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), an),
                    ascan.as<uint64_t>(), P + 1));
        hipLaunchKernelGGL(k_rescue_anchors, seed_grid(x, P), dim3(256), 0, st, an, ascan.as<uint64_t>(), P,
                           aidx.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        // 3b. the window scans
        RsArgs a{};
        a.tw = x->text_w;
        a.n = x->n;
        a.lkey = an.lkey;
        a.ldist = ps.ldist.as<uint8_t>();
        a.aidx = aidx.as<uint64_t>();
        a.na = ascan.as<uint64_t>() + P;
        a.B = B;
        a.nq = nq;
        a.ebits = an.ebits;
        a.k_rescue = c.k_rescue;
        a.min_frag = c.min_frag;
        a.max_frag = c.max_frag;
        a.cpa = (c.max_frag - c.min_frag) / RS_CHUNK + 1;  // ceil((spread + 1) / RS_CHUNK)
        a.rmin = rmin;
        a.rcnt = rcnt;
        // the grid is capped and strides over the item count, which stays on the device
        const uint64_t upper = P * (uint64_t)a.cpa;
        const dim3 rgrid(tile_grid(std::min(grid_for(upper, RS_BLOCK), (unsigned)x->num_cus * 8)));
        a.lay = x->lay;
        with_ed_words(B, [&](auto NW) { with_bool(x->lay.nseq != 0, [&](auto LAY) {
            hipLaunchKernelGGL((k_pair_rescue<decltype(NW)::value, decltype(LAY)::value>), rgrid, dim3(RS_BLOCK), 0, st, a);
        }); });
        HIP_TRY(hipGetLastError());
    }
    return pair_finish<true>(x, c, ps, rmin, rcnt, o, st, flags);
}

extern "C" int sas_map_pairs_rescue(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff,
                                    const uint32_t* qlen, uint64_t npairs, uint32_t k, uint32_t k_rescue,
                                    uint64_t max_seed_hits, uint32_t min_frag, uint32_t max_frag, uint64_t max_anchors,
                                    void* out_end, void* out_start, uint8_t* out_dist, uint8_t* out_strand,
                                    uint32_t* out_nbest, uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs,
                                    uint8_t* out_qflags, uint8_t* out_pflags, uint32_t* out_npairs,
                                    uint32_t* out_nbestpairs, uint32_t* out_nrescue, void* stream, uint32_t flags) {
    const PairOut o{{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags},
                    out_pflags, out_npairs, out_nbestpairs, out_nrescue};
    const PairCall c{k, k_rescue, max_seed_hits, min_frag, max_frag, max_anchors, true};
    return pairs_impl("sas_map_pairs_rescue", x, QueryArgs{qbytes, qoff, qlen, 0, true}, npairs, c, rescue_device, o,
                      stream, flags);
}

extern "C" int sas_map_pairs_rescue_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t npairs,
                                          uint32_t k, uint32_t k_rescue, uint64_t max_seed_hits, uint32_t min_frag,
                                          uint32_t max_frag, uint64_t max_anchors, void* out_end, void* out_start,
                                          uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                                          uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs,
                                          uint8_t* out_qflags, uint8_t* out_pflags, uint32_t* out_npairs,
                                          uint32_t* out_nbestpairs, uint32_t* out_nrescue, void* stream,
                                          uint32_t flags) {
    const PairOut o{{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags},
                    out_pflags, out_npairs, out_nbestpairs, out_nrescue};
    const PairCall c{k, k_rescue, max_seed_hits, min_frag, max_frag, max_anchors, true};
    return pairs_impl("sas_map_pairs_rescue_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, npairs, c,
                      rescue_device, o, stream, flags);
}
