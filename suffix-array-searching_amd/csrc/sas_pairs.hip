// sas_pairs.hip -- paired-end mapping with a fragment-length join (sas.h: sas_map_pairs,
// sas_map_pairs_fixed), and what sas_rescue.hip shares with it (pair_path.hpp has the steps and
// the declarations): the batch, the loci and the join (pair_join_batch), the records and one
// alignment per read (pair_finish), the argument checks and the host-pointer path (pairs_impl),
// and every k_pair_* kernel but k_pair_rescue.
#include "pair_path.hpp"

struct PrTile {  // LDS of one tile's segmented reduction
    uint64_t mn[MAP_T];   // per segment of the tile
    uint32_t cnt[MAP_T];
    uint32_t heads[MAP_CHUNKS], pre[MAP_CHUNKS + 1];
};

// The segmented reduction of one tile, for the whole workgroup of MAP_BLOCK threads.  Element
// el = u MAP_BLOCK + tid carries mn[u] (MAP_NONE: nothing) and ct[u]; head[u] starts a segment
// (element 0 must be a head).  Afterwards sg[u] is the element's segment (its rank in the tile),
// s.mn / s.cnt hold the segments' minimum and sum, and the number of segments is returned.  The
// caller puts a __syncthreads() between two tiles.
template <bool MIN, bool CNT>
__device__ __forceinline__ uint32_t pr_tile_reduce(PrTile& s, const bool (&valid)[MAP_PER], const bool (&head)[MAP_PER],
                                                   const uint64_t (&mn)[MAP_PER], const uint32_t (&ct)[MAP_PER],
                                                   uint32_t (&sg)[MAP_PER]) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t x = tid; x < MAP_T; x += MAP_BLOCK) {
        if (MIN) s.mn[x] = MAP_NONE;
        if (CNT) s.cnt[x] = 0;
    }
    uint64_t hb[MAP_PER];
#pragma unroll
    for (int u = 0; u < MAP_PER; u++) {
        hb[u] = __ballot(valid[u] && head[u]);
        if (lane == 0) s.heads[u * 4 + wave] = (uint32_t)__popcll(hb[u]);
    }
    __syncthreads();
    if (tid < MAP_CHUNKS) {  // exclusive scan of the chunks' head counts (half of wave 0)
        const uint32_t v = s.heads[tid];
        uint32_t inc = v;
#pragma unroll
        for (int off = 1; off < MAP_CHUNKS; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if ((int)tid >= off) inc += o;
        }
        s.pre[tid] = inc - v;
        if (tid == MAP_CHUNKS - 1) s.pre[MAP_CHUNKS] = inc;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MAP_PER; u++) {
        // the segment's rank in the tile: heads before and at this element, less one
        sg[u] = valid[u] ? s.pre[u * 4 + wave] + (uint32_t)__popcll(hb[u] & ((2ull << lane) - 1ull)) - 1u : 0xFFFFFFFFu;
        uint64_t m1 = mn[u];
        uint32_t c1 = ct[u];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {  // segmented inclusive scan of the wave's 64 elements
            const uint32_t so = __shfl_up(sg[u], off);
            const bool take = (int)lane >= off && so == sg[u];
            if (MIN) {
                const uint64_t mo = __shfl_up(m1, off);
                if (take && mo < m1) m1 = mo;
            }
            if (CNT) {
                const uint32_t co = __shfl_up(c1, off);
                if (take) c1 += co;
            }
        }
        const uint32_t nx = __shfl_down(sg[u], 1);
        if (valid[u] && sg[u] < MAP_T && (lane == 63 || nx != sg[u])) {  // the last of its segment in this wave
            if (MIN && m1 != MAP_NONE) atomicMin((unsigned long long*)&s.mn[sg[u]], (unsigned long long)m1);
            if (CNT && c1) atomicAdd(&s.cnt[sg[u]], c1);
        }
    }
    __syncthreads();
    return s.pre[MAP_CHUNKS];  // <= the tile's elements
}

struct PairLoci {
    const uint64_t* keys;   // P sorted proposals, (batch query << ebits) | end
    const uint8_t* vals;    // their distances
    uint64_t P;
    uint32_t ebits;
    uint64_t* toff;         // per tile: k_pair_heads writes its heads, the scan turns them into its first locus
    uint64_t* lmin;         // per locus: the least dist << 56 | end (MAP_NONE before k_pair_loci)
    uint64_t* lkey;         // per locus: batch query << ebits (k_pair_loci) | e_rep (k_pair_pack)
    uint8_t* ldist;
    uint64_t* meta;         // [0] = L, [1] = LF
    uint64_t nfwd;          // batch queries below it are forward strands
};

// Proposal p (key, its left neighbour prev) starts a locus: an end of the answer whose
// predecessor is not
__device__ __forceinline__ bool pr_locus_head(uint64_t p, uint64_t key, uint64_t prev, uint32_t ebits) {
    return p == 0 || (prev != key && !((prev >> ebits) == (key >> ebits) && prev + 1 == key));
}

__global__ __launch_bounds__(MAP_BLOCK) void k_pair_heads(PairLoci a) {
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t P = a.P, ntiles = (P + MAP_T - 1) / MAP_T;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MAP_T;
        if (tid == 0) s_n = 0;
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (int u = 0; u < MAP_PER; u++) {
            const uint64_t p = t0 + u * MAP_BLOCK + tid;
            bool h = false;
            if (p < P) h = pr_locus_head(p, a.keys[p], p ? a.keys[p - 1] : 0, a.ebits);
            c += (uint32_t)__popcll(__ballot(h));
        }
        if (lane == 0 && c) atomicAdd(&s_n, c);
        __syncthreads();
        if (tid == 0) a.toff[tile] = s_n;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MAP_BLOCK) void k_pair_loci(PairLoci a) {
    __shared__ PrTile s;
    const uint32_t tid = threadIdx.x;
    const uint64_t P = a.P, ntiles = (P + MAP_T - 1) / MAP_T;
    const uint64_t emask = (1ull << a.ebits) - 1ull;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MAP_T;
        const uint64_t t1 = t0 + MAP_T < P ? t0 + MAP_T : P;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t kb[MAP_PER], mn[MAP_PER];
        uint32_t ct[MAP_PER], sg[MAP_PER];
        bool valid[MAP_PER], head[MAP_PER], own[MAP_PER];
#pragma unroll
        for (int u = 0; u < MAP_PER; u++) {
            const uint32_t el = u * MAP_BLOCK + tid;
            const uint64_t p = t0 + el;
            valid[u] = el < n_el;
            kb[u] = 0;
            mn[u] = MAP_NONE;
            ct[u] = 0;
            head[u] = own[u] = false;
            if (valid[u]) {
                const uint64_t key = a.keys[p], prev = p ? a.keys[p - 1] : 0;
                own[u] = pr_locus_head(p, key, prev, a.ebits);
                head[u] = el == 0 || own[u];
                kb[u] = key & ~emask;
                if (p == 0 || prev != key) mn[u] = ((uint64_t)a.vals[p] << 56) | (key & emask);
            }
        }
        const uint32_t nseg = pr_tile_reduce<true, false>(s, valid, head, mn, ct, sg);
        // the tile's first element goes on a locus of the tile before it unless it is a head itself
        const bool first_own = pr_locus_head(t0, a.keys[t0], t0 ? a.keys[t0 - 1] : 0, a.ebits);
        const bool last_open = t1 < P && !pr_locus_head(t1, a.keys[t1], a.keys[t1 - 1], a.ebits);
        const uint64_t base = a.toff[tile] - (first_own ? 0u : 1u);
#pragma unroll
        for (int u = 0; u < MAP_PER; u++)
            if (valid[u] && own[u] && sg[u] < MAP_T) a.lkey[base + sg[u]] = kb[u];
        for (uint32_t sgi = tid; sgi < nseg && sgi < MAP_T; sgi += MAP_BLOCK) {
            const bool open = (sgi == 0 && !first_own) || (sgi == nseg - 1 && last_open);
            const uint64_t m1 = s.mn[sgi];
            if (!open) a.lmin[base + sgi] = m1;
            else if (m1 != MAP_NONE) atomicMin((unsigned long long*)&a.lmin[base + sgi], (unsigned long long)m1);
        }
        __syncthreads();  // the segment slots are reset by the next tile
    }
}

// L = the loci of all tiles; LF = the first locus of a reverse strand (the batch-query bits of
// lkey are complete after k_pair_loci)
__global__ void k_pair_meta(PairLoci a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t L = a.toff[(a.P + MAP_T - 1) / MAP_T];
    uint64_t l = 0, h = L;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if ((a.lkey[mid] >> a.ebits) < a.nfwd) l = mid + 1;
        else h = mid;
    }
    a.meta[0] = L;
    a.meta[1] = l;
}

__global__ void k_pair_pack(PairLoci a) {
    const uint64_t L = a.toff[(a.P + MAP_T - 1) / MAP_T];
    const uint64_t emask = (1ull << a.ebits) - 1ull;
    GRID_STRIDE(i, L < a.P ? L : a.P) {
        const uint64_t m1 = a.lmin[i];
        a.lkey[i] |= m1 & emask;
        a.ldist[i] = (uint8_t)(m1 >> 56);
    }
}

struct PairJoin {
    const uint64_t* lkey;
    const uint8_t* ldist;
    const uint64_t* meta;
    MmQueries B;            // the batch (the forward mate's length)
    uint64_t nfwd, n;       // 2 np; the text's chars
    uint32_t ebits, min_frag, max_frag;
    uint64_t* pmin;         // per pair: the least pass-1 key (MAP_NONE before pass 1)
    uint64_t* pcnt;         // per pair: proper candidates (0 before pass 1)
    uint64_t* pbest;        // per pair: those at the least sum (0 before pass 2)
    LayoutView lay;         // the index's sequence layout (nseq == 0: none)
};

template <int PASS>
__global__ __launch_bounds__(MAP_BLOCK) void k_pair_join(PairJoin a) {
    __shared__ PrTile s;
    __shared__ uint64_t s_q[MAP_T];  // per segment: its pair
    const uint32_t tid = threadIdx.x;
    const uint64_t L = a.meta[0], LF = a.meta[1], ntiles = (LF + MAP_T - 1) / MAP_T;
    const uint64_t emask = (1ull << a.ebits) - 1ull;
    const int64_t spread = (int64_t)a.max_frag - (int64_t)a.min_frag;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MAP_T;
        const uint64_t t1 = t0 + MAP_T < LF ? t0 + MAP_T : LF;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t pr[MAP_PER], mn[MAP_PER];
        uint32_t ct[MAP_PER], sg[MAP_PER];
        bool valid[MAP_PER], head[MAP_PER];
#pragma unroll
        for (int u = 0; u < MAP_PER; u++) {
            const uint32_t el = u * MAP_BLOCK + tid;
            const uint64_t p = t0 + el;
            valid[u] = el < n_el;
            pr[u] = 0;
            mn[u] = MAP_NONE;
            ct[u] = 0;
            head[u] = false;
            if (!valid[u]) continue;
            const uint64_t key = a.lkey[p], b = key >> a.ebits, ex = key & emask;
            const uint32_t dx = a.ldist[p];
            pr[u] = b >> 1;
            head[u] = el == 0 || (a.lkey[p - 1] >> (a.ebits + 1)) != pr[u];
            if (b >= a.nfwd) continue;
            const int64_t lo = (int64_t)ex - (int64_t)a.B.len(b) + (int64_t)a.min_frag, hi = lo + spread;
            if (hi < 0 || lo > (int64_t)a.n) continue;
            uint32_t need = 0;
            if (PASS == 2) {
                const uint64_t pm = a.pmin[pr[u]];
                if (pm == MAP_NONE || (uint32_t)(pm >> PR_SUM_SHIFT) < dx) continue;
                need = (uint32_t)(pm >> PR_SUM_SHIFT) - dx;
            }
            // the partner window: the reverse-strand loci of the other mate with lo <= e_y <= hi
            const uint64_t bv = (a.nfwd + (b ^ 1ull)) << a.ebits;
            int64_t wlo = lo < 0 ? 0 : lo, whi = hi > (int64_t)a.n ? (int64_t)a.n : hi;
            if (a.lay.nseq) {  // wave-uniform: both ends in one sequence, (seq_start[i], seq_start[i + 1]] of e_x
                const uint64_t sq = layout_seq_of_end(a.lay, ex);
                if (sq == LAYOUT_NONE) continue;
                const int64_t s0 = (int64_t)a.lay.seq_start[sq] + 1, s1 = (int64_t)a.lay.seq_start[sq + 1];
                wlo = wlo < s0 ? s0 : wlo;
                whi = whi > s1 ? s1 : whi;
                if (wlo > whi) continue;
            }
            const uint64_t klo = bv | (uint64_t)wlo;
            const uint64_t khi = bv | (uint64_t)whi;
            uint64_t l = LF, h = L;
            while (l < h) {  // the first locus with klo <= lkey
                const uint64_t mid = (l + h) >> 1;
                if (a.lkey[mid] < klo) l = mid + 1;
                else h = mid;
            }
            const uint64_t w0 = l;
            // loci are at least 2 apart: the window holds at most spread / 2 + 1 of them
            h = w0 + (uint64_t)(spread / 2 + 2);
            if (h > L) h = L;
            while (l < h) {  // the first locus with khi < lkey
                const uint64_t mid = (l + h) >> 1;
                if (a.lkey[mid] <= khi) l = mid + 1;
                else h = mid;
            }
            const uint64_t w1 = l;
            if (PASS == 1) {
                ct[u] = (uint32_t)(w1 - w0);
                uint64_t best = MAP_NONE;  // (D_y, e_y - lo) of the window
                for (uint64_t j = w0; j < w1; j++) {
                    const uint64_t v = ((uint64_t)a.ldist[j] << 16) | (uint64_t)((int64_t)(a.lkey[j] & emask) - lo);
                    best = v < best ? v : best;
                }
                if (w1 > w0)
                    mn[u] = ((uint64_t)(dx + (uint32_t)(best >> 16)) << PR_SUM_SHIFT) | ((b & 1ull) << PR_O_SHIFT) |
                            (ex << PR_EX_SHIFT) | (best & 0xFFFFull);
            } else {
                uint32_t c = 0;
                for (uint64_t j = w0; j < w1; j++) c += a.ldist[j] == need ? 1u : 0u;
                ct[u] = c;
            }
        }
        const uint32_t nseg = pr_tile_reduce<PASS == 1, true>(s, valid, head, mn, ct, sg);
#pragma unroll
        for (int u = 0; u < MAP_PER; u++)
            if (valid[u] && head[u] && sg[u] < MAP_T) s_q[sg[u]] = pr[u];
        __syncthreads();
        for (uint32_t sgi = tid; sgi < nseg && sgi < MAP_T; sgi += MAP_BLOCK) {
            const uint64_t pair = s_q[sgi];
            if (pair >= (a.nfwd >> 1)) continue;
            // a segment that goes on in a neighbouring tile shares its slot with that tile
            const bool open = (sgi == 0 && t0 > 0 && (a.lkey[t0 - 1] >> (a.ebits + 1)) == pair) ||
                              (sgi == nseg - 1 && t1 < LF && (a.lkey[t1] >> (a.ebits + 1)) == pair);
            const uint64_t m1 = s.mn[sgi], c1 = s.cnt[sgi];
            if (PASS == 1) {
                if (!open) {
                    a.pmin[pair] = m1;
                    a.pcnt[pair] = c1;
                } else {
                    if (m1 != MAP_NONE) atomicMin((unsigned long long*)&a.pmin[pair], (unsigned long long)m1);
                    if (c1) atomicAdd((unsigned long long*)&a.pcnt[pair], (unsigned long long)c1);
                }
            } else {
                if (!open) a.pbest[pair] = c1;
                else if (c1) atomicAdd((unsigned long long*)&a.pbest[pair], (unsigned long long)c1);
            }
        }
        __syncthreads();  // the segment slots are reset by the next tile
    }
}

struct PairFin {
    MmQueries B;            // the batch
    uint64_t np, n;
    uint32_t ebits, min_frag;
    const uint64_t* kmin;   // the single-read slots
    const uint64_t* nloci;
    const uint64_t* nbest;
    const uint8_t* efl;
    const uint64_t* lkey;   // the loci (null: none)
    const uint8_t* ldist;
    const uint64_t* meta;
    const uint64_t* pmin;   // the pairs' slots
    const uint64_t* pcnt;
    const uint64_t* pbest;
    const uint64_t* rmin;   // RESCUE: per pair the least rescue key (MAP_NONE: none), in the join's layout,
    const uint64_t* rcnt;   // and the candidate runs of its anchors' windows (both null: rescue is off)
    uint64_t max_anchors;
    PairOut o;
    uint64_t* aoff;         // the alignment request: 2 np + 1 offsets 0 .. 2 np,
    uint64_t* aqoff;        // each read's chosen strand in the batch
    uint32_t* aqlen;        // and its length (0: no alignment)
};

// The first locus of lkey[lo .. hi) that is not below `want`
__device__ __forceinline__ uint64_t pr_locus_lower(const uint64_t* __restrict__ lkey, uint64_t lo, uint64_t hi,
                                                   uint64_t want) {
    uint64_t l = lo, h = hi;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (lkey[mid] < want) l = mid + 1;
        else h = mid;
    }
    return l;
}

// RESCUE (sas_map_pairs_rescue): a pair without a proper candidate takes the rescue winner when
// there is one; the existing instantiation reads none of the rescue fields
template <bool U32, bool RESCUE>
__global__ void k_pair_finalize(PairFin a) {
    const uint64_t nq = 2 * a.np;
    GRID_STRIDE(i, a.np + 1) {
        if (i == a.np) {
            a.aoff[nq] = nq;
            continue;
        }
        const uint64_t pm = a.pmin[i];
        const bool proper = pm != MAP_NONE;
        uint64_t f = 0, ex = 0, ey = 0;
        uint32_t dx = 0, dy = 0;
        bool rescued = false, skipped = false;
        uint64_t got = nq;  // the read that the rescue placed
        if (RESCUE && !proper && a.max_anchors) {
            const uint64_t anchors = a.nloci[2 * i] + a.nloci[2 * i + 1] + a.nloci[nq + 2 * i] + a.nloci[nq + 2 * i + 1];
            skipped = anchors > a.max_anchors;
            const uint64_t rm = a.rmin ? a.rmin[i] : MAP_NONE;
            if (rm != MAP_NONE) {
                rescued = true;
                const uint32_t sum = (uint32_t)(rm >> PR_SUM_SHIFT);
                f = 2 * i + ((rm >> PR_O_SHIFT) & 1ull);
                ex = (rm >> PR_EX_SHIFT) & PR_EX_MASK;
                ey = (uint64_t)((int64_t)ex - (int64_t)a.B.len(f) + (int64_t)a.min_frag + (int64_t)(rm & 0xFFFFull));
                // the anchor's side: (f, e_x) is the representative of a forward locus, or else
                // (v, e_y) that of a reverse one (both at once would be a proper candidate)
                const uint64_t L = a.meta[0], LF = a.meta[1], v = 4 * i + 1 - f;
                const uint64_t wx = (f << a.ebits) | ex, wy = ((nq + v) << a.ebits) | ey;
                const uint64_t lx = pr_locus_lower(a.lkey, 0, LF, wx);
                if (lx < LF && a.lkey[lx] == wx) {
                    dx = a.ldist[lx];
                    dy = sum - dx;
                    got = v;
                } else {
                    const uint64_t ly = pr_locus_lower(a.lkey, LF, L, wy);
                    dy = a.ldist[ly < L ? ly : L - 1];  // a winner's anchor exists: L > 0
                    dx = sum - dy;
                    got = f;
                }
            }
        }
        if (proper) {
            const uint32_t sum = (uint32_t)(pm >> PR_SUM_SHIFT);
            f = 2 * i + ((pm >> PR_O_SHIFT) & 1ull);
            ex = (pm >> PR_EX_SHIFT) & PR_EX_MASK;
            ey = (uint64_t)((int64_t)ex - (int64_t)a.B.len(f) + (int64_t)a.min_frag + (int64_t)(pm & 0xFFFFull));
            // the forward mate's distance: that of its locus, whose representative is e_x
            const uint64_t want = (f << a.ebits) | ex;
            const uint64_t LF = a.meta[1];
            uint64_t l = 0, h = LF;
            while (l < h) {
                const uint64_t mid = (l + h) >> 1;
                if (a.lkey[mid] < want) l = mid + 1;
                else h = mid;
            }
            dx = a.ldist[l < LF ? l : LF - 1];  // a winner's locus exists: LF > 0
            dy = sum - dx;
        }
        for (uint64_t r = 2 * i; r < 2 * i + 2; r++) {
            const MapBest s = map_best_of(r, nq, 2u, SAS_MAP_FWD | SAS_MAP_REV, a.kmin, a.nloci, a.nbest, a.efl);
            bool mapped = s.best != MAP_NONE;
            uint64_t e = mapped ? s.best & ((1ull << 55) - 1ull) : a.n, bb = s.bb;
            uint32_t d = mapped ? (uint32_t)(s.best >> 56) : SAS_AL_NONE_DIST;
            uint32_t strand = mapped ? (uint32_t)((s.best >> 55) & 1ull) : 0u;
            if (proper || (RESCUE && rescued)) {
                mapped = true;
                strand = r == f ? 0u : 1u;
                e = strand ? ey : ex;
                d = strand ? dy : dx;
                bb = strand ? nq + r : r;
            }
            if (U32) static_cast<uint32_t*>(a.o.end)[r] = (uint32_t)e;
            else static_cast<uint64_t*>(a.o.end)[r] = e;
            a.o.dist[r] = (uint8_t)d;
            if (a.o.strand) a.o.strand[r] = (uint8_t)strand;
            if (a.o.nbest) a.o.nbest[r] = map_clamp32(s.nbst);
            if (a.o.nloci) a.o.nloci[r] = map_clamp32(s.nl);
            if (a.o.qflags) a.o.qflags[r] = (uint8_t)(s.fl | (RESCUE && r == got ? SAS_MAP_RESCUED : 0u));
            a.aoff[r] = r;
            a.aqoff[r] = a.B.off(bb);
            a.aqlen[r] = mapped ? a.B.len(bb) : 0u;
        }
        if (a.o.pflags)
            a.o.pflags[i] = (uint8_t)((proper ? SAS_PAIR_PROPER : 0u) | (RESCUE && rescued ? SAS_PAIR_RESCUED : 0u) |
                                      (RESCUE && skipped ? SAS_PAIR_RESCUE_SKIPPED : 0u));
        if (a.o.npairs) a.o.npairs[i] = map_clamp32(a.pcnt[i]);
        if (a.o.nbestpairs) a.o.nbestpairs[i] = map_clamp32(a.pbest[i]);
        if (RESCUE && a.o.nrescue) a.o.nrescue[i] = a.rcnt ? map_clamp32(a.rcnt[i]) : 0u;
    }
}

// All arrays on the device; Q: the caller's 2 np reads
int pair_join_batch(const sas_index* x, const MmQueries& Q, const PairCall& c, hipStream_t st, uint32_t flags,
                           PairState& ps) {
    const uint64_t nq = Q.nq, np = nq / 2;
    const uint32_t min_frag = c.min_frag, max_frag = c.max_frag;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    // 1. the batch of both strands, its sorted proposals, the single-read slots
    MapState& ms = ps.ms;
    TRY(map_select_batch(x, Q, c.k, c.max_seed_hits, SAS_MAP_FWD | SAS_MAP_REV, st, flags, ms));
    const MmQueries& B = ms.B;
    const EdState& s = ms.s;
    // the pairs' slots and the loci scratch, sized from P (the locus total stays on the device)
    PoolBuf &pslots = ps.pslots, &meta = ps.meta, &toff = ps.toff, &lmin = ps.lmin, &lkey = ps.lkey,
              &ldist = ps.ldist;
    TRY(pslots.alloc(pool, 3 * np * 8, st));
    HIP_TRY(hipMemsetAsync(pslots.p, 0xFF, np * 8, st));
    HIP_TRY(hipMemsetAsync(pslots.as<uint64_t>() + np, 0, 2 * np * 8, st));
    TRY(meta.alloc(pool, 16, st));
    HIP_TRY(hipMemsetAsync(meta.p, 0, 16, st));
    if (s.P) {
        const uint64_t tiles = (s.P + MAP_T - 1) / MAP_T;
        const dim3 tgrid((unsigned)tile_grid(std::min<uint64_t>(tiles, (uint64_t)x->num_cus * MAP_BPC)));
        TRY(toff.alloc(pool, (tiles + 1) * 8, st));
        TRY(lmin.alloc(pool, s.P * 8, st));
        TRY(lkey.alloc(pool, s.P * 8, st));
        TRY(ldist.alloc(pool, s.P, st));
        HIP_TRY(hipMemsetAsync(toff.p, 0, (tiles + 1) * 8, st));
        HIP_TRY(hipMemsetAsync(lmin.p, 0xFF, s.P * 8, st));
        // 2. the loci
        PairLoci a{};
        a.keys = s.skeys;
        a.vals = s.svals;
        a.P = s.P;
        a.ebits = s.ebits;
        a.toff = toff.as<uint64_t>();
        a.lmin = lmin.as<uint64_t>();
        a.lkey = lkey.as<uint64_t>();
        a.ldist = ldist.as<uint8_t>();
        a.meta = meta.as<uint64_t>();
        a.nfwd = nq;
        hipLaunchKernelGGL(k_pair_heads, tgrid, dim3(MAP_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
        TRY(pool_scan(pool, st, a.toff, a.toff, tiles + 1));
        hipLaunchKernelGGL(k_pair_loci, tgrid, dim3(MAP_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pair_meta, dim3(1), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pair_pack, seed_grid(x, s.P), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        // 3. the join
        PairJoin j{};
        j.lkey = a.lkey;
        j.ldist = a.ldist;
        j.meta = a.meta;
        j.B = B;
        j.nfwd = nq;
        j.n = x->n;
        j.lay = x->lay;
        j.ebits = s.ebits;
        j.min_frag = min_frag;
        j.max_frag = max_frag;
        j.pmin = pslots.as<uint64_t>();
        j.pcnt = j.pmin + np;
        j.pbest = j.pmin + 2 * np;
        hipLaunchKernelGGL(k_pair_join<1>, tgrid, dim3(MAP_BLOCK), 0, st, j);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pair_join<2>, tgrid, dim3(MAP_BLOCK), 0, st, j);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Steps 4 and 5 behind pair_join_batch.  RESCUE: rmin / rcnt are the rescue's slots (null: it
// found no work) and the alignments are made with k_rescue
template <bool RESCUE>
int pair_finish(const sas_index* x, const PairCall& c, PairState& ps, const uint64_t* rmin, const uint64_t* rcnt,
                const PairOut& o, hipStream_t st, uint32_t flags) {
    MapState& ms = ps.ms;
    const MmQueries& B = ms.B;
    const EdState& s = ms.s;
    const uint64_t nq = B.nq / 2, np = nq / 2;
    PoolBuf &pslots = ps.pslots, &meta = ps.meta, &lkey = ps.lkey, &ldist = ps.ldist;
    // 4. the records and the alignment request
    AlignReq areq;
    TRY(areq.alloc(x, nq, o.start, flags, st));
    PairFin f{};
    f.B = B;
    f.np = np;
    f.n = x->n;
    f.ebits = s.ebits;
    f.min_frag = c.min_frag;
    f.rmin = rmin;
    f.rcnt = rcnt;
    f.max_anchors = c.max_anchors;
    f.kmin = ms.kmin;
    f.nloci = ms.nloci;
    f.nbest = ms.nbest;
    f.efl = ms.efl.as<uint8_t>();
    f.lkey = lkey.as<uint64_t>();
    f.ldist = ldist.as<uint8_t>();
    f.meta = meta.as<uint64_t>();
    f.pmin = pslots.as<uint64_t>();
    f.pcnt = f.pmin + np;
    f.pbest = f.pmin + 2 * np;
    f.o = o;
    f.aoff = areq.aoff;
    f.aqoff = areq.aqoff;
    f.aqlen = areq.aqlen;
    with_bool(flags & SAS_LOCATE_U32, [&](auto U32) {
        hipLaunchKernelGGL((k_pair_finalize<decltype(U32)::value, RESCUE>), seed_grid(x, np + 1), dim3(256), 0, st, f);
    });
    HIP_TRY(hipGetLastError());
    // 5. one alignment per read
    return align_winners(x, B, areq, nq, RESCUE ? c.k_rescue : c.k, o, st, flags);
}

template int pair_finish<false>(const sas_index*, const PairCall&, PairState&, const uint64_t*, const uint64_t*,
                                const PairOut&, hipStream_t, uint32_t);
template int pair_finish<true>(const sas_index*, const PairCall&, PairState&, const uint64_t*, const uint64_t*,
                               const PairOut&, hipStream_t, uint32_t);

int pairs_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t np, const PairCall& c, PairDevice device,
               const PairOut& o, void* stream, uint32_t flags) {
    const std::string w(fn);
    const uint32_t k = c.k, min_frag = c.min_frag, max_frag = c.max_frag;
    if (min_frag > max_frag) SAS_FAIL(EINVAL, w + ": min_frag must not exceed max_frag");
    if (max_frag - min_frag > SAS_PAIR_MAX_SPREAD)
        SAS_FAIL(EINVAL, w + ": max_frag - min_frag must not exceed SAS_PAIR_MAX_SPREAD (" +
                             std::to_string(SAS_PAIR_MAX_SPREAD) + ")");
    if (c.rescue && (c.k_rescue < k || c.k_rescue > MM_MAX_K))
        SAS_FAIL(EINVAL, w + ": k_rescue must be k.." + std::to_string(MM_MAX_K));
    TRY(seed_index_checks(w, x, k, flags, stream));
    // the (batch query, end) sort key of two mates on two strands
    if (np >= (1ull << 61) || ed_bits(x->n) + (np ? ed_bits(4 * np - 1) : 0) > 64)
        SAS_FAIL(EINVAL, w + ": " + std::to_string(np) + " pairs on two strands and a text of " + std::to_string(x->n) +
                             " chars do not fit the 64-bit (query, end) sort key: split the batch");
    if (np == 0) return 0;
    const uint64_t nq = 2 * np;
    if (!q.null_ok(nq) || !o.end || !o.dist) SAS_FAIL(EINVAL, w + ": null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & SAS_DEVICE_PTRS) return device(x, q.device(nq), c, o, st, flags);
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated)
    const uint64_t esz = (flags & SAS_LOCATE_U32) ? 4 : 8, stride = 2 * (uint64_t)(c.rescue ? c.k_rescue : k) + 1;
    HostQueries hq;
    HostOutputs ho;
    MmQueries Q;
    PairOut d{};
    TRY(hq.stage("pair", q, nq, st, &Q));
    TRY(twin_reads(ho, o, nq, esz, stride, "pair", &d));
    TRY(ho.twin(o.pflags, np, "pair flags", &d.pflags));
    TRY(ho.twin(o.npairs, np * 4, "pair candidate counts", &d.npairs));
    TRY(ho.twin(o.nbestpairs, np * 4, "pair best candidate counts", &d.nbestpairs));
    TRY(ho.twin(o.nrescue, np * 4, "pair rescue counts", &d.nrescue));
    TRY(device(x, Q, c, d, st, flags | SAS_VALIDATE));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// All arrays on the device; Q: the caller's 2 np reads
static int pairs_device(const sas_index* x, const MmQueries& Q, const PairCall& c, const PairOut& o, hipStream_t st,
                        uint32_t flags) {
    PairState ps;
    TRY(pair_join_batch(x, Q, c, st, flags, ps));
    return pair_finish<false>(x, c, ps, nullptr, nullptr, o, st, flags);
}

extern "C" int sas_map_pairs(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                             uint64_t npairs, uint32_t k, uint64_t max_seed_hits, uint32_t min_frag,
                             uint32_t max_frag, void* out_end, void* out_start, uint8_t* out_dist,
                             uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci, uint8_t* out_nruns,
                             uint16_t* out_runs, uint8_t* out_qflags, uint8_t* out_pflags, uint32_t* out_npairs,
                             uint32_t* out_nbestpairs, void* stream, uint32_t flags) {
    const PairOut o{{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags},
                    out_pflags, out_npairs, out_nbestpairs, nullptr};
    const PairCall c{k, k, max_seed_hits, min_frag, max_frag, 0, false};
    return pairs_impl("sas_map_pairs", x, QueryArgs{qbytes, qoff, qlen, 0, true}, npairs, c, pairs_device, o, stream,
                      flags);
}

extern "C" int sas_map_pairs_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t npairs, uint32_t k,
                                   uint64_t max_seed_hits, uint32_t min_frag, uint32_t max_frag, void* out_end,
                                   void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                                   uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                                   uint8_t* out_pflags, uint32_t* out_npairs, uint32_t* out_nbestpairs, void* stream,
                                   uint32_t flags) {
    const PairOut o{{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags},
                    out_pflags, out_npairs, out_nbestpairs, nullptr};
    const PairCall c{k, k, max_seed_hits, min_frag, max_frag, 0, false};
    return pairs_impl("sas_map_pairs_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, npairs, c, pairs_device,
                      o, stream, flags);
}
