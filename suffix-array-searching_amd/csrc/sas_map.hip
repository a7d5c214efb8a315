// sas_map.hip -- one record per read on both strands (sas.h: sas_map_edit, sas_map_edit_fixed)
// and the reverse complement it needs (sas_revcomp, sas_revcomp_fixed).  Steps 1..3 are
// map_select_batch, declared in map_path.hpp and defined here with its kernels: sas_pairs.hip
// calls it too.
//
//   1. the batch      forward only: the caller's queries as they are.  Otherwise one scratch batch
//                     of the participating strands, forward as query i and reverse as query nq + i
//                     (reverse alone: query i): k_map_revcomp_fixed, or for ragged queries pool_scan
//                     over qlen, k_map_layout (offsets and lengths of the batch) and k_map_fill
//                     (output-centric over the batch's bytes: a workgroup owns a tile of output
//                     bytes and finds each one's query with al_tile_queries);
//   2. ed_prepare     the seed / verify / sort path of sas_edit.hip, once over that batch: the P
//                     sorted proposals, key = (batch query << ebits) | end, with their distances.
//                     Duplicates are adjacent; the first of a run of equal keys is the end itself;
//   3. k_map_select   output-centric over the sorted proposals, two passes.  A workgroup owns a
//                     tile of MAP_T consecutive proposals; the query of a proposal is in its key,
//                     and its left neighbour in the list tells whether it is a duplicate, the first
//                     end of its query or the first of an interval of consecutive ends, so the
//                     cost per proposal is the same whether 10^7 reads own one end each or one
//                     read owns 10^6.  Pass 1 reduces, per batch query, the minimum of
//                     dist << 56 | end and the number of interval starts; pass 2, with the read's
//                     least distance known from pass 1, the number of starts of intervals at that
//                     distance.  The reduction is segmented: inside the wave by shuffles, inside
//                     the tile by LDS atomics of one lane per (wave, segment) into the segment's
//                     slot (its rank in the tile, from a ballot scan of the segment heads).  A
//                     segment that lies inside the tile is then written with plain stores; only
//                     the (at most two) segments that cross a tile edge use 64-bit atomicMin /
//                     atomicAdd on the slots, which are initialised before the pass.  Integer min
//                     and add: the result does not depend on the order of arrival;
//   4. k_map_finalize one thread per read: the least (dist, strand, end) of the two strands'
//                     slots, the counts summed and clamped to 32 bits, the flags ORed, and the
//                     request of one alignment per read: off = 0 .. nq, the winner's bytes in the
//                     batch as a ragged query, length 0 (no alignment) for an unmapped read;
//   5. sas_align_edit over those nq alignments, chained on the stream.
#include "map_path.hpp"

#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

// Reverse complements of fixed-length queries: out[i m + j] = q[i m + m - 1 - j] ^ 3
__global__ void k_map_revcomp_fixed(const uint8_t* __restrict__ q, uint32_t m, uint64_t nq, uint8_t* __restrict__ out,
                                    uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    GRID_STRIDE(o, nq * (uint64_t)m) {
        const uint64_t i = o / m;
        const uint32_t j = (uint32_t)(o - i * m);
        const uint8_t c = q[i * m + (m - 1 - j)];
        b |= c;
        out[o] = c ^ 3u;
    }
    if (bad && (b & 0xFCu)) atomicOr(bad, 1u);
}

struct MapLenAt {  // qlen[i] as u64, 0 at and past nq (a scan over nq + 1 elements reads element nq)
    const uint32_t* qlen;
    uint64_t nq;
    __device__ __host__ uint64_t operator()(uint64_t i) const { return i < nq ? (uint64_t)qlen[i] : 0ull; }
};

// The ragged batch of `copies` copies of the queries back to back: scan = the exclusive sum of qlen
// (nq + 1 entries); boff has copies nq + 1 entries, blen copies nq
__global__ void k_map_layout(const uint64_t* __restrict__ scan, const uint32_t* __restrict__ qlen, uint64_t nq,
                             uint32_t copies, uint64_t* __restrict__ boff, uint32_t* __restrict__ blen) {
    const uint64_t total = scan[nq], nb = copies * nq;
    GRID_STRIDE(b, nb + 1) {
        const uint64_t c = b / nq, i = b - c * nq;
        boff[b] = c * total + scan[i];
        if (b < nb) blen[b] = qlen[i];
    }
}

// The bytes of a ragged batch: batch query b (b < nb, nb = nq or 2 nq) is query i = b mod nq, as it
// is for b < rev_from and reverse-complemented from there on.  boff: nb + 1 offsets into out
__global__ __launch_bounds__(AL_BLOCK) void k_map_fill(
    const uint8_t* __restrict__ q, const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qlen, uint64_t nq,
    const uint64_t* __restrict__ boff, uint64_t nb, uint64_t rev_from, uint8_t* __restrict__ out,
    uint32_t* __restrict__ bad) {
    __shared__ uint32_t rel[AL_SLICE];
    __shared__ uint64_t sh_p[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = boff[nb], ntiles = (total + AL_T - 1) / AL_T;
    uint32_t bits = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)AL_T;
        const uint64_t t1 = t0 + AL_T < total ? t0 + AL_T : total;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t qi[AL_PER];
        uint32_t ok[AL_PER];
        al_tile_queries(boff, nb, t0, n_el, rel, sh_p, qi, ok);
#pragma unroll
        for (int u = 0; u < AL_PER; u++) {
            if (!ok[u]) continue;
            const uint64_t o = t0 + u * AL_BLOCK + tid, b = qi[u];
            const uint64_t i = b >= nq ? b - nq : b;
            if (i >= nq) continue;
            const uint64_t j = o - boff[b];
            const uint32_t len = qlen[i];
            if (j >= len) continue;  // the offsets' own bounds
            const bool rev = b >= rev_from;
            const uint8_t c = q[qoff[i] + (rev ? len - 1 - j : j)];
            bits |= c;
            out[o] = rev ? (uint8_t)(c ^ 3u) : c;
        }
        __syncthreads();  // rel and sh_p are rewritten by the next tile
    }
    if (bad && (bits & 0xFCu)) atomicOr(bad, 1u);
}

template <int PASS>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_select(MapSel a) {
    __shared__ uint64_t s_min[MAP_T];  // per segment of the tile (a run of proposals of one query)
    __shared__ uint64_t s_q[MAP_T];
    __shared__ uint32_t s_cnt[MAP_T];
    __shared__ uint32_t s_heads[MAP_CHUNKS], s_pre[MAP_CHUNKS + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t P = a.P, ntiles = (P + MAP_T - 1) / MAP_T;
    const uint64_t emask = (1ull << a.ebits) - 1ull;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MAP_T;
        const uint64_t t1 = t0 + MAP_T < P ? t0 + MAP_T : P;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        for (uint32_t x = tid; x < MAP_T; x += MAP_BLOCK) {
            s_min[x] = MAP_NONE;
            s_cnt[x] = 0;
        }
        uint64_t qb[MAP_PER], mn[MAP_PER], heads[MAP_PER];
        uint32_t ct[MAP_PER];
        bool valid[MAP_PER], head[MAP_PER];
#pragma unroll
        for (int u = 0; u < MAP_PER; u++) {
            const uint32_t el = u * MAP_BLOCK + tid;
            const uint64_t p = t0 + el;
            valid[u] = el < n_el;
            qb[u] = 0;
            mn[u] = MAP_NONE;
            ct[u] = 0;
            head[u] = false;
            if (valid[u]) {
                const uint64_t key = a.keys[p], prev = p ? a.keys[p - 1] : 0;
                const uint32_t d = a.vals[p], pd = p ? a.vals[p - 1] : 0u;
                const uint64_t b = key >> a.ebits;
                const bool sameq = p != 0 && (prev >> a.ebits) == b;  // the left neighbour is of this query
                const bool uniq = p == 0 || prev != key;              // not a duplicate: an end of the answer
                const bool follows = sameq && prev + 1 == key;        // the end before it is in the answer too
                qb[u] = b;
                head[u] = el == 0 || !sameq;
                if (PASS == 1) {
                    if (uniq) mn[u] = ((uint64_t)d << 56) | (key & emask);
                    ct[u] = uniq && !follows ? 1u : 0u;
                } else {
                    const uint64_t o = a.nb == a.nq ? b : (b >= a.nq ? b - a.nq : b + a.nq);
                    const uint64_t k0 = b < a.nb ? a.kmin[b] : MAP_NONE, k1 = o < a.nb ? a.kmin[o] : MAP_NONE;
                    const uint32_t best = (uint32_t)((k0 < k1 ? k0 : k1) >> 56);
                    ct[u] = uniq && d == best && !(follows && pd == d) ? 1u : 0u;
                }
            }
            heads[u] = __ballot(head[u]);
            if (lane == 0) s_heads[u * 4 + wave] = (uint32_t)__popcll(heads[u]);
        }
        __syncthreads();
        if (tid < MAP_CHUNKS) {  // exclusive scan of the chunks' head counts (half of wave 0)
            const uint32_t v = s_heads[tid];
            uint32_t inc = v;
#pragma unroll
            for (int off = 1; off < MAP_CHUNKS; off <<= 1) {
                const uint32_t o = __shfl_up(inc, off);
                if ((int)tid >= off) inc += o;
            }
            s_pre[tid] = inc - v;
            if (tid == MAP_CHUNKS - 1) s_pre[MAP_CHUNKS] = inc;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAP_PER; u++) {
            // the segment's rank in the tile: heads before and at this element, less one
            const uint32_t sg = valid[u] ? s_pre[u * 4 + wave] + (uint32_t)__popcll(heads[u] & ((2ull << lane) - 1ull)) - 1u
                                         : 0xFFFFFFFFu;
            uint64_t m1 = mn[u];
            uint32_t c1 = ct[u];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {  // segmented inclusive scan of the wave's 64 proposals
                const uint64_t mo = __shfl_up(m1, off);
                const uint32_t co = __shfl_up(c1, off), so = __shfl_up(sg, off);
                if ((int)lane >= off && so == sg) {
                    m1 = mo < m1 ? mo : m1;
                    c1 += co;
                }
            }
            const uint32_t nx = __shfl_down(sg, 1);
            if (valid[u] && sg < MAP_T) {
                if (head[u]) s_q[sg] = qb[u];
                if (lane == 63 || nx != sg) {  // the last of its segment in this wave
                    if (PASS == 1 && m1 != MAP_NONE) atomicMin((unsigned long long*)&s_min[sg], (unsigned long long)m1);
                    if (c1) atomicAdd(&s_cnt[sg], c1);
                }
            }
        }
        __syncthreads();
        const uint32_t nseg = s_pre[MAP_CHUNKS];  // <= n_el
        for (uint32_t sgi = tid; sgi < nseg && sgi < MAP_T; sgi += MAP_BLOCK) {
            const uint64_t b = s_q[sgi];
            if (b >= a.nb) continue;
            // a segment that goes on in a neighbouring tile shares its slot with that tile
            const bool open = (sgi == 0 && t0 > 0 && (a.keys[t0 - 1] >> a.ebits) == b) ||
                              (sgi == nseg - 1 && t1 < P && (a.keys[t1] >> a.ebits) == b);
            const uint64_t m1 = s_min[sgi], c1 = s_cnt[sgi];
            if (PASS == 1) {
                if (!open) {
                    a.kmin[b] = m1;
                    a.nloci[b] = c1;
                } else {
                    if (m1 != MAP_NONE) atomicMin((unsigned long long*)&a.kmin[b], (unsigned long long)m1);
                    if (c1) atomicAdd((unsigned long long*)&a.nloci[b], (unsigned long long)c1);
                }
            } else {
                if (!open) a.nbest[b] = c1;
                else if (c1) atomicAdd((unsigned long long*)&a.nbest[b], (unsigned long long)c1);
            }
        }
        __syncthreads();  // the segment slots are reset by the next tile
    }
}

// Steps 1..3 (map_path.hpp).  All arrays on the device; Q: the caller's queries
int map_select_batch(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t strands,
                     hipStream_t st, uint32_t flags, MapState& ms) {
    const uint64_t nq = Q.nq;
    const uint32_t copies = strands == (SAS_MAP_FWD | SAS_MAP_REV) ? 2u : 1u;
    const uint64_t nb = copies * nq;
    ms.nb = nb;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    const unsigned cap_grid = (unsigned)x->num_cus * 8;
    // 1. the batch
    MmQueries& B = ms.B;
    B = Q;
    if (strands != SAS_MAP_FWD) {
        B.nq = nb;
        if (Q.qoff) {
            TRY(ms.bscan.alloc(pool, (nq + 1) * 8, st));
            TRY(pool_scan(pool, st,
                        rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0),
                                                         MapLenAt{Q.qlen, nq}),
                        ms.bscan.as<uint64_t>(), nq + 1));
            // ragged queries and a reverse strand: the batch's bytes are sized from their total
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, ms.bscan.as<uint64_t>() + nq, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            TRY(ms.bbytes.alloc(pool, copies * total + 64, st));
            TRY(ms.boff.alloc(pool, (nb + 1) * 8, st));
            TRY(ms.blen.alloc(pool, nb * 4, st));
            hipLaunchKernelGGL(k_map_layout, seed_grid(x, nb + 1), dim3(256), 0, st, ms.bscan.as<uint64_t>(), Q.qlen,
                               nq, copies, ms.boff.as<uint64_t>(), ms.blen.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            const uint64_t tiles = (copies * total + AL_T - 1) / AL_T;
            if (tiles) {
                const dim3 fgrid((unsigned)tile_grid(std::min<uint64_t>(tiles, cap_grid)));
                hipLaunchKernelGGL(k_map_fill, fgrid, dim3(AL_BLOCK), 0, st, Q.qbytes, Q.qoff, Q.qlen, nq,
                                   ms.boff.as<uint64_t>(), nb, copies == 2 ? nq : 0, ms.bbytes.as<uint8_t>(),
                                   (uint32_t*)nullptr);
                HIP_TRY(hipGetLastError());
            }
            B.qbytes = ms.bbytes.as<uint8_t>();
            B.qoff = ms.boff.as<uint64_t>();
            B.qlen = ms.blen.as<uint32_t>();
        } else {
            const uint64_t span = nq * (uint64_t)Q.m;
            TRY(ms.bbytes.alloc(pool, copies * span + 64, st));
            uint8_t* rev = ms.bbytes.as<uint8_t>() + (copies == 2 ? span : 0);
            if (copies == 2 && span)
                HIP_TRY(hipMemcpyAsync(ms.bbytes.p, Q.qbytes, span, hipMemcpyDeviceToDevice, st));
            if (span) {
                hipLaunchKernelGGL(k_map_revcomp_fixed, seed_grid(x, span), dim3(256), 0, st, Q.qbytes, Q.m, nq, rev,
                                   (uint32_t*)nullptr);
                HIP_TRY(hipGetLastError());
            }
            B.qbytes = ms.bbytes.as<uint8_t>();
        }
    }
    // 2. the ends of every batch query, as sorted proposals
    EdState& s = ms.s;
    TRY(ms.eoff.alloc(pool, (nb + 1) * 8, st));
    TRY(ms.efl.alloc(pool, nb, st));
    TRY(ed_prepare(x, B, k, max_seed_hits, ms.eoff.as<uint64_t>(), ms.efl.as<uint8_t>(), nullptr, st, flags, s));
    // 3. select
    TRY(ms.slots.alloc(pool, 3 * nb * 8, st));
    HIP_TRY(hipMemsetAsync(ms.slots.p, 0xFF, nb * 8, st));
    HIP_TRY(hipMemsetAsync(ms.slots.as<uint64_t>() + nb, 0, 2 * nb * 8, st));
    ms.kmin = ms.slots.as<uint64_t>();
    ms.nloci = ms.kmin + nb;
    ms.nbest = ms.kmin + 2 * nb;
    if (s.P) {
        MapSel a{};
        a.keys = s.skeys;
        a.vals = s.svals;
        a.P = s.P;
        a.ebits = s.ebits;
        a.nq = nq;
        a.nb = nb;
        a.kmin = ms.kmin;
        a.nloci = ms.nloci;
        a.nbest = ms.nbest;
        const uint64_t tiles = (s.P + MAP_T - 1) / MAP_T;
        const dim3 sgrid((unsigned)tile_grid(std::min<uint64_t>(tiles, (uint64_t)x->num_cus * MAP_BPC)));
        hipLaunchKernelGGL(k_map_select<1>, sgrid, dim3(MAP_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_map_select<2>, sgrid, dim3(MAP_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

struct MapFin {
    MmQueries B;            // the batch
    uint64_t nq, n;
    uint32_t strands;
    const uint64_t* kmin;
    const uint64_t* nloci;
    const uint64_t* nbest;
    const uint8_t* efl;     // the batch queries' SAS_ED_* flags
    void* out_end;
    uint8_t* out_dist;
    uint8_t* out_strand;    // may be null, as the three below
    uint32_t* out_nbest;
    uint32_t* out_nloci;
    uint8_t* out_qflags;
    uint64_t* aoff;         // the alignment request: nq + 1 offsets 0 .. nq,
    uint64_t* aqoff;        // the winner's bytes in the batch
    uint32_t* aqlen;        // and their length (0: no alignment)
};

template <bool U32>
__global__ void k_map_finalize(MapFin a) {
    const uint32_t copies = a.strands == (SAS_MAP_FWD | SAS_MAP_REV) ? 2u : 1u;
    GRID_STRIDE(i, a.nq + 1) {
        a.aoff[i] = i;
        if (i == a.nq) continue;
        const MapBest r = map_best_of(i, a.nq, copies, a.strands, a.kmin, a.nloci, a.nbest, a.efl);
        const uint64_t best = r.best;
        const bool mapped = best != MAP_NONE;
        const uint64_t e = mapped ? best & ((1ull << 55) - 1ull) : a.n;
        if (U32) static_cast<uint32_t*>(a.out_end)[i] = (uint32_t)e;
        else static_cast<uint64_t*>(a.out_end)[i] = e;
        a.out_dist[i] = mapped ? (uint8_t)(best >> 56) : (uint8_t)SAS_AL_NONE_DIST;
        if (a.out_strand) a.out_strand[i] = mapped ? (uint8_t)((best >> 55) & 1ull) : 0;
        if (a.out_nbest) a.out_nbest[i] = map_clamp32(r.nbst);
        if (a.out_nloci) a.out_nloci[i] = map_clamp32(r.nl);
        if (a.out_qflags) a.out_qflags[i] = (uint8_t)r.fl;
        a.aqoff[i] = a.B.off(r.bb);
        a.aqlen[i] = mapped ? a.B.len(r.bb) : 0u;
    }
}

int twin_reads(HostOutputs& ho, const ReadOut& host, uint64_t nq, uint64_t esz, uint64_t stride, const char* label,
               ReadOut* dev) {
    const std::string l(label);
    TRY(ho.twin(host.end, nq * esz, (l + " ends").c_str(), &dev->end));
    TRY(ho.twin(host.dist, nq, (l + " distances").c_str(), &dev->dist));
    TRY(ho.twin(host.start, nq * esz, (l + " starts").c_str(), &dev->start));
    TRY(ho.twin(host.strand, nq, (l + " strands").c_str(), &dev->strand));
    TRY(ho.twin(host.nbest, nq * 4, (l + " best counts").c_str(), &dev->nbest));
    TRY(ho.twin(host.nloci, nq * 4, (l + " locus counts").c_str(), &dev->nloci));
    TRY(ho.twin(host.nruns, nq, (l + " run counts").c_str(), &dev->nruns));
    TRY(ho.twin(host.runs, nq * stride * 2, (l + " runs").c_str(), &dev->runs));
    TRY(ho.twin(host.qflags, nq, (l + " query flags").c_str(), &dev->qflags));
    return 0;
}

// All arrays on the device; Q: the caller's queries
static int map_device(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t strands,
                      const ReadOut& o, hipStream_t st, uint32_t flags) {
    const uint64_t nq = Q.nq;
    // 1..3. the batch, its sorted proposals, the slots
    MapState ms;
    TRY(map_select_batch(x, Q, k, max_seed_hits, strands, st, flags, ms));
    // 4. the records and the alignment request
    AlignReq areq;
    TRY(areq.alloc(x, nq, o.start, flags, st));
    MapFin f{};
    f.B = ms.B;
    f.nq = nq;
    f.n = x->n;
    f.strands = strands;
    f.kmin = ms.kmin;
    f.nloci = ms.nloci;
    f.nbest = ms.nbest;
    f.efl = ms.efl.as<uint8_t>();
    f.out_end = o.end;
    f.out_dist = o.dist;
    f.out_strand = o.strand;
    f.out_nbest = o.nbest;
    f.out_nloci = o.nloci;
    f.out_qflags = o.qflags;
    f.aoff = areq.aoff;
    f.aqoff = areq.aqoff;
    f.aqlen = areq.aqlen;
    with_bool(flags & SAS_LOCATE_U32, [&](auto U32) {
        hipLaunchKernelGGL(k_map_finalize<decltype(U32)::value>, seed_grid(x, nq + 1), dim3(256), 0, st, f);
    });
    HIP_TRY(hipGetLastError());
    // 5. one alignment per read
    return align_winners(x, ms.B, areq, nq, k, o, st, flags);
}

static int map_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint32_t k,
                    uint64_t max_seed_hits, uint32_t strands, const ReadOut& o, void* stream, uint32_t flags) {
    const std::string w(fn);
    if (strands == 0 || strands > (SAS_MAP_FWD | SAS_MAP_REV))
        SAS_FAIL(EINVAL, w + ": strands must be SAS_MAP_FWD, SAS_MAP_REV or both");
    TRY(seed_index_checks(w, x, k, flags, stream));
    // the (batch query, end) sort key of both strands
    if (ed_bits(x->n) + (nq ? ed_bits(2 * nq - 1) : 0) > 64)
        SAS_FAIL(EINVAL, w + ": " + std::to_string(nq) + " reads on two strands and a text of " + std::to_string(x->n) +
                             " chars do not fit the 64-bit (query, end) sort key: split the batch");
    if (nq == 0) return 0;
    if (!q.null_ok(nq) || !o.end || !o.dist) SAS_FAIL(EINVAL, w + ": null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & SAS_DEVICE_PTRS) return map_device(x, q.device(nq), k, max_seed_hits, strands, o, st, flags);
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated)
    HostQueries hq;
    HostOutputs ho;
    MmQueries Q;
    ReadOut d{};
    TRY(hq.stage("map", q, nq, st, &Q));
    TRY(twin_reads(ho, o, nq, (flags & SAS_LOCATE_U32) ? 4 : 8, 2 * (uint64_t)k + 1, "map", &d));
    TRY(map_device(x, Q, k, max_seed_hits, strands, d, st, flags | SAS_VALIDATE));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_map_edit(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                            uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint32_t strands, void* out_end,
                            void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                            uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                            void* stream, uint32_t flags) {
    const ReadOut o{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags};
    return map_impl("sas_map_edit", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, k, max_seed_hits, strands, o, stream,
                    flags);
}

extern "C" int sas_map_edit_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                                  uint64_t max_seed_hits, uint32_t strands, void* out_end, void* out_start,
                                  uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci,
                                  uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags, void* stream,
                                  uint32_t flags) {
    const ReadOut o{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags};
    return map_impl("sas_map_edit_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, k, max_seed_hits,
                    strands, o, stream, flags);
}

// Device arrays, on the current device (the call takes no index): scratch from its default pool
static int revcomp_device(const char* fn, const uint8_t* q, const uint64_t* qoff, const uint32_t* qlen, uint32_t m,
                          uint64_t nq, uint8_t* out, uint64_t* out_off, hipStream_t st, bool validate) {
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const unsigned cap_grid = (unsigned)std::max(cus, 1) * 8;
    BadFlag bflag;  // armed when it is read back
    if (validate) TRY(bflag.arm(st));
    if (qoff) {
        hipMemPool_t pool;
        HIP_TRY(hipDeviceGetDefaultMemPool(&pool, dev));
        TRY(pool_scan(pool, st,
                    rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), MapLenAt{qlen, nq}),
                    out_off, nq + 1));
        // the grid does not wait for the byte total: the tiles are strided over it
        hipLaunchKernelGGL(k_map_fill, dim3(tile_grid(cap_grid)), dim3(AL_BLOCK), 0, st, q, qoff, qlen,
                           nq, out_off, nq, (uint64_t)0, out, bflag.ptr());
    } else {
        hipLaunchKernelGGL(k_map_revcomp_fixed, dim3(tile_grid(std::min(grid_for(nq * (uint64_t)m), cap_grid))),
                           dim3(256), 0, st, q, m, nq, out, bflag.ptr());
    }
    HIP_TRY(hipGetLastError());
    if (validate) {
        uint32_t hbad = 0;
        TRY(bflag.read(st, &hbad));
        if (hbad) SAS_FAIL(EINVAL, std::string(fn) + ": query bytes must be DNA codes 0..3");
    }
    return 0;
}

static int revcomp_impl(const char* fn, const QueryArgs& q, uint64_t nq, uint8_t* out_bytes, uint64_t* out_off,
                        void* stream, uint32_t flags) {
    const std::string w(fn);
    const uint8_t* qbytes = q.qbytes;
    const bool ragged = q.ragged;
    const bool dev = (flags & SAS_DEVICE_PTRS) != 0;
    if (ragged && !out_off) SAS_FAIL(EINVAL, w + ": null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq == 0) {
        if (ragged) {
            if (dev) HIP_TRY(hipMemsetAsync(out_off, 0, 8, st));
            else out_off[0] = 0;
        }
        return 0;
    }
    if (ragged && (!q.qoff || !q.qlen)) SAS_FAIL(EINVAL, w + ": null argument");
    if (dev) {
        if (!qbytes || !out_bytes) SAS_FAIL(EINVAL, w + ": null argument");
        return revcomp_device(fn, qbytes, ragged ? q.qoff : nullptr, q.qlen, q.m, nq, out_bytes, out_off, st,
                              (flags & SAS_VALIDATE) != 0);
    }
    // host arrays: copy in, the kernel, copy out (synchronous; bytes always validated)
    uint64_t total = nq * (uint64_t)q.m;
    if (ragged) {
        total = 0;
        for (uint64_t i = 0; i < nq; i++) total += q.qlen[i];
    }
    if (total && (!qbytes || !out_bytes)) SAS_FAIL(EINVAL, w + ": null argument");
    HostQueries hq;
    HostOutputs ho;
    MmQueries Q;
    TRY(hq.stage("revcomp", q, nq, st, &Q));
    uint8_t* dout;
    uint64_t* doff;
    TRY(ho.twin(out_bytes, total, "revcomp output", &dout));  // may be null when there is no byte to write
    TRY(ho.twin(out_off, (nq + 1) * 8, "revcomp offsets", &doff));
    TRY(revcomp_device(fn, Q.qbytes, Q.qoff, Q.qlen, q.m, nq, dout, doff, st, true));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_revcomp(const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
                           uint8_t* out_bytes, uint64_t* out_off, void* stream, uint32_t flags) {
    return revcomp_impl("sas_revcomp", QueryArgs{qbytes, qoff, qlen, 0, true}, nq, out_bytes, out_off, stream, flags);
}

extern "C" int sas_revcomp_fixed(const uint8_t* qbytes, uint32_t m, uint64_t nq, uint8_t* out_bytes, void* stream,
                                 uint32_t flags) {
    return revcomp_impl("sas_revcomp_fixed", QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, out_bytes, nullptr,
                        stream, flags);
}
