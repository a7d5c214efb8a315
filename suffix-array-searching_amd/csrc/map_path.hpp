// map_path.hpp -- what the read-mapping calls share (sas_map.hip: sas_map_edit, one record per
// read; sas_pairs.hip: sas_map_pairs, the fragment-length join of two mates): the batch of both
// strands, the seed / verify / sort path over it, the per-(read, strand) slots of the
// output-centric select, the single-read winner of the two strands' slots, and the segmented
// reduction of a tile that the kernels over sorted lists are built from.
#pragma once
#include "edit_path.hpp"

#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>

#define MAP_BLOCK 256
#define MAP_T 2048                    // proposals per tile
#define MAP_PER (MAP_T / MAP_BLOCK)
#define MAP_CHUNKS (MAP_T / 64)       // (wave, round) pairs of a tile: 64 consecutive proposals each
#define MAP_BPC 4                     // workgroups per CU that size the grids
#define MAP_NONE (~0ull)

static_assert(MAP_CHUNKS == 32, "the chunk scan is one shuffle scan over 32 lanes");

// Reverse complements of fixed-length queries: out[i m + j] = q[i m + m - 1 - j] ^ 3
[[maybe_unused]] static __global__ void k_map_revcomp_fixed(const uint8_t* __restrict__ q, uint32_t m, uint64_t nq,
                                                            uint8_t* __restrict__ out, uint32_t* __restrict__ bad) {
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
[[maybe_unused]] static __global__ void k_map_layout(const uint64_t* __restrict__ scan,
                                                     const uint32_t* __restrict__ qlen, uint64_t nq, uint32_t copies,
                                                     uint64_t* __restrict__ boff, uint32_t* __restrict__ blen) {
    const uint64_t total = scan[nq], nb = copies * nq;
    GRID_STRIDE(b, nb + 1) {
        const uint64_t c = b / nq, i = b - c * nq;
        boff[b] = c * total + scan[i];
        if (b < nb) blen[b] = qlen[i];
    }
}

// The bytes of a ragged batch: batch query b (b < nb, nb = nq or 2 nq) is query i = b mod nq, as it
// is for b < rev_from and reverse-complemented from there on.  boff: nb + 1 offsets into out
[[maybe_unused]] static __global__ __launch_bounds__(AL_BLOCK) void k_map_fill(
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

struct MapSel {
    const uint64_t* keys;   // P sorted proposals, (batch query << ebits) | end
    const uint8_t* vals;    // their distances
    uint64_t P;
    uint32_t ebits;
    uint64_t nq, nb;        // reads; batch queries (nq, or 2 nq: the strands of read i are i and nq + i)
    uint64_t* kmin;         // per batch query: the least dist << 56 | end (MAP_NONE before pass 1)
    uint64_t* nloci;        // per batch query: intervals of consecutive ends (0 before pass 1)
    uint64_t* nbest;        // per batch query: those at the read's least distance (0 before pass 2)
};

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

// The single-read record of read i from the slots of its `copies` strands (batch queries
// c nq + i): the least (dist, strand, end), the counts summed and the flags ORed
struct MapBest {
    uint64_t best;  // dist << 56 | strand << 55 | end (an end has at most 41 bits); MAP_NONE: unmapped
    uint64_t bb;    // the winner's batch query
    uint64_t nl, nbst;
    uint32_t fl;
};

__device__ __forceinline__ MapBest map_best_of(uint64_t i, uint64_t nq, uint32_t copies, uint32_t strands,
                                               const uint64_t* __restrict__ kmin, const uint64_t* __restrict__ nloci,
                                               const uint64_t* __restrict__ nbest, const uint8_t* __restrict__ efl) {
    MapBest r{MAP_NONE, i, 0, 0, 0};
    for (uint32_t c = 0; c < copies; c++) {
        const uint64_t b = c * nq + i;
        const uint64_t strand = copies == 2 ? c : (strands == SAS_MAP_REV ? 1u : 0u);
        const uint64_t km = kmin[b];
        r.fl |= efl[b];
        r.nl += nloci[b];
        r.nbst += nbest[b];
        if (km != MAP_NONE) {
            const uint64_t key = km | (strand << 55);
            if (key < r.best) {
                r.best = key;
                r.bb = b;
            }
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t map_clamp32(uint64_t v) {
    return (uint32_t)(v < 0xFFFFFFFFull ? v : 0xFFFFFFFFull);
}

// Steps 1..3 of sas_map.hip: the batch of the participating strands, its sorted proposals and
// the slots of the two select passes.  The scratch lives as long as the state
struct MapState {
    MmQueries B;                // the batch: nb = copies nq queries
    uint64_t nb = 0;
    MmPoolBuf bbytes, bscan, boff, blen, eoff, efl, slots;
    EdState s;
    uint64_t* kmin = nullptr;   // nb each
    uint64_t* nloci = nullptr;
    uint64_t* nbest = nullptr;
};

// All arrays on the device; Q: the caller's queries
[[maybe_unused]] static int map_select_batch(const sas_index* x, const MmQueries& Q, uint32_t k,
                                             uint64_t max_seed_hits, uint32_t strands, hipStream_t st, uint32_t flags,
                                             MapState& ms) {
    const uint64_t nq = Q.nq;
    const uint32_t copies = strands == (SAS_MAP_FWD | SAS_MAP_REV) ? 2u : 1u;
    const uint64_t nb = copies * nq;
    ms.nb = nb;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    const unsigned cap_grid = (unsigned)x->num_cus * 8;
    const auto grid = [&](uint64_t count) { return dim3(tile_grid(std::min(grid_for(count), cap_grid))); };
    // 1. the batch
    MmQueries& B = ms.B;
    B = Q;
    if (strands != SAS_MAP_FWD) {
        B.nq = nb;
        if (Q.qoff) {
            TRY(ms.bscan.alloc(pool, (nq + 1) * 8, st));
            TRY(mm_scan(pool, st,
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
            hipLaunchKernelGGL(k_map_layout, grid(nb + 1), dim3(256), 0, st, ms.bscan.as<uint64_t>(), Q.qlen, nq,
                               copies, ms.boff.as<uint64_t>(), ms.blen.as<uint32_t>());
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
                hipLaunchKernelGGL(k_map_revcomp_fixed, grid(span), dim3(256), 0, st, Q.qbytes, Q.m, nq, rev,
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
