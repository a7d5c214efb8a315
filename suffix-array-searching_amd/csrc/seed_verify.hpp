// seed_verify.hpp -- what the seed-and-verify calls share (sas_mismatch.hip: Hamming distance,
// sas_edit.hip: edit distance): the query batch as the kernels see it, the cut of a query into
// k + 1 pieces, the output-centric tiling of the candidates (one candidate = one occurrence of
// one piece) and of the elements of a CSR list (sas_align.hip: alignments, sas_map.hip: the bytes
// of a ragged batch), stream-ordered scratch and a scan helper.
#pragma once
#include "build_util.hpp"

#include <rocprim/device/device_scan.hpp>

#define MM_BLOCK 256
#define MM_T 2048          // candidates per tile
#define MM_PER (MM_T / MM_BLOCK)
#define MM_SLICE 4096      // candidate offsets of a tile staged in LDS (16 KiB)
#define MM_MAX_GRID (1u << 20)
#define MM_MAX_K 15

struct MmQueries {
    const uint8_t* qbytes;
    const uint64_t* qoff;  // null: fixed-length queries of m chars
    const uint32_t* qlen;
    uint32_t m;
    uint64_t nq;
    __device__ __forceinline__ uint64_t off(uint64_t q) const { return qoff ? qoff[q] : q * (uint64_t)m; }
    __device__ __forceinline__ uint32_t len(uint64_t q) const { return qoff ? qlen[q] : m; }
};

// b_j: the first char of piece j of a query of m chars cut into kp1 pieces
__device__ __forceinline__ uint32_t mm_piece_start(uint32_t j, uint32_t m, uint32_t kp1) {
    return (uint32_t)(((uint64_t)j * m) / kp1);
}

[[maybe_unused]] static __global__ void k_mm_pieces(MmQueries Q, uint32_t kp1, uint64_t* __restrict__ poff,
                                   uint32_t* __restrict__ plen) {
    GRID_STRIDE(i, Q.nq * kp1) {
        const uint64_t q = i / kp1;
        const uint32_t j = (uint32_t)(i - q * kp1), m = Q.len(q);
        const uint32_t b0 = mm_piece_start(j, m, kp1), b1 = mm_piece_start(j + 1, m, kp1);
        poff[i] = Q.off(q) + b0;
        plen[i] = b1 - b0;
    }
}

// the last i in [0, np] with off[i] <= v (off[0] = 0): for v below the total a non-empty piece
__device__ __forceinline__ uint64_t mm_piece_of(const uint64_t* __restrict__ off, uint64_t np, uint64_t v) {
    uint64_t l = 0, h = np + 1;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (off[mid] <= v) l = mid + 1;
        else h = mid;
    }
    return l ? l - 1 : 0;
}

// The candidates [t0, t0 + n_el) of one tile (n_el <= MM_T), for the whole workgroup of MM_BLOCK
// threads: element e = u MM_BLOCK + tid is occurrence c - coff[pi] of piece pi[u] (found by
// bisecting the tile's slice of the candidate offsets, staged in `rel` when it fits) and lies
// at text position pv[u] = SA[lo[pi] + c - coff[pi]]; ok[u] = 0 for an element past the tile or
// one that fails the offsets' own bounds.  All SA reads of a thread are issued before the
// first is used.  `rel` (MM_SLICE words) and `sh_p` (2 words) are LDS; the caller puts a
// __syncthreads() between two tiles.
template <class SA>
__device__ __forceinline__ void mm_tile_candidates(const SA& sa, const uint64_t* __restrict__ coff,
                                                   const uint64_t* __restrict__ lo, uint64_t np, uint64_t n,
                                                   uint64_t t0, uint32_t n_el, uint32_t* rel, uint64_t* sh_p,
                                                   uint64_t (&pi)[MM_PER], uint64_t (&pv)[MM_PER],
                                                   uint32_t (&ok)[MM_PER]) {
    const uint32_t tid = threadIdx.x;
    // the pieces of the tile's first and last candidate (both non-empty)
    if (tid < 2) sh_p[tid] = mm_piece_of(coff, np, tid ? t0 + n_el - 1 : t0);
    __syncthreads();
    const uint64_t p0 = sh_p[0];
    uint64_t p1 = sh_p[1];
    if (p1 < p0) p1 = p0;
    if (p1 > np - 1) p1 = np - 1;
    const uint64_t nps = p1 - p0 + 1;
    const uint32_t staged = nps <= MM_SLICE ? 1u : 0u;
    if (staged) {
        for (uint32_t x = tid; x < (uint32_t)nps; x += MM_BLOCK) {
            const uint64_t o = coff[p0 + x];
            rel[x] = o <= t0 ? 0u : (o - t0 >= MM_T ? (uint32_t)MM_T : (uint32_t)(o - t0));
        }
        __syncthreads();
    }
    // element e of the tile belongs to the last piece x in [p0, p1] with coff[x] <= t0 + e
    uint64_t rk[MM_PER];
#pragma unroll
    for (int u = 0; u < MM_PER; u++) {
        const uint32_t e = u * MM_BLOCK + tid;
        const uint64_t c = t0 + e;
        ok[u] = e < n_el ? 1u : 0u;
        pi[u] = rk[u] = 0;
        if (ok[u]) {
            uint64_t l = 1, h = nps;
            if (staged) {
                while (l < h) {
                    const uint64_t mid = (l + h) >> 1;
                    if (rel[mid] <= e) l = mid + 1;
                    else h = mid;
                }
            } else {
                while (l < h) {
                    const uint64_t mid = (l + h) >> 1;
                    if (coff[p0 + mid] <= c) l = mid + 1;
                    else h = mid;
                }
            }
            pi[u] = p0 + l - 1;
            const uint64_t o = coff[pi[u]];
            rk[u] = lo[pi[u]] + (c - o);
            ok[u] = (o <= c && c < coff[pi[u] + 1] && rk[u] < n) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int u = 0; u < MM_PER; u++) pv[u] = ok[u] ? sa[rk[u]] : 0;
}

#define AL_BLOCK 256
#define AL_T 1024           // elements per tile
#define AL_PER (AL_T / AL_BLOCK)
#define AL_SLICE 2048       // query offsets of a tile staged in LDS (8 KiB)

// The queries of the elements [t0, t0 + n_el) of one tile of a CSR list (n_el <= AL_T; off: its
// nq + 1 offsets), for the whole workgroup of AL_BLOCK threads: element e = u AL_BLOCK + tid
// belongs to the last query qi[u] with off[qi] <= t0 + e (bisecting the tile's slice of `off`,
// staged in `rel` when it fits); ok[u] = 0 for an element past the tile or one that fails the
// offsets' own bounds.  The caller puts a __syncthreads() between two tiles.
__device__ __forceinline__ void al_tile_queries(const uint64_t* __restrict__ off, uint64_t nq, uint64_t t0,
                                                uint32_t n_el, uint32_t* rel, uint64_t* sh_p, uint64_t (&qi)[AL_PER],
                                                uint32_t (&ok)[AL_PER]) {
    const uint32_t tid = threadIdx.x;
    // the queries of the tile's first and last element (both non-empty)
    if (tid < 2) sh_p[tid] = mm_piece_of(off, nq, tid ? t0 + n_el - 1 : t0);
    __syncthreads();
    const uint64_t p0 = sh_p[0];
    uint64_t p1 = sh_p[1];
    if (p1 < p0) p1 = p0;
    if (p1 > nq - 1) p1 = nq - 1;
    const uint64_t nps = p1 - p0 + 1;
    const uint32_t staged = nps <= AL_SLICE ? 1u : 0u;
    if (staged) {
        for (uint32_t x = tid; x < (uint32_t)nps; x += AL_BLOCK) {
            const uint64_t o = off[p0 + x];
            rel[x] = o <= t0 ? 0u : (o - t0 >= AL_T ? (uint32_t)AL_T : (uint32_t)(o - t0));
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < AL_PER; u++) {
        const uint32_t e = u * AL_BLOCK + tid;
        const uint64_t c = t0 + e;
        ok[u] = e < n_el ? 1u : 0u;
        qi[u] = 0;
        if (ok[u]) {
            uint64_t l = 1, h = nps;
            if (staged) {
                while (l < h) {
                    const uint64_t mid = (l + h) >> 1;
                    if (rel[mid] <= e) l = mid + 1;
                    else h = mid;
                }
            } else {
                while (l < h) {
                    const uint64_t mid = (l + h) >> 1;
                    if (off[p0 + mid] <= c) l = mid + 1;
                    else h = mid;
                }
            }
            qi[u] = p0 + l - 1;
            ok[u] = (off[qi[u]] <= c && c < off[qi[u] + 1]) ? 1u : 0u;
        }
    }
}

struct MmPoolBuf {  // stream-ordered scratch from the index's pool
    void* p = nullptr;
    hipStream_t st = nullptr;
    ~MmPoolBuf() { if (p) (void)hipFreeAsync(p, st); }
    template <class T> T* as() { return static_cast<T*>(p); }
    int alloc(hipMemPool_t pool, size_t bytes, hipStream_t s) {
        st = s;
        HIP_TRY(hipMallocFromPoolAsync(&p, bytes ? bytes : 8, pool, s));
        return 0;
    }
};

// out[i] = sum of in[0 .. i) over `count` elements of an iterator of u64 (out may be in)
template <class In>
static int mm_scan(hipMemPool_t pool, hipStream_t st, In in, uint64_t* out, uint64_t count) {
    size_t tbytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tbytes, in, out, (uint64_t)0, (size_t)count, rocprim::plus<uint64_t>(),
                                    st));
    MmPoolBuf tmp;
    TRY(tmp.alloc(pool, tbytes, st));
    HIP_TRY(rocprim::exclusive_scan(tmp.p, tbytes, in, out, (uint64_t)0, (size_t)count, rocprim::plus<uint64_t>(),
                                    st));
    return 0;
}
