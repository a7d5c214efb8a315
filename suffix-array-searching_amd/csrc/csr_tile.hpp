// csr_tile.hpp -- who owns element v of a CSR list: the one bisect behind every output-centric
// tiled kernel (k_mm_verify, k_ed_verify, k_al_align, k_map_fill; k_locate_tiles and
// k_locate_fill's unpartitioned path use the scalar alone).  `off` holds n + 1 ascending offsets
// with off[0] = 0; owner i owns the elements [off[i], off[i + 1]), so among equal offsets the
// last is the non-empty owner and runs of empty owners are skipped by the bisection itself.
//
// The scalar pieces are __host__ __device__ so that tests/cpp/csr_tile_check.cpp drives the very
// code the kernels run; the workgroup routine on top of them is device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the last i in [0, n] with off[i] <= v: for v below the total a non-empty owner, n from there on
__host__ __device__ __forceinline__ uint64_t csr_owner_of(const uint64_t* __restrict__ off, uint64_t n, uint64_t v) {
    uint64_t l = 0, h = n + 1;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (off[mid] <= v) l = mid + 1;
        else h = mid;
    }
    return l ? l - 1 : 0;
}

// The owners [p0, p0 + nps) that a tile can meet, from the owners of its first and its last
// element (csr_owner_of; p_last is cut to the last owner, n - 1)
__host__ __device__ __forceinline__ uint64_t csr_slice_len(uint64_t p0, uint64_t p_last, uint64_t n) {
    uint64_t p1 = p_last;
    if (p1 < p0) p1 = p0;
    if (p1 > n - 1) p1 = n - 1;
    return p1 - p0 + 1;
}

// offset o relative to the tile [t0, t0 + T), clamped into [0, T]: a u32 whatever o and t0 are
__host__ __device__ __forceinline__ uint32_t csr_rel(uint64_t o, uint64_t t0, uint32_t T) {
    return o <= t0 ? 0u : (o - t0 >= T ? T : (uint32_t)(o - t0));
}

// Where the tile's element e = c - t0 falls among the nps owners [p0, p0 + nps) of the slice: the
// number l in [1, nps] of them that start at or before it, so its owner is p0 + l - 1.  Staged:
// over rel[x] = csr_rel(off[p0 + x], t0, T) <= e; unstaged: over off[x] <= c, `off` pointing at
// off[p0].  Owner p0 is the first element's and counts unprobed
__host__ __device__ __forceinline__ uint64_t csr_bisect_staged(const uint32_t* rel, uint64_t nps, uint32_t e) {
    uint64_t l = 1, h = nps;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (rel[mid] <= e) l = mid + 1;
        else h = mid;
    }
    return l;
}
__host__ __device__ __forceinline__ uint64_t csr_bisect_offsets(const uint64_t* __restrict__ off, uint64_t nps,
                                                                uint64_t c) {
    uint64_t l = 1, h = nps;
    while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if (off[mid] <= c) l = mid + 1;
        else h = mid;
    }
    return l;
}

#ifdef __HIPCC__
// the offsets' own bounds: element c lies in its owner's span
__device__ __forceinline__ bool csr_in_bounds(const uint64_t* __restrict__ off, uint64_t owner, uint64_t c) {
    return off[owner] <= c && c < off[owner + 1];
}

// The owners of the elements [t0, t0 + n_el) of one tile (n_el <= T), for the whole workgroup of
// BLOCK threads: element e = u BLOCK + tid belongs to owner own[u], found by bisecting the tile's
// slice of `off`, staged in `rel` when it is at most SLICE owners long; ok[u] = 0 for an element
// past the tile or one that accept(u, c, owner) turns down: csr_in_bounds, the offsets' own
// bounds, and whatever else the caller asks of element c = t0 + e.  `rel` (SLICE words) and
// `sh_p` (2 words) are LDS; the caller puts a __syncthreads() between two tiles.
template <int T, int SLICE, int BLOCK, class Accept>
__device__ __forceinline__ void csr_tile_owners(const uint64_t* __restrict__ off, uint64_t n, uint64_t t0,
                                                uint32_t n_el, uint32_t* rel, uint64_t* sh_p,
                                                uint64_t (&own)[T / BLOCK], uint32_t (&ok)[T / BLOCK],
                                                Accept accept) {
    const uint32_t tid = threadIdx.x;
    // the owners of the tile's first and last element (both non-empty)
    if (tid < 2) sh_p[tid] = csr_owner_of(off, n, tid ? t0 + n_el - 1 : t0);
    __syncthreads();
    const uint64_t p0 = sh_p[0];
    const uint64_t nps = csr_slice_len(p0, sh_p[1], n);
    const uint32_t staged = nps <= SLICE ? 1u : 0u;
    if (staged) {
        for (uint32_t x = tid; x < (uint32_t)nps; x += BLOCK) rel[x] = csr_rel(off[p0 + x], t0, T);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < T / BLOCK; u++) {
        const uint32_t e = u * BLOCK + tid;
        const uint64_t c = t0 + e;
        ok[u] = e < n_el ? 1u : 0u;
        own[u] = 0;
        if (ok[u]) {
            own[u] = p0 + (staged ? csr_bisect_staged(rel, nps, e) : csr_bisect_offsets(off + p0, nps, c)) - 1;
            ok[u] = accept(u, c, own[u]) ? 1u : 0u;
        }
    }
}
#endif
