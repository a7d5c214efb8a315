// sas_locate.hip -- batched locate: the occurrence positions of every query of a batch in CSR
// form (sas.h: sas_locate_offsets, sas_locate_fill, sas_locate, sas_locate_fixed).
//
// The range search gives each query its SA rank range [lo, hi); the positions are SA[lo..hi).
// The expansion is ragged and heavily skewed (a 4-char query on a 2^30 text owns 4 x 10^6
// ranks, a 32-char one a single rank, a random one none), so the fill kernel is
// output-centric: a workgroup owns tiles of LOC_T consecutive OUTPUT elements and maps each
// element back to its query through out_off.
//
//   * element j belongs to query upper_bound(out_off, j) - 1: among equal offsets the last
//     is the non-empty query, so runs of empty queries are skipped by the bisection itself
//     and no loop runs over a query's range or over a run of empties;
//   * a tile's first query comes from a partition pre-pass (k_locate_tiles: one thread per
//     tile boundary, capacity / LOC_T + 1 of them, scratch from the index's pool) that leaves
//     a 32-B record per tile {query, its two offsets, its lo}; the fill reads its record in
//     one request, and the next tile's while it copies, instead of a chain of ~log2(nq)
//     dependent reads per tile
//     (with SAS_LOCATE_NO_PARTITION two threads of each workgroup bisect instead: the A/B
//     hook of tools/bench_locate.py);
//   * a tile inside one query is a straight coalesced copy (u32 SA: 16-B loads and stores
//     when source and destination are 16-B aligned);
//   * otherwise the tile's slice of out_off is staged in LDS relative to the tile start
//     (u32, up to LOC_SLICE entries) and bisected there per element; a longer slice (long
//     runs of empty queries) is bisected in global memory, where it is L2-resident;
//   * element e of a tile is handled by thread e % 256, so stores are coalesced in every
//     case; all of a thread's SA reads are issued before the first is used.
//
// SAS_BUILD_TAG_LINES has no SA array: a rank is looked up through tl_sa_at (common.hpp), a
// binary search over the buckets' first ranks per element.  That path is correct, not tuned.
#include "call_io.hpp"
#include "csr_tile.hpp"

#include <type_traits>
#include <vector>

#define LOC_BLOCK 256
#define LOC_T 2048        // output elements per tile (<= 8192)
#define LOC_PER (LOC_T / LOC_BLOCK)
#define LOC_SLICE 4096    // out_off entries of a tile staged in LDS (16 KiB)
#define LOC_BLOCKS_PER_CU 8
#define LOC_MAX_GRID (1u << 20)

// SA[r] of a bucket-line index (no SA array)
struct TlView {
    const uint64_t* lines;
    const uint64_t* ovf;
    const uint64_t* first;
    uint64_t keys;
    uint32_t sb;
    __device__ __forceinline__ uint64_t operator[](uint64_t r) const { return tl_sa_at(lines, ovf, first, keys, sb, r); }
};

// out_off[k] = ranks of [lo[k], hi[k]) this index holds, capped; out_off[nq] = 0 (the scan
// turns it into the total)
__global__ void k_locate_count(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi, uint64_t nq,
                               uint64_t rank_lo, uint64_t sa_n, uint64_t max_per_query,
                               uint64_t* __restrict__ out_off) {
    GRID_STRIDE(k, nq + 1) {
        uint64_t c = 0;
        if (k < nq) {
            const uint64_t l = lo[k] > rank_lo ? lo[k] : rank_lo;
            const uint64_t h = hi[k] < rank_lo + sa_n ? hi[k] : rank_lo + sa_n;
            c = (hi[k] >= lo[k] && h > l) ? h - l : 0;
            if (max_per_query && c > max_per_query) c = max_per_query;
        }
        out_off[k] = c;
    }
}

// What a tile needs before it touches the SA, one 32-B record per tile boundary t in
// [0, ntiles]: the query q of output element t * LOC_T, off[q], off[q + 1] and lo[q] (zeros
// past the total).  The fill reads its tile's record in one request and the next tile's
// while it copies, instead of a chain of dependent reads per tile.
struct __attribute__((aligned(32))) LocTile {
    uint64_t q, o0, o1, l0;
};

__device__ __forceinline__ LocTile locate_tile_of(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ off,
                                                  uint64_t nq, uint64_t q) {
    LocTile r{q, 0, 0, 0};
    if (q < nq) {
        r.o0 = off[q];
        r.o1 = off[q + 1];
        r.l0 = lo[q];
    }
    return r;
}

__global__ void k_locate_tiles(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ off, uint64_t nq,
                               uint64_t ntiles, LocTile* __restrict__ tiles) {
    GRID_STRIDE(t, ntiles + 1) tiles[t] = locate_tile_of(lo, off, nq, csr_owner_of(off, nq, t * (uint64_t)LOC_T));
}

template <class SA, bool U32>
__global__ __launch_bounds__(LOC_BLOCK) void k_locate_fill(SA sa, uint64_t sa_n, uint64_t rank_lo,
                                                           const uint64_t* __restrict__ lo,
                                                           const uint64_t* __restrict__ off, uint64_t nq,
                                                           void* __restrict__ out_v, uint64_t capacity,
                                                           const LocTile* __restrict__ tiles, uint64_t ntiles) {
    typedef typename std::conditional<U32, uint32_t, uint64_t>::type OutT;
    OutT* __restrict__ out = static_cast<OutT*>(out_v);
    __shared__ uint32_t rel[LOC_SLICE];
    __shared__ uint64_t sh_q[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = off[nq];
    const uint64_t end = total < capacity ? total : capacity;
    LocTile r{}, nx{};
    if (tiles && blockIdx.x < ntiles) r = tiles[blockIdx.x];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, r = nx) {
        const uint64_t t0 = tile * (uint64_t)LOC_T;
        if (t0 >= end) break;  // tiles only grow: nothing left for this workgroup
        const uint64_t t1 = t0 + LOC_T < end ? t0 + LOC_T : end;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t q1 = 0;
        if (tiles) {
            if (tile + gridDim.x < ntiles) nx = tiles[tile + gridDim.x];  // in flight during this tile's copy
        } else {
            if (tid < 2) sh_q[tid] = csr_owner_of(off, nq, t0 + (uint64_t)tid * LOC_T);
            __syncthreads();
            r = locate_tile_of(lo, off, nq, sh_q[0]);
            q1 = sh_q[1];
            __syncthreads();
        }
        const uint64_t q0 = r.q;
        if (q0 >= nq) break;  // offsets that are no scan of counts: write nothing
        const uint64_t o0 = r.o0;
        if (r.o1 >= t1 && o0 <= t0) {
            // the whole tile lies inside query q0: a straight copy of SA[base .. base + n_el)
            const uint64_t l0 = r.l0;
            const uint64_t base = (l0 > rank_lo ? l0 - rank_lo : 0) + (t0 - o0);
            if (base + n_el <= sa_n) {
                if constexpr (std::is_same<SA, SaView<4>>::value) {
                    const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(sa.p) + base;
                    OutT* __restrict__ d = out + t0;
                    if (((base & 3) | (reinterpret_cast<uintptr_t>(d) & 15)) == 0) {
                        const uint32_t ngrp = n_el >> 2;
                        for (uint32_t g = tid; g < ngrp; g += LOC_BLOCK) {
                            const uint4 v = reinterpret_cast<const uint4*>(s)[g];
                            if (U32) {
                                reinterpret_cast<uint4*>(d)[g] = v;
                            } else {
                                ulonglong2* d2 = reinterpret_cast<ulonglong2*>(d) + 2 * (uint64_t)g;
                                d2[0] = make_ulonglong2(v.x, v.y);
                                d2[1] = make_ulonglong2(v.z, v.w);
                            }
                        }
                        const uint32_t e = (ngrp << 2) + tid;
                        if (e < n_el) d[e] = (OutT)s[e];
                        continue;
                    }
                }
                uint64_t v[LOC_PER];
#pragma unroll
                for (int i = 0; i < LOC_PER; i++) {
                    const uint32_t e = i * LOC_BLOCK + tid;
                    v[i] = e < n_el ? sa[base + e] : 0;
                }
#pragma unroll
                for (int i = 0; i < LOC_PER; i++) {
                    const uint32_t e = i * LOC_BLOCK + tid;
                    if (e < n_el) out[t0 + e] = (OutT)v[i];
                }
                continue;
            }
        }
        // several queries meet in the tile: element e belongs to the last query k in
        // [q0, q1] with off[k] <= t0 + e
        if (tiles) q1 = tiles[tile + 1].q;
        if (q1 < q0) q1 = q0;
        if (q1 > nq - 1) q1 = nq - 1;
        const uint64_t nqs = q1 - q0 + 1;
        const bool staged = nqs <= LOC_SLICE;
        if (staged) {
            for (uint32_t k = tid; k < (uint32_t)nqs; k += LOC_BLOCK) {
                const uint64_t o = off[q0 + k];
                rel[k] = o <= t0 ? 0u : (o - t0 >= LOC_T ? (uint32_t)LOC_T : (uint32_t)(o - t0));
            }
            __syncthreads();
        }
        uint64_t rk[LOC_PER];
        bool ok[LOC_PER];
#pragma unroll
        for (int i = 0; i < LOC_PER; i++) {
            const uint32_t e = i * LOC_BLOCK + tid;
            const uint64_t j = t0 + e;
            ok[i] = e < n_el;
            rk[i] = 0;
            if (ok[i]) {
                uint64_t l = 1, h = nqs;  // entry 0 (q0) is <= every element of the tile
                if (staged) {
                    while (l < h) {
                        const uint64_t mid = (l + h) >> 1;
                        if (rel[mid] <= e) l = mid + 1;
                        else h = mid;
                    }
                } else {
                    while (l < h) {
                        const uint64_t mid = (l + h) >> 1;
                        if (off[q0 + mid] <= j) l = mid + 1;
                        else h = mid;
                    }
                }
                const uint64_t k = q0 + l - 1;
                const uint64_t o = off[k], lk = lo[k];
                rk[i] = (lk > rank_lo ? lk - rank_lo : 0) + (j - o);
                ok[i] = o <= j && rk[i] < sa_n;
            }
        }
        uint64_t v[LOC_PER];
#pragma unroll
        for (int i = 0; i < LOC_PER; i++) v[i] = ok[i] ? sa[rk[i]] : 0;
#pragma unroll
        for (int i = 0; i < LOC_PER; i++)
            if (ok[i]) out[t0 + i * LOC_BLOCK + tid] = (OutT)v[i];
        if (staged) __syncthreads();  // rel is rewritten by the next tile
    }
}

extern "C" uint32_t sas_tile_grid_cap(void) { return tile_grid_cap(); }

static int locate_checks(const char* fn, const sas_index* x, uint32_t flags) {
    if ((flags & SAS_LOCATE_U32) && x->n >= (1ull << 32))
        SAS_FAIL(EINVAL, std::string(fn) + ": SAS_LOCATE_U32 needs a text of n < 2^32 chars");
    return 0;
}

extern "C" int sas_locate_offsets(const sas_index* x, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                                  uint64_t max_per_query, uint64_t* out_off, void* stream, uint32_t flags) {
    if (!x || !out_off || (nq && (!lo || !hi))) SAS_FAIL(EINVAL, "sas_locate_offsets: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_locate_offsets: device pointers only (SAS_DEVICE_PTRS)");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 8, st));
        return 0;
    }
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    uint64_t blocks = (nq + 1 + LOC_BLOCK - 1) / LOC_BLOCK;
    const uint64_t capb = (uint64_t)x->num_cus * LOC_BLOCKS_PER_CU;
    if (blocks > capb) blocks = capb;
    hipLaunchKernelGGL(k_locate_count, dim3((unsigned)blocks), dim3(LOC_BLOCK), 0, st, lo, hi, nq, x->rank_lo, x->sa_n,
                       max_per_query, out_off);
    HIP_TRY(hipGetLastError());
    return pool_scan(pool, st, out_off, out_off, nq + 1);
}

template <class SA>
static void launch_fill(bool u32, dim3 grid, hipStream_t st, SA sa, const sas_index* x, const uint64_t* lo,
                        const uint64_t* off, uint64_t nq, void* out, uint64_t capacity, const LocTile* tile_q,
                        uint64_t ntiles) {
    with_bool(u32, [&](auto U32) {
        hipLaunchKernelGGL((k_locate_fill<SA, decltype(U32)::value>), grid, dim3(LOC_BLOCK), 0, st, sa, x->sa_n,
                           x->rank_lo, lo, off, nq, out, capacity, tile_q, ntiles);
    });
}

extern "C" int sas_locate_fill(const sas_index* x, const uint64_t* lo, const uint64_t* out_off, uint64_t nq,
                               void* out_pos, uint64_t capacity, void* stream, uint32_t flags) {
    if (!x || !out_off || (nq && !lo) || (capacity && !out_pos)) SAS_FAIL(EINVAL, "sas_locate_fill: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_locate_fill: device pointers only (SAS_DEVICE_PTRS)");
    TRY(locate_checks("sas_locate_fill", x, flags));
    if (nq == 0 || capacity == 0) return 0;
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t ntiles = (capacity + LOC_T - 1) / LOC_T;
    // the partition pre-pass unless the caller turns it off (the measured choice: DESIGN.md)
    const bool partition = !(flags & SAS_LOCATE_NO_PARTITION);
    PoolBuf tiles;
    LocTile* tile_q = nullptr;
    if (partition) {
        hipMemPool_t pool;
        TRY(sas_scratch_pool(x, &pool));
        TRY(tiles.alloc(pool, (ntiles + 1) * sizeof(LocTile), st));
        tile_q = tiles.as<LocTile>();
        uint64_t pb = (ntiles + 1 + LOC_BLOCK - 1) / LOC_BLOCK;
        if (pb > (uint64_t)x->num_cus * LOC_BLOCKS_PER_CU) pb = (uint64_t)x->num_cus * LOC_BLOCKS_PER_CU;
        hipLaunchKernelGGL(k_locate_tiles, dim3((unsigned)pb), dim3(LOC_BLOCK), 0, st, lo, out_off, nq, ntiles, tile_q);
    }
    // one workgroup per tile (the hardware hands tiles out as workgroups retire: a grid of
    // resident workgroups striding over the tiles left the last eighth of them to a nearly
    // empty chip at 7 waves per SIMD, 0.84 against 0.60 ms on shape C); past LOC_MAX_GRID
    // workgroups they stride.  Workgroups whose tile starts past the total exit at once
    uint64_t blocks = ntiles;
    if (blocks > LOC_MAX_GRID) blocks = LOC_MAX_GRID;
    const dim3 grid((unsigned)tile_grid(blocks));
    const bool u32 = (flags & SAS_LOCATE_U32) != 0;
    if (x->tag_lines)
        launch_fill(u32, grid, st, TlView{x->tag_lines, x->tag_ovf, x->tag_first, 1ull << (2 * x->tag_p), x->tag_sb}, x,
                    lo, out_off, nq, out_pos, capacity, tile_q, ntiles);
    else if (x->sa_w == 8)
        launch_fill(u32, grid, st, SaView<8>{x->sa}, x, lo, out_off, nq, out_pos, capacity, tile_q, ntiles);
    else
        with_sa_w(x->sa_w, [&](auto W) {
            launch_fill(u32, grid, st, SaView<decltype(W)::value>{x->sa}, x, lo, out_off, nq, out_pos, capacity, tile_q, ntiles);
        });
    HIP_TRY(hipGetLastError());
    return 0;
}

static int locate_ranges(const sas_index* x, const QueryArgs& q, uint64_t nq, uint64_t* lo, uint64_t* hi, void* stream,
                         uint32_t flags) {
    return q.ragged ? sas_search_range(x, q.qbytes, q.qoff, q.qlen, nq, lo, hi, stream, flags)
                    : sas_search_range_fixed(x, q.qbytes, q.m, nq, lo, hi, stream, flags);
}

// range search, offsets, fill; ragged (qoff, qlen) or fixed-length
static int locate_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint64_t max_per_query,
                       uint64_t* out_off, void* out_pos, uint64_t capacity, uint64_t* out_total, void* stream,
                       uint32_t flags) {
    if (!x || !out_off || (nq && !q.qbytes) || (capacity && !out_pos))
        SAS_FAIL(EINVAL, std::string(fn) + ": null argument");
    TRY(locate_checks(fn, x, flags));
    const uint32_t sflags = flags & ~(uint32_t)(SAS_LOCATE_U32 | SAS_LOCATE_NO_PARTITION);
    const uint32_t lflags = (flags & (SAS_LOCATE_U32 | SAS_LOCATE_NO_PARTITION)) | SAS_DEVICE_PTRS;
    const uint64_t esz = (flags & SAS_LOCATE_U32) ? 4 : 8;
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & SAS_DEVICE_PTRS) {
        hipMemPool_t pool;
        TRY(sas_scratch_pool(x, &pool));
        PoolBuf lohi;
        TRY(lohi.alloc(pool, nq * 16, st));
        uint64_t* lo = lohi.as<uint64_t>();
        uint64_t* hi = lo + nq;
        int rc = locate_ranges(x, q, nq, lo, hi, stream, sflags);
        if (!rc) rc = sas_locate_offsets(x, lo, hi, nq, max_per_query, out_off, stream, lflags);
        if (!rc) rc = sas_locate_fill(x, lo, out_off, nq, out_pos, capacity, stream, lflags);
        if (!rc && out_total && hipMemcpyAsync(out_total, out_off + nq, 8, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = EIO;
            sas_set_error(rc, std::string(fn) + ": copy of the total failed");
        }
        return rc;
    }
    // host arrays: ranges through the staged host pipeline, then one device result buffer
    std::vector<uint64_t> hr(nq ? 2 * nq : 1);  // lo, then hi: one buffer and one copy
    TRY(locate_ranges(x, q, nq, hr.data(), hr.data() + nq, stream, sflags));
    DevBuf dr;
    HostOutputs ho;
    TRY(host_copy_in(dr, hr.data(), nq * 16, "locate ranges"));
    uint64_t* lo = dr.as<uint64_t>();
    uint64_t* doff;
    TRY(ho.twin(out_off, (nq + 1) * 8, "locate offsets", &doff));
    TRY(sas_locate_offsets(x, lo, lo + nq, nq, max_per_query, doff, stream, lflags));
    uint64_t total;
    TRY(host_list_total(ho, st, fn, "positions", "out_pos", out_off, nq, capacity, out_total, &total));
    if (total == 0) return 0;
    void* dpos;
    TRY(ho.twin(out_pos, total * esz, "locate positions", &dpos));
    TRY(sas_locate_fill(x, lo, doff, nq, dpos, total, stream, lflags));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_locate(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                          uint64_t nq, uint64_t max_per_query, uint64_t* out_off, void* out_pos, uint64_t capacity,
                          uint64_t* out_total, void* stream, uint32_t flags) {
    if (nq && (!qoff || !qlen)) SAS_FAIL(EINVAL, "sas_locate: null qoff/qlen");
    return locate_impl("sas_locate", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, max_per_query, out_off, out_pos,
                       capacity, out_total, stream, flags);
}

extern "C" int sas_locate_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                                uint64_t max_per_query, uint64_t* out_off, void* out_pos, uint64_t capacity,
                                uint64_t* out_total, void* stream, uint32_t flags) {
    return locate_impl("sas_locate_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, max_per_query, out_off,
                       out_pos, capacity, out_total, stream, flags);
}
