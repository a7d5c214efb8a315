// sas_route.hip -- the sharded step's send and receive sides: sas_route(_batch), sas_route_pack(_cap)
// and sas_shard_gather.
#include "call_io.hpp"
#include "search_args.hpp"

#include <cstdlib>

// ------------------------------------------------------------------ sharded-mode routing
// Routing compares a query with the splitter suffixes by their first 32 chars (staged in
// LDS once per block: sk[w] = text_chars32 at splitter w) and reads the text only on a tie
// of those keys (distinct 32-char keys order as the strings do, zero padding included,
// as sector_ge relies on): the shard of q = the number of splitter suffixes < q.
__device__ __forceinline__ void stage_split_keys(const uint64_t* __restrict__ tw, const uint64_t* __restrict__ sp,
                                                 uint32_t nsplit, uint64_t* sk) {
    for (uint32_t w = threadIdx.x; w < nsplit; w += blockDim.x) sk[w] = text_chars32(tw, sp[w]);
}

template <int QW>
__device__ __forceinline__ uint32_t route_of(const uint64_t* __restrict__ tw, uint64_t n,
                                             const uint64_t* __restrict__ sp, const uint64_t* sk, uint32_t nsplit,
                                             const QueryRegs<QW>& q) {
    uint32_t lo = 0, hi = nsplit, lcp;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t kk = sk[mid];
        const bool less = kk != q.w[0] ? kk < q.w[0] : suffix_less_from<QW>(tw, n, sp[mid], q, 0, &lcp);
        if (less) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_route(const uint64_t* __restrict__ tw, uint64_t n,
                                               const uint64_t* __restrict__ sp, uint32_t nsplit,
                                               const uint8_t* __restrict__ qbytes, uint32_t m,
                                               const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qlen,
                                               uint64_t nq, uint32_t* __restrict__ out, uint32_t* bad) {
    __shared__ uint64_t sk[SAS_MAX_SPLIT];
    stage_split_keys(tw, sp, nsplit, sk);
    __syncthreads();
    uint32_t b = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x) {
        QueryRegs<4> q;
        if (qoff) q.load(qbytes + qoff[i], qlen[i], &b);  // ragged (sas_route_batch)
        else q.load(qbytes + i * (uint64_t)m, m, &b);
        out[i] = route_of<4>(tw, n, sp, sk, nsplit, q);
    }
    if (b) atomicOr(bad, 1u);
}

// Fixed-length (qoff == nullptr) or ragged routing, host or device pointers.
static int route_impl(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit, const uint8_t* qbytes,
                      uint32_t m, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq, uint32_t* out_shard,
                      void* stream, uint32_t flags) {
    if (!x || (nsplit && !splitter_pos) || (nq && (!qbytes || !out_shard))) SAS_FAIL(EINVAL, "sas_route: null argument");
    if (qoff && !qlen) SAS_FAIL(EINVAL, "sas_route_batch: qoff without qlen");
    if (nsplit > SAS_MAX_SPLIT) SAS_FAIL(EINVAL, "sas_route: too many splitters");
    if (nq == 0) return 0;
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool dev = flags & SAS_DEVICE_PTRS;
    DevBuf bsp;
    HostQueries hq;
    HostOutputs ho;
    const uint64_t* dsp = splitter_pos;
    MmQueries Q{qbytes, qoff, qlen, m, nq};
    uint32_t* dout = out_shard;
    if (!dev) {  // host arrays: copy in, the kernel, copy out (synchronous; bytes not validated)
        TRY(host_copy_in(bsp, splitter_pos, nsplit * 8, "route splitters"));
        dsp = bsp.as<uint64_t>();
        TRY(hq.stage("route", QueryArgs{qbytes, qoff, qlen, m, qoff != nullptr}, nq, st, &Q));
        TRY(ho.twin(out_shard, nq * 4, "route shards", &dout));
    }
    uint64_t blocks = (nq + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_route, dim3((unsigned)blocks), dim3(256), 0, st, x->text_w, x->n, dsp, nsplit, Q.qbytes, m,
                       Q.qoff, Q.qlen, nq, dout, x->scratch);
    HIP_TRY(hipGetLastError());
    if (!dev) {
        TRY(ho.copy_back(st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int sas_route(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit, const uint8_t* qbytes,
                         uint32_t m, uint64_t nq, uint32_t* out_shard, void* stream, uint32_t flags) {
    return route_impl(x, splitter_pos, nsplit, qbytes, m, nullptr, nullptr, nq, out_shard, stream, flags);
}

extern "C" int sas_route_batch(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit,
                               const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
                               uint32_t* out_shard, void* stream, uint32_t flags) {
    if (nq && (!qoff || !qlen)) SAS_FAIL(EINVAL, "sas_route_batch: null qoff/qlen");
    return route_impl(x, splitter_pos, nsplit, qbytes, 0, qoff, qlen, nq, out_shard, stream, flags);
}

// ------------------------------------------------------------------ route + pack (sharded step)
// One sharded-mode step needs the queries grouped by destination shard.  This is
// a counting sort by destination, fused with the routing and the byte copy:
//   k_route_count    dest[i] (as in sas_route) + per-block histogram of dest (LDS
//                    atomics) -> cnt[w * nblk + b] (+ the packed word, SAS_ROUTE_PACKED)
//   exclusive scan   -> base[w * nblk + b] = first send slot of (bucket w, block b)
//   k_pack_scatter   slot = base + LDS-atomic rank; copy the query's m bytes to
//                    send[slot * m]; slot_of[i] = slot (positions come back in
//                    send order and are gathered with it)
// Order inside a bucket is not stable (it need not be: every slot is recorded).
#define PACK_BLOCK 1024
#define PACK_ITEMS 8
#define PACK_CHUNK (PACK_BLOCK * PACK_ITEMS)
#ifndef SAS_ROUTE_ITEMS
#define SAS_ROUTE_ITEMS 8
#endif

// route + per-block histogram in one pass over the queries: dest[i] = the shard of query i
// (as k_route; no splitters: shard 0 without reading the query), and with PACKED its 2-bit
// word for the scatter (SAS_ROUTE_PACKED), so the query bytes are read once
template <bool PACKED>
__global__ __launch_bounds__(PACK_BLOCK) void k_route_count(const uint64_t* __restrict__ tw, uint64_t n,
                                                            const uint64_t* __restrict__ sp, uint32_t nsplit,
                                                            const uint8_t* __restrict__ qbytes, uint32_t m, uint64_t nq,
                                                            uint64_t nblk, uint64_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ dest, uint64_t* __restrict__ words) {
    __shared__ uint32_t h[SAS_MAX_SPLIT + 1];
    __shared__ uint64_t sk[SAS_MAX_SPLIT];
    const uint32_t W = nsplit + 1;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) h[w] = 0;
    stage_split_keys(tw, sp, nsplit, sk);
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PACK_CHUNK;
    for (int it = 0; it < PACK_ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * PACK_BLOCK + threadIdx.x;
        if (i >= nq) continue;
        uint32_t lo = 0;
        if (PACKED || nsplit) {
            uint32_t b = 0;
            QueryRegs<PACKED ? 1 : 4> q;
            q.load(qbytes + i * (uint64_t)m, m, &b);
            if (PACKED) words[i] = q.w[0];
            lo = route_of<PACKED ? 1 : 4>(tw, n, sp, sk, nsplit, q);
        }
        dest[i] = lo;
        atomicAdd(&h[lo], 1u);
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) cnt[(uint64_t)w * nblk + blockIdx.x] = h[w];
}

// cap == 0: buckets packed back to back (slot = the exclusive scan); cap > 0: bucket w
// owns slots [w * cap, (w + 1) * cap) and a query past its bucket's cap is not copied (its
// slot is clamped to the last one; the caller sees the overflow in out_counts > cap)
__global__ __launch_bounds__(PACK_BLOCK) void k_pack_scatter(const uint32_t* __restrict__ dest, uint64_t nq,
                                                             uint32_t W, uint64_t nblk,
                                                             const uint64_t* __restrict__ base_slot,
                                                             const uint8_t* __restrict__ qbytes, uint32_t m,
                                                             uint8_t* __restrict__ send,
                                                             uint64_t* __restrict__ slot_of, uint64_t cap,
                                                             bool packed, const uint64_t* __restrict__ words) {
    __shared__ uint32_t h[SAS_MAX_SPLIT + 1];
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) h[w] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PACK_CHUNK;
    const bool vec = (m & 15) == 0 && ((((uintptr_t)qbytes) | ((uintptr_t)send)) & 15) == 0;
    for (int it = 0; it < PACK_ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * PACK_BLOCK + threadIdx.x;
        if (i >= nq) continue;
        const uint32_t w = dest[i];
        uint64_t slot = base_slot[(uint64_t)w * nblk + blockIdx.x] + atomicAdd(&h[w], 1u);
        if (cap) {
            const uint64_t r = slot - base_slot[(uint64_t)w * nblk];  // rank inside bucket w
            if (r >= cap) {
                slot_of[i] = (uint64_t)W * cap - 1;
                continue;
            }
            slot = (uint64_t)w * cap + r;
        }
        slot_of[i] = slot;
        const uint8_t* src = qbytes + i * (uint64_t)m;
        if (packed) {  // SAS_ROUTE_PACKED: the query's 2-bit word (m <= 32), 8 B per slot
            uint32_t bad = 0;
            reinterpret_cast<uint64_t*>(send)[slot] = words ? words[i] : pack_query_word(src, m, 0, &bad);
            continue;
        }
        uint8_t* dst = send + slot * (uint64_t)m;
        if (vec) {
            for (uint32_t k = 0; k < m; k += 16)
                *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
        } else {
            for (uint32_t k = 0; k < m; k++) dst[k] = src[k];
        }
    }
}

// cap > 0 in one pass over the queries (no dest array, no scan, no second read):
//   1. each thread routes (and with SAS_ROUTE_PACKED packs) its PACK_ITEMS queries; per
//      item, each wave takes one LDS atomic per destination present in it (leader lane,
//      popcount of the ballot), so a lane's rank inside its (block, bucket) share is
//      that share's running offset + the lanes below it with the same destination;
//   2. one global atomic per (block, bucket) claims the share's first rank in bucket w
//      (counts[w], zeroed by the caller of the launch, ends as the bucket's total);
//   3. query i goes to slot w * cap + claimed + rank, or past the cap is clamped as above.
template <bool PACKED, int ITEMS>
__global__ __launch_bounds__(PACK_BLOCK) void k_route_scatter_cap(
    const uint64_t* __restrict__ tw, uint64_t n, const uint64_t* __restrict__ sp, uint32_t nsplit,
    const uint8_t* __restrict__ qbytes, uint32_t m, uint64_t nq, uint64_t cap, unsigned long long* __restrict__ counts,
    uint8_t* __restrict__ send, uint64_t* __restrict__ slot_of) {
    __shared__ uint32_t h[SAS_MAX_SPLIT + 1];
    __shared__ uint64_t claimed[SAS_MAX_SPLIT + 1];
    __shared__ uint64_t sk[SAS_MAX_SPLIT];
    const uint32_t W = nsplit + 1;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) h[w] = 0;
    stage_split_keys(tw, sp, nsplit, sk);
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * (PACK_BLOCK * ITEMS);
    const int lane = (int)(threadIdx.x & 63);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t dst[ITEMS], rk[ITEMS];
    uint64_t wd[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * PACK_BLOCK + threadIdx.x;
        const bool valid = i < nq;
        uint32_t lo = 0;
        wd[it] = 0;
        if (valid && (PACKED || nsplit)) {
            uint32_t b = 0;
            QueryRegs<PACKED ? 1 : 4> q;
            q.load(qbytes + i * (uint64_t)m, m, &b);
            wd[it] = q.w[0];
            lo = route_of<PACKED ? 1 : 4>(tw, n, sp, sk, nsplit, q);
        }
        dst[it] = lo;
        rk[it] = 0;
        uint64_t todo = __ballot(valid);
        while (todo) {  // wave-uniform: one pass per distinct destination in the wave
            const int leader = __builtin_ctzll(todo);
            const uint32_t d = (uint32_t)__shfl((int)lo, leader, 64);
            const uint64_t same = __ballot(valid && lo == d);
            uint32_t r0 = 0;
            if (lane == leader) r0 = atomicAdd(&h[d], (uint32_t)__popcll(same));
            r0 = (uint32_t)__shfl((int)r0, leader, 64);
            if (valid && lo == d) rk[it] = r0 + (uint32_t)__popcll(same & below);
            todo &= ~same;
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x)
        claimed[w] = h[w] ? (uint64_t)atomicAdd(&counts[w], (unsigned long long)h[w]) : 0ull;
    __syncthreads();
    const bool vec = (m & 15) == 0 && ((((uintptr_t)qbytes) | ((uintptr_t)send)) & 15) == 0;
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * PACK_BLOCK + threadIdx.x;
        if (i >= nq) continue;
        const uint32_t w = dst[it];
        const uint64_t r = claimed[w] + rk[it];
        if (r >= cap) {
            slot_of[i] = (uint64_t)W * cap - 1;
            continue;
        }
        const uint64_t slot = (uint64_t)w * cap + r;
        slot_of[i] = slot;
        if (PACKED) {
            reinterpret_cast<uint64_t*>(send)[slot] = wd[it];
            continue;
        }
        const uint8_t* src = qbytes + i * (uint64_t)m;  // read again: the block read it in pass 1
        uint8_t* dp = send + slot * (uint64_t)m;
        if (vec) {
            for (uint32_t k = 0; k < m; k += 16)
                *reinterpret_cast<uint4*>(dp + k) = *reinterpret_cast<const uint4*>(src + k);
        } else {
            for (uint32_t k = 0; k < m; k++) dp[k] = src[k];
        }
    }
}

// The sharded step's receive side: out[i] = back[slot_of[i]] (the positions returned in
// send-slot order, put back in query order); block 0 also raises *overflow (plain store
// of 1, never cleared here) when a bucket's count passed its capacity.
__global__ void k_shard_gather(const uint64_t* __restrict__ back, const uint64_t* __restrict__ slot_of, uint64_t nq,
                               const uint64_t* __restrict__ counts, uint32_t W, uint64_t cap,
                               uint64_t* __restrict__ out, uint32_t* __restrict__ overflow) {
    if (blockIdx.x == 0 && overflow) {
        bool over = false;
        for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) over |= counts[w] > cap;
        if (over) overflow[0] = 1u;
    }
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = back[slot_of[i]];
}

__global__ void k_pack_totals(const uint64_t* __restrict__ base_slot, uint32_t W, uint64_t nblk, uint64_t nq,
                              uint64_t* __restrict__ out_counts) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        const uint64_t lo = base_slot[(uint64_t)w * nblk];
        const uint64_t hi = (w + 1 < W) ? base_slot[(uint64_t)(w + 1) * nblk] : nq;
        out_counts[w] = hi - lo;
    }
}

static int route_pack_impl(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit,
                           const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t cap, uint64_t* out_counts,
                           uint8_t* out_send, uint64_t* out_slot, void* stream, uint32_t flags) {
    if (!x || (nsplit && !splitter_pos) || !out_counts || (nq && (!qbytes || !out_send || !out_slot)))
        SAS_FAIL(EINVAL, "sas_route_pack: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_route_pack: device pointers only (SAS_DEVICE_PTRS)");
    if (nsplit > SAS_MAX_SPLIT) SAS_FAIL(EINVAL, "sas_route_pack: too many splitters");
    if ((flags & SAS_ROUTE_PACKED) && m > 32) SAS_FAIL(EINVAL, "sas_route_pack: SAS_ROUTE_PACKED needs m <= 32");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t W = nsplit + 1;
    if (nq == 0) {
        HIP_TRY(hipMemsetAsync(out_counts, 0, W * 8, st));
        return 0;
    }
    const uint64_t nblk = (nq + PACK_CHUNK - 1) / PACK_CHUNK;
    const bool packed = (flags & SAS_ROUTE_PACKED) != 0;
    if (cap) {  // fixed-capacity buckets: one pass, no scratch
        HIP_TRY(hipMemsetAsync(out_counts, 0, W * 8, st));
        auto* c = reinterpret_cast<unsigned long long*>(out_counts);
        // queries per thread (A/B knob SAS_ROUTE_ITEMS = 2 / 4 / 8)
        static const int items = [] {
            const char* e = getenv("SAS_ROUTE_ITEMS");
            const int v = e ? atoi(e) : SAS_ROUTE_ITEMS;
            return (v == 2 || v == 4 || v == 8) ? v : SAS_ROUTE_ITEMS;
        }();
        const dim3 grid((unsigned)((nq + (uint64_t)PACK_BLOCK * items - 1) / ((uint64_t)PACK_BLOCK * items)));
#define SAS_RSC(P, I)                                                                                              \
    hipLaunchKernelGGL((k_route_scatter_cap<P, I>), grid, dim3(PACK_BLOCK), 0, st, x->text_w, x->n, splitter_pos, \
                       nsplit, qbytes, m, nq, cap, c, out_send, out_slot)
        if (packed) {
            if (items == 2) SAS_RSC(true, 2);
            else if (items == 4) SAS_RSC(true, 4);
            else SAS_RSC(true, 8);
        } else {
            if (items == 2) SAS_RSC(false, 2);
            else if (items == 4) SAS_RSC(false, 4);
            else SAS_RSC(false, 8);
        }
#undef SAS_RSC
        HIP_TRY(hipGetLastError());
        return 0;
    }
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    // with splitters the routing reads each query anyway and packs it on the way (words);
    // without (one part) the routing reads nothing and the scatter packs from the bytes
    const bool pack_in_route = packed && nsplit > 0;
    PoolBuf dest, cnt, words;
    TRY(dest.alloc(pool, nq * 4, st));
    TRY(cnt.alloc(pool, nblk * W * 8, st));
    if (pack_in_route) TRY(words.alloc(pool, nq * 8, st));
    if (pack_in_route)
        hipLaunchKernelGGL(k_route_count<true>, dim3((unsigned)nblk), dim3(PACK_BLOCK), 0, st, x->text_w, x->n,
                           splitter_pos, nsplit, qbytes, m, nq, nblk, cnt.as<uint64_t>(), dest.as<uint32_t>(),
                           words.as<uint64_t>());
    else
        hipLaunchKernelGGL(k_route_count<false>, dim3((unsigned)nblk), dim3(PACK_BLOCK), 0, st, x->text_w, x->n,
                           splitter_pos, nsplit, qbytes, m, nq, nblk, cnt.as<uint64_t>(), dest.as<uint32_t>(),
                           (uint64_t*)nullptr);
    TRY(pool_scan(pool, st, cnt.as<uint64_t>(), cnt.as<uint64_t>(), nblk * W));
    hipLaunchKernelGGL(k_pack_scatter, dim3((unsigned)nblk), dim3(PACK_BLOCK), 0, st, dest.as<uint32_t>(), nq, W, nblk,
                       cnt.as<uint64_t>(), qbytes, m, out_send, out_slot, cap, packed, words.as<const uint64_t>());
    hipLaunchKernelGGL(k_pack_totals, dim3(1), dim3(256), 0, st, cnt.as<uint64_t>(), W, nblk, nq, out_counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sas_route_pack(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit,
                              const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t* out_counts,
                              uint8_t* out_send, uint64_t* out_slot, void* stream, uint32_t flags) {
    return route_pack_impl(x, splitter_pos, nsplit, qbytes, m, nq, 0, out_counts, out_send, out_slot, stream, flags);
}

extern "C" int sas_route_pack_cap(const sas_index* x, const uint64_t* splitter_pos, uint32_t nsplit,
                                  const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t cap, uint64_t* out_counts,
                                  uint8_t* out_send, uint64_t* out_slot, void* stream, uint32_t flags) {
    if (cap == 0) SAS_FAIL(EINVAL, "sas_route_pack_cap: cap must be > 0");
    return route_pack_impl(x, splitter_pos, nsplit, qbytes, m, nq, cap, out_counts, out_send, out_slot, stream, flags);
}

extern "C" int sas_shard_gather(const sas_index* x, const uint64_t* back, const uint64_t* slot, uint64_t nq,
                                const uint64_t* counts, uint32_t nparts, uint64_t cap, uint64_t* out,
                                uint32_t* overflow, void* stream, uint32_t flags) {
    if (!x || (nq && (!back || !slot || !out)) || (overflow && (!counts || nparts == 0)))
        SAS_FAIL(EINVAL, "sas_shard_gather: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_shard_gather: device pointers only (SAS_DEVICE_PTRS)");
    if (nq == 0 && !overflow) return 0;
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t blocks = (nq + 255) / 256;
    const uint64_t capb = (uint64_t)x->num_cus * 8;
    if (blocks > capb) blocks = capb;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_shard_gather, dim3((unsigned)blocks), dim3(256), 0, st, back, slot, nq, counts, nparts, cap,
                       out, overflow);
    HIP_TRY(hipGetLastError());
    return 0;
}
