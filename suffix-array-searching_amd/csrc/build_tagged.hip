// build_tagged.hip -- the two layouts of SAS_ALGO_TAGGED, both made from the plain SA and
// replacing it: the tagged SA with its bucket table (SAS_BUILD_TAGGED) and the bucket lines
// (SAS_BUILD_TAG_LINES), which take their first ranks from the bucket table's fill.
#include "build_util.hpp"
#include "build_steps.hpp"

#include <rocprim/device/device_scan.hpp>

// ------------------------------------------------------------------ tagged SA + bucket table
// SAS_BUILD_TAGGED: entry r = SA[r] | chars [p, p+12) of suffix SA[r] << 40
// (zero padded past the text end), so the entries of a p-char bucket carry the suffixes'
// (p+12)-char keys next to their positions.  The bucket table is the reference's prefix
// table (sas/sa_search.rs:59-75) with p live, u64 entries {first rank with key >= x |
// min(count, 2^24 - 1) << 40}: one aligned 8-B read gives a bucket's whole rank range.
template <int W>
__global__ void k_tag_entries(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n, uint32_t p,
                              uint64_t* __restrict__ out) {
    GRID_STRIDE(r, sa_n) {
        const uint64_t s = sa[r];
        const uint64_t tag = (text_chars32(tw, s) << (2 * p)) >> 40;
        out[r] = s | (tag << 40);
    }
}

// p-char key of the suffix at rank r (S: SaView<4|5> over an SA, SaView<8> over tagged entries)
template <class S>
__device__ __forceinline__ uint64_t tag_key(const uint64_t* tw, S ent, uint64_t r, uint32_t p) {
    return text_chars32(tw, ent[r]) >> (64 - 2 * p);
}

// Rank r with a new p-char key fills table(key(r-1), key(r)] = r (rank sa_n fills the rest
// up to 4^p); gaps longer than PT_SMALL go to a list that whole workgroups fill.
template <class S>
__global__ void k_tt_fill(const uint64_t* __restrict__ tw, S ent, uint64_t sa_n,
                          uint32_t p, uint64_t* __restrict__ table, uint64_t* __restrict__ big,
                          unsigned long long* __restrict__ nbig, uint64_t big_cap) {
    const uint64_t top = 1ull << (2 * p);
    GRID_STRIDE(r, sa_n + 1) {
        const uint64_t kr = r < sa_n ? tag_key(tw, ent, r, p) : top;
        const uint64_t lo = r > 0 ? tag_key(tw, ent, r - 1, p) + 1 : 0;
        if (lo > kr) continue;
        if (kr - lo < PT_SMALL) {
            for (uint64_t x = lo; x <= kr; x++) table[x] = r;
        } else {
            const unsigned long long slot = atomicAdd(nbig, 1ull);
            if (slot < big_cap) {
                big[3 * slot] = lo;
                big[3 * slot + 1] = kr;
                big[3 * slot + 2] = r;
            }
        }
    }
}

__global__ void k_tt_big(const uint64_t* __restrict__ big, const unsigned long long* __restrict__ nbig,
                         uint64_t big_cap, uint64_t* __restrict__ table) {
    const uint64_t nb = *nbig < big_cap ? *nbig : big_cap;  // the host fails the build past the cap
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x)
        for (uint64_t x = big[3 * b] + threadIdx.x; x <= big[3 * b + 1]; x += blockDim.x) table[x] = big[3 * b + 2];
}

// count field: entry x gets min(table[x+1] - table[x], 2^24 - 1) in bits 40..63.  Thread
// x+1 only ever changes the high bits of entry x+1, so the rank read here is stable.
__global__ void k_tt_count(uint64_t* __restrict__ table, uint64_t keys) {
    GRID_STRIDE(x, keys) {
        const uint64_t a = table[x] & (SAS_SA40_MAX - 1), b = table[x + 1] & (SAS_SA40_MAX - 1);
        const uint64_t c = b - a < 0xFFFFFFull ? b - a : 0xFFFFFFull;
        table[x] = a | (c << 40);
    }
}

#ifndef SAS_TAG_ALLOC_FLAGS
#define SAS_TAG_ALLOC_FLAGS 0  // hipExtMallocWithFlags flags of the entries and table (A/B)
#endif
int build_tagged(sas_index* x, uint32_t p) {
    const uint64_t sa_n = x->sa_n;
    if (p == 0) {
        uint32_t l4 = 0;  // ceil(log4(sa_n)): ~1-4 suffixes per bucket
        while (l4 < 32 && (1ull << (2 * l4)) < sa_n) l4++;
        p = l4 < 1 ? 1 : (l4 > 16 ? 16 : l4);
    }
    if (p > 17) SAS_FAIL(EINVAL, "SAS_BUILD_TAGGED: p must be 1..17");
    DevBuf ent;
    TRY(ent.alloc_flags(sa_n * 8 + 16, "tagged SA entries", SAS_TAG_ALLOC_FLAGS));
    HIP_TRY(hipMemset(ent.as<uint8_t>() + sa_n * 8, 0, 16));
    const dim3 g(grid_for(sa_n)), b(256);
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(k_tag_entries<W>, g, b, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, p, ent.as<uint64_t>());
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    // the entries hold every SA value: the plain SA goes (80 GiB at n = 2^34)
    (void)hipFree(x->sa);
    x->sa = ent.as<uint8_t>();
    x->sa_w = 8;
    ent.release();
    const uint64_t keys = 1ull << (2 * p);
    const uint64_t cap = (keys + 1) / (PT_SMALL + 1) + 2;
    DevBuf t, big, nbig;
    TRY(t.alloc_flags((keys + 1) * 8 + 8, "tagged bucket table", SAS_TAG_ALLOC_FLAGS));
    TRY(big.alloc(cap * 24, "bucket table gap list"));
    TRY(nbig.alloc(8, "bucket table gap count"));
    HIP_TRY(hipMemset(nbig.p, 0, 8));
    hipLaunchKernelGGL(k_tt_fill<SaView<8>>, dim3(grid_for(sa_n + 1)), b, 0, 0, x->text_w, SaView<8>{x->sa}, sa_n, p,
                       t.as<uint64_t>(), big.as<uint64_t>(), nbig.as<unsigned long long>(), cap);
    hipLaunchKernelGGL(k_tt_big, dim3(4096), b, 0, 0, big.as<uint64_t>(), nbig.as<unsigned long long>(), cap,
                       t.as<uint64_t>());
    hipLaunchKernelGGL(k_tt_count, dim3(grid_for(keys)), b, 0, 0, t.as<uint64_t>(), keys);
    HIP_TRY(hipGetLastError());
    uint64_t nb = 0;
    HIP_TRY(hipMemcpy(&nb, nbig.p, 8, hipMemcpyDeviceToHost));
    if (nb > cap) SAS_FAIL(EFAULT, "bucket table: gap list overflow");  // cannot happen: gaps are disjoint
    x->tag_table = t.as<uint64_t>();
    t.release();
    x->tag_p = p;
    return 0;
}

// ------------------------------------------------------------------ bucket lines
// SAS_BUILD_TAG_LINES: the tagged entries as one 128-B line per p-char bucket (common.hpp,
// sas_index::tag_lines): the header {overflow offset | min(count, 2^24 - 1) << 40} and the
// 48-bit entries {SA | tag << sb} of ranks first .. first + 19, split into u16 high and u32
// low halves; the overflow array with the entries of ranks first + 20 .. first + count of
// every bucket of >= 20 suffixes; the first-rank table (range and SA-by-rank calls, saturated
// counts); a second copy of the packed text 64 B off the 128-B line grid (tl_text).  Built
// from the SA: first ranks (k_tt_fill), overflow offsets (a block scan of max(count - 19,
// 0)), then every slot and overflow entry from SA[r] and its text.  Peak: the SA, the lines
// and the first-rank table.
#define TL_BLOCK 1024
#define TL_PER 4  // buckets per thread in the offset scan

// the entry of rank r: {SA | tag << sb}; rank sa_n (past the index): every bit set, the SA
// field standing for next_pos and the tag the maximum
template <int W>
__device__ __forceinline__ uint64_t tl_make(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n, uint64_t r,
                                            uint32_t p, uint32_t sb) {
    if (r >= sa_n) return (1ull << 48) - 1;
    const uint64_t s = sa[r];
    return s | ((uint64_t)tl_tag_of_key(text_chars32(tw, s), p, tl_tag_bits(sb)) << sb);
}
__device__ __forceinline__ uint64_t tl_tag_max(uint64_t e, uint32_t sb) { return e | (((1ull << 48) - 1) & ~tl_sa_mask(sb)); }

// overflow entries of bucket b: ranks first + 20 .. first + count (the last, rank first + count,
// is the next bucket's first suffix)
__device__ __forceinline__ uint64_t tl_ovf_need(const uint64_t* __restrict__ t, uint64_t b) {
    const uint64_t c = t[b + 1] - t[b];
    return c >= SAS_TL_SLOTS ? c - SAS_TL_SLOTS + 1 : 0;
}

__device__ __forceinline__ uint64_t tl_block_excl_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((long long)inc, o, 64);
        if (lane >= (uint32_t)o) inc += t;
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (uint32_t w = 0; w < nw; w++) {
            const uint64_t t = lds[w];
            lds[w] = acc;
            acc += t;
        }
        lds[nw] = acc;
    }
    __syncthreads();
    *total = lds[nw];
    return lds[wid] + inc - v;
}

__global__ __launch_bounds__(TL_BLOCK) void k_tl_sums(const uint64_t* __restrict__ t, uint64_t keys,
                                                      uint64_t* __restrict__ bsum) {
    __shared__ uint64_t lds[TL_BLOCK / 64 + 1];
    const uint64_t b0 = ((uint64_t)blockIdx.x * TL_BLOCK + threadIdx.x) * TL_PER;
    uint64_t v = 0;
    for (int k = 0; k < TL_PER; k++)
        if (b0 + k < keys) v += tl_ovf_need(t, b0 + k);
    uint64_t tot;
    tl_block_excl_scan(v, lds, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// headers: line b's {overflow offset | count << 40} (bsum: exclusive block offsets)
__global__ __launch_bounds__(TL_BLOCK) void k_tl_hdr(const uint64_t* __restrict__ t, uint64_t keys,
                                                     const uint64_t* __restrict__ bsum, uint64_t* __restrict__ lines) {
    __shared__ uint64_t lds[TL_BLOCK / 64 + 1];
    const uint64_t b0 = ((uint64_t)blockIdx.x * TL_BLOCK + threadIdx.x) * TL_PER;
    uint64_t need[TL_PER], v = 0;
    for (int k = 0; k < TL_PER; k++) {
        need[k] = b0 + k < keys ? tl_ovf_need(t, b0 + k) : 0;
        v += need[k];
    }
    uint64_t tot;
    uint64_t off = bsum[blockIdx.x] + tl_block_excl_scan(v, lds, &tot);
    for (int k = 0; k < TL_PER; k++) {
        const uint64_t b = b0 + k;
        if (b < keys) {
            const uint64_t c = t[b + 1] - t[b];
            lines[b * 16] = off | ((c < 0xFFFFFFull ? c : 0xFFFFFFull) << 40);
            off += need[k];
        }
    }
}

// slot j of line b: rank first + j; a slot past the bucket's count (a later bucket's suffix,
// > every query routed to b) carries the maximal tag, so a lookup's count of the slots whose
// tag is < q's never passes it and needs no count
template <int W>
__global__ void k_tl_slots(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n, uint32_t p, uint32_t sb,
                           uint64_t keys, const uint64_t* __restrict__ t, uint64_t* __restrict__ lines) {
    GRID_STRIDE(k, keys * SAS_TL_SLOTS) {
        const uint64_t b = k / SAS_TL_SLOTS, j = k - b * SAS_TL_SLOTS;
        const uint64_t first = t[b], c = t[b + 1] - first;
        uint64_t e = tl_make<W>(tw, sa, sa_n, first + j, p, sb);
        if (j >= c) e = tl_tag_max(e, sb);
        reinterpret_cast<uint16_t*>(lines + b * 16)[4 + j] = (uint16_t)(e >> 32);
        reinterpret_cast<uint32_t*>(lines + b * 16)[12 + j] = (uint32_t)e;
    }
}

// A bucket's overflow entries, ranks first + 20 .. first + count (the last one the next
// bucket's first suffix with the maximal tag).  One thread per bucket writes up to
// TL_OVF_SMALL of them; a longer bucket (a low-complexity text: a poly-A run at p = 15 is
// millions of suffixes) goes to a list whose buckets whole workgroups fill (k_tl_ovf_big),
// so no bucket waits on one thread's serial tail.
#define TL_OVF_SMALL 256
template <int W>
__global__ void k_tl_ovf(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n, uint32_t p, uint32_t sb,
                         uint64_t keys, const uint64_t* __restrict__ t, const uint64_t* __restrict__ lines,
                         uint64_t* __restrict__ ovf, uint64_t* __restrict__ big, unsigned long long* __restrict__ nbig,
                         uint64_t cap) {
    GRID_STRIDE(b, keys) {
        const uint64_t first = t[b], c = t[b + 1] - first;
        if (c < SAS_TL_SLOTS) continue;
        if (c - SAS_TL_SLOTS >= TL_OVF_SMALL) {
            const unsigned long long k = atomicAdd(nbig, 1ull);
            if (k < cap) big[k] = b;
            continue;
        }
        const uint64_t o = lines[b * 16] & (SAS_SA40_MAX - 1);
        for (uint64_t j = SAS_TL_SLOTS; j <= c; j++) {
            const uint64_t e = tl_make<W>(tw, sa, sa_n, first + j, p, sb);
            ovf[o + j - SAS_TL_SLOTS] = j == c ? tl_tag_max(e, sb) : e;
        }
    }
}

template <int W>
__global__ void k_tl_ovf_big(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n, uint32_t p, uint32_t sb,
                             const uint64_t* __restrict__ t, const uint64_t* __restrict__ lines,
                             uint64_t* __restrict__ ovf, const uint64_t* __restrict__ big,
                             const unsigned long long* __restrict__ nbig, uint64_t big_cap) {
    const uint64_t nb = *nbig < big_cap ? *nbig : big_cap;  // the host fails the build past the cap
    for (uint64_t k = blockIdx.x; k < nb; k += gridDim.x) {
        const uint64_t b = big[k];
        const uint64_t first = t[b], c = t[b + 1] - first;
        const uint64_t o = lines[b * 16] & (SAS_SA40_MAX - 1);
        for (uint64_t j = SAS_TL_SLOTS + threadIdx.x; j <= c; j += blockDim.x) {
            const uint64_t e = tl_make<W>(tw, sa, sa_n, first + j, p, sb);
            ovf[o + j - SAS_TL_SLOTS] = j == c ? tl_tag_max(e, sb) : e;
        }
    }
}

template <int W>
static int build_tag_lines_w(sas_index* x, uint32_t p) {
    const uint64_t sa_n = x->sa_n, keys = 1ull << (2 * p);
    uint32_t sb = 32;  // SA bits: the all-ones field (rank sa_n) must exceed every position < n
    while (sb < 40 && (x->n >> sb) != 0) sb++;
    if ((x->n >> sb) != 0) SAS_FAIL(ENOTSUP, "SAS_BUILD_TAG_LINES: n >= 2^40");
    const dim3 b(256);
    // 1. first rank of every bucket (the tagged table's fill, from the SA)
    const uint64_t cap = (keys + 1) / (PT_SMALL + 1) + 2;
    DevBuf t, big, nbig;
    TRY(t.alloc((keys + 1) * 8 + 8, "bucket first ranks"));
    TRY(big.alloc(cap * 24, "bucket table gap list"));
    TRY(nbig.alloc(8, "bucket table gap count"));
    HIP_TRY(hipMemset(nbig.p, 0, 8));
    hipLaunchKernelGGL(k_tt_fill<SaView<W>>, dim3(grid_for(sa_n + 1)), b, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, p,
                       t.as<uint64_t>(), big.as<uint64_t>(), nbig.as<unsigned long long>(), cap);
    hipLaunchKernelGGL(k_tt_big, dim3(4096), b, 0, 0, big.as<uint64_t>(), nbig.as<unsigned long long>(), cap,
                       t.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    uint64_t nb = 0;
    HIP_TRY(hipMemcpy(&nb, nbig.p, 8, hipMemcpyDeviceToHost));
    if (nb > cap) SAS_FAIL(EFAULT, "bucket lines: gap list overflow");
    big.alloc(0, "free");
    // 2. overflow offsets: block sums, their exclusive scan, the headers
    const uint64_t per_blk = (uint64_t)TL_BLOCK * TL_PER;
    const uint64_t nblk = (keys + per_blk - 1) / per_blk;
    DevBuf bsum, tmp, lines;
    TRY(bsum.alloc(nblk * 8, "bucket lines block sums"));
    hipLaunchKernelGGL(k_tl_sums, dim3((unsigned)nblk), dim3(TL_BLOCK), 0, 0, t.as<uint64_t>(), keys,
                       bsum.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    uint64_t last = 0;
    HIP_TRY(hipMemcpy(&last, bsum.as<uint64_t>() + nblk - 1, 8, hipMemcpyDeviceToHost));
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, bsum.as<uint64_t>(), bsum.as<uint64_t>(), (uint64_t)0, (size_t)nblk,
                                    rocprim::plus<uint64_t>(), (hipStream_t)0));
    TRY(tmp.alloc(tb ? tb : 8, "scan scratch"));
    HIP_TRY(rocprim::exclusive_scan(tmp.p, tb, bsum.as<uint64_t>(), bsum.as<uint64_t>(), (uint64_t)0, (size_t)nblk,
                                    rocprim::plus<uint64_t>(), (hipStream_t)0));
    uint64_t lastx = 0;
    HIP_TRY(hipMemcpy(&lastx, bsum.as<uint64_t>() + nblk - 1, 8, hipMemcpyDeviceToHost));
    const uint64_t novf = lastx + last;
    TRY(lines.alloc(keys * 128, "bucket lines"));
    hipLaunchKernelGGL(k_tl_hdr, dim3((unsigned)nblk), dim3(TL_BLOCK), 0, 0, t.as<uint64_t>(), keys,
                       bsum.as<uint64_t>(), lines.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    bsum.alloc(0, "free");
    tmp.alloc(0, "free");
    // 3. the slots and the overflow entries, from the SA and the text
    DevBuf ovf;
    TRY(ovf.alloc(novf * 8 + 32, "bucket lines overflow"));
    HIP_TRY(hipMemset(ovf.as<uint8_t>() + novf * 8, 0, 32));  // pair loads may read 2 entries past the end
    hipLaunchKernelGGL(k_tl_slots<W>, dim3(grid_for(keys * SAS_TL_SLOTS)), b, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n,
                       p, sb, keys, t.as<uint64_t>(), lines.as<uint64_t>());
    {
        // buckets of > TL_OVF_SMALL overflow entries: at most novf / TL_OVF_SMALL of them
        const uint64_t bcap = novf / TL_OVF_SMALL + 2;
        DevBuf bl, nbl;
        TRY(bl.alloc(bcap * 8, "overflow big-bucket list"));
        TRY(nbl.alloc(8, "overflow big-bucket count"));
        HIP_TRY(hipMemset(nbl.p, 0, 8));
        hipLaunchKernelGGL(k_tl_ovf<W>, dim3(grid_for(keys)), b, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, p, sb,
                           keys, t.as<uint64_t>(), lines.as<uint64_t>(), ovf.as<uint64_t>(), bl.as<uint64_t>(),
                           nbl.as<unsigned long long>(), bcap);
        hipLaunchKernelGGL(k_tl_ovf_big<W>, dim3(4096), b, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, p, sb,
                           t.as<uint64_t>(), lines.as<uint64_t>(), ovf.as<uint64_t>(), bl.as<uint64_t>(),
                           nbl.as<unsigned long long>(), bcap);
        HIP_TRY(hipGetLastError());
        uint64_t nb = 0;
        HIP_TRY(hipMemcpy(&nb, nbl.p, 8, hipMemcpyDeviceToHost));
        if (nb > bcap) SAS_FAIL(EFAULT, "bucket lines: overflow big-bucket list overflow");
        HIP_TRY(hipDeviceSynchronize());
    }
    // the lines and the overflow hold every SA value: the plain SA goes
    (void)hipFree(x->sa);
    x->sa = nullptr;
    x->sa_w = 8;
    x->tag_lines = lines.as<uint64_t>();
    lines.release();
    x->tag_ovf = ovf.as<uint64_t>();
    ovf.release();
    x->tag_first = t.as<uint64_t>();
    t.release();
    x->tag_ovf_n = novf;
    x->tag_p = p;
    x->tag_sb = sb;
    // 4. the second text copy, its word 0 at byte 64 of a 128-B line
    DevBuf t2;
    TRY(t2.alloc(x->text_words * 8 + 128, "packed text, second copy"));
    HIP_TRY(hipMemcpy(t2.as<uint8_t>() + 64, x->text_w, x->text_words * 8, hipMemcpyDeviceToDevice));
    x->text2_base = t2.release();
    x->text2 = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(x->text2_base) + 64);
    return 0;
}

int build_tag_lines(sas_index* x, uint32_t p) {
    if (p == 0) {
        uint32_t l4 = 0;  // ceil(log4(sa_n)) - 2: ~4-16 suffixes per line
        while (l4 < 32 && (1ull << (2 * l4)) < x->sa_n) l4++;
        p = l4 < 3 ? 1 : l4 - 2;
        if (p > 15) p = 15;
    }
    if (p < 1 || p > 15) SAS_FAIL(EINVAL, "SAS_BUILD_TAG_LINES: p must be 1..15 (4^15 lines are 128 GiB)");
    int rc = 0;
    with_sa_w(x->sa_w, [&](auto Wc) { rc = build_tag_lines_w<decltype(Wc)::value>(x, p); });
    return rc;
}
