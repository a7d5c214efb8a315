// build_prefix.hip -- the prefix table over the quad leaves (SAS_BUILD_PREFIX and its inline forms).
//
// The reference's prefix table (fill_prefix_table / prefix_range, sas/sa_search.rs:59-95,
// dead there because p = 0 at :31): table[x] = the first SA rank whose p-char key
// (zero padded, so key order is SA order) is >= x, for x in [0, 4^p]; the suffixes
// whose key is x are the ranks [table[x], table[x+1]).  Rank r with a new key fills
// table(key(r-1), key(r)] = r (rank sa_n fills the rest up to 4^p); a gap longer than
// PT_SMALL goes to a list that whole workgroups fill.  Keys come from the quad leaves.
// Entries are u32, or packed 40-bit (SaView<5> / sa_put<5>) beside a 40-bit SA, or
// (SAS_BUILD_PREFIX_INLINE, TW = 16) {key64, rank, SA} of that first suffix, so a lookup
// whose answer is the first suffix of its range needs this one read.
#include "build_util.hpp"
#include "build_steps.hpp"

#ifndef SAS_PREFIX_ALLOC_FLAGS
#define SAS_PREFIX_ALLOC_FLAGS 0  // hipExtMallocWithFlags flags for the table (A/B: contiguous, uncached)
#endif
template <bool KO>
__device__ __forceinline__ uint64_t pt_key64(const uint4* leaves, uint64_t r) {
    if (KO) return reinterpret_cast<const uint64_t*>(leaves)[r];
    const uint2 k = reinterpret_cast<const uint2*>(leaves)[2 * r];
    return (uint64_t)k.x | ((uint64_t)k.y << 32);
}

// inline entry for rank r (fused leaves: entry r = {key lo, key hi, SA lo32, SA hi8});
// r = sa_n (nothing >= the key): key MAX, and the kernel answers next_pos
__device__ __forceinline__ uint4 pt_inline_entry(const uint4* leaves, uint64_t sa_n, uint64_t r) {
    if (r >= sa_n) return make_uint4(~0u, ~0u, (uint32_t)sa_n, 0u);
    const uint4 e = leaves[r];
    return make_uint4(e.x, e.y, (uint32_t)r, e.z);
}

// Entry x <- rank r: TW = 4 / 5 bytes of rank, or TW / 16 inline slots (ranks r, r+1, ..)
template <int TW>
__device__ __forceinline__ void pt_fill_range(uint8_t* t, uint64_t lo, uint64_t hi, uint64_t step, uint64_t r,
                                              const uint4* leaves, uint64_t sa_n) {
    if (TW >= 16) {
        constexpr int G = TW >= 16 ? TW / 16 : 1;
        uint4 ev[G];
#pragma unroll
        for (int j = 0; j < G; j++) ev[j] = pt_inline_entry(leaves, sa_n, r + j);
        if (G >= 2) {  // bits 32..39 of every slot's SA value, in slot 1's (unread) rank word
            uint32_t hb = 0;
#pragma unroll
            for (int j = 0; j < G; j++)
                if (r + j < sa_n) hb |= (leaves[r + j].w & 0xFFu) << (8 * j);
            // two slots: bits 32..39 of slot 0's rank too (a part of >= 2^32 suffixes)
            if (G == 2) hb |= (uint32_t)((r < sa_n ? r : sa_n) >> 32 & 0xFFu) << 16;
            ev[G >= 2 ? 1 : 0].z = hb;
        }
        for (uint64_t x = lo; x <= hi; x += step) {
#pragma unroll
            for (int j = 0; j < G; j++) reinterpret_cast<uint4*>(t)[G * x + j] = ev[j];
        }
    } else {
        for (uint64_t x = lo; x <= hi; x += step) sa_put<TW>(t, x, r);
    }
}

// Keys base .. base + entries - 1 (local entries 0 .. entries - 1): the whole key space (base 0,
// 4^p + 1 entries), or a part's key interval (its first key .. its last key + 2, so the two
// entries past its last key hold rank sa_n)
template <bool KO, int TW>
__global__ void k_pt_fill(const uint4* __restrict__ leaves, uint64_t sa_n, uint32_t p, uint64_t base,
                          uint64_t entries, uint8_t* __restrict__ table, uint64_t* __restrict__ big,
                          unsigned long long* __restrict__ nbig, uint64_t big_cap) {
    const uint32_t sh = 64 - 2 * p;
    const uint64_t top = entries - 1;
    GRID_STRIDE(r, sa_n + 1) {
        const uint64_t kr = r < sa_n ? (pt_key64<KO>(leaves, r) >> sh) - base : top;
        const uint64_t lo = r > 0 ? (pt_key64<KO>(leaves, r - 1) >> sh) - base + 1 : 0;
        if (lo > kr) continue;  // same key as rank r - 1
        if (kr - lo < PT_SMALL) {
            pt_fill_range<TW>(table, lo, kr, 1, r, leaves, sa_n);
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

template <int TW>
__global__ void k_pt_big(const uint64_t* __restrict__ big, const unsigned long long* __restrict__ nbig,
                         uint64_t big_cap, uint8_t* __restrict__ table, const uint4* __restrict__ leaves,
                         uint64_t sa_n) {
    const uint64_t nb = *nbig < big_cap ? *nbig : big_cap;  // the host fails the build past the cap
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x)
        pt_fill_range<TW>(table, big[3 * b] + threadIdx.x, big[3 * b + 1], blockDim.x, big[3 * b + 2], leaves, sa_n);
}

int build_prefix(sas_index* x, uint32_t p, uint32_t inl) {
    const uint64_t sa_n = x->sa_n;
    if (!x->quad_leaves) SAS_FAIL(EINVAL, "SAS_BUILD_PREFIX needs SAS_BUILD_QUAD (keys and SA values of the leaves)");
    // inline entries hold a u32 rank and the low 32 bits of each slot's SA value: fused
    // leaves and ranks below 2^32; the one-suffix table also needs positions below 2^32, the
    // two/four-suffix ones carry bits 32..39 in slot 1 (a part index of a 2^33-char text), and
    // the two-suffix one there also bits 32..39 of the rank (a part of >= 2^32 suffixes)
    const bool hi40 = inl >= 2 && x->n > 0xFFFFFFFFull;
    if (inl && (x->quad_compact || (sa_n >= 0xFFFFFFFFull && !(inl == 2 && hi40)) ||
                (inl == 1 && x->n > 0xFFFFFFFFull)))
        SAS_FAIL(ENOTSUP, "SAS_BUILD_PREFIX_INLINE / _INLINE2 / _INLINE4 need fused quad leaves and fewer than "
                          "2^32 - 1 SA entries (SAS_BUILD_PREFIX_INLINE2 on a text of n >= 2^32: any count; "
                          "SAS_BUILD_PREFIX_INLINE also n < 2^32)");
    // u32 entries for a u32 SA, packed 40-bit ones beside a 40-bit SA, 16-B inline ones
    const uint32_t tw = inl ? 16 * inl : (x->sa_w == 5 ? 5 : 4);
    if (tw != 5 && !(tw == 32 && hi40) && sa_n >= 0xFFFFFFFFull)
        SAS_FAIL(ENOTSUP, "SAS_BUILD_PREFIX: u32 ranks need fewer than 2^32 - 1 SA entries");
    if (p == 0) {
        uint32_t l4 = 0;  // ceil(log4(sa_n))
        while (l4 < 32 && (1ull << (2 * l4)) < sa_n) l4++;
        p = l4 + 1 < 16 ? l4 + 1 : 16;
    }
    if (p > 17) SAS_FAIL(EINVAL, "SAS_BUILD_PREFIX_P: p must be 1..17");
    // the keys the table covers: every p-char key for a whole index; for a part (a contiguous
    // SA rank range) the interval from its first suffix's key to its last one's,
    // plus two entries of rank sa_n.  Keys are monotone over the ranks (zero padding), so a
    // part's suffixes are exactly that interval's, and a query outside it clamps to a
    // neighbouring entry whose suffixes are all > q (below) or to rank sa_n (above)
    // (pt_slot, common.hpp).  At 8 parts of a random text: 1/8 of the 4^p keys each
    uint64_t base = 0, entries = (1ull << (2 * p)) + 1;
    if (sa_n < x->n) {
        const uint32_t sh = 64 - 2 * p;
        uint64_t k0 = 0, k1 = 0;
        const uint8_t* lv = reinterpret_cast<const uint8_t*>(x->quad_leaves);
        const uint64_t eb = x->quad_compact ? 8 : 16;
        HIP_TRY(hipMemcpy(&k0, lv, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&k1, lv + (sa_n - 1) * eb, 8, hipMemcpyDeviceToHost));
        base = k0 >> sh;
        entries = (k1 >> sh) - base + 3;
    }
    const uint64_t cap = entries / (PT_SMALL + 1) + 2;
    DevBuf t, big, nbig;
    TRY(t.alloc_flags(entries * tw + 8, "prefix table", SAS_PREFIX_ALLOC_FLAGS));
    TRY(big.alloc(cap * 24, "prefix table gap list"));
    TRY(nbig.alloc(8, "prefix table gap count"));
    HIP_TRY(hipMemset(nbig.p, 0, 8));
    uint8_t* tb = t.as<uint8_t>();
    uint64_t* bl = big.as<uint64_t>();
    unsigned long long* nb_d = nbig.as<unsigned long long>();
    // the fill and then the long gaps, for the leaf format (KO: key-only) and the entry bytes TW
    auto fill = [&](auto KO, auto TW) {
        hipLaunchKernelGGL((k_pt_fill<decltype(KO)::value, decltype(TW)::value>), dim3(grid_for(sa_n + 1)), dim3(256), 0,
                           0, x->quad_leaves, sa_n, p, base, entries, tb, bl, nb_d, cap);
        hipLaunchKernelGGL(k_pt_big<decltype(TW)::value>, dim3(4096), dim3(256), 0, 0, bl, nb_d, cap, tb,
                           x->quad_leaves, sa_n);
    };
    using std::integral_constant;
    if (tw == 64) fill(std::false_type{}, integral_constant<int, 64>{});
    else if (tw == 32) fill(std::false_type{}, integral_constant<int, 32>{});
    else if (tw == 16) fill(std::false_type{}, integral_constant<int, 16>{});
    else if (x->quad_compact && tw == 5) fill(std::true_type{}, integral_constant<int, 5>{});
    else if (x->quad_compact) fill(std::true_type{}, integral_constant<int, 4>{});
    else if (tw == 5) fill(std::false_type{}, integral_constant<int, 5>{});
    else fill(std::false_type{}, integral_constant<int, 4>{});
    HIP_TRY(hipGetLastError());
    uint64_t nb = 0;
    HIP_TRY(hipMemcpy(&nb, nbig.p, 8, hipMemcpyDeviceToHost));
    if (nb > cap) SAS_FAIL(EFAULT, "prefix table: gap list overflow");  // cannot happen: gaps are disjoint
    x->prefix = t.as<uint8_t>();
    t.release();
    x->prefix_chars = p;
    x->prefix_w = tw;
    x->prefix_key_lo = base;
    x->prefix_entries = entries;
    x->prefix_hi40 = hi40;
    return 0;
}
