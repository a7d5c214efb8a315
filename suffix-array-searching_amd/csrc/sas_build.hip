// sas_build.hip -- index construction, the sas_build* entry points.
//
// Replaces SaNaive::build (sas/sa_search.rs:30-57): the reference calls libsais
// (sais64::parallel::sais, :33), casts to u32 (:35), asserts adjacent suffixes increase
// (:36-38) and fills a (dead, p = 0) prefix table (:59-74).  Here everything is built on the
// GPU into HBM, and build_impl is the sequence of its stages:
//   1. the text to 2 bits/char: packed from byte codes (k_pack_text, rejects codes > 3) or
//      generated into the words (build_gen.hip),
//   2. the suffix array: one part's rank range (sas_build40.hip), the caller's (load_sa), or
//      built here (build_sa.hip: u32; sas_build40.hip: packed 40-bit); then a shard's cut of it,
//   3. the structures the flags ask for, each a build_* step of the unit that owns its kernels
//      (build_steps.hpp): LCP, LLCP, S-tree, sector tree, quad tree, prefix table, the pivot
//      blocks, the tagged SA or the bucket lines,
//   4. the stats.
#include "build_util.hpp"
#include "build_steps.hpp"

#include <chrono>

// ------------------------------------------------------------------ text packing
__global__ void k_pack_text(const uint8_t* __restrict__ text, uint64_t n, uint64_t* __restrict__ tw,
                            uint64_t words, uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    GRID_STRIDE(w, words) {
        uint64_t base = w * 32;
        uint64_t v = 0;
        if (base < n) {
            uint32_t m = n - base < 32 ? (uint32_t)(n - base) : 32;
            v = pack_query_word(text + base, m, 0, &b);
        }
        tw[w] = v;
    }
    if (b) atomicOr(bad, 1u);
}

// Stage 1: the text as packed words, from byte codes (host or device) or generated (gen)
static int pack_text(sas_index* x, const uint8_t* text, bool dev, const ChaKey* gen) {
    const uint64_t n = x->n;
    DevBuf tbytes, bad, tw;
    x->text_words = (n + 31) / 32 + SAS_TEXT_PAD_WORDS;
    TRY(tw.alloc(x->text_words * 8, "packed text"));
    if (gen) {
        TRY(gen_packed_text(*gen, n, tw.as<uint64_t>(), x->text_words));
    } else {
        const uint8_t* dtext = text;
        if (!dev) {
            TRY(tbytes.alloc(n, "text bytes"));
            HIP_TRY(hipMemcpy(tbytes.p, text, n, hipMemcpyHostToDevice));
            dtext = tbytes.as<uint8_t>();
        }
        TRY(bad.alloc(4, "flag"));
        HIP_TRY(hipMemset(bad.p, 0, 4));
        hipLaunchKernelGGL(k_pack_text, dim3(grid_for(x->text_words)), dim3(256), 0, 0, dtext, n, tw.as<uint64_t>(),
                           x->text_words, bad.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        uint32_t hbad = 0;
        HIP_TRY(hipMemcpy(&hbad, bad.p, 4, hipMemcpyDeviceToHost));
        if (hbad) SAS_FAIL(EINVAL, "sas_build: text bytes must be DNA codes 0..3");
        tbytes.alloc(0, "free");
    }
    x->text_w = tw.as<uint64_t>();
    tw.release();
    return 0;
}

// ------------------------------------------------------------------ the suffix array
static uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int copy_in_sa(const void* src, uint8_t* dst, uint64_t bytes, bool dev) {
    HIP_TRY(hipMemcpy(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return 0;
}

// Caller's SA (host or device, 4 / 5 / 8 bytes per entry) -> this index's width.  A narrowing
// store drops the high bits, so the range check is made here, on the caller's own value
// (bad, if given: bit 0 for an entry >= n); verify_sa only ever sees the stored one.
template <int WI, int WO>
__global__ void k_convert_sa(const uint8_t* __restrict__ in, uint64_t n, uint8_t* __restrict__ out,
                             uint32_t* __restrict__ bad) {
    GRID_STRIDE(i, n) {
        uint64_t v;
        if (WI == 8) v = reinterpret_cast<const uint64_t*>(in)[i];
        else v = SaView<WI>{in}[i];
        if (bad && v >= n) atomicOr(bad, 1u);
        sa_put<WO>(out, i, v);
    }
}

// check (SAS_BUILD_VERIFY): fail on an entry >= n at the caller's width.  Equal widths are a
// plain copy: verify_sa reads every bit of those.
static int load_sa(const void* src, uint64_t n, int wi, bool dev, uint8_t* dst, uint32_t wo, bool check) {
    const uint64_t bytes = n * (uint64_t)wi;
    if ((uint32_t)wi == wo)
        return copy_in_sa(src, dst, bytes, dev);
    DevBuf staged, bad;
    TRY(staged.alloc(bytes + 8, "caller SA staging"));
    TRY(copy_in_sa(src, staged.as<uint8_t>(), bytes, dev));
    uint32_t* flag = nullptr;
    if (check) {
        TRY(bad.alloc(4, "caller SA range flag"));
        HIP_TRY(hipMemset(bad.p, 0, 4));
        flag = bad.as<uint32_t>();
    }
    const uint8_t* in = staged.as<uint8_t>();
    const dim3 g(grid_for(n)), b(256);
    if (wi == 4 && wo == 5) hipLaunchKernelGGL((k_convert_sa<4, 5>), g, b, 0, 0, in, n, dst, flag);
    else if (wi == 5 && wo == 4) hipLaunchKernelGGL((k_convert_sa<5, 4>), g, b, 0, 0, in, n, dst, flag);
    else if (wi == 8 && wo == 4) hipLaunchKernelGGL((k_convert_sa<8, 4>), g, b, 0, 0, in, n, dst, flag);
    else hipLaunchKernelGGL((k_convert_sa<8, 5>), g, b, 0, 0, in, n, dst, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (check) {
        uint32_t h = 0;
        HIP_TRY(hipMemcpy(&h, bad.p, 4, hipMemcpyDeviceToHost));
        if (h & 1) SAS_FAIL(EINVAL, "suffix array holds an entry >= n");
    }
    return 0;
}

// Stage 2, part mode: only this part's SA rank range is ever built (sas_build40.hip)
static int sa_of_part(sas_index* x, uint32_t part, uint32_t parts, uint32_t flags) {
    uint64_t s0 = now_ns(), lo = 0, cnt = 0, np = 0;
    uint8_t* local = nullptr;
    TRY(build_sa_part40(x->text_w, x->n, part, parts, &local, &lo, &cnt, &np, &x->stats.sa_rounds));
    x->sa = local;
    x->rank_lo = lo;
    x->sa_n = cnt;
    x->next_pos = np;
    HIP_TRY(hipDeviceSynchronize());
    x->stats.build_sa_ns = now_ns() - s0;
    if (flags & SAS_BUILD_VERIFY) TRY(verify_sa(x->text_w, x->n, x->sa, x->sa_w, x->sa_n, false));
    return 0;
}

// Stage 2 otherwise: the global suffix array (caller's or built here), then this index's rank
// range [rank_lo, rank_hi) of it
static int sa_of_text(sas_index* x, const void* sa_or_null, int sa_width, uint32_t flags, uint64_t rank_lo,
                      uint64_t rank_hi) {
    const uint64_t n = x->n;
    const uint32_t W = x->sa_w;
    DevBuf sa;
    // 40-bit: the pair loads' pad; u32: PLAIN's SA run loads the 16-B chunks covering its ranks
    const uint64_t sa_bytes_full = n * W + (W == 5 ? SAS_SA40_PAD : 16);
    TRY(sa.alloc(sa_bytes_full, "suffix array"));
    if (sa_or_null) {
        TRY(load_sa(sa_or_null, n, sa_width, flags & SAS_DEVICE_PTRS, sa.as<uint8_t>(), W,
                    (flags & SAS_BUILD_VERIFY) != 0));
    } else {
        uint64_t s0 = now_ns();
        if (W == 5) {
            HIP_TRY(hipMemset(sa.p, 0, sa_bytes_full));
            uint64_t buckets = 0;
            TRY(build_sa_gpu40(x->text_w, n, sa.as<uint8_t>(), &x->stats.sa_rounds, &buckets));
        } else {
            TRY(build_sa_gpu(x->text_w, n, sa.as<uint32_t>(), &x->stats.sa_rounds, flags & SAS_BUILD_WIDE));
        }
        HIP_TRY(hipDeviceSynchronize());
        x->stats.build_sa_ns = now_ns() - s0;
    }
    if (flags & SAS_BUILD_VERIFY) TRY(verify_sa(x->text_w, n, sa.as<uint8_t>(), W, n, true));
    if (rank_hi < n) {
        uint8_t b[8] = {};
        HIP_TRY(hipMemcpy(b, sa.as<uint8_t>() + rank_hi * W, W, hipMemcpyDeviceToHost));
        uint64_t np = 0;
        for (uint32_t k = 0; k < W; k++) np |= (uint64_t)b[k] << (8 * k);
        x->next_pos = np;
    } else {
        x->next_pos = n;
    }
    if (x->sa_n == n) {
        x->sa = static_cast<uint8_t*>(sa.release());
    } else {
        DevBuf part;
        const uint64_t pb = x->sa_n * W + (W == 5 ? SAS_SA40_PAD : 16);
        TRY(part.alloc(pb, "suffix array shard"));
        HIP_TRY(hipMemset(part.p, 0, pb));
        HIP_TRY(hipMemcpy(part.p, sa.as<uint8_t>() + rank_lo * W, x->sa_n * W, hipMemcpyDeviceToDevice));
        sa.alloc(0, "free");
        x->sa = static_cast<uint8_t*>(part.release());
    }
    return 0;
}

// ------------------------------------------------------------------ build_impl
static int check_args(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width, uint32_t flags,
                      uint64_t rank_lo, uint64_t rank_hi, const ChaKey* gen) {
    if (n == 0) SAS_FAIL(EINVAL, "sas_build: empty text");
    if (!text && !gen) SAS_FAIL(EINVAL, "sas_build: null text");
    if (n >= SAS_SA40_MAX - 64) SAS_FAIL(ENOTSUP, "sas_build: n >= 2^40 - 64");
    if (sa_or_null && sa_width != 4 && sa_width != 5 && sa_width != 8)
        SAS_FAIL(EINVAL, "sas_build: sa_width must be 4 (u32), 5 (packed 40-bit) or 8 (u64)");
    if (sa_or_null && sa_width == 4 && n > 0xFFFFFFFFull) SAS_FAIL(EINVAL, "sas_build: a u32 SA cannot index n >= 2^32");
    if (rank_lo >= rank_hi || rank_hi > n) SAS_FAIL(EINVAL, "sas_build_shard: empty or out-of-range rank range");
    if ((flags & SAS_BUILD_TAGGED) &&
        (flags & (SAS_BUILD_STREE | SAS_BUILD_SECTOR | SAS_BUILD_QUAD | SAS_BUILD_QUAD_COMPACT | SAS_BUILD_LLCP |
                  SAS_BUILD_PREFIX | SAS_BUILD_PREFIX_INLINE | SAS_BUILD_PREFIX_INLINE2 | SAS_BUILD_PREFIX_INLINE4)))
        SAS_FAIL(ENOTSUP, "SAS_BUILD_TAGGED replaces the SA: it combines with SAS_BUILD_LCP only, not with the "
                          "trees, LLCP or the prefix tables");
    // a bucket-line index serves SAS_ALGO_TAGGED only (no SA array): an LCP array, or the
    // binary-search pivot array, would be HBM nothing reads (64 GiB of LCP at n = 2^34)
    if ((flags & SAS_BUILD_TAG_LINES) && !(flags & SAS_BUILD_TAGGED))
        SAS_FAIL(EINVAL, "SAS_BUILD_TAG_LINES needs SAS_BUILD_TAGGED");
    if ((flags & SAS_BUILD_TAG_LINES) && (flags & (SAS_BUILD_LCP | SAS_BUILD_LLCP)))
        SAS_FAIL(ENOTSUP, "SAS_BUILD_TAG_LINES serves SAS_ALGO_TAGGED only: no LCP array");
    return 0;
}

// Stage 3: the structures the flags ask for, over the index's text and SA
static int build_structures(sas_index* x, uint32_t flags) {
    const uint32_t p = (flags >> 16) & 31;  // SAS_BUILD_PREFIX_P: chars of the prefix / bucket table, 0 = from sa_n
    if (flags & (SAS_BUILD_LCP | SAS_BUILD_LLCP)) TRY(build_lcp(x));
    if (flags & SAS_BUILD_LLCP) TRY(build_llcp(x));
    if (flags & SAS_BUILD_STREE) TRY(build_stree(x));
    if (flags & SAS_BUILD_SECTOR) TRY(build_sector(x));
    if (flags & (SAS_BUILD_QUAD | SAS_BUILD_QUAD_COMPACT))
        TRY(build_quad(x, (flags & SAS_BUILD_QUAD_COMPACT) != 0, flags & (SAS_BUILD_QUAD_ABS | SAS_BUILD_QUAD_REL)));
    if (flags & (SAS_BUILD_PREFIX | SAS_BUILD_PREFIX_INLINE | SAS_BUILD_PREFIX_INLINE2 | SAS_BUILD_PREFIX_INLINE4))
        TRY(build_prefix(x, p,
                         (flags & SAS_BUILD_PREFIX_INLINE4)   ? 4u
                         : (flags & SAS_BUILD_PREFIX_INLINE2) ? 2u
                         : (flags & SAS_BUILD_PREFIX_INLINE)  ? 1u : 0u));
    // the binary search's pivots (not for a bucket-line index: TAGGED never reads them)
    x->iters = 64 - __builtin_clzll(x->sa_n);  // ilog2(len) + 1 (sas/sa_search.rs:171)
    if (!(flags & SAS_BUILD_TAG_LINES)) TRY(build_rel(x, (flags >> 27) & 31u));
    if ((flags & SAS_BUILD_TAGGED) && (flags & SAS_BUILD_TAG_LINES)) TRY(build_tag_lines(x, p));
    else if (flags & SAS_BUILD_TAGGED) TRY(build_tagged(x, p));
    return 0;
}

// Stage 4.  t0: when the build began
static void fill_stats(sas_index* x, uint64_t t0) {
    const uint64_t sa_n = x->sa_n;
    sas_stats& st = x->stats;
    st.n = x->n;
    st.text_bytes = x->text_words * 8;
    st.sa_bytes = x->tag_lines ? x->tag_ovf_n * 8 : sa_n * x->sa_w;  // bucket lines: the overflow array
    st.sa_width = x->sa_w;
    st.lcp_bytes = x->lcp ? sa_n * 4 : 0;
    st.llcp_bytes = x->llcp ? sa_n * 16 : 0;
    st.prefix_bytes = x->prefix ? x->prefix_entries * x->prefix_w : 0;
    st.prefix_chars = x->prefix_chars;
    st.prefix_key_lo = x->prefix ? x->prefix_key_lo : 0;
    st.prefix_entries = x->prefix ? x->prefix_entries : 0;
    st.stree_bytes = x->stree_nodes * 64;
    st.stree_layers = x->stree_height;
    st.stree_lds_layers = x->stree_lds_layers;
    st.top_levels = x->rel ? x->rel_lay.levels < SAS_REL_LDS_LEVELS ? x->rel_lay.levels : SAS_REL_LDS_LEVELS : 0;
    st.iterations = x->iters;
    st.rank_lo = x->rank_lo;
    st.sa_entries = sa_n;
    st.next_pos = x->next_pos;
    st.sector_bytes = (x->sec_inner_nodes + x->sec_leaf_count) * 32;
    st.sector_layers = x->sec_leaves ? x->sec_inner_layers + 1 : 0;
    st.sector_lds_layers = x->sec_lds_layers;
    st.quad_bytes = (x->quad_inner_nodes + x->quad_leaf_count) * 64;
    st.quad_layers = x->quad_leaves ? x->quad_inner_layers + 1 : 0;
    st.quad_lds_layers = x->quad_lds_layers;
    st.quad_entry_bytes = x->quad_leaves ? (x->quad_compact ? 8 : 16) : 0;
    st.quad_fan = x->quad_leaves ? x->quad_fan : 0;
    st.top2_levels = x->rel ? x->rel_lay.levels : 0;
    st.tag_chars = x->tag_p;
    st.tag_table_bytes = x->tag_table   ? ((1ull << (2 * x->tag_p)) + 1) * 8
                         : x->tag_lines ? (1ull << (2 * x->tag_p)) * 128 + ((1ull << (2 * x->tag_p)) + 1) * 8 : 0;
    st.tag_line_slots = x->tag_lines ? SAS_TL_SLOTS : 0;
    st.tag_line_tag_bits = x->tag_lines ? tl_tag_bits(x->tag_sb) : 0;
    st.text2_bytes = x->text2 ? x->text_words * 8 : 0;
    st.tag_overflow_entries = x->tag_ovf_n;
    st.top2_bytes = 0;  // round 4: every pivot level is in the rel blocks
    st.rel_levels = x->rel ? x->rel_lay.levels : 0;
    st.rel_bytes = x->rel ? x->rel_lay.bytes : 0;
    st.index_bytes = st.text_bytes + st.sa_bytes + st.lcp_bytes + st.llcp_bytes + st.prefix_bytes + st.stree_bytes +
                     st.sector_bytes + st.quad_bytes + st.tag_table_bytes + st.text2_bytes + st.top2_bytes +
                     st.rel_bytes;
    st.build_total_ns = now_ns() - t0;
}

// Common builder.  [rank_lo, rank_hi) = the SA ranks this index holds (the whole SA for
// sas_build, a shard's range for sas_build_shard); parts > 0: part `part` of the SA
// (sas_build_part); gen: the text is random_string(n) of this key, not `text`
static int build_impl(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width, uint32_t flags,
                      uint64_t rank_lo, uint64_t rank_hi, sas_index** out, uint32_t part = 0, uint32_t parts = 0,
                      const ChaKey* gen = nullptr) {
    if (!out) SAS_FAIL(EINVAL, "sas_build: null out");
    *out = nullptr;
    TRY(check_args(text, n, sa_or_null, sa_width, flags, rank_lo, rank_hi, gen));
    const uint64_t t0 = now_ns();
    sas_index* x = new sas_index();
    x->n = n;
    x->rank_lo = rank_lo;
    x->sa_n = rank_hi - rank_lo;
    x->sa_w = ((flags & SAS_BUILD_SA40) || n >= (1ull << 32) - 64 || parts > 0) ? 5 : 4;
    HIP_TRY(hipGetDevice(&x->device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, x->device) == hipSuccess) x->num_cus = prop.multiProcessorCount;
    struct Guard { sas_index*& p; ~Guard() { if (p) free_index(p); } } guard{x};

    TRY(pack_text(x, text, flags & SAS_DEVICE_PTRS, gen));
    if (parts > 0) TRY(sa_of_part(x, part, parts, flags));
    else TRY(sa_of_text(x, sa_or_null, sa_width, flags, rank_lo, rank_hi));
    TRY(build_structures(x, flags));
    HIP_TRY(hipMalloc(&x->scratch, 64));
    HIP_TRY(hipMemset(x->scratch, 0, 64));
    HIP_TRY(hipDeviceSynchronize());
    fill_stats(x, t0);
    *out = x;
    x = nullptr;  // disarm guard
    return 0;
}

extern "C" int sas_build(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width, uint32_t flags,
                         sas_index** out) {
    return build_impl(text, n, sa_or_null, sa_width, flags, 0, n, out);
}

extern "C" int sas_build_shard(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width,
                               uint64_t rank_lo, uint64_t rank_hi, uint32_t flags, sas_index** out) {
    return build_impl(text, n, sa_or_null, sa_width, flags, rank_lo, rank_hi, out);
}

extern "C" int sas_build_part(const uint8_t* text, uint64_t n, uint32_t part, uint32_t parts, uint32_t flags,
                              sas_index** out) {
    if (parts == 0 || part >= parts) SAS_FAIL(EINVAL, "sas_build_part: need part < parts");
    return build_impl(text, n, nullptr, 5, flags, 0, n, out, part, parts);
}

extern "C" int sas_build_gen(uint64_t seed, uint64_t n, uint32_t flags, sas_index** out) {
    ChaKey key;
    gen_key(seed, &key);
    return build_impl(nullptr, n, nullptr, 4, flags & ~SAS_DEVICE_PTRS, 0, n, out, 0, 0, &key);
}

extern "C" int sas_build_part_gen(uint64_t seed, uint64_t n, uint32_t part, uint32_t parts, uint32_t flags,
                                  sas_index** out) {
    if (parts == 0 || part >= parts) SAS_FAIL(EINVAL, "sas_build_part_gen: need part < parts");
    ChaKey key;
    gen_key(seed, &key);
    return build_impl(nullptr, n, nullptr, 5, flags & ~SAS_DEVICE_PTRS, 0, n, out, part, parts, &key);
}
