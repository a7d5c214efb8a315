// sas_index.hip -- what every unit needs of a built index: the library's error state, its
// scratch pool (sas_scratch_pool), freeing an index, its stats, and copying its arrays out
// (SA, LCP, substrings of the packed text).
#include "build_util.hpp"
#include "build_steps.hpp"

#include <mutex>

// ------------------------------------------------------------------ error state
static thread_local std::string g_err = "ok";

void sas_set_error(int code, const std::string& msg) {
    g_err = "[" + std::to_string(code) + "] " + msg;
}
int sas_errno_of(hipError_t e) {
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return ENOMEM;
    if (e == hipErrorInvalidValue) return EINVAL;
    return EIO;
}
extern "C" const char* sas_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------ scratch pool, free, stats
// The scratch of an exact (variable-size) sharded step comes from a stream-ordered pool
// owned by the index (created on first use, destroyed by sas_free).  Its release threshold
// of "never" keeps freed blocks for the next step; the device's default pool, which other
// libraries in the process share, is left alone.
int sas_scratch_pool(const sas_index* x, hipMemPool_t* out) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (!x->scratch_pool) {
        hipMemPoolProps pp{};
        pp.allocType = hipMemAllocationTypePinned;
        pp.location.type = hipMemLocationTypeDevice;
        pp.location.id = x->device;
        hipMemPool_t pool = nullptr;
        HIP_TRY(hipMemPoolCreate(&pool, &pp));
        uint64_t thr = UINT64_MAX;
        HIP_TRY(hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr));
        x->scratch_pool = pool;
    }
    *out = x->scratch_pool;
    return 0;
}

void free_index(sas_index* x) {
    if (!x) return;
    void* ptrs[] = {x->text_w, x->sa, x->lcp, x->llcp, x->prefix, x->stree, x->rel, x->scratch,
                     x->sec_inner, x->sec_leaves, x->quad_inner, x->quad_leaves, x->tag_table, x->tag_lines, x->tag_ovf,
                     x->tag_first, x->text2_base, x->lay_dev};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    sas_stage_pool_free(x->stage);
    if (x->scratch_pool) {  // its blocks were freed stream-ordered: drain before destroying
        (void)hipSetDevice(x->device);
        (void)hipDeviceSynchronize();
        (void)hipMemPoolDestroy(x->scratch_pool);
    }
    delete x;
}

extern "C" int sas_free(sas_index* index) {
    free_index(index);
    return 0;
}

extern "C" int sas_get_stats(const sas_index* index, sas_stats* out) {
    if (!index || !out) SAS_FAIL(EINVAL, "sas_get_stats: null argument");
    *out = index->stats;
    return 0;
}

// ------------------------------------------------------------------ copy-out
static int copy_out(const void* src, void* dst, uint64_t bytes, uint32_t flags) {
    HIP_TRY(hipMemcpy(dst, src, bytes, (flags & SAS_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sas_copy_sa(const sas_index* index, uint32_t* dst, uint64_t count, uint32_t flags) {
    if (!index || !dst) SAS_FAIL(EINVAL, "sas_copy_sa: null argument");
    if (index->sa_w != 4) SAS_FAIL(EINVAL, "sas_copy_sa: the SA is not u32 (40-bit for n >= 2^32 or SAS_BUILD_SA40, or tagged): use sas_copy_sa64");
    if (count > index->sa_n) SAS_FAIL(EINVAL, "sas_copy_sa: count > number of SA entries");
    return copy_out(index->sa, dst, count * 4, flags);
}

extern "C" int sas_copy_sa_range(const sas_index* index, uint64_t start, uint64_t count, uint32_t* dst,
                                 uint32_t flags) {
    if (!index || (count && !dst)) SAS_FAIL(EINVAL, "sas_copy_sa_range: null argument");
    if (index->sa_w != 4) SAS_FAIL(EINVAL, "sas_copy_sa_range: the SA is not u32 (40-bit or tagged): use sas_copy_sa64");
    if (start < index->rank_lo || start - index->rank_lo + count > index->sa_n)
        SAS_FAIL(EINVAL, "sas_copy_sa_range: ranks outside this index");
    if (count == 0) return 0;
    return copy_out(index->sa + (start - index->rank_lo) * 4, dst, count * 4, flags);
}

// Substrings of the indexed text as byte codes: out[out_off[i] .. + len[i]) = text[pos[i] ..
// + len[i]), read from the packed copy, so a caller may drop its own byte copy of a large
// text after sas_build and still cut queries from it or check answers (the c3 bench).
// One thread per substring; bytes past the text end read 0 (the padding).
__global__ void k_extract(const uint64_t* __restrict__ tw, uint64_t n, const uint64_t* __restrict__ pos,
                          const uint32_t* __restrict__ len, const uint64_t* __restrict__ out_off, uint64_t count,
                          uint8_t* __restrict__ out) {
    GRID_STRIDE(i, count) {
        const uint64_t p = pos[i], o = out_off[i];
        const uint32_t L = len[i];
        for (uint32_t j = 0; j < L; j++) {
            const uint64_t c = p + j;
            out[o + j] = c < n ? (uint8_t)((tw[c >> 5] >> (62 - 2 * (c & 31))) & 3u) : (uint8_t)0;
        }
    }
}

extern "C" int sas_extract(const sas_index* index, const uint64_t* pos, const uint32_t* len, const uint64_t* out_off,
                           uint64_t count, uint8_t* out, void* stream, uint32_t flags) {
    if (!index || (count && (!pos || !len || !out_off || !out))) SAS_FAIL(EINVAL, "sas_extract: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_extract: device pointers only (SAS_DEVICE_PTRS)");
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(index->device));
    hipLaunchKernelGGL(k_extract, dim3(grid_for(count)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       index->text_w, index->n, pos, len, out_off, count, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int W>
__global__ void k_widen_sa(SaView<W> sa, uint64_t start, uint64_t count, uint64_t* __restrict__ out) {
    GRID_STRIDE(i, count) out[i] = sa[start + i];
}

// SAS_BUILD_TAG_LINES: SA[r] from the line of r's bucket (the last bucket whose first rank is
// <= r: a binary search over the first-rank table), its slot or its overflow entry
__global__ void k_tl_sa(const uint64_t* __restrict__ lines, const uint64_t* __restrict__ ovf,
                        const uint64_t* __restrict__ first, uint64_t keys, uint32_t sb, uint64_t start, uint64_t count,
                        uint64_t* __restrict__ out) {
    GRID_STRIDE(i, count) out[i] = tl_sa_at(lines, ovf, first, keys, sb, start + i);
}

extern "C" int sas_copy_sa64(const sas_index* index, uint64_t start, uint64_t count, uint64_t* dst, uint32_t flags) {
    if (!index || (count && !dst)) SAS_FAIL(EINVAL, "sas_copy_sa64: null argument");
    if (start < index->rank_lo || start - index->rank_lo + count > index->sa_n)
        SAS_FAIL(EINVAL, "sas_copy_sa64: ranks outside this index");
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(index->device));
    DevBuf tmp;
    uint64_t* out = dst;
    if (!(flags & SAS_DEVICE_PTRS)) {
        TRY(tmp.alloc(count * 8, "sa64 staging"));
        out = tmp.as<uint64_t>();
    }
    uint64_t s0 = start - index->rank_lo;
    if (index->tag_lines)
        hipLaunchKernelGGL(k_tl_sa, dim3(grid_for(count)), dim3(256), 0, 0, index->tag_lines, index->tag_ovf,
                           index->tag_first, 1ull << (2 * index->tag_p), index->tag_sb, s0, count, out);
    else if (index->sa_w == 8)
        hipLaunchKernelGGL(k_widen_sa<8>, dim3(grid_for(count)), dim3(256), 0, 0, SaView<8>{index->sa}, s0, count, out);
    else
        with_sa_w(index->sa_w, [&](auto Wc) {
            constexpr int W = decltype(Wc)::value;
            hipLaunchKernelGGL(k_widen_sa<W>, dim3(grid_for(count)), dim3(256), 0, 0, SaView<W>{index->sa}, s0, count, out);
        });
    HIP_TRY(hipGetLastError());
    if (!(flags & SAS_DEVICE_PTRS)) HIP_TRY(hipMemcpy(dst, out, count * 8, hipMemcpyDeviceToHost));
    else HIP_TRY(hipDeviceSynchronize());
    return 0;
}

extern "C" int sas_copy_lcp(const sas_index* index, uint32_t* dst, uint64_t count, uint32_t flags) {
    if (!index || !dst) SAS_FAIL(EINVAL, "sas_copy_lcp: null argument");
    if (!index->lcp) SAS_FAIL(EINVAL, "sas_copy_lcp: index built without SAS_BUILD_LCP");
    if (count > index->sa_n) SAS_FAIL(EINVAL, "sas_copy_lcp: count > number of SA entries");
    return copy_out(index->lcp, dst, count * 4, flags);
}
