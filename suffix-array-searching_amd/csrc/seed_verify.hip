// seed_verify.hip -- the stages that every seed-and-verify call runs, defined once
// (seed_verify.hpp declares them): the index preconditions, the seed stage up to the candidate
// offsets and the call path of the two-pass calls.
#include "seed_verify.hpp"

static_assert(SAS_MM_TRUNCATED == SAS_ED_TRUNCATED && SAS_MM_SHORT == SAS_ED_SHORT,
              "k_seed_gate writes one set of flag bits for sas_locate_mismatch and sas_locate_edit");

int seed_index_checks(const std::string& w, const sas_index* x, uint32_t k, uint32_t flags, void* stream, bool probe) {
    if (!x) SAS_FAIL(EINVAL, w + ": null index");
    if (k > MM_MAX_K) SAS_FAIL(EINVAL, w + ": k must be 0.." + std::to_string(MM_MAX_K));
    if (x->tag_lines || x->sa_w == 8)
        SAS_FAIL(ENOTSUP, w + ": a tagged index (SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES) is not served");
    if (x->rank_lo != 0 || x->sa_n != x->n)
        SAS_FAIL(ENOTSUP, w + ": needs a whole index (a shard or part holds only a rank range of the SA)");
    if (!x->sa || (x->sa_w != 4 && x->sa_w != 5)) SAS_FAIL(ENOTSUP, w + ": needs a u32 or packed 40-bit SA array");
    if ((flags & SAS_LOCATE_U32) && x->n >= (1ull << 32))
        SAS_FAIL(EINVAL, w + ": SAS_LOCATE_U32 needs a text of n < 2^32 chars");
    // the range search's own requirements (its error is passed on)
    if (probe) TRY(sas_search_range_fixed(x, nullptr, 1, 0, nullptr, nullptr, stream, flags & SAS_DEVICE_PTRS));
    return 0;
}

__global__ void k_mm_pieces(MmQueries Q, uint32_t kp1, uint64_t* __restrict__ poff, uint32_t* __restrict__ plen) {
    GRID_STRIDE(i, Q.nq * kp1) {
        const uint64_t q = i / kp1;
        const uint32_t j = (uint32_t)(i - q * kp1), m = Q.len(q);
        const uint32_t b0 = mm_piece_start(j, m, kp1), b1 = mm_piece_start(j + 1, m, kp1);
        poff[i] = Q.off(q) + b0;
        plen[i] = b1 - b0;
    }
}

// One thread per query: skipped seeds, short queries (m <= k) and long ones (m > max_m) lose
// their ranges
__global__ void k_seed_gate(MmQueries Q, uint32_t kp1, uint64_t max_seed_hits, uint32_t max_m,
                            uint64_t* __restrict__ lo, uint64_t* __restrict__ hi, uint16_t* __restrict__ skip,
                            uint8_t* __restrict__ qflags) {
    GRID_STRIDE(q, Q.nq) {
        const uint32_t m = Q.len(q);
        uint32_t mask = 0, fl = m < kp1 ? SAS_ED_SHORT : (m > max_m ? SAS_ED_LONG : 0u);
        const bool none = fl != 0;
        for (uint32_t j = 0; j < kp1; j++) {
            const uint64_t i = q * kp1 + j;
            const uint64_t cnt = hi[i] > lo[i] ? hi[i] - lo[i] : 0;
            const bool over = !none && max_seed_hits && cnt > max_seed_hits;
            if (over) fl |= SAS_ED_TRUNCATED;
            if (over || none) {
                mask |= 1u << j;
                lo[i] = 0;
                hi[i] = 0;
            }
        }
        if (skip) skip[q] = (uint16_t)mask;
        qflags[q] = (uint8_t)fl;
    }
}

int seed_alloc(const sas_index* x, uint64_t np, hipStream_t st, SeedState& s) {
    TRY(sas_scratch_pool(x, &s.pool));
    TRY(s.poff.alloc(s.pool, np * 8, st));
    TRY(s.plen.alloc(s.pool, np * 4, st));
    TRY(s.lohi.alloc(s.pool, np * 16, st));
    TRY(s.coff.alloc(s.pool, (np + 1) * 8, st));
    s.lo = s.lohi.as<uint64_t>();
    s.hi = s.lo + np;
    return 0;
}

int seed_ranges(const sas_index* x, const uint8_t* qbytes, uint64_t np, hipStream_t st, uint32_t flags, SeedState& s) {
    const uint32_t rflags = (flags & (SAS_NO_PREFIX_TABLE | SAS_VALIDATE)) | SAS_DEVICE_PTRS;
    return sas_search_range(x, qbytes, s.poff.as<uint64_t>(), s.plen.as<uint32_t>(), np, s.lo, s.hi, st, rflags);
}

int seed_offsets(const sas_index* x, uint64_t np, hipStream_t st, SeedState& s) {
    return sas_locate_offsets(x, s.lo, s.hi, np, 0, s.coff.as<uint64_t>(), st, SAS_DEVICE_PTRS);
}

int seed_candidates(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t max_m,
                    bool skip_mask, uint8_t* qflags, hipStream_t st, uint32_t flags, SeedState& s) {
    const uint32_t kp1 = k + 1;
    const uint64_t nq = Q.nq, np = nq * kp1;
    TRY(seed_alloc(x, np, st, s));
    if (skip_mask) TRY(s.skip.alloc(s.pool, nq * 2, st));
    if (!qflags) {
        TRY(s.qfl.alloc(s.pool, nq, st));
        qflags = s.qfl.as<uint8_t>();
    }
    hipLaunchKernelGGL(k_mm_pieces, seed_grid(x, np), dim3(256), 0, st, Q, kp1, s.poff.as<uint64_t>(),
                       s.plen.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    TRY(seed_ranges(x, Q.qbytes, np, st, flags, s));
    hipLaunchKernelGGL(k_seed_gate, seed_grid(x, nq), dim3(256), 0, st, Q, kp1, max_seed_hits, max_m, s.lo, s.hi,
                       s.skip.as<uint16_t>(), qflags);
    HIP_TRY(hipGetLastError());
    return seed_offsets(x, np, st, s);
}

int seed_list_call(const ListCall& c, const sas_index* x, const QueryArgs& q, uint64_t nq, uint64_t* out_off,
                   uint8_t* out_qflags, const ListOut* outs, int nouts, uint64_t capacity, uint64_t* out_total,
                   void* stream, uint32_t flags, const ListPrepare& prepare, const ListScatter& scatter) {
    const bool dev = (flags & SAS_DEVICE_PTRS) != 0;
    const std::string fn(c.fn);
    if (nouts > HostOutputs::MAX) SAS_FAIL(EINVAL, fn + ": more payload outputs than HostOutputs holds");
    bool null = !out_off || !q.null_ok(nq) || (!dev && !out_total);
    void* out[HostOutputs::MAX];
    for (int i = 0; i < nouts; i++) {
        null = null || (capacity && outs[i].required && !outs[i].ptr);
        out[i] = outs[i].ptr;
    }
    if (null) SAS_FAIL(EINVAL, fn + ": null argument");
    if (c.check) TRY(c.check());
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq == 0) {
        if (dev) return seed_nothing(out_off, 0, out_total, st);
        out_off[0] = 0;
        *out_total = 0;
        return 0;
    }
    if (dev) {
        TRY(prepare(q.device(nq), out_off, out_qflags, out_total, st, flags));
        return scatter(out, capacity, st);
    }
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated)
    const std::string l(c.label);
    HostQueries hq;
    HostOutputs ho;
    MmQueries Q;
    TRY(hq.stage(c.label, q, nq, st, &Q));
    uint64_t *doff, total;
    uint8_t* dfl;
    TRY(ho.twin(out_off, (nq + 1) * 8, (l + " result offsets").c_str(), &doff));
    TRY(ho.twin(out_qflags, nq, (l + " query flags").c_str(), &dfl));
    TRY(prepare(Q, doff, dfl, nullptr, st, flags | SAS_VALIDATE));
    TRY(host_list_total(ho, st, fn, c.noun, c.hint, out_off, nq, capacity, out_total, &total));
    if (total == 0) return 0;
    for (int i = 0; i < nouts; i++) TRY(ho.twin_bytes(outs[i].ptr, total * outs[i].esz, outs[i].label, &out[i]));
    TRY(scatter(out, total, st));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
