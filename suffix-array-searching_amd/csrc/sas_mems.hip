// sas_mems.hip -- maximal exact matches of every query, by seed and extend (sas.h: sas_mems,
// sas_mems_fixed).
//
// A match (i, j, len) of at least L chars starts with the window p[i .. i + L) of the query, so
// the occurrences of the windows of all query offsets are the only candidates, and a candidate is
// a maximal match exactly when it cannot be extended to the left; its length is how far it
// extends to the right:
//
//   1. k_mem_count     windows per query: m - L + 1, or one window of all m chars for a query
//                      with m < L (it finds nothing: the gate empties it; its bytes are validated
//                      with the others); writes SAS_MEM_SHORT.  A scan gives the first window of
//                      every query; a ragged batch reads the window total back (a fixed-length
//                      batch computes it);
//      k_mem_windows   offsets and lengths of the windows (they overlap in the caller's bytes,
//                      which the range search takes) and, for a ragged batch, each window's query;
//   2. sas_search_range over all windows: their SA rank ranges;
//   3. k_mem_gate      one thread per window: empties the range of a window that occurs more than
//                      max_hits times (its query gets SAS_MEM_TRUNCATED) and of a short query's;
//   4. sas_locate_offsets on the gated ranges: the candidate offsets (the scratch, 2 and 4 are
//                      seed_verify.hip's, shared with the approximate calls); the host reads the
//                      candidate total C;
//   5. k_mem_verify    output-centric over the C candidates (mm_tile_candidates: tiles of MM_T,
//                      owners bisected in LDS, all SA reads of a thread issued before the first
//                      use).  Candidate = (window (q, i), j = SA[rank]).  First the rejections,
//                      which read one text char and one query byte and no window of text: the
//                      left chars of all candidates of a thread are requested together; a
//                      candidate with p[i - 1] = t[j - 1] is part of the match that starts one
//                      char earlier and ends here (in a long match all candidates but one); a
//                      window that leaves the text, or with a layout (template bool LAY) does not
//                      lie inside one segment (one bisect), is none.  The others extend to the
//                      right from L, 32 chars a step (text_chars32 against pack_query_word, XOR,
//                      count-leading-zeros: mem_extend.hpp), the last word masked to the bound
//                      min(m - i, hi - j).  With UNIQ the two SA neighbours of the candidate's
//                      rank are compared with it, text against text, over len chars.  One verdict
//                      per candidate: len, or 0 (no match has length 0: L >= 1), j and i beside it;
//   6. rocprim exclusive scan of the accept flags, k_mem_offsets (out_off[q] = the scan at the
//      first candidate of query q's first window) and k_mem_scatter (bounded by capacity).
//      Order is kept: (query offset, SA rank).
#include "mem_extend.hpp"
#include "seed_verify.hpp"

#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>

// windows of a query of m chars
__host__ __device__ __forceinline__ uint64_t mem_windows_of(uint32_t m, uint32_t L) {
    return m >= L ? (uint64_t)(m - L) + 1 : 1;
}

// wcnt[q] = windows of query q (0 at nq: the scan's total); the SHORT flag
__global__ void k_mem_count(MmQueries Q, uint32_t L, uint64_t* __restrict__ wcnt, uint8_t* __restrict__ qflags) {
    GRID_STRIDE(q, Q.nq + 1) {
        if (q == Q.nq) {
            if (wcnt) wcnt[q] = 0;
            continue;
        }
        const uint32_t m = Q.len(q);
        if (wcnt) wcnt[q] = mem_windows_of(m, L);
        qflags[q] = m < L ? SAS_MEM_SHORT : 0;
    }
}

// The windows as the kernels address them: woff (ragged batch: first window per query, nq + 1;
// every query has at least one, so no two are equal) or `per` windows for each query
struct MemWindows {
    const uint64_t* woff;
    uint64_t per;
    uint64_t nw;
    __device__ __forceinline__ uint64_t first(uint64_t q) const { return woff ? woff[q] : q * per; }
};

__global__ void k_mem_windows(MmQueries Q, uint32_t L, MemWindows W, uint64_t* __restrict__ poff,
                              uint32_t* __restrict__ plen, uint64_t* __restrict__ wq) {
    GRID_STRIDE(w, W.nw) {
        const uint64_t q = W.woff ? csr_owner_of(W.woff, Q.nq, w) : w / W.per;
        const uint32_t m = Q.len(q);
        poff[w] = Q.off(q) + (w - W.first(q));
        plen[w] = m < L ? m : L;
        if (wq) wq[w] = q;
    }
}

// One thread per window.  Every writer of a query's flag byte writes the same value (a short
// query has one window and is never truncated), after k_mem_count's on the stream
__global__ void k_mem_gate(MmQueries Q, uint32_t L, MemWindows W, const uint64_t* __restrict__ wq, uint64_t max_hits,
                           uint64_t* __restrict__ lo, uint64_t* __restrict__ hi, uint8_t* __restrict__ qflags) {
    GRID_STRIDE(w, W.nw) {
        const uint64_t q = wq ? wq[w] : w / W.per;
        const bool none = Q.len(q) < L;
        const uint64_t cnt = hi[w] > lo[w] ? hi[w] - lo[w] : 0;
        const bool over = !none && max_hits && cnt > max_hits;
        if (over) qflags[q] = SAS_MEM_TRUNCATED;
        if (over || none) {
            lo[w] = 0;
            hi[w] = 0;
        }
    }
}

struct MemArgs {
    const uint64_t* tw;
    uint64_t n;
    const uint8_t* sa;
    MmQueries Q;
    uint32_t L;
    MemWindows W;
    const uint64_t* wq;     // ragged batch: the query of every window
    const uint64_t* lo;     // gated first rank per window
    const uint64_t* coff;   // candidate offsets, nw + 1
    uint64_t C;             // candidates
    LayoutView lay;         // LAY: the index's sequence layout
    uint32_t* verdict;      // per candidate: the match length, or 0
    uint64_t* cpos;         // per accepted candidate: j
    uint32_t* cqpos;        // per accepted candidate: i
};

// lcp(t[a ..], t[b ..]) >= len, for b + len <= n: a suffix that ends before len chars is shorter
__device__ __forceinline__ bool mem_same_prefix(const uint64_t* __restrict__ tw, uint64_t n, uint64_t a, uint64_t b,
                                                uint64_t len) {
    if (a + len > n) return false;
    for (uint64_t off = 0; off < len; off += 32) {
        const uint32_t c = len - off < 32 ? (uint32_t)(len - off) : 32u;
        if (mem_first_diff(text_chars32(tw, a + off), text_chars32(tw, b + off), c) != c) return false;
    }
    return true;
}

template <int W, bool LAY, bool UNIQ>
__global__ __launch_bounds__(MM_BLOCK) void k_mem_verify(MemArgs a) {
    __shared__ uint32_t rel[MM_SLICE];
    __shared__ uint64_t sh_p[2];
    const SaView<W> sa{a.sa};
    const uint32_t tid = threadIdx.x;
    const uint64_t C = a.C, ntiles = (C + MM_T - 1) / MM_T;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MM_T;
        const uint64_t t1 = t0 + MM_T < C ? t0 + MM_T : C;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t pi[MM_PER], pv[MM_PER];
        uint32_t ok[MM_PER];
        mm_tile_candidates(sa, a.coff, a.lo, a.W.nw, a.n, t0, n_el, rel, sh_p, pi, pv, ok);
        // the rejections: the query and offset of every candidate, then the left chars of all of
        // them, text and query, requested before the first is compared
        uint64_t qq[MM_PER], qbase[MM_PER];
        uint32_t qi[MM_PER], qm[MM_PER], lt[MM_PER], lq[MM_PER];
#pragma unroll
        for (int u = 0; u < MM_PER; u++) {
            qq[u] = 0, qbase[u] = 0, qi[u] = 0, qm[u] = 0;
            if (ok[u]) {
                const uint64_t w = pi[u], q = a.wq ? a.wq[w] : w / a.W.per;
                qq[u] = q;
                qi[u] = (uint32_t)(w - a.W.first(q));
                qm[u] = a.Q.len(q);
                qbase[u] = a.Q.off(q);
                // the window lies in the text: nothing behind the text end takes part
                if (pv[u] + a.L > a.n) ok[u] = 0;
            }
        }
#pragma unroll
        for (int u = 0; u < MM_PER; u++) {
            const bool left = ok[u] && qi[u] > 0 && pv[u] > 0;
            lt[u] = left ? mem_text_char(a.tw, pv[u] - 1) : 4u;
            lq[u] = left ? a.Q.qbytes[qbase[u] + qi[u] - 1] : 5u;
        }
#pragma unroll
        for (int u = 0; u < MM_PER; u++) {
            const uint32_t e = u * MM_BLOCK + tid;
            if (e >= n_el) continue;
            uint32_t len = 0;
            bool live = ok[u] != 0;
            const bool lefteq = lt[u] == lq[u];
            const uint64_t j = pv[u];
            uint64_t hi = a.n;
            if (LAY) {
                if (live) {  // [j, j + L) inside one segment: that of j; its lo stops the left test
                    const uint64_t g = layout_seg_of_pos(a.lay, j);
                    if (g == LAYOUT_NONE || a.lay.seg_hi[g] - j < a.L) live = false;
                    else {
                        hi = a.lay.seg_hi[g];
                        if (lefteq && j > a.lay.seg_lo[g]) live = false;
                    }
                }
            } else if (lefteq) {
                live = false;
            }
            if (live) {
                const uint32_t i = qi[u], m = qm[u];
                const uint64_t bound = std::min<uint64_t>(m - i, hi - j);
                // word s of the query's chars from i + L on
                const uint8_t* qb = a.Q.qbytes + qbase[u] + i + a.L;
                const uint32_t rest = m - i - a.L;
                uint64_t l = a.L;
                uint32_t s = 0, bad = 0;
                bool more = l < bound;
                while (more) {
                    const uint64_t t = text_chars32(a.tw, j + l);
                    const uint64_t w = pack_query_word(qb, rest, s++, &bad);
                    l = mem_extend_step(t, w, l, bound, &more);
                }
                len = (uint32_t)l;
                if (UNIQ) {  // the string occurs once: neither SA neighbour shares len chars with it
                    const uint64_t p = pi[u], r = a.lo[p] + (t0 + e - a.coff[p]);
                    if (r > 0 && mem_same_prefix(a.tw, a.n, sa[r - 1], j, len)) len = 0;
                    if (len && r + 1 < a.n && mem_same_prefix(a.tw, a.n, sa[r + 1], j, len)) len = 0;
                }
            }
            a.verdict[t0 + e] = len;
            if (len) {
                a.cpos[t0 + e] = j;
                a.cqpos[t0 + e] = qi[u];
            }
        }
        __syncthreads();  // rel and sh_p are rewritten by the next tile
    }
}

// a kernel of its own for an index with a layout, as k_mm_verify has
static void mem_launch_verify(const sas_index* x, bool uniq, dim3 grid, hipStream_t st, const MemArgs& a) {
    with_sa_w(x->sa_w, [&](auto W) { with_bool(x->lay.nseq != 0, [&](auto LAY) { with_bool(uniq, [&](auto UNIQ) {
        hipLaunchKernelGGL((k_mem_verify<decltype(W)::value, decltype(LAY)::value, decltype(UNIQ)::value>), grid,
                           dim3(MM_BLOCK), 0, st, a);
    }); }); });
}

struct MemAccept {
    __device__ __host__ uint64_t operator()(uint32_t v) const { return v ? 1ull : 0ull; }
};

// out_off[q] = accepted candidates before the first candidate of query q's first window
__global__ void k_mem_offsets(MemWindows W, const uint64_t* __restrict__ coff, const uint64_t* __restrict__ scan,
                              uint64_t nq, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_total) {
    GRID_STRIDE(q, nq + 1) {
        const uint64_t v = scan[coff[q < nq ? W.first(q) : W.nw]];
        out_off[q] = v;
        if (q == nq && out_total) *out_total = v;
    }
}

template <bool U32>
__global__ void k_mem_scatter(const uint32_t* __restrict__ verdict, const uint64_t* __restrict__ scan,
                              const uint64_t* __restrict__ cpos, const uint32_t* __restrict__ cqpos, uint64_t C,
                              uint32_t* __restrict__ out_qpos, void* __restrict__ out_tpos,
                              uint32_t* __restrict__ out_len, uint64_t capacity) {
    GRID_STRIDE(c, C) {
        const uint32_t v = verdict[c];
        if (v == 0) continue;
        const uint64_t o = scan[c];
        if (o >= capacity) continue;
        if (out_qpos) out_qpos[o] = cqpos[c];
        if (out_tpos) {
            if (U32) static_cast<uint32_t*>(out_tpos)[o] = (uint32_t)cpos[c];
            else static_cast<uint64_t*>(out_tpos)[o] = cpos[c];
        }
        if (out_len) out_len[o] = v;
    }
}

// SAS_MEM_TIMING=1: the verify kernel of every call is timed; sas_mems_verify_ms returns the
// calling thread's last figure
static thread_local SeedTiming mem_timing{"SAS_MEM_TIMING"};

extern "C" double sas_mems_verify_ms(uint64_t* candidates) { return mem_timing.get(0, candidates); }

// Steps 1..6 up to the offsets; the scratch the scatter needs stays in the state
struct MemState {
    SeedState seed;
    PoolBuf woff, wq, qfl, verdict, cpos, cqpos, scan;
    uint64_t C = 0;
};

// All arrays on the device (out_total may be null).  Host reads: the window total of a ragged
// batch, and the candidate total
static int mem_prepare(const sas_index* x, const MmQueries& Q, uint32_t L, uint64_t max_hits, uint64_t* out_off,
                       uint8_t* out_qflags, uint64_t* out_total, hipStream_t st, uint32_t flags, MemState& s) {
    const uint64_t nq = Q.nq;
    const bool ragged = Q.qoff != nullptr;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    if (!out_qflags) {
        TRY(s.qfl.alloc(pool, nq, st));
        out_qflags = s.qfl.as<uint8_t>();
    }
    MemWindows W{nullptr, mem_windows_of(Q.m, L), 0};
    if (ragged) TRY(s.woff.alloc(pool, (nq + 1) * 8, st));
    hipLaunchKernelGGL(k_mem_count, seed_grid(x, nq + 1), dim3(256), 0, st, Q, L, s.woff.as<uint64_t>(), out_qflags);
    HIP_TRY(hipGetLastError());
    if (ragged) {
        W.woff = s.woff.as<uint64_t>();
        TRY(pool_scan(pool, st, s.woff.as<uint64_t>(), s.woff.as<uint64_t>(), nq + 1));
        TRY(seed_read_total(W.woff + nq, st, &W.nw));
        TRY(s.wq.alloc(pool, W.nw * 8, st));
    } else {
        W.nw = nq * W.per;
    }
    const uint64_t nw = W.nw;
    const uint64_t* wq = ragged ? s.wq.as<uint64_t>() : nullptr;
    TRY(seed_alloc(x, nw, st, s.seed));
    hipLaunchKernelGGL(k_mem_windows, seed_grid(x, nw), dim3(256), 0, st, Q, L, W, s.seed.poff.as<uint64_t>(),
                       s.seed.plen.as<uint32_t>(), s.wq.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    TRY(seed_ranges(x, Q.qbytes, nw, st, flags, s.seed));
    hipLaunchKernelGGL(k_mem_gate, seed_grid(x, nw), dim3(256), 0, st, Q, L, W, wq, max_hits, s.seed.lo, s.seed.hi,
                       out_qflags);
    HIP_TRY(hipGetLastError());
    TRY(seed_offsets(x, nw, st, s.seed));
    uint64_t* coff = s.seed.coff.as<uint64_t>();
    TRY(seed_read_total(coff + nw, st, &s.C));
    const uint64_t C = s.C;
    mem_timing.reset(C);
    if (C == 0) return seed_nothing(out_off, nq, out_total, st);
    TRY(s.verdict.alloc(pool, (C + 1) * 4, st));
    TRY(s.cpos.alloc(pool, C * 8, st));
    TRY(s.cqpos.alloc(pool, C * 4, st));
    TRY(s.scan.alloc(pool, (C + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(s.verdict.as<uint32_t>() + C, 0, 4, st));
    MemArgs a{};
    a.tw = x->text_w;
    a.n = x->n;
    a.sa = x->sa;
    a.Q = Q;
    a.L = L;
    a.W = W;
    a.wq = wq;
    a.lo = s.seed.lo;
    a.coff = coff;
    a.C = C;
    a.lay = x->lay;
    a.verdict = s.verdict.as<uint32_t>();
    a.cpos = s.cpos.as<uint64_t>();
    a.cqpos = s.cqpos.as<uint32_t>();
    SeedTimer timer(mem_timing.on(), st);
    TRY(timer.start());
    mem_launch_verify(x, (flags & SAS_MEM_UNIQUE) != 0, seed_verify_grid(C), st, a);
    HIP_TRY(hipGetLastError());
    TRY(timer.stop(&mem_timing.ms[0]));
    TRY(pool_scan(pool, st, rocprim::make_transform_iterator(s.verdict.as<uint32_t>(), MemAccept{}),
                  s.scan.as<uint64_t>(), C + 1));
    hipLaunchKernelGGL(k_mem_offsets, seed_grid(x, nq + 1), dim3(256), 0, st, W, coff, s.scan.as<uint64_t>(), nq,
                       out_off, out_total);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int mem_scatter(const sas_index* x, MemState& s, uint32_t* out_qpos, void* out_tpos, uint32_t* out_len,
                       uint64_t capacity, hipStream_t st, uint32_t flags) {
    if (s.C == 0 || capacity == 0) return 0;
    const dim3 grid(std::min(grid_for(s.C), (unsigned)x->num_cus * 8));
    with_bool(flags & SAS_LOCATE_U32, [&](auto U32) {
        hipLaunchKernelGGL(k_mem_scatter<decltype(U32)::value>, grid, dim3(256), 0, st, s.verdict.as<uint32_t>(),
                           s.scan.as<uint64_t>(), s.cpos.as<uint64_t>(), s.cqpos.as<uint32_t>(), s.C, out_qpos, out_tpos,
                           out_len, capacity);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

static int mems_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint32_t min_len,
                     uint64_t max_hits, uint64_t* out_off, uint32_t* out_qpos, void* out_tpos, uint32_t* out_len,
                     uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream, uint32_t flags) {
    const std::string w(fn);
    if (min_len == 0) SAS_FAIL(EINVAL, w + ": min_len must be at least 1");
    TRY(seed_index_checks(w, x, 0, flags, stream));
    MemState s;
    const ListOut outs[] = {{out_qpos, 4, "mems query offsets", true},
                            {out_tpos, (flags & SAS_LOCATE_U32) ? 4u : 8u, "mems text positions", true},
                            {out_len, 4, "mems lengths", true}};
    return seed_list_call(
        {fn, "mems", "matches", "the outputs", nullptr}, x, q, nq, out_off, out_qflags, outs, 3, capacity, out_total, stream, flags,
        [&](const MmQueries& Q, uint64_t* off, uint8_t* qfl, uint64_t* total, hipStream_t st, uint32_t fl) {
            return mem_prepare(x, Q, min_len, max_hits, off, qfl, total, st, fl, s);
        },
        [&](void* const* out, uint64_t cap, hipStream_t st) {
            return mem_scatter(x, s, static_cast<uint32_t*>(out[0]), out[1], static_cast<uint32_t*>(out[2]), cap, st,
                               flags);
        });
}

extern "C" int sas_mems(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                        uint64_t nq, uint32_t min_len, uint64_t max_hits, uint64_t* out_off, uint32_t* out_qpos,
                        void* out_tpos, uint32_t* out_len, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total,
                        void* stream, uint32_t flags) {
    return mems_impl("sas_mems", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, min_len, max_hits, out_off, out_qpos,
                     out_tpos, out_len, out_qflags, capacity, out_total, stream, flags);
}

extern "C" int sas_mems_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t min_len,
                              uint64_t max_hits, uint64_t* out_off, uint32_t* out_qpos, void* out_tpos,
                              uint32_t* out_len, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total,
                              void* stream, uint32_t flags) {
    return mems_impl("sas_mems_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, min_len, max_hits, out_off,
                     out_qpos, out_tpos, out_len, out_qflags, capacity, out_total, stream, flags);
}
