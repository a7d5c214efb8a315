// sas_edit.hip -- k-difference locate (unit-cost edit distance) by seed and verify (sas.h:
// sas_locate_edit, sas_locate_edit_fixed).
//
// For a query q of m chars, D(e) = min over s <= e of ed(q, t[s .. e)) is defined for every
// end e in [0, n]; the answer is every e with D(e) <= k (Sellers' problem).  The query is cut
// as for sas_locate_mismatch, into k + 1 pieces with b_j = floor(j m / (k + 1)): an alignment
// with at most k edits leaves one piece untouched, so that piece occurs exactly at some text
// position pv, and with s0 = pv - b_j (signed) the alignment ends in [s0 + m - k, s0 + m + k].
// A candidate is one occurrence of one piece:
//
//   1. k_mm_pieces, 2. sas_search_range, 4. sas_locate_offsets: as in sas_mismatch.hip
//                      (seed_candidates, seed_verify.hip);
//   3. k_seed_gate     empties the range of every piece that occurs more than max_seed_hits
//                      times, and every piece of a query with m <= k or m > SAS_ED_MAX_M; writes
//                      the per-query flags;
//   5. k_ed_verify     output-centric over the C candidates (mm_tile_candidates).  Per candidate
//                      Myers' bit-vector algorithm in its search form (free start: the
//                      horizontal delta into row 0 is 0; the score starts at m and follows the
//                      Ph / Mh bit of row m - 1) over the columns of the window
//                      t[max(0, s0 - 2k) .. min(n, s0 + m + k)).  Every alignment of cost <= k
//                      that ends in the candidate's interval starts at or after s0 - 2k, so the
//                      score there, capped at k + 1, is D(e) itself, whichever candidate
//                      computes it.  The query is two bit planes per 64 rows (the low and the
//                      high bit of each char); the match vector of a text char c is
//                      ~(L ^ -(c & 1)) & ~(H ^ -(c >> 1)), masked to m: no table indexed by the
//                      char.  The number of 64-row words is a template parameter (1, 2 or 4;
//                      ragged batches switch per thread), so the planes and Pv / Mv stay in
//                      named registers.  Text chars come 32 columns per text_chars32, never from
//                      a column >= n.  A candidate stops once score - columns left > k (the
//                      score falls by at most 1 per column: nothing later can be reported).
//                      Output per candidate: a mask of the accepted ends (bit i: e = s0 + m - k
//                      + i), their distances 4 bits each, and the sort key of bit 0.
//                      On an index with a sequence layout (template bool LAY, layout.hpp) one
//                      bisect finds the segment [lo, hi) of the seed occurrence, a seed that
//                      is not inside one segment is no candidate, and the window is cut to
//                      [max(lo, s0 - 2k), min(hi, s0 + m + k)) where it was cut to 0 and n.  The
//                      exactness argument carries over: the alignments inside the segment are
//                      a subset of all, so one of cost <= k that ends in the candidate's
//                      interval still starts at or after s0 - 2k, and the score, capped at
//                      k + 1, is D_L(e) of sas.h whichever candidate of that segment computes
//                      it.  An end at or before lo or past hi gets no column, so a candidate
//                      proposes ends of its own segment only, which is what sas.h asks of a
//                      SAS_ED_TRUNCATED query;
//   6. de-duplication  the same end is proposed by several pieces and, in repeats, by several
//                      occurrences: popcount of the masks, exclusive scan, the host reads the
//                      proposal total P (the call's second read-back: it sizes the sort), k_ed_emit
//                      writes one (key, dist) pair per proposal with key = (query << ebits) | e,
//                      rocprim::radix_sort_pairs over the ebits + qbits significant bits, an
//                      exclusive scan of "first of its run of equal keys", k_ed_offsets
//                      (out_off[q] = unique keys below query q, by bisection) and k_ed_scatter
//                      (out_end / out_dist, bounded by capacity).  Equal keys carry equal
//                      distances, so which duplicate is kept does not matter.
#include "edit_path.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>

struct EdArgs {
    const uint64_t* tw;
    uint64_t n;
    const uint8_t* sa;
    MmQueries Q;
    uint32_t k;
    uint32_t ebits;         // key = (query << ebits) | end
    const uint64_t* lo;     // gated first rank per piece
    const uint64_t* coff;   // candidate offsets, np + 1
    uint64_t np;            // pieces
    uint64_t C;             // candidates
    uint32_t* mask;         // per candidate: bit i = the end s0 + m - k + i is accepted
    uint64_t* kbase;        // per candidate: the key of bit 0 (modulo 2^64: s0 + m - k may be < 0)
    ulonglong2* dists;      // per candidate: the distance of bit i in bits [4 i, 4 i + 4)
    LayoutView lay;         // LAY: the index's sequence layout
};

// Candidate = an occurrence of piece i at text position pv.  NW words of 64 rows (m <= 64 NW)
// [t_lo, t_hi): the text the window is cut to: [0, n), or with a layout the seed's segment
template <int NW>
__device__ __forceinline__ void ed_verify_one(const EdArgs& a, uint32_t m, int64_t s0, int64_t t_lo, int64_t t_hi,
                                              const uint8_t* __restrict__ qb, uint32_t* mask_out, uint64_t* d0_out,
                                              uint64_t* d1_out) {
    const int64_t k = (int64_t)a.k;
    const int64_t w0 = s0 - 2 * k > t_lo ? s0 - 2 * k : t_lo;       // the window's columns [w0, w1)
    const int64_t w1 = s0 + m + k < t_hi ? s0 + (int64_t)m + k : t_hi;
    const int64_t e0 = s0 + (int64_t)m - k;                         // the end of bit 0
    uint32_t mask = 0;
    uint64_t d0 = 0, d1 = 0;
    EdMyers<NW> my;
    my.init(qb, m);
    int64_t score = m;
    for (int64_t col = w0; col < w1; col += 32) {
        uint64_t tx = text_chars32(a.tw, (uint64_t)col);            // col < w1 <= n
        const int64_t cend = col + 32 < w1 ? col + 32 : w1;
        for (int64_t c = col; c < cend; c++, tx <<= 2) {
            score += my.column(tx);
            const int64_t e = c + 1;                                // the score is D of end c + 1
            if (score <= k && e >= e0) {
                const uint32_t i = (uint32_t)(e - e0);              // <= 2k: e <= w1 <= s0 + m + k
                mask |= 1u << i;
                if (i < 16) d0 |= (uint64_t)score << (4 * i);
                else d1 |= (uint64_t)score << (4 * (i - 16));
            }
            if (score - (w1 - e) > k) {                             // out of reach for every later end
                col = w1;
                break;
            }
        }
    }
    *mask_out = mask;
    *d0_out = d0;
    *d1_out = d1;
}

// NW: 1, 2, 4 words of 64 rows for every query of the batch (fixed length), 0: by each query's m
template <int W, int NW, bool LAY>
__global__ __launch_bounds__(MM_BLOCK) void k_ed_verify(EdArgs a) {
    __shared__ uint32_t rel[MM_SLICE];
    __shared__ uint64_t sh_p[2];
    const SaView<W> sa{a.sa};
    const uint32_t tid = threadIdx.x, kp1 = a.k + 1;
    const uint64_t C = a.C, ntiles = (C + MM_T - 1) / MM_T;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)MM_T;
        const uint64_t t1 = t0 + MM_T < C ? t0 + MM_T : C;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t pi[MM_PER], pv[MM_PER];
        uint32_t ok[MM_PER];
        mm_tile_candidates(sa, a.coff, a.lo, a.np, a.n, t0, n_el, rel, sh_p, pi, pv, ok);
#pragma unroll
        for (int u = 0; u < MM_PER; u++) {
            const uint32_t e = u * MM_BLOCK + tid;
            if (e < n_el) {
                uint32_t mask = 0;
                uint64_t d0 = 0, d1 = 0, kb = 0;
                if (ok[u]) {
                    const uint64_t q = pi[u] / kp1;
                    const uint32_t j = (uint32_t)(pi[u] - q * kp1), m = a.Q.len(q);
                    const int64_t s0 = (int64_t)pv[u] - (int64_t)mm_piece_start(j, m, kp1);
                    const uint8_t* qb = a.Q.qbytes + a.Q.off(q);
                    kb = (q << a.ebits) + (uint64_t)(s0 + (int64_t)m - (int64_t)a.k);
                    int64_t t_lo = 0, t_hi = (int64_t)a.n;
                    bool seed_ok = true;
                    if (LAY) {  // the seed occurrence [pv, pv + len) must lie inside one segment
                        const uint64_t g = layout_seg_of_pos(a.lay, pv[u]);
                        const uint32_t len = mm_piece_start(j + 1, m, kp1) - mm_piece_start(j, m, kp1);
                        seed_ok = g != LAYOUT_NONE && a.lay.seg_hi[g] - pv[u] >= len;
                        if (seed_ok) {
                            t_lo = (int64_t)a.lay.seg_lo[g];
                            t_hi = (int64_t)a.lay.seg_hi[g];
                        }
                    }
                    if (seed_ok && m >= kp1 && m <= SAS_ED_MAX_M) {  // gated already: a guard for the word count
                        if (NW == 1 || (NW == 0 && m <= 64)) ed_verify_one<1>(a, m, s0, t_lo, t_hi, qb, &mask, &d0, &d1);
                        else if (NW == 2 || (NW == 0 && m <= 128))
                            ed_verify_one<2>(a, m, s0, t_lo, t_hi, qb, &mask, &d0, &d1);
                        else ed_verify_one<4>(a, m, s0, t_lo, t_hi, qb, &mask, &d0, &d1);
                    }
                }
                a.mask[t0 + e] = mask;
                a.kbase[t0 + e] = kb;
                a.dists[t0 + e] = make_ulonglong2(d0, d1);
            }
        }
        __syncthreads();  // rel and sh_p are rewritten by the next tile
    }
}

struct EdPopcount {
    __device__ __host__ uint64_t operator()(uint32_t v) const { return (uint64_t)__builtin_popcount(v); }
};

// One (key, dist) pair per accepted end of every candidate, at the scan of the mask popcounts
__global__ void k_ed_emit(const uint32_t* __restrict__ mask, const uint64_t* __restrict__ kbase,
                          const ulonglong2* __restrict__ dists, const uint64_t* __restrict__ pscan, uint64_t C,
                          uint64_t* __restrict__ keys, uint8_t* __restrict__ vals) {
    GRID_STRIDE(c, C) {
        uint32_t mk = mask[c];
        if (!mk) continue;
        const uint64_t kb = kbase[c];
        const ulonglong2 d = dists[c];
        uint64_t o = pscan[c];
        while (mk) {
            const uint32_t i = (uint32_t)__builtin_ctz(mk);
            mk &= mk - 1;
            keys[o] = kb + i;
            vals[o] = (uint8_t)(((i < 16 ? d.x >> (4 * i) : d.y >> (4 * (i - 16)))) & 15ull);
            o++;
        }
    }
}

// 1 for the first of each run of equal keys in the sorted proposals, 0 at and past P
struct EdFirst {
    const uint64_t* keys;
    uint64_t P;
    __device__ __host__ uint64_t operator()(uint64_t p) const {
        return p < P && (p == 0 || keys[p] != keys[p - 1]) ? 1ull : 0ull;
    }
};

// out_off[q] = unique keys below (q << ebits): uscan at the first proposal of a query >= q
__global__ void k_ed_offsets(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ uscan, uint64_t P,
                             uint64_t nq, uint32_t ebits, uint64_t* __restrict__ out_off,
                             uint64_t* __restrict__ out_total) {
    GRID_STRIDE(q, nq + 1) {
        uint64_t l = 0, h = P;
        while (l < h) {
            const uint64_t mid = (l + h) >> 1;
            if ((keys[mid] >> ebits) < q) l = mid + 1;
            else h = mid;
        }
        const uint64_t v = uscan[l];
        out_off[q] = v;
        if (q == nq && out_total) *out_total = v;
    }
}

template <bool U32>
__global__ void k_ed_scatter(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ vals,
                             const uint64_t* __restrict__ uscan, uint64_t P, uint32_t ebits,
                             void* __restrict__ out_end, uint8_t* __restrict__ out_dist, uint64_t capacity) {
    GRID_STRIDE(p, P) {
        const uint64_t key = keys[p];
        if (p && keys[p - 1] == key) continue;
        const uint64_t o = uscan[p];
        if (o >= capacity) continue;
        const uint64_t e = key & ((1ull << ebits) - 1ull);
        if (U32) static_cast<uint32_t*>(out_end)[o] = (uint32_t)e;
        else static_cast<uint64_t*>(out_end)[o] = e;
        if (out_dist) out_dist[o] = vals[p];
    }
}

// SAS_ED_TIMING=1: the verify kernel and the de-duplication (k_ed_emit .. k_ed_offsets) of every
// call are timed; sas_locate_edit_verify_ms and sas_locate_edit_dedup_ms return the calling
// thread's last figures
static thread_local SeedTiming ed_timing{"SAS_ED_TIMING"};

extern "C" double sas_locate_edit_verify_ms(uint64_t* candidates) { return ed_timing.get(0, candidates); }

extern "C" double sas_locate_edit_dedup_ms(uint64_t* proposals) { return ed_timing.get(1, proposals); }

// a kernel of its own for an index with a layout: without one the parent's instructions run
static void ed_launch_verify(const sas_index* x, dim3 grid, hipStream_t st, const EdArgs& a) {
    with_sa_w(x->sa_w, [&](auto W) { with_ed_words(a.Q, [&](auto NW) { with_bool(x->lay.nseq != 0, [&](auto LAY) {
        hipLaunchKernelGGL((k_ed_verify<decltype(W)::value, decltype(NW)::value, decltype(LAY)::value>), grid,
                           dim3(MM_BLOCK), 0, st, a);
    }); }); });
}

// All arrays on the device (out_total may be null).  Two host reads: the candidate total and
// the proposal total (edit_path.hpp)
int ed_prepare(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off,
               uint8_t* out_qflags, uint64_t* out_total, hipStream_t st, uint32_t flags, EdState& s) {
    const uint32_t kp1 = k + 1;
    const uint64_t nq = Q.nq, np = nq * kp1;
    s.ebits = ed_bits(x->n);
    // 1 to 4: a query of more than SAS_ED_MAX_M chars gets no seeds
    TRY(seed_candidates(x, Q, k, max_seed_hits, SAS_ED_MAX_M, false, out_qflags, st, flags, s.seed));
    hipMemPool_t pool = s.seed.pool;
    uint64_t* coff = s.seed.coff.as<uint64_t>();
    TRY(seed_read_total(coff + np, st, &s.C));
    const uint64_t C = s.C;
    ed_timing.reset(C);
    if (C == 0) return seed_nothing(out_off, nq, out_total, st);
    TRY(s.mask.alloc(pool, (C + 1) * 4, st));
    TRY(s.kbase.alloc(pool, C * 8, st));
    TRY(s.dists.alloc(pool, C * 16, st));
    TRY(s.pscan.alloc(pool, (C + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(s.mask.as<uint32_t>() + C, 0, 4, st));
    EdArgs a{};
    a.tw = x->text_w;
    a.n = x->n;
    a.sa = x->sa;
    a.Q = Q;
    a.k = k;
    a.ebits = s.ebits;
    a.lo = s.seed.lo;
    a.coff = coff;
    a.np = np;
    a.C = C;
    a.mask = s.mask.as<uint32_t>();
    a.kbase = s.kbase.as<uint64_t>();
    a.dists = s.dists.as<ulonglong2>();
    a.lay = x->lay;
    SeedTimer timer(ed_timing.on(), st);
    TRY(timer.start());
    ed_launch_verify(x, seed_verify_grid(C), st, a);
    HIP_TRY(hipGetLastError());
    TRY(timer.stop(&ed_timing.ms[0]));
    // proposals: one per accepted end of every candidate
    TRY(pool_scan(pool, st, rocprim::make_transform_iterator(s.mask.as<uint32_t>(), EdPopcount{}),
                s.pscan.as<uint64_t>(), C + 1));
    TRY(seed_read_total(s.pscan.as<uint64_t>() + C, st, &s.P));
    const uint64_t P = s.P;
    ed_timing.count[1] = P;
    if (P == 0) return seed_nothing(out_off, nq, out_total, st);
    TRY(timer.start());
    TRY(s.keys.alloc(pool, 2 * P * 8, st));
    TRY(s.vals.alloc(pool, 2 * P, st));
    TRY(s.uscan.alloc(pool, (P + 1) * 8, st));
    uint64_t* keys = s.keys.as<uint64_t>();
    uint8_t* vals = s.vals.as<uint8_t>();
    hipLaunchKernelGGL(k_ed_emit, seed_grid(x, C), dim3(256), 0, st, s.mask.as<uint32_t>(), s.kbase.as<uint64_t>(),
                       s.dists.as<ulonglong2>(), s.pscan.as<uint64_t>(), C, keys, vals);
    HIP_TRY(hipGetLastError());
    const uint32_t kbits = std::min<uint32_t>(64, s.ebits + (nq > 1 ? ed_bits(nq - 1) : 0));
    rocprim::double_buffer<uint64_t> kdb(keys, keys + P);
    rocprim::double_buffer<uint8_t> vdb(vals, vals + P);
    {
        size_t tbytes = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tbytes, kdb, vdb, (size_t)P, 0, kbits, st));
        PoolBuf tmp;
        TRY(tmp.alloc(pool, tbytes, st));
        HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tbytes, kdb, vdb, (size_t)P, 0, kbits, st));
    }
    s.skeys = kdb.current();
    s.svals = vdb.current();
    TRY(pool_scan(pool, st,
                rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), EdFirst{s.skeys, P}),
                s.uscan.as<uint64_t>(), P + 1));
    hipLaunchKernelGGL(k_ed_offsets, seed_grid(x, nq + 1), dim3(256), 0, st, s.skeys, s.uscan.as<uint64_t>(), P, nq,
                       s.ebits, out_off, out_total);
    HIP_TRY(hipGetLastError());
    return timer.stop(&ed_timing.ms[1]);
}

static int ed_scatter(const sas_index* x, EdState& s, void* out_end, uint8_t* out_dist, uint64_t capacity,
                      hipStream_t st, uint32_t flags) {
    if (s.P == 0 || capacity == 0) return 0;
    const dim3 grid(std::min(grid_for(s.P), (unsigned)x->num_cus * 8));
    with_bool(flags & SAS_LOCATE_U32, [&](auto U32) {
        hipLaunchKernelGGL(k_ed_scatter<decltype(U32)::value>, grid, dim3(256), 0, st, s.skeys, s.svals,
                           s.uscan.as<uint64_t>(), s.P, s.ebits, out_end, out_dist, capacity);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

static int edit_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint32_t k,
                     uint64_t max_seed_hits, uint64_t* out_off, void* out_end, uint8_t* out_dist, uint8_t* out_qflags,
                     uint64_t capacity, uint64_t* out_total, void* stream, uint32_t flags) {
    const std::string w(fn);
    TRY(seed_index_checks(w, x, k, flags, stream));
    EdState s;
    const ListOut outs[] = {{out_end, (flags & SAS_LOCATE_U32) ? 4u : 8u, "edit ends", true},
                            {out_dist, 1, "edit distances", false}};
    // the (query, end) sort key: the bits of an end in [0, n] above those of a query number
    const auto key_fits = [&]() {
        if (ed_bits(x->n) + (nq > 1 ? ed_bits(nq - 1) : 0) > 64)
            SAS_FAIL(EINVAL, w + ": " + std::to_string(nq) + " queries on a text of " + std::to_string(x->n) +
                                 " chars do not fit the 64-bit (query, end) sort key: split the batch");
        return 0;
    };
    return seed_list_call(
        {fn, "edit", "ends", "out_end", key_fits}, x, q, nq, out_off, out_qflags, outs, 2, capacity, out_total, stream,
        flags,
        [&](const MmQueries& Q, uint64_t* off, uint8_t* qfl, uint64_t* total, hipStream_t st, uint32_t fl) {
            return ed_prepare(x, Q, k, max_seed_hits, off, qfl, total, st, fl, s);
        },
        [&](void* const* out, uint64_t cap, hipStream_t st) {
            return ed_scatter(x, s, out[0], static_cast<uint8_t*>(out[1]), cap, st, flags);
        });
}

extern "C" int sas_locate_edit(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                               uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off, void* out_end,
                               uint8_t* out_dist, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total,
                               void* stream, uint32_t flags) {
    return edit_impl("sas_locate_edit", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, k, max_seed_hits, out_off, out_end,
                     out_dist, out_qflags, capacity, out_total, stream, flags);
}

extern "C" int sas_locate_edit_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                                     uint64_t max_seed_hits, uint64_t* out_off, void* out_end, uint8_t* out_dist,
                                     uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream,
                                     uint32_t flags) {
    return edit_impl("sas_locate_edit_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, k, max_seed_hits,
                     out_off, out_end, out_dist, out_qflags, capacity, out_total, stream, flags);
}
