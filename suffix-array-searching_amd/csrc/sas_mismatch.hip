// sas_mismatch.hip -- k-mismatch locate (Hamming distance) by seed and verify (sas.h:
// sas_locate_mismatch, sas_locate_mismatch_fixed).
//
// A query of m chars with a budget of k substitutions is cut into k + 1 pieces, piece j =
// chars [b_j, b_{j+1}) with b_j = floor(j m / (k + 1)).  An alignment with at most k mismatches
// matches at least one piece exactly (pigeonhole), so the occurrences of the pieces are the
// only candidates:
//
//   1. k_mm_pieces     offsets and lengths of the nq (k + 1) pieces (ragged queries that overlap
//                      in the caller's bytes, which the range search takes);
//   2. sas_search_range over all pieces: their SA rank ranges;
//   3. k_seed_gate     empties the range of every piece that occurs more than max_seed_hits
//                      times (a skipped seed) and of every piece of a query with m <= k; writes
//                      the per-query flags and a per-query mask of skipped pieces;
//   4. sas_locate_offsets on the gated ranges: the candidate offsets, one candidate per
//                      occurrence of a piece (steps 1 to 4 are seed_candidates, seed_verify.hip,
//                      shared with sas_edit.hip); the host reads the candidate total C (the
//                      call's one read-back: it sizes the candidate scratch and the grids);
//   5. k_mm_verify     output-centric over the C candidates as k_locate_fill is over positions:
//                      a workgroup owns tiles of MM_T consecutive candidates, finds each one's
//                      piece by bisecting the tile's slice of the candidate offsets in LDS, reads
//                      SA[lo + i] and derives the alignment s = SA - b_j.  Alignments that leave
//                      the text are rejected before any text read, and on an index with a
//                      sequence layout (template bool LAY, layout.hpp) those that do not lie
//                      inside one segment: one bisect per candidate.  q and t[s .. s + m) are
//                      compared 32 chars a step (text_chars32, XOR, popcount of the 2-bit
//                      differences; the last word masked to m), stopping once the distance
//                      exceeds k.  The mismatch bits of each step are also tested against the
//                      regions of the pieces before j: a candidate of piece j is dropped when a
//                      non-skipped piece j' < j has no mismatch at this alignment (that piece
//                      reports it), so every alignment is reported once and nothing is sorted;
//                      one verdict byte per candidate: the distance, or 0xFF;
//   6. rocprim exclusive scan of the accept flags, k_mm_offsets (a query's candidates are one
//      contiguous span, so out_off[q] = the scan at the first candidate of piece q (k + 1)) and
//      k_mm_scatter (out_pos / out_dist, bounded by capacity).  Order is kept: (piece, SA rank).
//
// The query words of a compare are packed from the caller's bytes per candidate
// (pack_query_word: the candidates of a query are neighbours, so its bytes are read from L2).
// SAS_MM_QWORDS=packed in the environment packs every query once into scratch instead
// (k_mm_prepack) and reads one 8-B word per step: the verify kernel is then faster on long
// queries, the whole call slower on every shape measured (the A/B of tools/bench_mismatch.py;
// DESIGN.md has both figures).
#include "seed_verify.hpp"

#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MM_REJECT 0xFFu

// words of query q in the packed scratch: ceil(m / 32)
__global__ void k_mm_wcount(MmQueries Q, uint64_t* __restrict__ woff) {
    GRID_STRIDE(q, Q.nq + 1) woff[q] = q < Q.nq ? ((uint64_t)Q.len(q) + 31) >> 5 : 0;
}

__global__ void k_mm_prepack(MmQueries Q, const uint64_t* __restrict__ woff, uint64_t* __restrict__ qw) {
    uint32_t bad = 0;
    GRID_STRIDE(q, Q.nq) {
        const uint32_t m = Q.len(q), nw = (uint32_t)(((uint64_t)m + 31) >> 5);
        const uint8_t* b = Q.qbytes + Q.off(q);
        uint64_t* w = qw + woff[q];
        for (uint32_t j = 0; j < nw; j++) w[j] = pack_query_word(b, m, j, &bad);
    }
}

struct MmArgs {
    const uint64_t* tw;
    uint64_t n;
    const uint8_t* sa;
    MmQueries Q;
    uint32_t k;
    const uint64_t* lo;     // gated first rank per piece
    const uint64_t* coff;   // candidate offsets, np + 1
    uint64_t np;            // pieces
    uint64_t C;             // candidates
    const uint16_t* skip;   // per query: bit j = piece j is no seed
    const uint64_t* woff;   // PRE: first packed word per query
    const uint64_t* qw;     // PRE: packed query words
    uint8_t* verdict;       // per candidate: distance, or MM_REJECT
    LayoutView lay;         // LAY: the index's sequence layout
    uint64_t* cpos;         // per accepted candidate: the alignment
};

// Candidate `c` = occurrence `rank` of piece i at text position pv: the verdict for the
// alignment s = pv - b_j
template <bool PRE, bool LAY>
__device__ __forceinline__ uint32_t mm_verify_one(const MmArgs& a, uint64_t i, uint64_t pv, uint64_t* s_out) {
    const uint32_t kp1 = a.k + 1;
    const uint64_t q = i / kp1;
    const uint32_t j = (uint32_t)(i - q * kp1), m = a.Q.len(q);
    const uint32_t bj = mm_piece_start(j, m, kp1);
    if (pv < bj || pv - bj + m > a.n) return MM_REJECT;  // leaves the text: no text read
    const uint64_t s = pv - bj;
    if (LAY) {  // the alignment [s, s + m) must lie inside one segment: that of its first char
        const uint64_t g = layout_seg_of_pos(a.lay, s);
        if (g == LAYOUT_NONE || a.lay.seg_hi[g] - s < m) return MM_REJECT;
    }
    *s_out = s;
    const uint32_t skipm = a.skip[q];
    const uint8_t* qb = PRE ? nullptr : a.Q.qbytes + a.Q.off(q);
    const uint64_t* qw = PRE ? a.qw + a.woff[q] : nullptr;
    uint32_t dist = 0, dirty = 0, jp = 0, jb = 0, je = mm_piece_start(1, m, kp1), bad = 0;
    for (uint32_t off = 0; off < m; off += 32) {
        const uint32_t c = m - off < 32 ? m - off : 32;
        const uint64_t t = text_chars32(a.tw, s + off);
        const uint64_t w = PRE ? qw[off >> 5] : pack_query_word(qb, m, off >> 5, &bad);
        const uint64_t x = t ^ w;
        const uint64_t d = (x | (x >> 1)) & 0x5555555555555555ull & chars_mask(c);  // one bit per differing char
        dist += (uint32_t)__popcll(d);
        if (dist > a.k) return MM_REJECT;
        // the pieces before j that meet chars [off, off + c): a mismatch in one makes it dirty
        while (jp < j) {
            const uint32_t r0 = jb > off ? jb - off : 0, r1 = je < off + c ? je - off : c;
            if (r0 < r1 && (d & chars_mask(r1) & ~chars_mask(r0))) dirty |= 1u << jp;
            if (je > off + c) break;  // continues in the next word
            jp++;
            jb = je;
            je = mm_piece_start(jp + 1, m, kp1);
        }
    }
    // a non-skipped earlier piece matches exactly here: that piece reports the alignment
    if (~dirty & ~skipm & ((1u << j) - 1u)) return MM_REJECT;
    return dist;
}

template <int W, bool PRE, bool LAY>
__global__ __launch_bounds__(MM_BLOCK) void k_mm_verify(MmArgs a) {
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
        mm_tile_candidates(sa, a.coff, a.lo, a.np, a.n, t0, n_el, rel, sh_p, pi, pv, ok);
#pragma unroll
        for (int u = 0; u < MM_PER; u++) {
            const uint32_t e = u * MM_BLOCK + tid;
            if (e < n_el) {
                uint64_t s = 0;
                const uint32_t v = ok[u] ? mm_verify_one<PRE, LAY>(a, pi[u], pv[u], &s) : MM_REJECT;
                a.verdict[t0 + e] = (uint8_t)v;
                if (v != MM_REJECT) a.cpos[t0 + e] = s;
            }
        }
        __syncthreads();  // rel and sh_p are rewritten by the next tile
    }
}

// a kernel of its own for an index with a layout: without one the parent's instructions run
static void mm_launch_verify(const sas_index* x, bool pre, dim3 grid, hipStream_t st, const MmArgs& a) {
    with_sa_w(x->sa_w, [&](auto W) { with_bool(pre, [&](auto PRE) { with_bool(x->lay.nseq != 0, [&](auto LAY) {
        hipLaunchKernelGGL((k_mm_verify<decltype(W)::value, decltype(PRE)::value, decltype(LAY)::value>), grid,
                           dim3(MM_BLOCK), 0, st, a);
    }); }); });
}

struct MmAccept {
    __device__ __host__ uint64_t operator()(uint8_t v) const { return v != MM_REJECT ? 1ull : 0ull; }
};

// out_off[q] = accepted candidates before the first candidate of query q's first piece
__global__ void k_mm_offsets(const uint64_t* __restrict__ coff, const uint64_t* __restrict__ scan, uint64_t nq,
                             uint32_t kp1, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_total) {
    GRID_STRIDE(q, nq + 1) {
        const uint64_t v = scan[coff[q * kp1]];
        out_off[q] = v;
        if (q == nq && out_total) *out_total = v;
    }
}

template <bool U32>
__global__ void k_mm_scatter(const uint8_t* __restrict__ verdict, const uint64_t* __restrict__ scan,
                             const uint64_t* __restrict__ cpos, uint64_t C, void* __restrict__ out_pos,
                             uint8_t* __restrict__ out_dist, uint64_t capacity) {
    GRID_STRIDE(c, C) {
        const uint32_t v = verdict[c];
        if (v == MM_REJECT) continue;
        const uint64_t o = scan[c];
        if (o >= capacity) continue;
        if (U32) static_cast<uint32_t*>(out_pos)[o] = (uint32_t)cpos[c];
        else static_cast<uint64_t*>(out_pos)[o] = cpos[c];
        if (out_dist) out_dist[o] = (uint8_t)v;
    }
}

// SAS_MM_QWORDS=packed: pack every query once into scratch (the A/B knob; read at every call,
// so one process can measure both)
static bool mm_prepacked() {
    const char* e = getenv("SAS_MM_QWORDS");
    return e && strcmp(e, "packed") == 0;
}

// SAS_MM_TIMING=1: the verify kernel of every call is timed; sas_locate_mismatch_verify_ms
// returns the calling thread's last figure
static thread_local SeedTiming mm_timing{"SAS_MM_TIMING"};

extern "C" double sas_locate_mismatch_verify_ms(uint64_t* candidates) { return mm_timing.get(0, candidates); }

// Steps 1..6 up to the offsets; the scratch the scatter needs stays in the state
struct MmState {
    SeedState seed;
    PoolBuf woff, qw, verdict, cpos, scan;
    uint64_t C = 0;
};

// All arrays on the device (out_total may be null).  The one host read: the candidate total
static int mm_prepare(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off,
                      uint8_t* out_qflags, uint64_t* out_total, hipStream_t st, uint32_t flags, MmState& s) {
    const uint32_t kp1 = k + 1;
    const uint64_t nq = Q.nq, np = nq * kp1;
    // 1 to 4, with the mask of skipped pieces: no query is too long for the compare
    TRY(seed_candidates(x, Q, k, max_seed_hits, 0xFFFFFFFFu, true, out_qflags, st, flags, s.seed));
    hipMemPool_t pool = s.seed.pool;
    uint64_t* coff = s.seed.coff.as<uint64_t>();
    // SAS_MM_QWORDS=packed: ceil(m / 32) words per query; for ragged queries their total is read
    // back together with the candidate total (one synchronisation)
    const bool pre = mm_prepacked();
    uint64_t words = nq * (((uint64_t)Q.m + 31) >> 5);
    if (pre) {
        TRY(s.woff.alloc(pool, (nq + 1) * 8, st));
        hipLaunchKernelGGL(k_mm_wcount, seed_grid(x, nq + 1), dim3(256), 0, st, Q, s.woff.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        TRY(pool_scan(pool, st, s.woff.as<uint64_t>(), s.woff.as<uint64_t>(), nq + 1));
        if (Q.qoff) HIP_TRY(hipMemcpyAsync(&words, s.woff.as<uint64_t>() + nq, 8, hipMemcpyDeviceToHost, st));
    }
    TRY(seed_read_total(coff + np, st, &s.C));
    const uint64_t C = s.C;
    mm_timing.reset(C);
    if (C == 0) return seed_nothing(out_off, nq, out_total, st);
    if (pre) {
        TRY(s.qw.alloc(pool, words * 8, st));
        hipLaunchKernelGGL(k_mm_prepack, seed_grid(x, nq), dim3(256), 0, st, Q, s.woff.as<uint64_t>(),
                           s.qw.as<uint64_t>());
        HIP_TRY(hipGetLastError());
    }
    TRY(s.verdict.alloc(pool, C + 1, st));
    TRY(s.cpos.alloc(pool, C * 8, st));
    TRY(s.scan.alloc(pool, (C + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(s.verdict.as<uint8_t>() + C, MM_REJECT, 1, st));
    MmArgs a{};
    a.tw = x->text_w;
    a.n = x->n;
    a.sa = x->sa;
    a.Q = Q;
    a.k = k;
    a.lo = s.seed.lo;
    a.coff = coff;
    a.np = np;
    a.C = C;
    a.skip = s.seed.skip.as<uint16_t>();
    a.woff = s.woff.as<uint64_t>();
    a.qw = s.qw.as<uint64_t>();
    a.verdict = s.verdict.as<uint8_t>();
    a.cpos = s.cpos.as<uint64_t>();
    a.lay = x->lay;
    SeedTimer timer(mm_timing.on(), st);
    TRY(timer.start());
    mm_launch_verify(x, pre, seed_verify_grid(C), st, a);
    HIP_TRY(hipGetLastError());
    TRY(timer.stop(&mm_timing.ms[0]));
    TRY(pool_scan(pool, st, rocprim::make_transform_iterator(s.verdict.as<uint8_t>(), MmAccept{}),
                s.scan.as<uint64_t>(), C + 1));
    hipLaunchKernelGGL(k_mm_offsets, seed_grid(x, nq + 1), dim3(256), 0, st, coff, s.scan.as<uint64_t>(), nq, kp1,
                       out_off, out_total);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int mm_scatter(const sas_index* x, MmState& s, void* out_pos, uint8_t* out_dist, uint64_t capacity,
                      hipStream_t st, uint32_t flags) {
    if (s.C == 0 || capacity == 0) return 0;
    const dim3 grid(std::min(grid_for(s.C), (unsigned)x->num_cus * 8));
    with_bool(flags & SAS_LOCATE_U32, [&](auto U32) {
        hipLaunchKernelGGL(k_mm_scatter<decltype(U32)::value>, grid, dim3(256), 0, st,
                           s.verdict.as<uint8_t>(), s.scan.as<uint64_t>(), s.cpos.as<uint64_t>(), s.C, out_pos, out_dist,
                           capacity);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

static int mismatch_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint32_t k,
                         uint64_t max_seed_hits, uint64_t* out_off, void* out_pos, uint8_t* out_dist,
                         uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream, uint32_t flags) {
    const std::string w(fn);
    TRY(seed_index_checks(w, x, k, flags, stream));
    MmState s;
    const ListOut outs[] = {{out_pos, (flags & SAS_LOCATE_U32) ? 4u : 8u, "mismatch positions", true},
                            {out_dist, 1, "mismatch distances", false}};
    return seed_list_call(
        {fn, "mismatch", "positions", "out_pos", nullptr}, x, q, nq, out_off, out_qflags, outs, 2, capacity, out_total, stream, flags,
        [&](const MmQueries& Q, uint64_t* off, uint8_t* qfl, uint64_t* total, hipStream_t st, uint32_t fl) {
            return mm_prepare(x, Q, k, max_seed_hits, off, qfl, total, st, fl, s);
        },
        [&](void* const* out, uint64_t cap, hipStream_t st) {
            return mm_scatter(x, s, out[0], static_cast<uint8_t*>(out[1]), cap, st, flags);
        });
}

extern "C" int sas_locate_mismatch(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff,
                                   const uint32_t* qlen, uint64_t nq, uint32_t k, uint64_t max_seed_hits,
                                   uint64_t* out_off, void* out_pos, uint8_t* out_dist, uint8_t* out_qflags,
                                   uint64_t capacity, uint64_t* out_total, void* stream, uint32_t flags) {
    return mismatch_impl("sas_locate_mismatch", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, k, max_seed_hits, out_off,
                         out_pos, out_dist, out_qflags, capacity, out_total, stream, flags);
}

extern "C" int sas_locate_mismatch_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                                         uint64_t max_seed_hits, uint64_t* out_off, void* out_pos, uint8_t* out_dist,
                                         uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream,
                                         uint32_t flags) {
    return mismatch_impl("sas_locate_mismatch_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, k,
                         max_seed_hits, out_off, out_pos, out_dist, out_qflags, capacity, out_total, stream, flags);
}
