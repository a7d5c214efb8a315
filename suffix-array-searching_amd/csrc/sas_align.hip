// sas_align.hip -- where an approximate match starts and its edit script (sas.h: sas_align_edit,
// sas_align_edit_fixed), for the ends that sas_locate_edit reports.
//
// For a query q of m chars, an end e and the bound k, R[i][j] = ed(q[i .. m), t[j .. e)) is the
// backward dynamic program with its origin fixed at (m, e): R[m][j] = e - j, R[i][e] = m - i.
// Every cell on a path of cost <= k has R <= k and R[i][j] >= |(m - i) - (e - j)|, so only the
// 2k + 1 diagonals around the main one (j - i = e - m) matter.  One thread per alignment:
//
//   1. k_al_align     output-centric over the alignments (al_tile_queries: a workgroup owns a tile
//                     of AL_T consecutive alignments and finds each one's query by bisecting the
//                     tile's slice of `off`, staged in LDS).  Per alignment a banded pass, row by
//                     row from i = m - 1 down to 0, over the cells x = j - (e - m + i) + KB of the
//                     band (KB = 1, 3, 7 or 15 >= k, a template parameter: the band's values stay
//                     in named registers).  Values are capped at k + 1: a capped cell is never on
//                     a reported path, and a cell of value <= k is exact, because the cheapest
//                     path from it stays inside the band.  Cells with j > e are capped by
//                     position; cells with j < 0 feed no cell of a larger j and are skipped when
//                     row 0 is read.  The 2 KB + 1 text chars of a row sit in one 64-bit window
//                     that moves down by one char per row: it starts from one text_chars32 and
//                     is fed from one aligned text word per 32 rows.  The query comes 32 chars
//                     per pack_query_word.  The row's mismatch bits are (win ^ q[i] 0x5555..)
//                     folded to one bit per char: no table indexed by the char.
//                     Per cell the pass records 2 bits: the first of sas.h's three rules that
//                     reaches the cell's value, as the op it emits (=, X, I, D).  A row's
//                     records are one word of 8, 16, 32 or 64 bits (by KB) in global scratch at
//                     scr[(m - 1 - i) T + thread], T = the threads of the grid: lanes write row r
//                     together, coalesced.  Row m is all D and is not stored.
//   2.                d = the least value of row 0 over j >= 0, s = the largest such j (the scan
//                     runs from the band's upper end).  d > k: no alignment.
//   3.                the walk from (0, s) to (m, e) reads one record word per query char and
//                     writes the run-length encoded script.
//
// On an index with a sequence layout (template bool LAY, layout.hpp) one bisect finds the segment
// of e: an end in none has no alignment, and step 2 scans j >= lo of that segment where it
// scanned j >= 0, which is w0 = max(lo, e - m - k) of sas.h.
//
// Scratch is T x rows x word bytes, T <= num_cus AL_BPC AL_BLOCK, rows = m (fixed length) or
// SAS_ED_MAX_M (ragged): bounded by the grid, not by the number of alignments.
#include "seed_verify.hpp"

#include <algorithm>
#include <cstring>

#define AL_BPC 4            // workgroups per CU that size the grid and the scratch

struct AlArgs {
    const uint64_t* tw;
    uint64_t n;
    MmQueries Q;
    uint32_t k;
    const uint64_t* off;    // nq + 1
    const void* end;        // u64, or u32 (template)
    uint64_t na;
    void* out_start;
    uint8_t* out_dist;      // may be null
    uint8_t* out_nruns;     // may be null
    uint16_t* out_runs;     // may be null; 2k + 1 slots per alignment
    void* scr;              // direction words, [row][thread of the grid]
    LayoutView lay;         // LAY: the index's sequence layout
};

template <int KB> struct AlWord;
template <> struct AlWord<1> { typedef uint8_t type; };
template <> struct AlWord<3> { typedef uint16_t type; };
template <> struct AlWord<7> { typedef uint32_t type; };
template <> struct AlWord<15> { typedef uint64_t type; };

// One alignment: 1 <= m <= SAS_ED_MAX_M, e <= n.  scr: this thread's column of the direction
// words, row r at scr[r T].  Returns the distance (SAS_AL_NONE_DIST: none) and sets *s_out and
// *nruns_out; the runs go to `runs` (2k + 1 slots, when not null), the unused slots as 0.
// jmin: the least start, 0 or with a layout the lo of e's segment.  R[i][j] depends on t[j .. e)
// alone and a cell feeds no cell of a larger j, so cutting the starts is all that a segment asks
template <int KB>
__device__ __forceinline__ uint32_t al_one(const AlArgs& a, uint32_t m, uint64_t e, int64_t jmin,
                                           const uint8_t* __restrict__ qb,
                                           typename AlWord<KB>::type* __restrict__ scr, uint64_t T, uint64_t* s_out,
                                           uint32_t* nruns_out, uint16_t* __restrict__ runs) {
    typedef typename AlWord<KB>::type DT;
    constexpr int BW = 2 * KB + 1;
    const uint32_t k = a.k, kcap = k + 1, stride = 2 * k + 1;
    const int64_t se = (int64_t)e;
    uint32_t v[BW];
#pragma unroll
    for (int x = 0; x < BW; x++) {  // row m: R[m][e + x - KB] = KB - x
        const uint32_t d = x <= KB ? (uint32_t)(KB - x) : kcap;
        v[x] = d < kcap ? d : kcap;
    }
    // the window: char x of `win` (bits 63 - 2x, 62 - 2x) is t[e - r - KB + x] in row i = m - r
    int64_t p0 = se - 1 - KB;
    uint64_t win = p0 >= 0 ? text_chars32(a.tw, (uint64_t)p0) : (text_chars32(a.tw, 0) >> (2 * (uint32_t)(-p0)));
    uint64_t fwi = ~0ull, feed = 0, qword = 0;
    uint32_t bad = 0;
    bool alive = true;
    for (uint32_t r = 1; r <= m && alive; r++) {
        const uint32_t i = m - r;
        if (r > 1) {  // one char down: t[p0] comes in at the top (0 before the text)
            p0--;
            uint64_t ch = 0;
            if (p0 >= 0) {
                const uint64_t wi = (uint64_t)p0 >> 5;
                if (wi != fwi) {
                    fwi = wi;
                    feed = a.tw[wi];
                }
                ch = (feed >> (62 - 2 * ((uint32_t)p0 & 31u))) & 3ull;
            }
            win = (win >> 2) | (ch << 62);
        }
        if (r == 1 || (i & 31u) == 31u) qword = pack_query_word(qb, m, i >> 5, &bad);
        const uint64_t qc = (qword >> (62 - 2 * (i & 31u))) & 3ull;
        const uint64_t xr = win ^ (qc * 0x5555555555555555ull);
        const uint64_t ne = (xr | (xr >> 1)) & 0x5555555555555555ull;  // bit 62 - 2x: q[i] != char x
        const uint32_t lim = r + KB;  // cell x lies at j <= e iff x <= lim
        DT dirs = 0;
        uint32_t right = kcap, rowmin = kcap;
#pragma unroll
        for (int x = BW - 1; x >= 0; x--) {
            const uint32_t nq1 = (uint32_t)(ne >> (62 - 2 * x)) & 1u;
            const uint32_t cd = v[x] + nq1;                       // rule 1: (i + 1, j + 1)
            const uint32_t cr = right + 1;                        // rule 2: (i, j + 1)
            const uint32_t cdn = (x > 0 ? v[x > 0 ? x - 1 : 0] : kcap) + 1;  // rule 3: (i + 1, j)
            uint32_t nv = cd < cr ? cd : cr;
            nv = nv < cdn ? nv : cdn;
            nv = nv < kcap ? nv : kcap;
            const uint32_t code = cd == nv ? nq1 : (cr == nv ? SAS_AL_DEL : SAS_AL_INS);
            if ((uint32_t)x > lim) nv = kcap;
            v[x] = nv;
            right = nv;
            rowmin = nv < rowmin ? nv : rowmin;
            dirs |= (DT)((DT)code << (2 * x));
        }
        scr[(uint64_t)(r - 1) * T] = dirs;
        alive = rowmin <= k;  // every later row is at least this row's least value
    }
    *nruns_out = 0;
    *s_out = a.n;
    uint32_t d = kcap;
    int sx = -1;
    if (alive) {
        const int64_t j0 = se - (int64_t)m - KB;  // cell x of row 0 is column j0 + x
#pragma unroll
        for (int x = BW - 1; x >= 0; x--) {
            if (j0 + x >= jmin && v[x] < d) {
                d = v[x];
                sx = x;
            }
        }
    }
    if (d > k || sx < 0) {
        if (runs)
            for (uint32_t r = 0; r < stride; r++) runs[r] = 0;
        return SAS_AL_NONE_DIST;
    }
    const uint64_t s = (uint64_t)(se - (int64_t)m - KB + sx);
    // the walk: (i, j) from (0, s) to (m, e); x = j - (e - m + i) + KB
    uint32_t i = 0, nr = 0, op = 4, len = 0;
    uint64_t j = s;
    int x = sx;
    const uint32_t max_steps = 2 * m + 2 * KB + 2;
    for (uint32_t step = 0; step < max_steps && (i < m || j < e); step++) {
        uint32_t code = SAS_AL_DEL;
        if (i < m) {
            if (x < 0 || x >= BW) break;
            code = (uint32_t)(scr[(uint64_t)(m - 1 - i) * T] >> (2 * x)) & 3u;
        }
        if (code != op) {
            if (len && runs && nr < stride) runs[nr] = (uint16_t)((len << 2) | op);
            nr += len ? 1u : 0u;
            op = code;
            len = 0;
        }
        len++;
        if (code == SAS_AL_DEL) {
            j++;
            x++;
        } else if (code == SAS_AL_INS) {
            i++;
            x--;
        } else {
            i++;
            j++;
        }
    }
    if (len && runs && nr < stride) runs[nr] = (uint16_t)((len << 2) | op);
    nr += len ? 1u : 0u;
    if (runs)
        for (uint32_t r = nr; r < stride; r++) runs[r] = 0;
    *s_out = s;
    *nruns_out = nr;
    return d;
}

template <int KB, bool U32, bool LAY>
__global__ __launch_bounds__(AL_BLOCK) void k_al_align(AlArgs a) {
    typedef typename AlWord<KB>::type DT;
    __shared__ uint32_t rel[AL_SLICE];
    __shared__ uint64_t sh_p[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t T = (uint64_t)gridDim.x * AL_BLOCK;
    DT* scr = static_cast<DT*>(a.scr) + ((uint64_t)blockIdx.x * AL_BLOCK + tid);
    uint64_t total = a.off[a.Q.nq];  // nothing at or past min(na, off[nq]) is written
    if (total > a.na) total = a.na;
    const uint64_t ntiles = (total + AL_T - 1) / AL_T;
    const uint32_t stride = 2 * a.k + 1;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)AL_T;
        const uint64_t t1 = t0 + AL_T < total ? t0 + AL_T : total;
        const uint32_t n_el = (uint32_t)(t1 - t0);
        uint64_t qi[AL_PER];
        uint32_t ok[AL_PER];
        al_tile_queries(a.off, a.Q.nq, t0, n_el, rel, sh_p, qi, ok);
#pragma unroll 1
        for (int u = 0; u < AL_PER; u++) {
            const uint32_t el = u * AL_BLOCK + tid;
            if (el >= n_el) continue;
            const uint64_t al = t0 + el;
            uint16_t* runs = a.out_runs ? a.out_runs + al * stride : nullptr;
            uint64_t s = a.n;
            uint32_t d = SAS_AL_NONE_DIST, nr = 0;
            const uint64_t e = U32 ? (uint64_t)static_cast<const uint32_t*>(a.end)[al]
                                   : static_cast<const uint64_t*>(a.end)[al];
            const uint32_t m = ok[u] ? a.Q.len(qi[u]) : 0u;
            int64_t jmin = 0;
            bool in_seg = true;
            if (LAY && e <= a.n) {  // one bisect on e: an end in no segment has no alignment
                const uint64_t g = layout_seg_of_end(a.lay, e);
                in_seg = g != LAYOUT_NONE;
                if (in_seg) jmin = (int64_t)a.lay.seg_lo[g];
            }
            if (m >= 1 && m <= SAS_ED_MAX_M && e <= a.n && in_seg) {
                d = al_one<KB>(a, m, e, jmin, a.Q.qbytes + a.Q.off(qi[u]), scr, T, &s, &nr, runs);
            } else if (runs) {
                for (uint32_t r = 0; r < stride; r++) runs[r] = 0;
            }
            if (U32) static_cast<uint32_t*>(a.out_start)[al] = (uint32_t)s;
            else static_cast<uint64_t*>(a.out_start)[al] = s;
            if (a.out_dist) a.out_dist[al] = (uint8_t)d;
            if (a.out_nruns) a.out_nruns[al] = (uint8_t)nr;
        }
        __syncthreads();  // rel and sh_p are rewritten by the next tile
    }
}

// SAS_VALIDATE: every byte of every query must be a DNA code 0..3 (fixed-length queries cover
// one contiguous span of `total` bytes)
__global__ void k_al_validate(const uint8_t* __restrict__ qb, const uint64_t* __restrict__ qoff,
                              const uint32_t* __restrict__ qlen, uint64_t nq, uint64_t total,
                              uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    if (qoff) {
        GRID_STRIDE(i, nq) {
            const uint8_t* q = qb + qoff[i];
            const uint32_t m = qlen[i];
            for (uint32_t c = 0; c < m; c++) b |= q[c];
        }
    } else {
        GRID_STRIDE(c, total) b |= qb[c];
    }
    if (b & 0xFCu) atomicOr(bad, 1u);
}

// kb: the band's k rounded up to 1, 3, 7 or 15.  A kernel of its own for an index with a layout:
// without one the parent's instructions run
static void al_launch(uint32_t kb, bool u32, dim3 grid, hipStream_t st, const AlArgs& a) {
    const auto launch = [&](auto KB) { with_bool(u32, [&](auto U32) { with_bool(a.lay.nseq != 0, [&](auto LAY) {
        hipLaunchKernelGGL((k_al_align<decltype(KB)::value, decltype(U32)::value, decltype(LAY)::value>), grid,
                           dim3(AL_BLOCK), 0, st, a);
    }); }); };
    if (kb == 1) launch(std::integral_constant<int, 1>{});
    else if (kb == 3) launch(std::integral_constant<int, 3>{});
    else if (kb == 7) launch(std::integral_constant<int, 7>{});
    else launch(std::integral_constant<int, 15>{});
}

// All arrays on the device.  No host read unless `validate`
static int al_device(const char* fn, const sas_index* x, const MmQueries& Q, uint32_t k, const uint64_t* off,
                     const void* end, uint64_t na, void* out_start, uint8_t* out_dist, uint8_t* out_nruns,
                     uint16_t* out_runs, hipStream_t st, uint32_t flags, bool validate) {
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    BadFlag bflag;  // armed when it is read back
    if (validate) {
        TRY(bflag.arm(st));
        const uint64_t total = Q.qoff ? Q.nq : Q.nq * (uint64_t)Q.m;
        hipLaunchKernelGGL(k_al_validate, dim3(tile_grid(grid_for(total))), dim3(256), 0, st, Q.qbytes, Q.qoff, Q.qlen,
                           Q.nq, total, bflag.ptr());
        HIP_TRY(hipGetLastError());
    }
    uint64_t blocks = (na + AL_T - 1) / AL_T;
    const uint64_t capb = (uint64_t)x->num_cus * AL_BPC;
    if (blocks > capb) blocks = capb;
    blocks = tile_grid(blocks);  // before the scratch is sized from it
    const uint32_t kb = k <= 1 ? 1u : (k <= 3 ? 3u : (k <= 7 ? 7u : 15u));
    const uint32_t wbytes = kb == 1 ? 1u : (kb == 3 ? 2u : (kb == 7 ? 4u : 8u));
    // direction words: one per row of the longest query that is served, per thread of the grid
    const uint64_t rows = Q.qoff ? SAS_ED_MAX_M : std::min<uint64_t>(std::max<uint32_t>(Q.m, 1u), SAS_ED_MAX_M);
    PoolBuf scr;
    TRY(scr.alloc(pool, blocks * AL_BLOCK * rows * wbytes, st));
    AlArgs a{};
    a.tw = x->text_w;
    a.n = x->n;
    a.Q = Q;
    a.k = k;
    a.off = off;
    a.end = end;
    a.na = na;
    a.out_start = out_start;
    a.out_dist = out_dist;
    a.out_nruns = out_nruns;
    a.out_runs = out_runs;
    a.scr = scr.p;
    a.lay = x->lay;
    al_launch(kb, (flags & SAS_LOCATE_U32) != 0, dim3((unsigned)blocks), st, a);
    HIP_TRY(hipGetLastError());
    if (validate) {
        uint32_t hbad = 0;
        TRY(bflag.read(st, &hbad));
        if (hbad) SAS_FAIL(EINVAL, std::string(fn) + ": query bytes must be DNA codes 0..3");
    }
    return 0;
}

static int align_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t nq, uint32_t k,
                      const uint64_t* off, const void* end, uint64_t na, void* out_start, uint8_t* out_dist,
                      uint8_t* out_nruns, uint16_t* out_runs, void* stream, uint32_t flags) {
    const std::string w(fn);
    if (!x) SAS_FAIL(EINVAL, w + ": null index");
    if (k > MM_MAX_K) SAS_FAIL(EINVAL, w + ": k must be 0.." + std::to_string(MM_MAX_K));
    if ((flags & SAS_LOCATE_U32) && x->n >= (1ull << 32))
        SAS_FAIL(EINVAL, w + ": SAS_LOCATE_U32 needs a text of n < 2^32 chars");
    if (!x->text_w) SAS_FAIL(ENOTSUP, w + ": the index holds no packed text");
    if (na == 0) return 0;
    if (!off || !end || !out_start || !q.null_ok(nq)) SAS_FAIL(EINVAL, w + ": null argument");
    if (nq == 0) return 0;  // off[0] = 0: no alignment
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t stride = 2 * k + 1;
    if (flags & SAS_DEVICE_PTRS) {
        return al_device(fn, x, q.device(nq), k, off, end, na, out_start, out_dist, out_nruns, out_runs, st, flags,
                         (flags & SAS_VALIDATE) != 0);
    }
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated)
    const uint64_t count = std::min(na, off[nq]);
    if (count == 0) return 0;
    const uint64_t esz = (flags & SAS_LOCATE_U32) ? 4 : 8;
    HostQueries hq;
    HostOutputs ho;
    DevBuf doff, dend;
    MmQueries Q;
    TRY(hq.stage("align", q, nq, st, &Q));
    TRY(host_copy_in(doff, off, (nq + 1) * 8, "align offsets"));
    TRY(host_copy_in(dend, end, count * esz, "align ends"));
    void* dstart;
    uint8_t *ddist, *dnr;
    uint16_t* druns;
    TRY(ho.twin(out_start, count * esz, "align starts", &dstart));
    TRY(ho.twin(out_dist, count, "align distances", &ddist));
    TRY(ho.twin(out_nruns, count, "align run counts", &dnr));
    TRY(ho.twin(out_runs, count * stride * 2, "align runs", &druns));
    TRY(al_device(fn, x, Q, k, doff.as<uint64_t>(), dend.p, count, dstart, ddist, dnr, druns, st, flags, true));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_align_edit(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                              uint64_t nq, uint32_t k, const uint64_t* off, const void* end, uint64_t na,
                              void* out_start, uint8_t* out_dist, uint8_t* out_nruns, uint16_t* out_runs, void* stream,
                              uint32_t flags) {
    return align_impl("sas_align_edit", x, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, k, off, end, na, out_start,
                      out_dist, out_nruns, out_runs, stream, flags);
}

extern "C" int sas_align_edit_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                                    const uint64_t* off, const void* end, uint64_t na, void* out_start,
                                    uint8_t* out_dist, uint8_t* out_nruns, uint16_t* out_runs, void* stream,
                                    uint32_t flags) {
    return align_impl("sas_align_edit_fixed", x, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, k, off, end, na,
                      out_start, out_dist, out_nruns, out_runs, stream, flags);
}
