// sas_match.hip -- longest-prefix match and matching statistics on the suffix array (sas.h:
// sas_match, sas_match_fixed, sas_match_stats).
//
// For a query q of m chars: lb = the number of suffixes < q (the rank every search here
// returns).  The longest prefix of q that occurs in the text is an lcp of q with one of the
// two suffixes next to that rank, SA[lb - 1] and SA[lb]: any suffix s < q has
// lcp(s, q) <= lcp(SA[lb - 1], q) (the suffixes between s and q in sorted order share at least
// lcp(s, q) chars with both), and symmetrically for s >= q.  So one lower-bound search that
// keeps the exact lcps of its two bounds (Manber-Myers' llcp / rlcp, which k_sa_binary's LCP
// mode carries and drops) answers len, and the bound that attains it gives a position.
//
//   * one lane per query, the wave64 in lock step, grid-stride (k_sa_binary's block and
//     occupancy: MATCH_BLOCK x MATCH_BPC);
//   * with a prefix table and m >= p the search starts from the table's range for q's first
//     p chars (one read, any entry format: common.hpp prefix_range) instead of [0, n);
//   * every compare starts at min(llcp, rlcp) of the bounds it has PROBED.  The table's range
//     ends were never probed and count as lcp 0: a suffix shorter than p chars is keyed zero
//     padded (build_prefix, build_prefix.hip), so a bucket may hold a suffix that shares fewer
//     than p chars with q (text ..AC$, p = 4, q = ACAAG: suffix AC sits in bucket ACAA);
//   * a bound the search never moved (the table's range end; both, for an empty bucket) has no
//     tracked lcp: one direct compare of that neighbour suffix measures it.  The compare is
//     skipped when the other bound's tracked lcp is >= p: the unmoved bound lies in another
//     bucket, its padded key differs from q's first p chars, so its lcp is < p and cannot win;
//   * the matching statistics of a pattern are the same kernel with query i =
//     pattern[i .. min(i + max_len, plen)) derived from i (no offset / length arrays);
//   * the ranks [lo, hi) of q[0 .. len) are the existing range search's, run on the same bytes
//     with qlen = out_len (for fixed / stats queries the kernel leaves their offsets in scratch).
#include "seed_verify.hpp"

#include <type_traits>
#include <vector>

// k_sa_binary's workgroup (search_args.hpp SAS_BIN_BLOCK / SAS_BIN_BPC): 768 lanes, two
// workgroups a CU, 6 waves per SIMD -> at most 80 VGPRs
#define MATCH_BLOCK 768
#define MATCH_BPC 2
#define MATCH_WAVES (MATCH_BLOCK * MATCH_BPC / 256)

#define MATCH_RAGGED 0  // query i = qbytes[qoff[i] .. qoff[i] + qlen[i])
#define MATCH_FIXED 1   // query i = qbytes[i m .. (i + 1) m)
#define MATCH_STATS 2   // query i = qbytes[i .. min(i + m, nq)): nq = the pattern's length

struct MatchArgs {
    const uint64_t* tw;
    uint64_t n;              // text length = SA entries (a whole index)
    const uint8_t* sa;       // SaView<W>
    PrefixView pt;           // prefix == nullptr: every query starts from [0, n)
    const uint8_t* qbytes;
    const uint64_t* qoff;
    const uint32_t* qlen;
    uint32_t m;              // MATCH_FIXED: the length; MATCH_STATS: max_len
    uint32_t mode;
    uint64_t nq;
    uint32_t* out_len;
    uint64_t* out_pos;       // may be null
    uint64_t* out_qoff;      // may be null: query i's byte offset (for the range search)
    uint32_t* bad;
};

template <int QW, int W>
__global__ __launch_bounds__(MATCH_BLOCK, MATCH_WAVES) void k_sa_match(MatchArgs a) {
    // ranks and SA values fit 32 bits beside a u32 SA (n < 2^32)
    using rank_t = typename std::conditional<W == 4, uint32_t, uint64_t>::type;
    const SaView<W> sa{a.sa};
    const uint64_t n = a.n;
    const uint32_t p = a.pt.prefix ? a.pt.prefix_chars : 0u;
    uint32_t bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t qo;
        uint32_t m;
        if (a.mode == MATCH_RAGGED) {
            qo = a.qoff[i];
            m = a.qlen[i];
        } else if (a.mode == MATCH_STATS) {
            const uint64_t rem = a.nq - i;
            qo = i;
            m = rem < (uint64_t)a.m ? (uint32_t)rem : a.m;
        } else {
            qo = i * (uint64_t)a.m;
            m = a.m;
        }
        QueryRegs<QW> q;
        q.load(a.qbytes + qo, m, &bad);

        // lower bound of q over [l, r), with the exact lcps of the bounds probed so far:
        // llcp = lcp(q, SA[l - 1]) once lv, rlcp = lcp(q, SA[r]) once rv (pl / pr: those SA values)
        rank_t l = 0, r = m ? (rank_t)n : (rank_t)0;  // the empty query: every suffix is >= it
        const bool tab = p != 0 && m >= p;
        if (tab) {
            uint64_t l64, r64;
            prefix_range(a.pt, q.w[0] >> (64 - 2 * p), &l64, &r64);
            l = (rank_t)l64;
            r = (rank_t)r64;
        }
        uint32_t llcp = 0, rlcp = 0;
        rank_t pl = 0, pr = 0;
        // integers, not bool: as bool the compiler kept the two flags as lane masks in SGPRs and
        // the QW = 2 / 40-bit SA instance then returned short lcps for whole waves, differently
        // from run to run, on the MI355X (hipcc of ROCm 7; every other instance was right).  The
        // emitted code read correct and the cause was not found; with the flags in VGPRs all six
        // instances match the brute force in repeated runs (longest-prefix match)
        uint32_t lv = 0, rv = 0;
        while (l < r) {
            const rank_t mid = (rank_t)(((uint64_t)l + r) >> 1);
            const uint32_t h = llcp < rlcp ? llcp : rlcp;
            const rank_t pv = (rank_t)sa[mid];
            uint32_t lcp;
            if (suffix_less_from<QW>(a.tw, n, pv, q, h, &lcp)) {
                l = mid + 1;
                llcp = lcp;
                pl = pv;
                lv = 1;
            } else {
                r = mid;
                rlcp = lcp;
                pr = pv;
                rv = 1;
            }
        }
        // the two neighbours of the lower bound l.  Without the table an unmoved bound is the
        // array's end (no neighbour there); with it, one compare unless the bound cannot win
        uint32_t av = 0, bv = 0;
        if ((uint64_t)l < n) {
            if (rv) {
                bv = rlcp;
            } else if (!(tab && lv && llcp >= p)) {
                pr = (rank_t)sa[l];
                (void)suffix_less_from<QW>(a.tw, n, pr, q, 0u, &bv);
            }
        }
        if (l > 0) {
            if (lv) {
                av = llcp;
            } else if (!(tab && rv && rlcp >= p)) {
                pl = (rank_t)sa[l - 1];
                (void)suffix_less_from<QW>(a.tw, n, pl, q, 0u, &av);
            }
        }
        // a skipped neighbour keeps lcp 0 < p <= the other's, so it never equals len below
        const uint32_t len = av > bv ? av : bv;
        a.out_len[i] = len;
        if (a.out_pos) a.out_pos[i] = len == 0 ? n : ((uint64_t)l < n && bv == len ? (uint64_t)pr : (uint64_t)pl);
        if (a.out_qoff) a.out_qoff[i] = qo;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// The range search's answer for an empty prefix is made [0, n) here, whatever its kernels give
__global__ void k_match_empty_ranges(const uint32_t* __restrict__ len, uint64_t nq, uint64_t n,
                                     uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
    GRID_STRIDE(i, nq) {
        if (len[i] == 0) {
            lo[i] = 0;
            hi[i] = n;
        }
    }
}

// SAS_VALIDATE: every byte of every query must be a DNA code 0..3 (fixed / stats queries
// cover one contiguous span of `total` bytes)
__global__ void k_match_validate(const uint8_t* __restrict__ qb, const uint64_t* __restrict__ qoff,
                                 const uint32_t* __restrict__ qlen, uint64_t nq, uint64_t total,
                                 uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    if (qoff) {
        GRID_STRIDE(i, nq) {
            const uint8_t* q = qb + qoff[i];
            const uint32_t m = qlen[i];
            for (uint32_t k = 0; k < m; k++) b |= q[k];
        }
    } else {
        GRID_STRIDE(k, total) b |= qb[k];
    }
    if (b & 0xFCu) atomicOr(bad, 1u);
}

template <int W>
static void launch_match_w(int qw, dim3 grid, hipStream_t st, const MatchArgs& a) {
    if (qw == 1) hipLaunchKernelGGL((k_sa_match<1, W>), grid, dim3(MATCH_BLOCK), 0, st, a);
    else if (qw == 2) hipLaunchKernelGGL((k_sa_match<2, W>), grid, dim3(MATCH_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_sa_match<4, W>), grid, dim3(MATCH_BLOCK), 0, st, a);
}

// query words held in registers: 1 for m <= 32, 2 for m <= 64, else 4 (QueryRegs<4> repacks
// the words past 128 chars from the bytes); an unknown longest query (0) gives 4
static int match_qw(uint64_t maxlen) { return maxlen == 0 ? 4 : maxlen <= 32 ? 1 : maxlen <= 64 ? 2 : 4; }

// All arrays on the device.  maxlen: the batch's longest query when the host knows it, else 0
static int match_device(const char* fn, const sas_index* x, int mode, const uint8_t* qbytes, const uint64_t* qoff,
                        const uint32_t* qlen, uint32_t m, uint64_t nq, uint64_t maxlen, bool validate,
                        uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi, hipStream_t st,
                        uint32_t flags) {
    const bool ranges = out_lo || out_hi;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    PoolBuf sqoff, srange;
    if (ranges && mode != MATCH_RAGGED) TRY(sqoff.alloc(pool, nq * 8, st));
    if (ranges && !(out_lo && out_hi)) {  // the range search writes both bounds
        TRY(srange.alloc(pool, nq * 8, st));
        (out_lo ? out_hi : out_lo) = static_cast<uint64_t*>(srange.p);
    }
    BadFlag bflag;  // armed when it is read back
    if (validate) TRY(bflag.arm(st));
    MatchArgs a{};
    a.tw = x->text_w;
    a.n = x->n;
    a.sa = x->sa;
    if (x->prefix && !(flags & SAS_NO_PREFIX_TABLE))
        a.pt = PrefixView{x->prefix, x->prefix_chars, x->prefix_w, x->prefix_hi40 ? 1u : 0u, x->prefix_key_lo,
                          x->prefix_entries >= 2 ? x->prefix_entries - 2 : 0};
    a.qbytes = qbytes;
    a.qoff = qoff;
    a.qlen = qlen;
    a.m = m;
    a.mode = (uint32_t)mode;
    a.nq = nq;
    a.out_len = out_len;
    a.out_pos = out_pos;
    a.out_qoff = static_cast<uint64_t*>(sqoff.p);
    a.bad = validate ? bflag.ptr() : x->scratch;
    if (validate) {
        const uint64_t total = mode == MATCH_FIXED ? nq * (uint64_t)m : nq;
        hipLaunchKernelGGL(k_match_validate, dim3(grid_for(mode == MATCH_RAGGED ? nq : total)), dim3(256), 0, st,
                           qbytes, mode == MATCH_RAGGED ? qoff : nullptr, qlen, nq, total, bflag.ptr());
    }
    uint64_t blocks = (nq + MATCH_BLOCK - 1) / MATCH_BLOCK;
    const uint64_t capb = (uint64_t)x->num_cus * MATCH_BPC;
    if (blocks > capb) blocks = capb;
    const int qw = match_qw(maxlen);
    with_sa_w(x->sa_w, [&](auto W) { launch_match_w<decltype(W)::value>(qw, dim3((unsigned)blocks), st, a); });
    HIP_TRY(hipGetLastError());
    if (ranges) {
        const uint32_t rflags = (flags & (SAS_NO_PREFIX_TABLE | SAS_RANGE_NO_INLINE)) | SAS_DEVICE_PTRS;
        TRY(sas_search_range(x, qbytes, mode == MATCH_RAGGED ? qoff : a.out_qoff, out_len, nq, out_lo, out_hi, st,
                             rflags));
        hipLaunchKernelGGL(k_match_empty_ranges, dim3(grid_for(nq)), dim3(256), 0, st, out_len, nq, x->n, out_lo,
                           out_hi);
        HIP_TRY(hipGetLastError());
    }
    if (validate) {
        uint32_t hbad = 0;
        TRY(bflag.read(st, &hbad));
        if (hbad) SAS_FAIL(EINVAL, std::string(fn) + ": query bytes must be DNA codes 0..3");
    }
    return 0;
}

// q.ragged: MATCH_RAGGED; q.m: the length of MATCH_FIXED, the cap of MATCH_STATS
static int match_impl(const char* fn, const sas_index* x, int mode, const QueryArgs& q, uint64_t nq, uint32_t* out_len,
                      uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi, void* stream, uint32_t flags) {
    const std::string w(fn);
    // no k and no SAS_LOCATE_U32 here; the range search is asked only when it will run
    TRY(seed_index_checks(w, x, 0, flags & SAS_DEVICE_PTRS, stream, out_lo || out_hi));
    if (nq == 0) return 0;
    if (!q.null_ok(nq) || !out_len) SAS_FAIL(EINVAL, w + ": null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & SAS_DEVICE_PTRS)
        return match_device(fn, x, mode, q.qbytes, q.qoff, q.qlen, q.m, nq, q.ragged ? 0 : (q.m ? q.m : 1),
                            (flags & SAS_VALIDATE) != 0, out_len, out_pos, out_lo, out_hi, st, flags);
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated).
    // The pattern of MATCH_STATS is copied as plen queries of one char
    const bool ragged = q.ragged;
    const uint32_t m = q.m;
    const uint64_t maxlen = ragged ? *std::max_element(q.qlen, q.qlen + nq) : m;
    HostQueries hq;
    HostOutputs ho;
    MmQueries Q;
    TRY(hq.stage("match", QueryArgs{q.qbytes, q.qoff, q.qlen, mode == MATCH_STATS ? 1 : m, ragged}, nq, st, &Q));
    uint32_t* dlen;
    uint64_t *dpos, *dlo, *dhi;
    TRY(ho.twin(out_len, nq * 4, "match lengths out", &dlen));
    TRY(ho.twin(out_pos, nq * 8, "match positions", &dpos));
    TRY(ho.twin(out_lo, nq * 8, "match range starts", &dlo));
    TRY(ho.twin(out_hi, nq * 8, "match range ends", &dhi));
    TRY(match_device(fn, x, mode, Q.qbytes, Q.qoff, ragged ? Q.qlen : nullptr, m, nq, maxlen ? maxlen : 1, true, dlen,
                     dpos, dlo, dhi, st, flags | SAS_DEVICE_PTRS));
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_match(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                         uint64_t nq, uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi,
                         void* stream, uint32_t flags) {
    return match_impl("sas_match", x, MATCH_RAGGED, QueryArgs{qbytes, qoff, qlen, 0, true}, nq, out_len, out_pos, out_lo,
                      out_hi, stream, flags);
}

extern "C" int sas_match_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t* out_len,
                               uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi, void* stream, uint32_t flags) {
    return match_impl("sas_match_fixed", x, MATCH_FIXED, QueryArgs{qbytes, nullptr, nullptr, m, false}, nq, out_len,
                      out_pos, out_lo, out_hi, stream, flags);
}

extern "C" int sas_match_stats(const sas_index* x, const uint8_t* pattern, uint64_t plen, uint32_t max_len,
                               uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi, void* stream,
                               uint32_t flags) {
    return match_impl("sas_match_stats", x, MATCH_STATS, QueryArgs{pattern, nullptr, nullptr, max_len, false}, plen,
                      out_len, out_pos, out_lo, out_hi, stream, flags);
}
