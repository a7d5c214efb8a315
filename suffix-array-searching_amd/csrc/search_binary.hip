// search_binary.hip -- PLAIN / LCP / LLCP: k_sa_binary and its launcher (the algorithms: sas_search.hip).
#include "search_keys.hpp"

// ------------------------------------------------------------------ PLAIN / LCP
// MODE 0: PLAIN, 1: LCP (mlr), 2: LLCP (Manber-Myers with the Llcp/Rlcp entries)
// RANGE (SAS_PREFIX_RANGE, PLAIN / LCP without the LDS top): start from the prefix
// table's range for q's first p chars instead of [0, sa_n), exactly as the reference's
// binary_search does (sas/sa_search.rs:98-101) once its p is not 0
// PLAIN over a u32 SA: a range of at most this many ranks (4 or 8; 0: off) has its SA words
// loaded together for the remaining probes
#ifndef SAS_PLAIN_SA_RUN
#define SAS_PLAIN_SA_RUN 8
#endif
static_assert(SAS_PLAIN_SA_RUN == 0 || SAS_PLAIN_SA_RUN == 4 || SAS_PLAIN_SA_RUN == 8, "SAS_PLAIN_SA_RUN: 0, 4 or 8");
#define BS_PLAIN 0
#define BS_MLR 1
#define BS_LLCP 2
// LLCP: a range of at most this many ranks (0: off, 2..4) has its 16-B entries loaded together
// (consecutive ranks: one or two lines) for the remaining probes (A/B hook)
#ifndef SAS_LLCP_RUN
#define SAS_LLCP_RUN 0
#endif
static_assert(SAS_LLCP_RUN == 0 || (SAS_LLCP_RUN >= 2 && SAS_LLCP_RUN <= 4), "SAS_LLCP_RUN: 0 or 2..4");
// EXQ (QW >= 4): launched only with m <= 32 QW, the query words all in registers (QueryRegsExact:
// no repacking code, fewer registers; the plain form repacks words past them from the bytes)
template <int QW, int MODE, bool TOP, int W, bool RANGE = false, bool EXQ = false>
__global__ __launch_bounds__(BIN_BLOCK(QW), BIN_WAVES(QW)) void k_sa_binary(SearchArgs a) {
    using QR = typename std::conditional<EXQ && (QW > 2), QueryRegsExact<QW>, QueryRegs<QW>>::type;
    // the prefix-relative pivot blocks, the first 15 levels' from LDS (common.hpp RelLayout)
    __shared__ uint4 s_rel[TOP ? SAS_REL_LDS_BYTES / 16 : 1];
    const SaView<W> sa{a.sa};
    if (TOP) {
        stage_rel(s_rel, a.rel, a.rel_lay.lds_bytes);
        __syncthreads();
    }
    uint32_t bad = 0;
    const uint64_t n = a.n;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (uint64_t)gridDim.x * blockDim.x) {
        if (!slot_live(a, i)) continue;
        const uint8_t* qb;
        uint32_t m;
        query_ptr(a, i, &qb, &m);
        QR q;
        q.load(qb, m, &bad);

        // ranks fit 32 bits beside a u32 SA (sa_n < 2^32): fewer registers for l, r, mid
        using rank_t = sa_val_t<W>;
        rank_t l = 0, r = (rank_t)a.sa_n;
        uint32_t k = 1, probes = 0, llcp = 0, rlcp = 0;
        sa_val_t<W> pr = 0;  // SA[r] while prv
        bool prv = false;
        if (RANGE) {
            uint64_t l64, r64;
            prefix_range(a, q.w[0] >> (64 - 2 * a.prefix_chars), &l64, &r64);
            l = (rank_t)l64;
            r = (rank_t)r64;
            probes = 1;  // the reference's cnt counts the table read (:87-89)
        }
        // one probe's outcome: the reference's l / r update (sas/sa_search.rs:102-110); pk:
        // p is known (PLAIN's blocked pivot levels may decide from the key alone)
        auto take = [&](rank_t mid, bool lt, uint32_t lcp, sa_val_t<W> p, bool pk) {
            probes++;
            if (lt) {
                l = mid + 1;
                llcp = lcp;
            } else {
                r = mid;
                rlcp = lcp;
                pr = p;
                prv = pk;
            }
        };
        uint32_t it = 0;
        if (TOP) {
            // the prefix-relative blocks, 4 levels from one 32-B block (LDS, or two 16-B loads
            // of one line: one request): the 8 chars after the block bounds' common prefix of P
            // chars decide each probe unless they tie with q's (then the SA value -- LLCP: from
            // its entry -- and the text from char P + c).  q starts with those P chars
            // (common.hpp), and a key padded past its suffix's end that differs from q there is
            // a proper prefix of q (key < q)
            for (uint32_t g = 0; g < a.rel_lay.groups; ++g) {
                const uint32_t hh = a.rel_lay.h[g];
                uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0;
                if (l < r) rel_block(a, s_rel, g, it, k, hh, b0, b1);
                const uint32_t P = b0.x & 0x7FFFu;
                const uint32_t c0 = q.m > P ? q.m - P : 0u;
                // LCP / LLCP need exact lcps: a block flagged (bit 15) as holding a pivot whose
                // suffix ends inside its key compares no key chars (every probe: the entry and
                // the text from P)
                const uint32_t c = (MODE != BS_PLAIN && (b0.x & 0x8000u)) ? 0u : c0 < 8 ? c0 : 8u;
                const uint32_t mk = c ? (0xFFFFu << (16 - 2 * c)) & 0xFFFFu : 0u;
                const uint32_t qk = (uint32_t)((q.w[0] << (2 * P)) >> 48) & mk;
                for (uint32_t t = 0; t < hh; ++t, ++it) {
                    if (!(l < r)) continue;
                    const rank_t mid = (rank_t)(((uint64_t)l + r) >> 1);
                    const uint32_t key = rel_slot(b0, b1, (1u << t) | (k & ((1u << t) - 1u))) & mk;
                    // LCP / LLCP: lcp = P + the first differing char
                    sa_val_t<W> p = 0;
                    uint32_t lcp = key != qk ? P + (((uint32_t)__clz(key ^ qk) - 16u) >> 1) : 0u;
                    bool lt, pk = false;
                    if (key != qk) {
                        lt = key < qk;
                    } else {
                        if (MODE == BS_LLCP) {
                            const uint4 e = a.llcp[mid];
                            p = (sa_val_t<W>)((uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32));
                        } else {
                            p = (sa_val_t<W>)sa[mid];
                        }
                        // chars [0, P + c) are known equal
                        lt = suffix_less_from<QW>(a.tw, n, p, q, P + c, &lcp);
                        pk = true;
                    }
                    k = 2 * k + (lt ? 1u : 0u);
                    take(mid, lt, lcp, p, pk);
                }
            }
        }
        bool run = false;  // PLAIN, u32 SA: the range's SA words are in sc0..sc2 (from rank rb)
        uint32_t rb = 0;   // LLCP (SAS_LLCP_RUN): the range's entries are in sc0..sc3 (from rank rl)
        uint4 sc0 = make_uint4(0, 0, 0, 0), sc1 = sc0, sc2 = sc0, sc3 = sc0;
        rank_t rl = 0;
        for (; it < a.iters; ++it) {
            if (l < r) {
                const rank_t mid = (rank_t)(((uint64_t)l + r) >> 1);
                const uint32_t h = MODE != BS_PLAIN ? (llcp < rlcp ? llcp : rlcp) : 0u;
                sa_val_t<W> p;
                uint32_t lcp;
                bool lt;
                if (MODE == BS_LLCP) {
                    // one 16-B read: SA[mid], the lcps of the pivot with the interval's
                    // bounds L = SA[l-1] (< q) and R = SA[r] (>= q), and 16 pivot chars
                    // after each.  Manber-Myers: with llcp >= rlcp, Llcp > llcp puts the
                    // pivot on L's side of q (< q, same lcp), Llcp < llcp on R's side
                    // (> q, lcp = Llcp); symmetric with Rlcp.  A tie (or a capped value)
                    // compares from the known lcp, first against the inlined chars.
                    uint4 e;
                    if (SAS_LLCP_RUN) {
                        if (!run && r - l <= SAS_LLCP_RUN) {
                            run = true;
                            rl = l;
                            const uint4* c = a.llcp + l;  // consecutive 16-B entries: one or two lines
                            sc0 = c[0];
                            if (r - l > 1) sc1 = c[1];
                            if (SAS_LLCP_RUN > 2 && r - l > 2) sc2 = c[2];
                            if (SAS_LLCP_RUN > 3 && r - l > 3) sc3 = c[3];
                        }
                        if (run) {
                            const uint32_t o = (uint32_t)(mid - rl);
                            e = o == 0 ? sc0 : o == 1 ? sc1 : (SAS_LLCP_RUN > 3 && o == 3) ? sc3 : sc2;
                        } else {
                            e = a.llcp[mid];
                        }
                    } else {
                        e = a.llcp[mid];
                    }
                    p = (sa_val_t<W>)((uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32));
                    const uint32_t x = (e.y >> 8) & SAS_LLCP_CAP, y = e.y >> 20;
                    uint32_t hh = 0, inl = 0;
                    bool decided = true;
                    if (llcp >= rlcp) {
                        if (x > llcp) { lt = true; lcp = llcp; }
                        else if (x < llcp && x < SAS_LLCP_CAP) { lt = false; lcp = x; }
                        else { decided = false; hh = x; inl = e.z; }
                    } else {
                        if (y > rlcp) { lt = false; lcp = rlcp; }
                        else if (y < rlcp && y < SAS_LLCP_CAP) { lt = true; lcp = y; }
                        else { decided = false; hh = y; inl = e.w; }
                    }
                    if (!decided) {
                        lt = llcp_tie_less<QW>(a.tw, n, p, q, hh, inl, &lcp);
                    }
                } else if (MODE == BS_PLAIN && W == 4 && SAS_PLAIN_SA_RUN) {
                    // the last probes' SA words: once the range holds <= SAS_PLAIN_SA_RUN ranks,
                    // the 16-B chunks covering it are loaded together (one request) and the
                    // remaining probes take their SA values from registers
                    if (!run && r - l <= SAS_PLAIN_SA_RUN) {
                        run = true;
                        rb = l & ~3u;
                        const uint4* c = reinterpret_cast<const uint4*>(a.sa) + (rb >> 2);
                        sc0 = c[0];
                        if (((uint32_t)r - 1) - rb >= 4) sc1 = c[1];
                        if (SAS_PLAIN_SA_RUN > 4 && ((uint32_t)r - 1) - rb >= 8) sc2 = c[2];
                    }
                    if (run) {
                        const uint32_t o = (uint32_t)mid - rb;
                        const uint4 v = o < 4 ? sc0 : (SAS_PLAIN_SA_RUN > 4 && o >= 8 ? sc2 : sc1);
                        const uint32_t oo = o & 3;
                        p = (sa_val_t<W>)(oo == 0 ? v.x : oo == 1 ? v.y : oo == 2 ? v.z : v.w);
                    } else {
                        p = (sa_val_t<W>)sa[mid];
                    }
                    lt = suffix_less_from<QW>(a.tw, n, p, q, h, &lcp);
                } else {
                    p = (sa_val_t<W>)sa[mid];
                    lt = suffix_less_from<QW>(a.tw, n, p, q, h, &lcp);
                }
                take(mid, lt, lcp, p, true);
            }
        }
        // SA[r] not seen yet: r never moved (RANGE: the table's range end) or moved last on a
        // pivot decided from its key alone (rare below a 23-level array: a right move on
        // every one of the last levels' SA probes would have to be missing)
        if (!prv && r < a.sa_n) {
            if (MODE == BS_LLCP) {  // LLCP reads its own entries only
                const uint4 e = a.llcp[r];
                pr = (sa_val_t<W>)((uint64_t)e.x | ((uint64_t)(e.y & 0xFFu) << 32));
            } else {
                pr = (sa_val_t<W>)sa[r];
            }
        }
        a.out_pos[i] = (r >= a.sa_n) ? a.next_pos : (uint64_t)pr;
        if (a.out_probes) a.out_probes[i] = probes;
    }
    if (bad) atomicOr(a.bad, 1u);
}

// PLAIN / LCP / LLCP: the query words all in registers when the batch's longest query is known
// to fit them
template <int MODE, int W>
static void launch_mode(const LaunchCtx& c, const SearchArgs& a, int qw, bool top) {
    with_qw_exq(qw, all_words_in_regs(a, qw), [&](auto Q, auto X) {
        constexpr int QW = decltype(Q)::value;
        constexpr bool EXQ = decltype(X)::value;
        if (top) launch(c, k_sa_binary<QW, MODE, true, W, false, EXQ>, a);
        else launch(c, k_sa_binary<QW, MODE, false, W, false, EXQ>, a);
    });
}

template <int MODE, int W>
static void launch_mode_range(const LaunchCtx& c, const SearchArgs& a, int qw) {
    with_qw(qw, [&](auto Q) { launch(c, k_sa_binary<decltype(Q)::value, MODE, false, W, true>, a); });
}

template <int W>
static void launch_binary_w(const LaunchCtx& c, const SearchArgs& a, int algo, int qw, bool top, bool range) {
    // tagged indexes (W = 8) serve PLAIN and LCP from the whole array only
    if constexpr (W != 8) {
        if (algo == SAS_ALGO_PLAIN && range) return launch_mode_range<BS_PLAIN, W>(c, a, qw);
        if (algo == SAS_ALGO_LCP && range) return launch_mode_range<BS_MLR, W>(c, a, qw);
        if (algo == SAS_ALGO_LLCP) return launch_mode<BS_LLCP, W>(c, a, qw, top);
    }
    if (algo == SAS_ALGO_PLAIN) launch_mode<BS_PLAIN, W>(c, a, qw, top);
    else launch_mode<BS_MLR, W>(c, a, qw, top);
}

void launch_binary(int num_cus, hipStream_t st, const SearchArgs& a, int algo, uint32_t sa_w, int qw, bool top,
                          bool range) {
    // k_sa_binary instances: QW = qw (1, 2, 4, and 8 for anything longer), one lane per query
    const LaunchCtx c = launch_ctx(a.nq, BIN_BLOCK(qw), (uint64_t)num_cus * SAS_BIN_BPC, st);
    if (sa_w == 8) launch_binary_w<8>(c, a, algo, qw, top, range);
    else if (sa_w == 5) launch_binary_w<5>(c, a, algo, qw, top, range);
    else launch_binary_w<4>(c, a, algo, qw, top, range);
}
