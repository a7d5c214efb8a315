// sas_search.hip -- batched suffix-array lookup kernels for gfx950 (MI355X).
//
// Every algorithm returns SA[lower_bound(q)] under Rust slice order, i.e. the
// result of binary_search (sas/sa_search.rs:98-112), bit for bit.
//
//   PLAIN  one lane per query, the whole wave64 walks 64 queries in lockstep for
//          ilog2(n)+1 iterations exactly like binary_search_batch<64>
//          (sas/sa_search.rs:157-196).  The first levels' pivots come from the
//          prefix-relative blocks (common.hpp RelLayout): 15 levels from LDS, then
//          4 levels per request, the rest from SA words and text windows.  The
//          lane remembers SA[r] of the last right move, so the final `sa[l]`
//          (:195) needs no extra load unless a key decided it.
//   LCP    PLAIN + Manber-Myers mlr skipping: chars [0, min(llcp, rlcp)) are known
//          equal and are not compared again (sas/sa_search.rs:344-345 TODO).
//   LLCP   PLAIN's probes with Manber-Myers' Llcp/Rlcp accelerant (SAS_BUILD_LLCP):
//          below the cached top levels a probe reads one 16-B {SA, Llcp, Rlcp,
//          16 chars after each} entry; it decides from the lcps alone unless they
//          tie, and a tie compares the inlined chars before any text.
//   SECTOR / QUAD  B-trees over the fused (32-char key, SA) leaf entries.
//   PREFIX the reference's prefix table made live (sas/sa_search.rs:59-95): the
//          rank range of q's first p chars, then binary_search over it on the
//          fused leaf entries; with inline tables one G-lane group reads the first
//          G suffixes of the range as one request (the headline, k_sa_prefix2).
//   STREE  descend an STree<16,16> over the 16-char keys of the SA (top layers in
//          LDS), giving the key range [r0, r1) of suffixes whose padded 16-char
//          prefix equals the query's; the lower bound lies in [r0, r1] and is
//          found by an exact binary search there (mlr skipping from char 16).
//
// Text compares are 2-bit packed: 32 chars per u64 compare.
//
// The kernels and their launchers live in one unit a family (search_binary / _stree / _sector / _quad /
// _quad_llcp / _prefix / _tagged .hip, over search_args.hpp, search_keys.hpp and search_quad.hpp); this
// unit holds the host dispatch (launch_search, launch_range), the host-pointer staging pipeline and the
// C entry points.  The sharded step's routing and packing are in sas_route.hip.
#include "call_io.hpp"
#include "host_stage.hpp"
#include "search_args.hpp"

#include <chrono>

// Validation pass (SAS_VALIDATE, host-pointer calls): every byte of every query must be a
// DNA code 0..3, including those past the words a search kernel holds in registers.
__global__ void k_validate_queries(const uint8_t* __restrict__ qb, const uint64_t* __restrict__ qoff,
                                   const uint32_t* __restrict__ qlen, uint32_t m_fixed, uint64_t nq,
                                   uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t* q = qoff ? qb + qoff[i] : qb + i * (uint64_t)m_fixed;
        const uint32_t m = qoff ? qlen[i] : m_fixed;
        for (uint32_t k = 0; k < m; k++) b |= q[k];
    }
    if (b & 0xFCu) atomicOr(bad, 1u);
}

static void launch_validate(hipStream_t st, const SearchArgs& a, uint64_t nq) {
    launch(launch_ctx(nq, 256, 65536, st), k_validate_queries, a.qbytes, a.qoff, a.qlen, a.m_fixed, nq, a.bad);
}

// ------------------------------------------------------------------ host dispatch
// Which family serves algo on this index.  PLAIN / LCP / LLCP, the S-tree kernels, TAGGED and
// QUAD_LLCP past 32 chars have workgroup shapes of their own and size their grids themselves.
static int launch_search(const sas_index* x, SearchArgs& a, int algo, int qw, uint32_t flags, hipStream_t st) {
    if (a.nq == 0) return 0;
    // PLAIN, LLCP and INLINE read the pivot levels past the LDS ones from the prefix-relative
    // blocks, which the build makes wherever the array has such levels
    const bool top = !(flags & SAS_NO_LDS_TOP);
    const bool range = (flags & SAS_PREFIX_RANGE) != 0;
    // the others: a lane per query; 4 lanes for QUAD at m <= 32; G on a G-slot inline prefix table
    const bool coop = (algo == SAS_ALGO_QUAD || algo == SAS_ALGO_QUAD_LLCP) && qw == 1;
    const uint64_t g = (algo == SAS_ALGO_PREFIX && x->prefix_w >= 32) ? x->prefix_w / 16 : 1;
    const LaunchCtx c = launch_ctx(a.nq * (coop ? QUAD_G : g), SEARCH_BLOCK, (uint64_t)x->num_cus * BLOCKS_PER_CU, st);
    const bool ko = x->quad_compact != 0;
    if (algo == SAS_ALGO_TAGGED) {
        launch_tagged(x->num_cus, st, a, qw, (flags & SAS_QUERIES_ARE_SLICES) != 0);
    } else if (algo == SAS_ALGO_INTERP) {
        launch_interp(c, a, x->quad_leaves && !ko, x->sa_w, qw, range);
    } else if (x->sa_w == 8 || algo == SAS_ALGO_PLAIN || algo == SAS_ALGO_LCP || algo == SAS_ALGO_LLCP) {
        // a tagged index (sa_w = 8): PLAIN / LCP reading the SA values from the entries
        launch_binary(x->num_cus, st, a, algo, x->sa_w, qw, top, range);
    } else if (algo == SAS_ALGO_STREE || algo == SAS_ALGO_STREE_LLCP) {
        launch_stree(x->num_cus, st, a, algo, x->sa_w, qw);
    } else if (algo == SAS_ALGO_QUAD_LLCP && qw == 1) {
        // m <= 32: QUAD (the 32-char key decides every entry)
        launch_quad(c, a, SAS_ALGO_QUAD, false, 4, qw, top);
    } else if (algo == SAS_ALGO_QUAD_LLCP) {
        launch_quad_llcp(x->num_cus, st, a, qw);
    } else if (algo == SAS_ALGO_QUAD || algo == SAS_ALGO_INLINE) {
        launch_quad(c, a, algo, ko, x->sa_w, qw, top);
    } else if (algo == SAS_ALGO_PREFIX) {
        launch_prefix(c, a, ko, x->sa_w, qw);
    } else {
        launch_sector(c, a, qw);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The index's side of the kernel arguments for a batch of nq queries (m_fixed chars each, or 0:
// ragged); bad-code flag: the index's write-only sink
static SearchArgs fill_args(const sas_index* x, uint64_t nq, uint32_t m_fixed) {
    SearchArgs a{};
    a.nq = nq;
    a.m_fixed = m_fixed;
    a.bad = x->scratch;
    a.tw = x->text_w;
    a.n = x->n;
    a.sa_n = x->sa_n;
    a.next_pos = x->next_pos;
    a.rank_lo = x->rank_lo;
    a.sa = x->sa;
    a.llcp = x->llcp;
    a.prefix = x->prefix;
    a.prefix_chars = x->prefix_chars;
    a.prefix_w = x->prefix_w;
    a.prefix_hi40 = x->prefix_hi40;
    a.pt_base = x->prefix_key_lo;
    a.pt_jmax = x->prefix_entries >= 2 ? x->prefix_entries - 2 : 0;
    a.rel = x->rel;
    a.rel_lay = x->rel_lay;
    a.iters = x->iters;
    a.stree = x->stree;
    for (int h = 0; h < SAS_STREE_MAX_LAYERS; h++) a.stree_off[h] = x->stree_off[h];
    a.stree_height = x->stree_height;
    a.stree_lds_layers = x->stree_lds_layers;
    a.stree_lds_nodes = x->stree_lds_nodes;
    a.sec_inner = x->sec_inner;
    a.sec_leaves = x->sec_leaves;
    for (int h = 0; h < SAS_SECTOR_MAX_LAYERS; h++) a.sec_off[h] = x->sec_off[h];
    a.sec_inner_layers = x->sec_inner_layers;
    a.sec_lds_layers = x->sec_lds_layers;
    a.sec_lds_nodes = x->sec_lds_nodes;
    // non-temporal levels, as for the quad tree below
    a.stree_leaf_nt = (x->sa_n + 15) / 16 * 64 > SAS_NT_BYTES;
    a.quad_inner = x->quad_inner;
    a.quad_leaves = x->quad_leaves;
    for (int h = 0; h < SAS_QUAD_MAX_LAYERS; h++) a.quad_off[h] = x->quad_off[h];
    a.quad_fan = x->quad_fan;
    {
        // non-temporal levels: footprint > 3x the 256 MiB Infinity Cache (see nt_load4)
        const uint64_t big = SAS_NT_BYTES / 64;  // in 64-B nodes
        const uint32_t H = x->quad_inner_layers;
        a.quad_nt_from = H;
        for (uint32_t h = 0; h < H; h++) {
            const uint64_t sz = (h + 1 < H ? x->quad_off[h + 1] : x->quad_inner_nodes) - x->quad_off[h];
            if (sz > big) { a.quad_nt_from = h; break; }
        }
        a.quad_leaf_nt = x->quad_leaf_count > big;
    }
    a.quad_leaf_count = x->quad_leaf_count;
    a.quad_inner_layers = x->quad_inner_layers;
    a.quad_lds_layers = x->quad_lds_layers;
    a.quad_lds_nodes = x->quad_lds_nodes;
    a.tag_table = x->tag_table;
    a.tag_p = x->tag_p;
    a.tag_lines = x->tag_lines;
    a.tag_ovf = x->tag_ovf;
    a.tag_first = x->tag_first;
    a.tw2 = x->text2 ? x->text2 : x->text_w;
    a.tag_sb = x->tag_sb;
    return a;
}

// Algorithm / index / flag compatibility, shared by the search entry points.
static int check_algo(const sas_index* x, int algo, uint32_t flags, const char* where) {
    const std::string w(where);
    if (algo < SAS_ALGO_PLAIN || algo > SAS_ALGO_QUAD_LLCP) SAS_FAIL(EINVAL, w + ": unknown algo");
    if ((flags & SAS_PREFIX_RANGE) &&
        (!x->prefix || (algo != SAS_ALGO_PLAIN && algo != SAS_ALGO_LCP && algo != SAS_ALGO_INTERP)))
        SAS_FAIL(EINVAL, "SAS_PREFIX_RANGE: PLAIN / LCP / INTERP on an index with SAS_BUILD_PREFIX");
    if (algo == SAS_ALGO_PREFIX && !x->prefix) SAS_FAIL(EINVAL, "SAS_ALGO_PREFIX needs SAS_BUILD_PREFIX");
    if (algo == SAS_ALGO_LLCP && !x->llcp) SAS_FAIL(EINVAL, w + ": SAS_ALGO_LLCP needs SAS_BUILD_LLCP");
    if ((algo == SAS_ALGO_QUAD || algo == SAS_ALGO_INLINE) && !x->quad_leaves)
        SAS_FAIL(EINVAL, w + ": SAS_ALGO_QUAD / SAS_ALGO_INLINE need SAS_BUILD_QUAD");
    if (algo == SAS_ALGO_STREE && !x->stree) SAS_FAIL(EINVAL, w + ": SAS_ALGO_STREE needs SAS_BUILD_STREE");
    if (algo == SAS_ALGO_STREE_LLCP && (!x->stree || !x->llcp))
        SAS_FAIL(EINVAL, w + ": SAS_ALGO_STREE_LLCP needs SAS_BUILD_STREE and SAS_BUILD_LLCP");
    if (algo == SAS_ALGO_QUAD_LLCP &&
        (!x->quad_leaves || x->quad_compact || x->quad_fan != SAS_QUAD_FAN || !x->llcp || x->sa_w == 8))
        SAS_FAIL(EINVAL, w + ": SAS_ALGO_QUAD_LLCP needs SAS_BUILD_LLCP and SAS_BUILD_QUAD with fused leaves in the "
                             "absolute layout (SAS_BUILD_QUAD_ABS)");
    if (algo == SAS_ALGO_SECTOR && !x->sec_leaves) SAS_FAIL(EINVAL, w + ": SAS_ALGO_SECTOR needs SAS_BUILD_SECTOR");
    if (algo == SAS_ALGO_TAGGED && !x->tag_table && !x->tag_lines)
        SAS_FAIL(EINVAL, w + ": SAS_ALGO_TAGGED needs SAS_BUILD_TAGGED");
    if (x->tag_lines && (algo != SAS_ALGO_TAGGED || (flags & SAS_PREFIX_RANGE)))
        SAS_FAIL(ENOTSUP, w + ": a bucket-line index (SAS_BUILD_TAG_LINES) has no SA array: SAS_ALGO_TAGGED only");
    if (x->sa_w == 8 && algo != SAS_ALGO_PLAIN && algo != SAS_ALGO_LCP && algo != SAS_ALGO_INTERP &&
        algo != SAS_ALGO_TAGGED)
        SAS_FAIL(EINVAL, w + ": a tagged index (SAS_BUILD_TAGGED) serves TAGGED, PLAIN, LCP and INTERP");
    if (algo == SAS_ALGO_INTERP && x->n >= (1ull << 32))
        SAS_FAIL(ENOTSUP, w + ": interpolation_search<16> needs n < 2^32 (the reference asserts r_val * r "
                              "fits a usize, sas/sa_search.rs:389-392)");
    return 0;
}

// Occurrence-range kernel for the index's structures (a.nq queries; lo to a.out_pos, hi to dhi)
static void launch_range(const sas_index* x, const SearchArgs& a, int qw, uint32_t flags, hipStream_t st,
                         uint64_t* dhi) {
    const bool quad = x->quad_leaves != nullptr;
    const bool ko = x->quad_compact != 0;
    // the prefix table, when built, replaces the two tree descents (one lane per query;
    // G lanes per query on a G-slot inline table)
    const bool ptab = quad && x->prefix && !(flags & SAS_NO_PREFIX_TABLE);
    const bool pair = ptab && !ko && (x->prefix_w == 32 || x->prefix_w == 64) && !(flags & SAS_RANGE_NO_INLINE);
    const uint64_t per = (quad && !ptab) ? QUAD_G : (pair ? x->prefix_w / 16 : 1);
    const LaunchCtx c = launch_ctx(a.nq * per, SEARCH_BLOCK, (uint64_t)x->num_cus * BLOCKS_PER_CU, st);
    if (x->tag_lines || x->tag_table) launch_tagged_range(c, a, qw, dhi);
    else if (ptab) launch_prefix_range(c, a, pair, ko, x->sa_w, qw, dhi);
    else if (quad) launch_quad_range(c, a, ko, x->sa_w, qw, dhi);
    else launch_sector_range(c, a, qw, dhi);
}

// ------------------------------------------------------------------ host-pointer pipeline
void sas_stage_pool_free(StagePool* p) {
    if (!p) return;
    for (StageSet* s : p->free_sets) stage_set_free(s);
    delete p;
}

enum HostMode {
    HM_FIXED = 0,   // fixed-length query bytes, staged as bytes
    HM_RAGGED = 1,  // ragged query bytes, gathered chunk by chunk
    HM_PACK = 2,    // fixed-length bytes, m <= 32, PREFIX: packed to 2-bit words on the host
    HM_WORDS = 3,   // the caller's packed words (sas_search_packed)
};

// Synchronous search of host arrays through the index's pinned staging slots (host_stage.hpp).
// Returns with out_pos / out_probes filled; EINVAL (after the whole batch) if a query byte
// is not a DNA code.
// out_hi non-null: occurrence ranges (launch_range) instead of a search; a chunk then holds
// at most cap_q / 2 queries and its lo and hi share the slot's position buffers.
static int host_pipeline(const sas_index* x, int mode, const uint8_t* qbytes, const uint64_t* qoff,
                         const uint32_t* qlen, const uint64_t* qwords, uint32_t m, uint64_t nq, int algo,
                         uint64_t* out_pos, uint32_t* out_probes, hipStream_t user_st, uint32_t flags,
                         uint64_t* out_hi = nullptr) {
    StageLease lease;
    TRY(stage_acquire(x, &lease));
    StageSet& S = *lease.set;
    const uint64_t cap_q = out_hi ? S.cap_q / 2 : S.cap_q;
    HIP_TRY(hipStreamSynchronize(user_st));  // the caller's earlier work on its stream
    const bool validate = mode == HM_FIXED || mode == HM_RAGGED;
    std::atomic<uint32_t> host_bad{0};
    uint32_t dev_bad = 0;
    HostPool& pool = HostPool::get();
    int err = 0;
    // pieces of one pool job: the copy-out of the slot's previous chunk (positions, probes;
    // the caller's pages are often touched here for the first time, so page faults spread
    // over the pool too) and the fill of the new chunk run together
    constexpr uint64_t OUT_PIECE = 1u << 17;  // positions per copy-out piece (1 MiB)
    auto copy_out = [&](const StageSlot& sl, uint64_t piece) {
        const uint64_t k = sl.e - sl.s, b = piece * OUT_PIECE, e = std::min(k, b + OUT_PIECE);
        memcpy(out_pos + sl.s + b, sl.h_out + b, (e - b) * 8);
        if (out_hi) memcpy(out_hi + sl.s + b, sl.h_out + k + b, (e - b) * 8);
        if (out_probes) memcpy(out_probes + sl.s + b, sl.h_pr + b, (e - b) * 4);
    };
    auto out_pieces = [&](const StageSlot& sl) -> int {
        return sl.busy ? (int)((sl.e - sl.s + OUT_PIECE - 1) / OUT_PIECE) : 0;
    };
    // SAS_STAGE_TRACE=1: per-phase host time of the call on stderr (tuning aid)
    static const bool trace = getenv("SAS_STAGE_TRACE") != nullptr;
    using clk = std::chrono::steady_clock;
    double t_wait = 0, t_job = 0, t_enq = 0;
    auto t_all = clk::now();
    uint64_t s = 0;
    int chunks = 0;
    for (int c = 0; s < nq && !err; c++, chunks++) {
        StageSlot& sl = S.slot[c % SAS_STAGE_SLOTS];
        auto t0 = clk::now();
        if (sl.busy) {
            HIP_TRY(hipStreamSynchronize(sl.st));
            if (validate) dev_bad |= *sl.h_bad;
        }
        auto t1 = clk::now();
        t_wait += std::chrono::duration<double, std::milli>(t1 - t0).count();
        const int po = out_pieces(sl);
        SearchArgs a = fill_args(x, 0, m);
        uint64_t k = 0, in_bytes = 0;
        int qw = 1;
        // the new chunk: its extent, and a fill function over `pi` pieces
        int pi_n = 0;
        std::function<void(int)> fill;
        if (mode == HM_FIXED || mode == HM_WORDS) {
            const uint64_t unit = mode == HM_FIXED ? std::max(m, 1u) : 8;
            k = std::min<uint64_t>(nq - s, std::min<uint64_t>(S.cap_bytes / unit, cap_q));
            in_bytes = k * unit;
            const uint8_t* src = mode == HM_FIXED ? qbytes + s * m : reinterpret_cast<const uint8_t*>(qwords + s);
            const uint64_t piece = 1u << 20;
            pi_n = (int)((in_bytes + piece - 1) / piece);
            fill = [&sl, src, in_bytes, piece](int i) {
                const uint64_t b = (uint64_t)i * piece;
                memcpy(sl.h_in + b, src + b, std::min(piece, in_bytes - b));
            };
            if (mode == HM_FIXED) qw = qw_for(m);
            a.m_max = mode == HM_FIXED ? m : 0;
        } else if (mode == HM_PACK) {
            // smaller chunks than the byte modes: the host packing is the longest stage, and
            // the pipeline fills and drains faster
            k = std::min<uint64_t>(nq - s, std::min<uint64_t>(cap_q, SAS_STAGE_PACK_Q));
            in_bytes = k * 8;
            constexpr uint64_t per = 16384;
            pi_n = (int)((k + per - 1) / per);
            uint64_t* w = reinterpret_cast<uint64_t*>(sl.h_in);
            const uint8_t* src = qbytes + s * m;
            fill = [&host_bad, w, src, k, m](int i) {
                const uint64_t b = (uint64_t)i * per, e = std::min(k, b + per);
                if (host_pack_words(src + b * m, m, e - b, w + b) & 0xFC) host_bad.fetch_or(1);
            };
        } else {  // ragged: consecutive queries up to the byte and count caps (at least one)
            uint64_t bytes = 0, e = s;
            uint32_t maxlen = 0;
            while (e < nq && e - s < cap_q && (e == s || bytes + qlen[e] <= S.cap_bytes)) {
                sl.h_off[e - s] = bytes;
                sl.h_len[e - s] = qlen[e];
                bytes += qlen[e];
                maxlen = std::max(maxlen, qlen[e]);
                e++;
            }
            k = e - s;
            in_bytes = bytes;
            constexpr uint64_t per = 4096;
            const uint64_t s0 = s;
            pi_n = (int)((k + per - 1) / per);
            fill = [&sl, qbytes, qoff, k, s0](int i) {
                const uint64_t b = (uint64_t)i * per, ee = std::min(k, b + per);
                for (uint64_t j = b; j < ee; j++) memcpy(sl.h_in + sl.h_off[j], qbytes + qoff[s0 + j], sl.h_len[j]);
            };
            qw = qw_for(maxlen);
            a.m_max = maxlen ? maxlen : 1;
        }
        // h_out of this slot is read by the copy-out pieces before the new chunk's D2H is
        // queued below, so both can run in one job
        pool.run(po + pi_n, [&](int i) {
            if (i < po) copy_out(sl, (uint64_t)i);
            else fill(i - po);
        });
        auto t2 = clk::now();
        t_job += std::chrono::duration<double, std::milli>(t2 - t1).count();
        sl.busy = false;
        HIP_TRY(hipMemcpyAsync(sl.d_in, sl.h_in, in_bytes, hipMemcpyHostToDevice, sl.st));
        if (mode == HM_RAGGED) {
            HIP_TRY(hipMemcpyAsync(sl.d_off, sl.h_off, k * 8, hipMemcpyHostToDevice, sl.st));
            HIP_TRY(hipMemcpyAsync(sl.d_len, sl.h_len, k * 4, hipMemcpyHostToDevice, sl.st));
            a.qoff = sl.d_off;
            a.qlen = sl.d_len;
        }
        if (mode == HM_WORDS || mode == HM_PACK) a.qwords = reinterpret_cast<const uint64_t*>(sl.d_in);
        else a.qbytes = sl.d_in;
        a.nq = k;
        a.out_pos = sl.d_out;
        a.out_probes = out_probes ? sl.d_pr : nullptr;
        if (validate) {
            HIP_TRY(hipMemsetAsync(sl.d_bad, 0, 4, sl.st));
            a.bad = sl.d_bad;
            launch_validate(sl.st, a, k);
        }
        if (out_hi) {
            launch_range(x, a, qw, flags, sl.st, sl.d_out + k);
            HIP_TRY(hipGetLastError());
        } else if ((err = launch_search(x, a, algo, qw, flags | SAS_DEVICE_PTRS, sl.st))) {
            break;
        }
        HIP_TRY(hipMemcpyAsync(sl.h_out, sl.d_out, (out_hi ? 2 : 1) * k * 8, hipMemcpyDeviceToHost, sl.st));
        if (out_probes) HIP_TRY(hipMemcpyAsync(sl.h_pr, sl.d_pr, k * 4, hipMemcpyDeviceToHost, sl.st));
        if (validate) HIP_TRY(hipMemcpyAsync(sl.h_bad, sl.d_bad, 4, hipMemcpyDeviceToHost, sl.st));
        sl.busy = true;
        sl.s = s;
        sl.e = s + k;
        s += k;
        t_enq += std::chrono::duration<double, std::milli>(clk::now() - t2).count();
    }
    // drain: the last chunks' copy-outs, all slots in one job
    if (!err) {
        int tot = 0, base[SAS_STAGE_SLOTS];
        for (int c = 0; c < SAS_STAGE_SLOTS; c++) {
            StageSlot& sl = S.slot[c];
            if (sl.busy) {
                HIP_TRY(hipStreamSynchronize(sl.st));
                if (validate) dev_bad |= *sl.h_bad;
            }
            base[c] = tot;
            tot += out_pieces(sl);
        }
        pool.run(tot, [&](int i) {
            int c = SAS_STAGE_SLOTS - 1;
            while (c > 0 && i < base[c]) c--;
            copy_out(S.slot[c], (uint64_t)(i - base[c]));
        });
        for (auto& sl : S.slot) sl.busy = false;
    }
    if (trace)
        fprintf(stderr, "[sas stage] mode %d nq %llu chunks %d threads %d: wait %.2f ms, fill+copy-out %.2f ms, "
                        "enqueue %.2f ms, total %.2f ms\n",
                mode, (unsigned long long)nq, chunks, pool.size(), t_wait, t_job, t_enq,
                std::chrono::duration<double, std::milli>(clk::now() - t_all).count());
    if (err) return err;
    if (dev_bad || host_bad.load()) SAS_FAIL(EINVAL, "search: query bytes must be DNA codes 0..3");
    return 0;
}

// Host arrays go through the pinned, chunked pipeline (host_pipeline) unless one query alone
// exceeds a staging chunk (qlen null: fixed length m_fixed)
static bool fits_stage(uint32_t m_fixed, const uint32_t* qlen, uint64_t nq) {
    uint64_t maxlen = m_fixed;
    for (uint64_t k = 0; qlen && k < nq; k++) maxlen = qlen[k] > maxlen ? qlen[k] : maxlen;
    return maxlen <= SAS_STAGE_BYTES;
}

// A direct call: device pointers, or host arrays with a query longer than a staging chunk.
// Such host arrays take the synchronous host-pointer path of call_io.hpp (HostQueries,
// HostOutputs), not the stream-ordered allocator.
// begin() wires a's query, bad-code and output pointers (dev_out[0] is a.out_pos), sets the
// batch's query words (qw, a.m_max) and launches the validation.  After the caller's kernels,
// end() copies host outputs out, synchronises if anything is read back and fails with
// "<what>: query bytes must be DNA codes 0..3" on an invalid code: the caller's arrays are
// filled even then.
struct DirectIo {  // the caller's arrays, host or device
    const uint8_t* qbytes;
    const uint64_t* qoff;  // null: fixed length a.m_fixed
    const uint32_t* qlen;
    int nout;  // position arrays: one for a search, two for a range
    uint64_t* out[2];
    uint32_t* probes;
};

struct DirectCall {
    int qw = 4;
    bool dev = false, check_bad = false;
    uint64_t* dev_out[2] = {};
    BadFlag bflag;
    HostQueries hq;
    HostOutputs ho;

    // a.nq and a.m_fixed are set
    int begin(const sas_index* x, hipStream_t st, uint32_t flags, SearchArgs& a, const DirectIo& io) {
        dev = (flags & SAS_DEVICE_PTRS) != 0;
        const bool ragged = io.qoff != nullptr;
        const uint64_t nq = a.nq;
        // invalid-code flag: a per-call word when it is read back, so that concurrent calls
        // on other streams (allowed: the index is immutable) never see each other's flags;
        // otherwise the index's write-only sink (fill_args)
        check_bad = !dev || (flags & SAS_VALIDATE);
        if (check_bad) {
            TRY(bflag.arm(st));
            a.bad = bflag.ptr();
        }
        if (dev) {  // ragged: the longest query is unknown
            qw = ragged ? 4 : qw_for(a.m_fixed);
            a.m_max = ragged ? 0 : a.m_fixed;
            a.qbytes = io.qbytes;
            a.qoff = io.qoff;
            a.qlen = io.qlen;
            dev_out[0] = io.out[0];
            dev_out[1] = io.out[1];
            a.out_probes = io.probes;
        } else {
            const uint32_t maxlen = ragged ? *std::max_element(io.qlen, io.qlen + nq) : a.m_fixed;
            qw = qw_for(maxlen);
            a.m_max = maxlen ? maxlen : 1;
            MmQueries Q;
            TRY(hq.stage("search", QueryArgs{io.qbytes, io.qoff, io.qlen, a.m_fixed, ragged}, nq, st, &Q));
            a.qbytes = Q.qbytes;
            a.qoff = Q.qoff;
            a.qlen = Q.qlen;
            for (int i = 0; i < io.nout; i++) TRY(ho.twin(io.out[i], nq * 8, "search positions", &dev_out[i]));
            TRY(ho.twin(io.probes, nq * 4, "search probes", &a.out_probes));
        }
        a.out_pos = dev_out[0];
        if (check_bad) launch_validate(st, a, nq);  // every query byte, not only those a kernel packs
        return 0;
    }

    int end(hipStream_t st, const char* what) {
        if (!check_bad) return 0;
        TRY(ho.copy_back(st));
        uint32_t hbad = 0;
        TRY(bflag.read(st, &hbad));
        if (hbad) SAS_FAIL(EINVAL, std::string(what) + ": query bytes must be DNA codes 0..3");
        return 0;
    }
};

// queries t[qoff[k] .. qoff[k] + qlen[k]) of the indexed text (SAS_QUERIES_ARE_SLICES)
__global__ void k_validate_slices(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qlen, uint64_t nq,
                                  uint64_t n, uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x)
        b |= (qoff[i] > n || qlen[i] > n - qoff[i]) ? 1u : 0u;
    if (b) atomicOr(bad, 1u);
}

static int slices_impl(const sas_index* x, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq, int algo,
                       uint64_t* out_pos, uint32_t* out_probes, void* stream, uint32_t flags) {
    if (algo != SAS_ALGO_TAGGED) SAS_FAIL(EINVAL, "SAS_QUERIES_ARE_SLICES: SAS_ALGO_TAGGED only");
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "SAS_QUERIES_ARE_SLICES: device pointers only (SAS_DEVICE_PTRS)");
    if (!qoff || !qlen) SAS_FAIL(EINVAL, "SAS_QUERIES_ARE_SLICES: null qoff/qlen");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SearchArgs a = fill_args(x, nq, 0);
    a.qoff = qoff;
    a.qlen = qlen;
    a.out_pos = out_pos;
    a.out_probes = out_probes;
    // every slice inside the text: checked first, always (an out-of-range slice would read
    // past the packed text); the call synchronises to read the flag back
    BadFlag bflag;
    TRY(bflag.arm(st));
    launch(launch_ctx(nq, 256, 65536, st), k_validate_slices, qoff, qlen, nq, x->n, bflag.ptr());
    uint32_t hbad = 0;
    TRY(bflag.read(st, &hbad));
    if (hbad) SAS_FAIL(EINVAL, "SAS_QUERIES_ARE_SLICES: a slice reaches past the text");
    return launch_search(x, a, algo, 4, flags, st);
}

static int search_impl(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                       uint32_t m_fixed, uint64_t nq, int algo, uint64_t* out_pos, uint32_t* out_probes,
                       void* stream, uint32_t flags) {
    if (!x) SAS_FAIL(EINVAL, "search: null index");
    TRY(check_algo(x, algo, flags, "search"));
    if (nq == 0) return 0;
    if (!out_pos) SAS_FAIL(EINVAL, "search: null out_pos");
    if (flags & SAS_QUERIES_ARE_SLICES) return slices_impl(x, qoff, qlen, nq, algo, out_pos, out_probes, stream, flags);
    if (!qbytes) SAS_FAIL(EINVAL, "search: null qbytes");
    bool ragged = qoff != nullptr;
    if (ragged && !qlen) SAS_FAIL(EINVAL, "search: qoff without qlen");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool dev = flags & SAS_DEVICE_PTRS;

    if (!dev && fits_stage(m_fixed, ragged ? qlen : nullptr, nq)) {
        const bool pack = !ragged && algo == SAS_ALGO_PREFIX && m_fixed > 0 && m_fixed <= 32 &&
                          !(flags & SAS_PREFIX_RANGE);
        return host_pipeline(x, ragged ? HM_RAGGED : (pack ? HM_PACK : HM_FIXED), qbytes, qoff, qlen, nullptr,
                             m_fixed, nq, algo, out_pos, out_probes, st, flags);
    }
    SearchArgs a = fill_args(x, nq, m_fixed);
    DirectCall call;
    TRY(call.begin(x, st, flags, a, {qbytes, qoff, qlen, 1, {out_pos, nullptr}, out_probes}));
    TRY(launch_search(x, a, algo, call.qw, flags, st));
    return call.end(st, "search");
}

extern "C" int sas_search_batch(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff,
                                const uint32_t* qlen, uint64_t nq, int algo, uint64_t* out_pos, uint32_t* out_probes,
                                void* stream, uint32_t flags) {
    if (nq && (!qoff || !qlen)) SAS_FAIL(EINVAL, "sas_search_batch: null qoff/qlen");
    return search_impl(index, qbytes, qoff, qlen, 0, nq, algo, out_pos, out_probes, stream, flags);
}

extern "C" int sas_search_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, int algo,
                                uint64_t* out_pos, uint32_t* out_probes, void* stream, uint32_t flags) {
    return search_impl(index, qbytes, nullptr, nullptr, m, nq, algo, out_pos, out_probes, stream, flags);
}

__global__ void k_pack_queries(const uint8_t* __restrict__ qb, uint32_t m, uint64_t nq, uint64_t* __restrict__ out,
                               uint32_t* __restrict__ bad) {
    uint32_t b = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = pack_query_word(qb + i * (uint64_t)m, m, 0, &b);
    if (b) atomicOr(bad, 1u);
}

extern "C" int sas_pack_queries(const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t* out_words, void* stream,
                                uint32_t flags) {
    if (m > 32) SAS_FAIL(EINVAL, "sas_pack_queries: m must be <= 32");
    if (nq == 0) return 0;
    if (!qbytes || !out_words) SAS_FAIL(EINVAL, "sas_pack_queries: null argument");
    if (!(flags & SAS_DEVICE_PTRS)) {  // host arrays: the staging pipeline's packer on the host pool
        std::atomic<uint32_t> bad{0};
        constexpr uint64_t per = 16384;
        HostPool::get().run((int)((nq + per - 1) / per), [&](int i) {
            const uint64_t b = (uint64_t)i * per, e = std::min(nq, b + per);
            if (host_pack_words(qbytes + b * m, m, e - b, out_words + b) & 0xFC) bad.fetch_or(1);
        });
        if (bad.load()) SAS_FAIL(EINVAL, "sas_pack_queries: query bytes must be DNA codes 0..3");
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    BadFlag bflag;
    TRY(bflag.arm(st));
    launch(launch_ctx(nq, 256, 65536, st), k_pack_queries, qbytes, m, nq, out_words, bflag.ptr());
    HIP_TRY(hipGetLastError());
    uint32_t hbad = 0;
    TRY(bflag.read(st, &hbad));
    if (hbad) SAS_FAIL(EINVAL, "sas_pack_queries: query bytes must be DNA codes 0..3");
    return 0;
}

extern "C" int sas_search_packed(const sas_index* x, const uint64_t* qwords, uint32_t m, uint64_t nq, int algo,
                                 uint64_t* out_pos, uint32_t* out_probes, void* stream, uint32_t flags) {
    if (!x) SAS_FAIL(EINVAL, "sas_search_packed: null index");
    if (algo != SAS_ALGO_PREFIX) SAS_FAIL(EINVAL, "sas_search_packed: SAS_ALGO_PREFIX only");
    if (!x->prefix) SAS_FAIL(EINVAL, "sas_search_packed: needs SAS_BUILD_PREFIX");
    if (m > 32) SAS_FAIL(EINVAL, "sas_search_packed: m must be <= 32");
    if (nq == 0) return 0;
    if (!qwords || !out_pos) SAS_FAIL(EINVAL, "sas_search_packed: null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!(flags & SAS_DEVICE_PTRS))  // host words: the pinned staging pipeline
        return host_pipeline(x, HM_WORDS, nullptr, nullptr, nullptr, qwords, m, nq, algo, out_pos, out_probes, st,
                             flags);
    SearchArgs a = fill_args(x, nq, m);  // packed words hold no invalid codes: no flag of its own
    a.qwords = qwords;
    a.out_pos = out_pos;
    a.out_probes = out_probes;
    return launch_search(x, a, algo, 1, flags, st);
}

extern "C" int sas_search_buckets(const sas_index* x, const void* queries, uint32_t m, uint32_t nbuckets,
                                  uint64_t cap, const uint64_t* counts, int algo, uint64_t* out_pos, void* stream,
                                  uint32_t flags) {
    if (!x) SAS_FAIL(EINVAL, "sas_search_buckets: null index");
    TRY(check_algo(x, algo, flags & ~SAS_PREFIX_RANGE, "sas_search_buckets"));
    if (!(flags & SAS_DEVICE_PTRS)) SAS_FAIL(EINVAL, "sas_search_buckets: device pointers only (SAS_DEVICE_PTRS)");
    if (flags & SAS_PREFIX_RANGE) SAS_FAIL(EINVAL, "sas_search_buckets: SAS_PREFIX_RANGE is not supported");
    const bool packed = (flags & SAS_ROUTE_PACKED) != 0;
    if (m == 0 || (packed && (m > 32 || algo != SAS_ALGO_PREFIX)))
        SAS_FAIL(EINVAL, "sas_search_buckets: m >= 1; packed words need SAS_ALGO_PREFIX and m <= 32");
    // the kernels that skip unfilled slots: one lane (or one lane group) per query
    const bool ok = algo == SAS_ALGO_PLAIN || algo == SAS_ALGO_LCP || algo == SAS_ALGO_LLCP ||
                    algo == SAS_ALGO_PREFIX || (algo == SAS_ALGO_QUAD && m <= 32);
    if (!ok || x->sa_w == 8) SAS_FAIL(ENOTSUP, "sas_search_buckets: PLAIN, LCP, LLCP, PREFIX, or QUAD with m <= 32");
    const uint64_t nq = (uint64_t)nbuckets * cap;
    if (nq == 0) return 0;
    if (cap >= (1ull << 32) || nq >= (1ull << 32)) SAS_FAIL(EINVAL, "sas_search_buckets: buckets x cap >= 2^32");
    if (!queries || !counts || !out_pos) SAS_FAIL(EINVAL, "sas_search_buckets: null argument");
    HIP_TRY(hipSetDevice(x->device));
    // device pointers: codes unchecked, as sas_search_fixed without SAS_VALIDATE
    SearchArgs a = fill_args(x, nq, m);
    a.m_max = m;
    if (packed) a.qwords = static_cast<const uint64_t*>(queries);
    else a.qbytes = static_cast<const uint8_t*>(queries);
    a.out_pos = out_pos;
    a.bcounts = counts;
    a.bcap = (uint32_t)cap;
    return launch_search(x, a, algo, packed ? 1 : qw_for(m), flags, static_cast<hipStream_t>(stream));
}

extern "C" int sas_time_fixed(const sas_index* x, const uint8_t* d_qbytes, uint32_t m, uint64_t nq, int algo,
                              uint64_t* d_out_pos, int reps, void* stream, uint32_t flags, double* kernel_ns,
                              double* call_ns) {
    if (!x || !d_qbytes || !d_out_pos || reps < 1) SAS_FAIL(EINVAL, "sas_time_fixed: bad argument");
    TRY(check_algo(x, algo, flags, "sas_time_fixed"));
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SearchArgs a = fill_args(x, nq, m);
    a.m_max = m;
    a.qbytes = d_qbytes;
    a.out_pos = d_out_pos;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipStreamSynchronize(st));
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(e0, st));
    for (int r = 0; r < reps; r++) {
        int rc = launch_search(x, a, algo, qw_for(m), flags | SAS_DEVICE_PTRS, st);
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    auto t1 = std::chrono::steady_clock::now();
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (kernel_ns) *kernel_ns = ms * 1e6 / reps;
    if (call_ns) *call_ns = std::chrono::duration<double, std::nano>(t1 - t0).count() / reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
}

// ragged (qoff, qlen) or fixed-length (qoff == nullptr: m_fixed chars per query)
static int range_impl(const sas_index* x, const uint8_t* qbytes, uint32_t m_fixed, const uint64_t* qoff,
                      const uint32_t* qlen, uint64_t nq, uint64_t* out_lo, uint64_t* out_hi, void* stream,
                      uint32_t flags) {
    if (!x) SAS_FAIL(EINVAL, "sas_search_range: null index");
    if (!x->sec_leaves && !x->quad_leaves && !x->tag_table && !x->tag_lines)
        SAS_FAIL(EINVAL, "sas_search_range: needs SAS_BUILD_QUAD, SAS_BUILD_SECTOR or SAS_BUILD_TAGGED");
    const bool ragged = qoff != nullptr || qlen != nullptr;
    if (nq == 0) return 0;
    if (!qbytes || !out_lo || !out_hi || (ragged && (!qoff || !qlen)))
        SAS_FAIL(EINVAL, "sas_search_range: null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool dev = flags & SAS_DEVICE_PTRS;
    if (!dev && fits_stage(m_fixed, ragged ? qlen : nullptr, nq))
        return host_pipeline(x, ragged ? HM_RAGGED : HM_FIXED, qbytes, qoff, qlen, nullptr, m_fixed, nq, -1, out_lo,
                             nullptr, st, flags, out_hi);
    SearchArgs a = fill_args(x, nq, ragged ? 0 : m_fixed);
    DirectCall call;
    TRY(call.begin(x, st, flags, a, {qbytes, ragged ? qoff : nullptr, qlen, 2, {out_lo, out_hi}, nullptr}));
    launch_range(x, a, call.qw, flags, st, call.dev_out[1]);
    HIP_TRY(hipGetLastError());
    return call.end(st, "sas_search_range");
}

extern "C" int sas_search_range(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                                uint64_t nq, uint64_t* out_lo, uint64_t* out_hi, void* stream, uint32_t flags) {
    if (nq && (!qoff || !qlen)) SAS_FAIL(EINVAL, "sas_search_range: null qoff/qlen");
    return range_impl(x, qbytes, 0, qoff, qlen, nq, out_lo, out_hi, stream, flags);
}

extern "C" int sas_search_range_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                                      uint64_t* out_lo, uint64_t* out_hi, void* stream, uint32_t flags) {
    return range_impl(x, qbytes, m, nullptr, nullptr, nq, out_lo, out_hi, stream, flags);
}
