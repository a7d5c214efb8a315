// search_args.hpp -- what every lookup kernel family (search_*.hip), the host dispatch (sas_search.hip)
// and the sharded step (sas_route.hip) share: the kernel arguments, the workgroup shapes, the launch
// helpers and the family launchers' declarations.  Host and device inline code only.
#pragma once
#include "common.hpp"

#include <type_traits>

#define SEARCH_BLOCK 1024
#define BLOCKS_PER_CU 2
// the binary searches (k_sa_binary: PLAIN, LCP, LLCP) and the S-tree descents (k_sa_stree,
// k_sa_stree4x: STREE, STREE_LLCP): workgroup size and workgroups per CU.
// The launch bound follows them (waves per SIMD = block x blocks / 256), which caps the VGPRs:
// 1024 x 2 -> 8 waves, 64 VGPRs; 768 x 2 -> 6 waves, 80 VGPRs (the LDS pivot groups, 72.5 KiB
// a workgroup, allow two workgroups a CU either way)
#ifndef SAS_BIN_BLOCK
#define SAS_BIN_BLOCK 768
#endif
#ifndef SAS_BIN_BPC
#define SAS_BIN_BPC 2
#endif
#define SAS_BIN_WAVES (SAS_BIN_BLOCK * SAS_BIN_BPC / 256)
// ... for queries past 64 chars (4 or 8 query words in registers): an A/B hook
#ifndef SAS_BIN_BLOCK_LONG
#define SAS_BIN_BLOCK_LONG SAS_BIN_BLOCK
#endif
#define BIN_BLOCK(QW) ((QW) <= 2 ? SAS_BIN_BLOCK : SAS_BIN_BLOCK_LONG)
#define BIN_WAVES(QW) (BIN_BLOCK(QW) * SAS_BIN_BPC / 256)

struct SearchArgs {
    const uint64_t* tw;
    uint64_t n;          // text length
    uint64_t sa_n;       // SA entries held by this index
    uint64_t next_pos;   // answer when the lower bound is sa_n (n for a whole index)
    uint64_t rank_lo;    // global rank of sa[0]
    const uint8_t* sa;       // SaView<W> (u32 or packed 40-bit)
    const uint4* llcp;       // SAS_BUILD_LLCP entries (k_sa_binary<.., BS_LLCP, ..>)
    const uint8_t* prefix;   // SAS_BUILD_PREFIX table (k_sa_prefix): u32 or packed 40-bit entries
    uint32_t prefix_chars;
    uint32_t prefix_w;       // bytes per table entry (4 or 5)
    uint32_t prefix_hi40;    // inline slots: SA bits 32..39 in slot 1's rank word
    uint64_t pt_base;        // the table's first key (0, or a part's first suffix's key)
    uint64_t pt_jmax;        // its last entry a lookup may start at (entries - 2)
    const uint8_t* rel;      // the prefix-relative pivot blocks (common.hpp RelLayout)
    RelLayout rel_lay;
    uint32_t iters;
    const uint32_t* stree;
    uint64_t stree_off[SAS_STREE_MAX_LAYERS];
    uint32_t stree_height;
    uint32_t stree_lds_layers;
    uint32_t stree_lds_nodes;
    const uint32_t* sec_inner;
    const uint4* sec_leaves;
    uint64_t sec_off[SAS_SECTOR_MAX_LAYERS];
    uint32_t sec_inner_layers;
    uint32_t sec_lds_layers;
    uint32_t sec_lds_nodes;
    const uint4* quad_inner;
    const uint4* quad_leaves;
    uint64_t quad_off[SAS_QUAD_MAX_LAYERS];
    uint64_t quad_leaf_count;
    uint32_t stree_leaf_nt;  // S-tree leaf layer (16-char keys) read non-temporal
    uint32_t quad_fan;
    uint32_t quad_nt_from;   // first inner layer read with non-temporal loads
    uint32_t quad_leaf_nt;   // leaves read with non-temporal loads
    uint32_t quad_inner_layers;
    uint32_t quad_lds_layers;
    uint32_t quad_lds_nodes;
    const uint64_t* tag_table;  // SAS_BUILD_TAGGED bucket table (sa = tagged entries, W = 8)
    uint32_t tag_p;
    const uint64_t* tag_lines;  // SAS_BUILD_TAG_LINES: 128-B bucket lines (common.hpp)
    const uint64_t* tag_ovf;    // and their overflow entries
    const uint64_t* tag_first;  // and the buckets' first ranks
    const uint64_t* tw2;        // and the second text copy (tl_text)
    uint32_t tag_sb;            // SA bits of a line entry
    const uint8_t* qbytes;
    const uint64_t* qwords;  // sas_search_packed: 2-bit packed fixed-length queries (PREFIX)
    const uint64_t* qoff;
    const uint32_t* qlen;
    uint32_t m_fixed;
    uint32_t m_max;          // longest query of the batch when the host knows it (0: unknown)
    uint64_t nq;
    uint64_t* out_pos;
    uint32_t* out_probes;
    uint32_t* bad;
    const uint64_t* bcounts; // sas_search_buckets: queries per bucket (null: every slot is a query)
    uint32_t bcap;           // slots per bucket
    // the prefix table as common.hpp's lookups read it
    __host__ __device__ __forceinline__ PrefixView pt() const {
        return PrefixView{prefix, prefix_chars, prefix_w, prefix_hi40, pt_base, pt_jmax};
    }
};

// sas_search_buckets (the sharded step's received slots): slot i is place i % bcap of
// bucket i / bcap, and only places below that bucket's count hold a query; the others are
// skipped (no reads, no output).  The host checks nq = buckets x bcap < 2^32.
__device__ __forceinline__ bool slot_live(const SearchArgs& a, uint64_t i) {
    if (!a.bcounts) return true;
    const uint32_t b = (uint32_t)i / a.bcap;
    return (uint64_t)((uint32_t)i - b * a.bcap) < a.bcounts[b];
}

__device__ __forceinline__ void query_ptr(const SearchArgs& a, uint64_t i, const uint8_t** qb, uint32_t* m) {
    if (a.qoff) {
        *qb = a.qbytes + a.qoff[i];
        *m = a.qlen[i];
    } else {
        *qb = a.qbytes + i * (uint64_t)a.m_fixed;
        *m = a.m_fixed;
    }
}

template <int W>
using sa_val_t = typename std::conditional<W == 4, uint32_t, uint64_t>::type;

// The prefix table lookups live in common.hpp (PrefixView: pt_slot, pt_rank, prefix_range);
// the kernels here hand them the view of their SearchArgs
__device__ __forceinline__ uint64_t pt_slot(const SearchArgs& a, uint64_t K) { return pt_slot(a.pt(), K); }
__device__ __forceinline__ void prefix_range(const SearchArgs& a, uint64_t K, uint64_t* lo, uint64_t* hi) {
    prefix_range(a.pt(), K, lo, hi);
}

// ------------------------------------------------------------------ launching
// One host launcher a family.  Those that take a LaunchCtx run SEARCH_BLOCK workgroups sized by
// launch_search / launch_range; those that take num_cus size their own (their A/B macros).
struct LaunchCtx { dim3 grid, block; hipStream_t st; };

// Workgroups of bs lanes for `lanes` lanes, at most max_blocks (the kernels stride over the batch)
inline LaunchCtx launch_ctx(uint64_t lanes, uint64_t bs, uint64_t max_blocks, hipStream_t st) {
    uint64_t blocks = (lanes + bs - 1) / bs;
    if (blocks > max_blocks) blocks = max_blocks;
    return {dim3((unsigned)blocks), dim3((unsigned)bs), st};
}

template <class K, class... A>
inline void launch(const LaunchCtx& c, K k, A... args) { hipLaunchKernelGGL(k, c.grid, c.block, 0, c.st, args...); }

// The kernels are instantiated per query words held in registers: qw (qw_for: 1, 2, 4, and 8
// for anything longer) as a compile-time constant, f(std::integral_constant<int, QW>)
template <class F>
void with_qw(int qw, F&& f) {
    switch (qw) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

// The batch's longest query is known and fits the qw register words: no word is ever repacked
// from the bytes (QueryRegsExact)
inline bool all_words_in_regs(const SearchArgs& a, int qw) {
    return a.m_max && a.m_max <= 32u * (uint32_t)qw && qw <= 8;
}

// with_qw and the register-resident variant, which exists at QW = 4 and 8 only:
// f(std::integral_constant<int, QW>, std::bool_constant<EXQ>)
template <class F>
void with_qw_exq(int qw, bool exq, F&& f) {
    with_qw(qw, [&](auto Q) {
        if constexpr (decltype(Q)::value >= 4) {
            if (exq) return f(Q, std::true_type{});
        }
        f(Q, std::false_type{});
    });
}

// The index's leaf format as compile-time constants, f(std::bool_constant<KO>,
// std::integral_constant<int, W>): fused leaves hold their SA values (the W = 4 instances, no
// SA reads); key-only leaves (SAS_BUILD_QUAD_COMPACT) read them through SaView<W>
template <class F>
void with_leaves(bool ko, uint32_t sa_w, F&& f) {
    if (!ko) f(std::false_type{}, std::integral_constant<int, 4>{});
    else if (sa_w == 5) f(std::true_type{}, std::integral_constant<int, 5>{});
    else f(std::true_type{}, std::integral_constant<int, 4>{});
}

inline int qw_for(uint64_t maxlen) {
    if (maxlen <= 32) return 1;
    if (maxlen <= 64) return 2;
    if (maxlen <= 128) return 4;
    return 8;
}

// The family launchers (search_*.hip), called by launch_search / launch_range (sas_search.hip)
void launch_binary(int num_cus, hipStream_t st, const SearchArgs& a, int algo, uint32_t sa_w, int qw, bool top,
                   bool range);
void launch_stree(int num_cus, hipStream_t st, const SearchArgs& a, int algo, uint32_t sa_w, int qw);
void launch_sector(const LaunchCtx& c, const SearchArgs& a, int qw);
void launch_sector_range(const LaunchCtx& c, const SearchArgs& a, int qw, uint64_t* dhi);
void launch_interp(const LaunchCtx& c, const SearchArgs& a, bool fused, uint32_t sa_w, int qw, uint32_t range);
void launch_quad(const LaunchCtx& c, const SearchArgs& a, int algo, bool ko, uint32_t sa_w, int qw, bool top);
void launch_quad_range(const LaunchCtx& c, const SearchArgs& a, bool ko, uint32_t sa_w, int qw, uint64_t* dhi);
void launch_quad_llcp(int num_cus, hipStream_t st, const SearchArgs& a, int qw);
void launch_prefix(const LaunchCtx& c, const SearchArgs& a, bool ko, uint32_t sa_w, int qw);
void launch_prefix_range(const LaunchCtx& c, const SearchArgs& a, bool inline_slots, bool ko, uint32_t sa_w,
                         int qw, uint64_t* dhi);
void launch_tagged(int num_cus, hipStream_t st, const SearchArgs& a, int qw, bool slices);
void launch_tagged_range(const LaunchCtx& c, const SearchArgs& a, int qw, uint64_t* dhi);
