// build_trees.hip -- the search trees over the SA and the binary search's pivot blocks: the
// S-tree over 16-char keys (the reference's STree<16,16> shape), the sector tree (9-ary, 32-B
// nodes), the quad tree (17-ary absolute or 31-ary prefix-relative, 64-B nodes) and the
// prefix-relative pivot blocks ("rel").
#include "build_util.hpp"
#include "build_steps.hpp"

// ------------------------------------------------------------------ S-tree over 16-char keys
template <int W>
__global__ void k_keys16(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n,
                         uint32_t* __restrict__ leaves, uint64_t leaf_words) {
    GRID_STRIDE(r, leaf_words) leaves[r] = r < sa_n ? (uint32_t)(text_chars32(tw, sa[r]) >> 32) : SAS_KEY_MAX;
}

// One internal layer (sst/s_tree.rs:149-172 with left_max = false):
// key j of node i = first key of child subtree j+1, MAX if beyond the keys.
__global__ void k_stree_layer(uint32_t* __restrict__ tree, uint64_t oh, uint64_t layer_nodes, uint64_t ol,
                              uint32_t h, uint32_t height, uint64_t nkeys) {
    const uint64_t B = SAS_STREE_B;
    GRID_STRIDE(i, B * layer_nodes) {
        uint64_t k = (i / B) * (B + 1) + (i % B) + 1;
        for (uint32_t l = h; l + 2 < height; l++) k *= (B + 1);
        tree[(oh + i / B) * 16 + (i % B)] = (k * B < nkeys) ? tree[(ol + k) * 16] : SAS_KEY_MAX;
    }
}

// TreeBase<16> (sst/s_tree.rs:22-45)
static uint64_t tb_blocks(uint64_t n) { return (n + 15) / 16; }
static uint64_t tb_prev(uint64_t n) { return (tb_blocks(n) + 16) / 17 * 16; }
static uint32_t tb_height(uint64_t n) { return n <= 16 ? 1 : tb_height(tb_prev(n)) + 1; }
static uint64_t tb_layer(uint64_t n, uint32_t h, uint32_t height) {
    for (uint32_t i = h; i + 1 < height; i++) n = tb_prev(n);
    return n;
}

int build_stree(sas_index* x) {
    uint64_t nk = x->sa_n;
    uint32_t height = tb_height(nk);
    if (height > SAS_STREE_MAX_LAYERS) SAS_FAIL(ENOTSUP, "S-tree too high");
    uint64_t ls[SAS_STREE_MAX_LAYERS], tot = 0;
    for (uint32_t h = 0; h < height; h++) {
        ls[h] = (tb_layer(nk, h, height) + 15) / 16;
        x->stree_off[h] = tot;
        tot += ls[h];
    }
    DevBuf t;
    TRY(t.alloc(tot * 64, "S-tree"));
    uint32_t* tree = t.as<uint32_t>();
    uint64_t ol = x->stree_off[height - 1];
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(k_keys16<W>, dim3(grid_for(ls[height - 1] * 16)), dim3(256), 0, 0, x->text_w,
                           SaView<W>{x->sa}, nk, tree + ol * 16, ls[height - 1] * 16);
    });
    for (int h = (int)height - 2; h >= 0; h--) {
        // internal nodes: slots B..N stay MAX (B == N == 16 here, so none)
        hipLaunchKernelGGL(k_stree_layer, dim3(grid_for(16 * ls[h])), dim3(256), 0, 0, tree, x->stree_off[h],
                           ls[h], ol, (uint32_t)h, height, nk);
    }
    HIP_TRY(hipGetLastError());
    x->stree = static_cast<uint32_t*>(t.release());
    x->stree_nodes = tot;
    x->stree_height = height;
    uint32_t lds_layers = 0;
    uint64_t lds_nodes = 0;
    for (uint32_t h = 0; h + 1 < height; h++) {
        if (lds_nodes + ls[h] > SAS_STREE_LDS_NODES) break;
        lds_nodes += ls[h];
        lds_layers++;
    }
    x->stree_lds_layers = lds_layers;
    x->stree_lds_nodes = (uint32_t)lds_nodes;
    return 0;
}

// ------------------------------------------------------------------ sector tree
// Leaves: leaf i = 32 B = one HBM sector = entries 2i, 2i+1 as {key lo, key hi} x2
// then {sa, sa, 0, 0}; key = 32-char packed prefix of the suffix (zero padded),
// padding entries key = ~0, sa = ~0.
// The SA values' bits 32..39 (n >= 2^32) ride in the otherwise unused third word.
template <int W>
__global__ void k_sector_leaves(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n,
                                uint4* __restrict__ leaves, uint64_t nleaves) {
    GRID_STRIDE(i, nleaves) {
        uint64_t r0 = 2 * i, r1 = 2 * i + 1;
        uint64_t k0 = ~0ull, k1 = ~0ull;
        uint64_t s0 = 0xFFFFFFFFu, s1 = 0xFFFFFFFFu;
        if (r0 < sa_n) { s0 = sa[r0]; k0 = text_chars32(tw, s0); }
        if (r1 < sa_n) { s1 = sa[r1]; k1 = text_chars32(tw, s1); }
        leaves[2 * i] = make_uint4((uint32_t)k0, (uint32_t)(k0 >> 32), (uint32_t)k1, (uint32_t)(k1 >> 32));
        uint32_t hi = (uint32_t)((s0 >> 32) & 0xFF) | ((uint32_t)((s1 >> 32) & 0xFF) << 8);
        leaves[2 * i + 1] = make_uint4((uint32_t)s0, (uint32_t)s1, (r0 < sa_n ? hi : 0u), 0u);
    }
}

// Internal layer, left_max style (sst/s_tree.rs:163-171 with left_max = true):
// separator j of node i = 16-char key (high word) of the LAST entry of child
// 9i+j's subtree, so count(sep < K16) lands exactly on the child holding the
// first entry with key16 >= K16.  child_span = leaves per child subtree.  The
// globally last child and nonexistent children get 0xFFFFFFFF, which no query
// key exceeds, so routing never leaves the tree.
__global__ void k_sector_layer(uint32_t* __restrict__ inner, uint64_t oh, uint64_t layer_nodes,
                               uint64_t child_span, uint64_t child_layer_nodes, const uint4* __restrict__ leaves,
                               uint64_t sa_n) {
    GRID_STRIDE(i, 8 * layer_nodes) {
        uint64_t node = i / 8, j = i % 8;
        uint64_t child = node * SAS_SECTOR_FAN + j;
        uint32_t sep = 0xFFFFFFFFu;
        if (child + 1 < child_layer_nodes) {
            uint64_t last = 2 * (child + 1) * child_span - 1;  // last entry rank of the subtree
            if (last >= sa_n) last = sa_n - 1;
            uint4 v = leaves[2 * (last >> 1)];
            sep = (last & 1) ? v.w : v.y;
        }
        inner[(oh + node) * 8 + j] = sep;
    }
}

// The inner layers of a fan-ary tree over nl leaves, layer 0 the root: nodes[h] of them at
// node offset off[h] (the index's own array), tot in all
struct LayerShape {
    uint64_t nodes[SAS_SECTOR_MAX_LAYERS];
    uint32_t H;
    uint64_t tot;
};
static_assert(SAS_QUAD_MAX_LAYERS <= SAS_SECTOR_MAX_LAYERS, "LayerShape holds either tree's layers");

static int layer_shape(uint64_t nl, uint32_t fan, uint32_t max_layers, const char* too_high, uint64_t* off,
                       LayerShape* s) {
    uint64_t sizes[SAS_SECTOR_MAX_LAYERS];  // bottom-up
    s->H = 0;
    uint64_t c = nl;
    do {
        c = (c + fan - 1) / fan;
        if (s->H >= max_layers) SAS_FAIL(ENOTSUP, too_high);
        sizes[s->H++] = c;
    } while (c > 1);
    s->tot = 0;
    for (uint32_t h = 0; h < s->H; h++) {
        off[h] = s->tot;
        s->tot += s->nodes[h] = sizes[s->H - 1 - h];
    }
    return 0;
}

// The top layers a lookup stages in LDS: as many as fit node_cap nodes, layer_cap at the most
static void lds_layers(const LayerShape& s, uint64_t node_cap, uint32_t* layers, uint32_t* nodes,
                       uint32_t layer_cap = UINT32_MAX) {
    uint32_t L = 0;
    uint64_t ln = 0;
    for (uint32_t h = 0; h < s.H; h++) {
        if (ln + s.nodes[h] > node_cap || L == layer_cap) break;
        ln += s.nodes[h];
        L++;
    }
    *layers = L;
    *nodes = (uint32_t)ln;
}

int build_sector(sas_index* x) {
    uint64_t sa_n = x->sa_n;
    uint64_t nl = (sa_n + 1) / 2;
    LayerShape s;
    TRY(layer_shape(nl, SAS_SECTOR_FAN, SAS_SECTOR_MAX_LAYERS, "sector tree too high", x->sec_off, &s));
    const uint32_t H = s.H;
    const uint64_t tot = s.tot;
    DevBuf leaves, inner;
    TRY(leaves.alloc(nl * 32, "sector leaves"));
    TRY(inner.alloc(tot * 32, "sector inner nodes"));
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(k_sector_leaves<W>, dim3(grid_for(nl)), dim3(256), 0, 0, x->text_w, SaView<W>{x->sa},
                           sa_n, leaves.as<uint4>(), nl);
    });
    uint64_t span = 1, child_nodes = nl;
    for (int h = (int)H - 1; h >= 0; h--) {
        uint64_t ln = s.nodes[h];
        hipLaunchKernelGGL(k_sector_layer, dim3(grid_for(8 * ln)), dim3(256), 0, 0, inner.as<uint32_t>(),
                           x->sec_off[h], ln, span, child_nodes, leaves.as<uint4>(), sa_n);
        span *= SAS_SECTOR_FAN;
        child_nodes = ln;
    }
    HIP_TRY(hipGetLastError());
    x->sec_leaves = static_cast<uint4*>(leaves.release());
    x->sec_inner = static_cast<uint32_t*>(inner.release());
    x->sec_leaf_count = nl;
    x->sec_inner_layers = H;
    x->sec_inner_nodes = tot;
    lds_layers(s, SAS_SECTOR_LDS_NODES, &x->sec_lds_layers, &x->sec_lds_nodes);
    return 0;
}

// ------------------------------------------------------------------ quad tree
// Leaf entry x (16 B) = {key64 lo, key64 hi, SA lo32, SA bits 32..39} for rank x;
// leaf i = entries 4i..4i+3 = 64 B, so lane j of a 4-lane group loads entry j
// and the group's load is one 64-B request.  Padding entries are all ones.
template <int W>
__global__ void k_quad_leaves(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n,
                              uint4* __restrict__ leaves, uint64_t entries) {
    GRID_STRIDE(x, entries) {
        if (x < sa_n) {
            uint64_t p = sa[x];
            uint64_t k = text_chars32(tw, p);
            leaves[x] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)p, (uint32_t)(p >> 32));
        } else {
            leaves[x] = make_uint4(~0u, ~0u, ~0u, ~0u);
        }
    }
}

// Compact leaves: entry x = key64 of rank x only; leaf i = entries 8i..8i+7 (lane j
// of a group loads keys 2j, 2j+1).  Padding keys are all ones.
template <int W>
__global__ void k_quad_keys(const uint64_t* __restrict__ tw, SaView<W> sa, uint64_t sa_n,
                            uint64_t* __restrict__ keys, uint64_t entries) {
    GRID_STRIDE(x, entries) keys[x] = x < sa_n ? text_chars32(tw, sa[x]) : ~0ull;
}

// Internal layer, left-max (as k_sector_layer, 17-ary): separator j of node i =
// 16-char key of the last entry of child 17i+j's subtree (child_span leaves of epl
// entries), 0xFFFFFFFF for the globally last child and beyond.  Fused leaves hold
// the key's high word at uint32 4x+1, compact ones at 2x+1.
__global__ void k_quad_layer(uint32_t* __restrict__ inner, uint64_t oh, uint64_t layer_nodes, uint64_t child_span,
                             uint64_t child_layer_nodes, const uint32_t* __restrict__ leaves, uint64_t sa_n,
                             uint32_t epl) {
    GRID_STRIDE(i, 16 * layer_nodes) {
        uint64_t node = i / 16, j = i % 16;
        uint64_t child = node * SAS_QUAD_FAN + j;
        uint32_t sep = 0xFFFFFFFFu;
        if (child + 1 < child_layer_nodes) {
            uint64_t last = epl * (child + 1) * child_span - 1;
            if (last >= sa_n) last = sa_n - 1;
            sep = leaves[(epl == 4 ? 4 : 2) * last + 1];
        }
        inner[(oh + node) * 16 + j] = sep;
    }
}

// Prefix-relative internal layer (quad_fan 31).  A node's whole subtree shares its
// first d chars P (d = LCP of the subtree's first and last 32-char keys, capped at
// SAS_QUAD_RMAXD), so its separators only need the 8 chars after them:
//   word 0   = d << 27 | P (2d bits, right-aligned): u16 slots 0 and 1
//   u16 slot 2 + s (s = 0..29) = chars [d, d+8) of the key of the LAST entry of child
//            31i+s (left-max, as k_quad_layer), 0xFFFF for the globally last child and
//            beyond; stored XOR 0x8000 so that a saturating packed i16 subtract compares
//            two of them at once (quad_rel_child).
// Within the subtree these 16-bit windows are monotone in rank (the keys agree on
// chars [0, d)), so "window < q's window" still implies "suffix < q" for a query
// whose first d chars equal P; the search decides the other two cases from P alone
// ("above P" = every entry < q: the last child).  The LAST node of a layer may have
// fewer than 31 children, so it always gets d = 0 (its windows are the first 8 chars,
// still monotone): "above P" cannot happen there and no child index leaves the layer.
__device__ __forceinline__ uint64_t quad_key_at(const uint32_t* __restrict__ leaves, uint32_t epl, uint64_t x) {
    const uint2 k = reinterpret_cast<const uint2*>(leaves)[epl == 4 ? 2 * x : x];
    return (uint64_t)k.x | ((uint64_t)k.y << 32);
}

__global__ void k_quad_rel_layer(uint32_t* __restrict__ inner, uint64_t oh, uint64_t layer_nodes,
                                 uint64_t child_span, uint64_t child_layer_nodes,
                                 const uint32_t* __restrict__ leaves, uint64_t sa_n, uint32_t epl) {
    GRID_STRIDE(i, 16 * layer_nodes) {
        const uint64_t node = i / 16, w = i % 16;
        const uint64_t span = epl * child_span;  // entries per child
        const uint64_t first = node * SAS_QUAD_RFAN * span;
        uint64_t last = (node + 1) * SAS_QUAD_RFAN * span;
        last = (last < sa_n ? last : sa_n) - 1;
        const uint64_t kf = quad_key_at(leaves, epl, first), kl = quad_key_at(leaves, epl, last);
        uint32_t d = (kf == kl) ? 32u : (uint32_t)__builtin_clzll(kf ^ kl) / 2;
        if (d > SAS_QUAD_RMAXD) d = SAS_QUAD_RMAXD;
        if (node + 1 == layer_nodes) d = 0;
        uint32_t word;
        if (w == 0) {
            word = (d << 27) | (d ? (uint32_t)(kf >> (64 - 2 * d)) : 0u);
        } else {
            uint32_t half[2];
            for (int e = 0; e < 2; e++) {
                const uint64_t child = node * SAS_QUAD_RFAN + (2 * w - 2 + e);
                half[e] = 0xFFFFu;
                if (child + 1 < child_layer_nodes)
                    half[e] = (uint32_t)(quad_key_at(leaves, epl, (child + 1) * span - 1) >> (48 - 2 * d)) & 0xFFFFu;
            }
            word = (half[0] | (half[1] << 16)) ^ 0x80008000u;
        }
        inner[(oh + node) * 16 + w] = word;
    }
}

// Levels (inner layers and the leaf layer) whose 64-B nodes outgrow the 256 MiB
// Infinity Cache: each costs one DRAM-level request per lookup.
static uint32_t quad_dram_levels(uint64_t nl, uint32_t fan) {
    const uint64_t mall_nodes = (256ull << 20) / 64;
    uint32_t cnt = 0;
    for (uint64_t c = nl;; c = (c + fan - 1) / fan) {
        cnt += c > mall_nodes;
        if (c <= 1) break;
    }
    return cnt;
}

// mode: SAS_BUILD_QUAD_ABS / SAS_BUILD_QUAD_REL force a layout; neither = the one
// with fewer levels beyond the Infinity Cache, the absolute layout on a tie
// (measured: at n = 2^30 both have two such levels and the absolute one is ~4%
// faster; at n = 2^34 with compact leaves the relative one saves a level, -8% on
// ragged 8..256 queries; tools/ab_quad_rel.py).
int build_quad(sas_index* x, bool compact, uint32_t mode) {
    const uint64_t sa_n = x->sa_n;
    const uint32_t epl = compact ? 8 : 4;  // entries per 64-B leaf
    const uint64_t nl = (sa_n + epl - 1) / epl;
    bool absolute = true;
    if (mode & SAS_BUILD_QUAD_REL) absolute = false;
    else if (!(mode & SAS_BUILD_QUAD_ABS))
        absolute = quad_dram_levels(nl, SAS_QUAD_RFAN) >= quad_dram_levels(nl, SAS_QUAD_FAN);
    const uint32_t fan = absolute ? SAS_QUAD_FAN : SAS_QUAD_RFAN;
    LayerShape s;
    TRY(layer_shape(nl, fan, SAS_QUAD_MAX_LAYERS, "quad tree too high", x->quad_off, &s));
    const uint32_t H = s.H;
    const uint64_t tot = s.tot;
    if (H > SAS_QUAD_MAX_INNER || nl > (1ull << 32)) SAS_FAIL(ENOTSUP, "quad tree: more than 2^32 leaves");
    DevBuf leaves, inner;
    TRY(leaves.alloc(nl * 64, "quad leaves"));
    TRY(inner.alloc(tot * 64, "quad inner nodes"));
    const dim3 lg(grid_for(epl * nl)), lb(256);
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if (compact)
            hipLaunchKernelGGL(k_quad_keys<W>, lg, lb, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, leaves.as<uint64_t>(), 8 * nl);
        else
            hipLaunchKernelGGL(k_quad_leaves<W>, lg, lb, 0, 0, x->text_w, SaView<W>{x->sa}, sa_n, leaves.as<uint4>(), 4 * nl);
    });
    uint64_t span = 1, child_nodes = nl;
    for (int h = (int)H - 1; h >= 0; h--) {
        uint64_t ln = s.nodes[h];
        if (absolute)
            hipLaunchKernelGGL(k_quad_layer, dim3(grid_for(16 * ln)), dim3(256), 0, 0, inner.as<uint32_t>(),
                               x->quad_off[h], ln, span, child_nodes, leaves.as<uint32_t>(), sa_n, epl);
        else
            hipLaunchKernelGGL(k_quad_rel_layer, dim3(grid_for(16 * ln)), dim3(256), 0, 0, inner.as<uint32_t>(),
                               x->quad_off[h], ln, span, child_nodes, leaves.as<uint32_t>(), sa_n, epl);
        span *= fan;
        child_nodes = ln;
    }
    HIP_TRY(hipGetLastError());
    x->quad_leaves = static_cast<uint4*>(leaves.release());
    x->quad_inner = static_cast<uint4*>(inner.release());
    x->quad_leaf_count = nl;
    x->quad_compact = compact ? 1 : 0;
    x->quad_fan = fan;
    x->quad_inner_layers = H;
    x->quad_inner_nodes = tot;
    lds_layers(s, SAS_QUAD_LDS_NODES, &x->quad_lds_layers, &x->quad_lds_nodes, SAS_QUAD_MAX_LDS);
    return 0;
}

// ------------------------------------------------------------------ pivot blocks of the binary search
// The prefix-relative pivot blocks (common.hpp RelLayout).  Node k (1-based Eytzinger) = the
// state after the path given by k's bits below the leading one (0 = went left: r = mid, 1 =
// right: l = mid + 1); at level d in group g it sits t = d - d0 levels below its block's
// root.  The root's interval [l0, r0) gives P = lcp(SA[l0 - 1], SA[r0]) (whole suffixes:
// never past either one's end; capped), the node's pivot SA[(l + r) / 2] its chars [P, P + 8)
// (zero past the text's end) in slot (1 << t) | (k's low t bits); the root thread writes P to
// slot 0.  Nodes whose interval is empty keep 0 (never read: the search stops probing there).
template <int W>
__global__ void k_rel(const uint64_t* __restrict__ tw, uint64_t n, SaView<W> sa, uint64_t sa_n,
                      uint8_t* __restrict__ rel, uint64_t nodes, const RelLayout lay) {
    GRID_STRIDE(i, nodes) {
        const uint64_t k = 1 + i;
        const int depth = 63 - __clzll(k);
        uint32_t g = 0;
        while (g + 1 < lay.groups && (int)lay.d0[g + 1] <= depth) g++;
        const int d0 = lay.d0[g];
        const uint32_t t = (uint32_t)(depth - d0);
        uint64_t l = 0, r = sa_n, l0 = 0, r0 = sa_n;
        bool live = true;
        for (int b = depth - 1; b >= 0; b--) {
            if (depth - 1 - b == d0) { l0 = l; r0 = r; }
            const uint64_t mid = (l + r) >> 1;
            if (l >= r) { live = false; break; }
            if ((k >> b) & 1) l = mid + 1; else r = mid;
        }
        if (depth == d0) { l0 = l; r0 = r; }
        if (!(l < r)) live = false;
        if (!(l0 < r0)) continue;  // the whole block is empty
        uint32_t P = 0;
        if (l0 > 0 && r0 < sa_n) {
            const uint64_t a = sa[l0 - 1], c = sa[r0];
            const uint64_t x = text_chars32(tw, a) ^ text_chars32(tw, c);
            uint64_t lc = x ? (uint64_t)(__clzll(x) >> 1) : 32;
            if (lc > n - a) lc = n - a;
            if (lc > n - c) lc = n - c;
            P = lc < SAS_REL_PMAX ? (uint32_t)lc : SAS_REL_PMAX;
        }
        const uint64_t k0 = k >> t;
        const uint32_t sh = lay.h[g] == SAS_REL_GROUP ? 5u : 4u;
        uint16_t* blk = reinterpret_cast<uint16_t*>(rel + lay.base[g] + ((k0 - (1ull << d0)) << sh));
        if (t == 0) {
            // bit 15: a pivot of the block ends inside its key (chars [P, P + 8) padded): its
            // first difference with q may lie in the padding, so LCP / LLCP compare the text
            uint32_t flag = 0;
            for (uint32_t j = 1; j < (1u << lay.h[g]) && !flag; j++) {
                uint64_t ll = l0, rr = r0;
                for (int bb = 30 - __clz(j); bb >= 0 && ll < rr; bb--) {
                    const uint64_t mm = (ll + rr) >> 1;
                    if ((j >> bb) & 1) ll = mm + 1; else rr = mm;
                }
                if (ll < rr && n - sa[(ll + rr) >> 1] < (uint64_t)P + 8) flag = 1;
            }
            blk[0] = (uint16_t)(P | (flag << 15));
        }
        if (live) {
            const uint64_t p = sa[(l + r) >> 1];
            blk[(1u << t) | (uint32_t)(k & ((1ull << t) - 1))] = (uint16_t)(text_chars32(tw, p + P) >> 48);
        }
    }
}

// The pivots of the first L iterations: SAS_TOP2_CACHE_LEVELS (27: 273 MiB of blocks) unless
// the caller asks for another depth (levels: SAS_BUILD_TOP2_LEVELS), rounded up to the 4-level
// grid past the LDS levels.  The depth is never taken from free memory, so a text always gets
// the same index.  The probe sequence, and so every result, is the same at any depth.
int build_rel(sas_index* x, uint32_t levels) {
    rel_layout(x->iters, levels ? levels : SAS_TOP2_CACHE_LEVELS, &x->rel_lay);
    const RelLayout& lay = x->rel_lay;
    DevBuf rl;
    TRY(rl.alloc(lay.bytes, "rel"));
    HIP_TRY(hipMemset(rl.p, 0, lay.bytes));
    const uint64_t cnt = (1ull << lay.levels) - 1;
    with_sa_w(x->sa_w, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(k_rel<W>, dim3(grid_for(cnt)), dim3(256), 0, 0, x->text_w, x->n, SaView<W>{x->sa}, x->sa_n,
                           rl.as<uint8_t>(), cnt, lay);
    });
    HIP_TRY(hipGetLastError());
    x->rel = static_cast<uint8_t*>(rl.release());
    return 0;
}
