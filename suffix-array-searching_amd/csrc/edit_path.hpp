// edit_path.hpp -- the seed / verify / sort path of sas_edit.hip for the calls built on it
// (sas_edit.hip: sas_locate_edit itself; sas_map.hip: sas_map_edit over both strands), Myers'
// bit-vector state and the dispatch on its word count (with_ed_words; sas_rescue.hip's too).
#pragma once
#include "seed_verify.hpp"

// Steps 1..6 of sas_edit.hip up to the offsets; the scratch that the calls behind them read
// stays in the state
struct EdState {
    SeedState seed;
    PoolBuf mask, kbase, dists, pscan, keys, vals, uscan;
    const uint64_t* skeys = nullptr;  // the P sorted proposals, key = (query << ebits) | end;
    const uint8_t* svals = nullptr;   // their distances (equal keys carry equal distances)
    uint64_t C = 0, P = 0;            // P == 0: nothing was proposed, skeys / svals are null
    uint32_t ebits = 0;
};

// even bits of x (bit 2 p -> bit p)
__device__ __forceinline__ uint32_t ed_even_bits(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// The bit planes of query chars [32 j, 32 j + 32): bit r of lo / hi = the low / high bit of char
// 32 j + r (pack_query_word has char r in bits 63 - 2 r, 62 - 2 r; zero behind m)
__device__ __forceinline__ void ed_planes32(const uint8_t* __restrict__ qb, uint32_t m, uint32_t j, uint32_t* lo,
                                            uint32_t* hi) {
    uint32_t bad = 0;
    const uint64_t w = pack_query_word(qb, m, j, &bad);
    *lo = __brev(ed_even_bits(w));
    *hi = __brev(ed_even_bits(w >> 1));
}

// Myers' bit-vector state of one query of m <= 64 NW chars in its search form (sas_edit.hip,
// step 5): two bit planes per word of 64 rows, the rows' mask, and the vertical deltas Pv / Mv
// of the column before the first (all + 1: D = i in row i, the empty text)
template <int NW>
struct EdMyers {
    uint64_t L[NW], H[NW], V[NW], Pv[NW], Mv[NW];
    uint32_t lw, lb;  // row m - 1: word and bit
    __device__ __forceinline__ void init(const uint8_t* __restrict__ qb, uint32_t m) {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            uint32_t l0, h0, l1, h1;
            ed_planes32(qb, m, 2 * w, &l0, &h0);
            ed_planes32(qb, m, 2 * w + 1, &l1, &h1);
            L[w] = ((uint64_t)l1 << 32) | l0;
            H[w] = ((uint64_t)h1 << 32) | h0;
            const uint32_t rows = m > 64u * w ? m - 64u * w : 0u;       // rows of the query in this word
            V[w] = rows >= 64 ? ~0ull : ((1ull << rows) - 1ull);
            Pv[w] = ~0ull;
            Mv[w] = 0;
        }
        lw = (m - 1) >> 6;
        lb = (m - 1) & 63;
    }
    // Back to the state before the first column, the query kept: what a lane does where a new
    // text begins under its columns (a segment's lo, sas_rescue.hip); the caller sets score = m
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            Pv[w] = ~0ull;
            Mv[w] = 0;
        }
    }
    // One column: the text char in the top two bits of tx.  Returns the change of the score,
    // the horizontal delta of row m - 1 (free start: 0 into row 0)
    __device__ __forceinline__ int64_t column(uint64_t tx) {
        const uint64_t cl = 0ull - ((tx >> 62) & 1ull), ch = 0ull - (tx >> 63);
        int64_t ds = 0;
        int hin = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            uint64_t Eq = ~(L[w] ^ cl) & ~(H[w] ^ ch) & V[w];
            const uint64_t Xv = Eq | Mv[w];
            Eq |= hin < 0 ? 1ull : 0ull;
            const uint64_t Xh = (((Eq & Pv[w]) + Pv[w]) ^ Pv[w]) | Eq;
            uint64_t Ph = Mv[w] | ~(Xh | Pv[w]);
            uint64_t Mh = Pv[w] & Xh;
            if ((uint32_t)w == lw) ds += (int64_t)((Ph >> lb) & 1ull) - (int64_t)((Mh >> lb) & 1ull);
            const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
            Ph = (Ph << 1) | (hin > 0 ? 1ull : 0ull);
            Mh = (Mh << 1) | (hin < 0 ? 1ull : 0ull);
            Pv[w] = Mh | ~(Xv | Ph);
            Mv[w] = Ph & Xv;
            hin = hout;
        }
        return ds;
    }
};

// bits that hold every value in [0, v]
static inline uint32_t ed_bits(uint64_t v) {
    uint32_t b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// The number of 64-row words of Myers' state that serves a batch, as a compile-time constant,
// f(std::integral_constant<int, NW>): 1, 2 or 4 for fixed-length queries of m <= 64, 128, more
// chars (a longer m is gated: any kernel serves), 0 for a ragged batch (by each query's m)
template <class F>
void with_ed_words(const MmQueries& Q, F&& f) {
    if (Q.qoff) f(std::integral_constant<int, 0>{});
    else if (Q.m <= 64) f(std::integral_constant<int, 1>{});
    else if (Q.m <= 128) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

// All arrays on the device (out_qflags and out_total may be null).  Writes out_off[0 .. nq] and
// the flags; two host reads: the candidate total and the proposal total
int ed_prepare(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off,
               uint8_t* out_qflags, uint64_t* out_total, hipStream_t st, uint32_t flags, EdState& s);
