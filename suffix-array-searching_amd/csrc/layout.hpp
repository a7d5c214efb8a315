// layout.hpp -- the sequence layout of an index (sas.h: sas_set_layout) as the kernels read it:
// where the sequences of the text start and which stretches of it are real bases.
//
//   seq_start[0 .. nseq]  ascending, seq_start[0] = 0, seq_start[nseq] = n; sequence i is the text
//                         [seq_start[i], seq_start[i + 1]), which may be empty;
//   seg_lo / seg_hi[nseg] the segments [lo, hi), lo < hi, ascending and disjoint, each inside one
//                         sequence; a position in no segment is a gap.
//
// The three bisects are __host__ __device__ so that tests/cpp/layout_host_check.cpp drives the
// very code the kernels run (the precedent of csr_tile.hpp and qllcp_bisect.hpp).  The arrays may
// live in global memory or in LDS (k_translate stages them).  nseq == 0: no layout; the kernels
// branch on a template bool and never call these then.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LAYOUT_NONE 0xFFFFFFFFFFFFFFFFull

struct LayoutView {
    const uint64_t* seq_start;  // nseq + 1
    uint64_t nseq;
    const uint64_t* seg_lo;     // nseg each
    const uint64_t* seg_hi;
    uint64_t nseg;
};

// the segment i with seg_lo[i] <= p < seg_hi[i], or LAYOUT_NONE: p lies in a gap (or past n)
__host__ __device__ __forceinline__ uint64_t layout_seg_of_pos(const LayoutView& y, uint64_t p) {
    uint64_t l = 0, h = y.nseg;
    while (l < h) {  // the number of segments with lo <= p
        const uint64_t mid = (l + h) >> 1;
        if (y.seg_lo[mid] <= p) l = mid + 1;
        else h = mid;
    }
    return l && p < y.seg_hi[l - 1] ? l - 1 : LAYOUT_NONE;
}

// the segment i with seg_lo[i] < e <= seg_hi[i], or LAYOUT_NONE: the one an alignment that ends
// at e (its last char is e - 1) lies in; no end 0 has one
__host__ __device__ __forceinline__ uint64_t layout_seg_of_end(const LayoutView& y, uint64_t e) {
    return e ? layout_seg_of_pos(y, e - 1) : LAYOUT_NONE;
}

// the sequence of an end e in [1, n]: the largest i with seq_start[i] < e, which is never an
// empty sequence and never nseq; LAYOUT_NONE for e == 0 or e > n
__host__ __device__ __forceinline__ uint64_t layout_seq_of_end(const LayoutView& y, uint64_t e) {
    if (e == 0 || y.nseq == 0 || e > y.seq_start[y.nseq]) return LAYOUT_NONE;
    uint64_t l = 0, h = y.nseq + 1;
    while (l < h) {  // the number of starts < e (at least one: seq_start[0] = 0)
        const uint64_t mid = (l + h) >> 1;
        if (y.seq_start[mid] < e) l = mid + 1;
        else h = mid;
    }
    return l - 1;
}
