// edit_path.hpp -- the seed / verify / sort path of sas_edit.hip for the calls built on it
// (sas_edit.hip: sas_locate_edit itself; sas_map.hip: sas_map_edit over both strands).
#pragma once
#include "seed_verify.hpp"

// Steps 1..6 of sas_edit.hip up to the offsets; the scratch that the calls behind them read
// stays in the state
struct EdState {
    hipMemPool_t pool = nullptr;
    MmPoolBuf poff, plen, lohi, coff, qfl, mask, kbase, dists, pscan, keys, vals, uscan;
    const uint64_t* skeys = nullptr;  // the P sorted proposals, key = (query << ebits) | end;
    const uint8_t* svals = nullptr;   // their distances (equal keys carry equal distances)
    uint64_t C = 0, P = 0;            // P == 0: nothing was proposed, skeys / svals are null
    uint32_t ebits = 0;
};

// bits that hold every value in [0, v]
static inline uint32_t ed_bits(uint64_t v) {
    uint32_t b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// All arrays on the device (out_qflags and out_total may be null).  Writes out_off[0 .. nq] and
// the flags; two host reads: the candidate total and the proposal total
int ed_prepare(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off,
               uint8_t* out_qflags, uint64_t* out_total, hipStream_t st, uint32_t flags, EdState& s);
