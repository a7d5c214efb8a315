// map_path.hpp -- what the read-mapping calls share (sas_map.hip: sas_map_edit, one record per
// read; sas_pairs.hip: sas_map_pairs, the fragment-length join of two mates): the tile constants
// of the kernels over sorted lists, the state of steps 1..3 of sas_map.hip (map_select_batch,
// defined there with its kernels: the batch of both strands, the seed / verify / sort path over
// it and the per-(read, strand) slots of the output-centric select), and the single-read winner
// of the two strands' slots, which the finalize kernels of both files inline.
#pragma once
#include "edit_path.hpp"

#define MAP_BLOCK 256
#define MAP_T 2048                    // proposals per tile
#define MAP_PER (MAP_T / MAP_BLOCK)
#define MAP_CHUNKS (MAP_T / 64)       // (wave, round) pairs of a tile: 64 consecutive proposals each
#define MAP_BPC 4                     // workgroups per CU that size the grids
#define MAP_NONE (~0ull)

static_assert(MAP_CHUNKS == 32, "the chunk scan is one shuffle scan over 32 lanes");

struct MapSel {
    const uint64_t* keys;   // P sorted proposals, (batch query << ebits) | end
    const uint8_t* vals;    // their distances
    uint64_t P;
    uint32_t ebits;
    uint64_t nq, nb;        // reads; batch queries (nq, or 2 nq: the strands of read i are i and nq + i)
    uint64_t* kmin;         // per batch query: the least dist << 56 | end (MAP_NONE before pass 1)
    uint64_t* nloci;        // per batch query: intervals of consecutive ends (0 before pass 1)
    uint64_t* nbest;        // per batch query: those at the read's least distance (0 before pass 2)
};

// The single-read record of read i from the slots of its `copies` strands (batch queries
// c nq + i): the least (dist, strand, end), the counts summed and the flags ORed
struct MapBest {
    uint64_t best;  // dist << 56 | strand << 55 | end (an end has at most 41 bits); MAP_NONE: unmapped
    uint64_t bb;    // the winner's batch query
    uint64_t nl, nbst;
    uint32_t fl;
};

__device__ __forceinline__ MapBest map_best_of(uint64_t i, uint64_t nq, uint32_t copies, uint32_t strands,
                                               const uint64_t* __restrict__ kmin, const uint64_t* __restrict__ nloci,
                                               const uint64_t* __restrict__ nbest, const uint8_t* __restrict__ efl) {
    MapBest r{MAP_NONE, i, 0, 0, 0};
    for (uint32_t c = 0; c < copies; c++) {
        const uint64_t b = c * nq + i;
        const uint64_t strand = copies == 2 ? c : (strands == SAS_MAP_REV ? 1u : 0u);
        const uint64_t km = kmin[b];
        r.fl |= efl[b];
        r.nl += nloci[b];
        r.nbst += nbest[b];
        if (km != MAP_NONE) {
            const uint64_t key = km | (strand << 55);
            if (key < r.best) {
                r.best = key;
                r.bb = b;
            }
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t map_clamp32(uint64_t v) {
    return (uint32_t)(v < 0xFFFFFFFFull ? v : 0xFFFFFFFFull);
}

// Steps 1..3 of sas_map.hip: the batch of the participating strands, its sorted proposals and
// the slots of the two select passes.  The scratch lives as long as the state
struct MapState {
    MmQueries B;                // the batch: nb = copies nq queries
    uint64_t nb = 0;
    PoolBuf bbytes, bscan, boff, blen, eoff, efl, slots;
    EdState s;
    uint64_t* kmin = nullptr;   // nb each
    uint64_t* nloci = nullptr;
    uint64_t* nbest = nullptr;
};

// All arrays on the device; Q: the caller's queries.  Defined in sas_map.hip with its kernels
int map_select_batch(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t strands,
                     hipStream_t st, uint32_t flags, MapState& ms);
