// map_path.hpp -- what the read-mapping calls share (sas_map.hip: sas_map_edit, one record per
// read; sas_pairs.hip: sas_map_pairs, the fragment-length join of two mates): the tile constants
// of the kernels over sorted lists, the state of steps 1..3 of sas_map.hip (map_select_batch,
// defined there with its kernels: the batch of both strands, the seed / verify / sort path over
// it and the per-(read, strand) slots of the output-centric select), the single-read winner of
// the two strands' slots, which the finalize kernels of both files inline, the per-read outputs
// (ReadOut) with their host-pointer twins (twin_reads), and the alignment of every read's winner
// behind the finalize kernel (AlignReq, align_winners).
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

// The per-read outputs of a mapping call; all but end and dist may be null
struct ReadOut {
    void* end;
    void* start;
    uint8_t* dist;
    uint8_t* strand;
    uint32_t* nbest;
    uint32_t* nloci;
    uint8_t* nruns;
    uint16_t* runs;
    uint8_t* qflags;
};

// Their twins on the host-pointer path: nq reads, positions of esz bytes, `stride` u16 of runs per
// read; label: the call's word in "<label> ends".  Defined in sas_map.hip
int twin_reads(HostOutputs& ho, const ReadOut& host, uint64_t nq, uint64_t esz, uint64_t stride, const char* label,
               ReadOut* dev);

// The request of one alignment per read that a finalize kernel writes, one scratch buffer: aoff
// (nq + 1) | aqoff (nq) | the starts, where the caller gives no out_start | aqlen (nq)
struct AlignReq {
    PoolBuf buf;
    uint64_t* aoff = nullptr;
    uint64_t* aqoff = nullptr;
    uint32_t* aqlen = nullptr;
    void* start = nullptr;  // the caller's out_start, or the scratch in its place
    int alloc(const sas_index* x, uint64_t nq, void* out_start, uint32_t flags, hipStream_t st) {
        const uint64_t esz = (flags & SAS_LOCATE_U32) ? 4 : 8;
        hipMemPool_t pool;
        TRY(sas_scratch_pool(x, &pool));
        TRY(buf.alloc(pool, (nq + 1) * 8 + nq * 8 + nq * 4 + (out_start ? 0 : nq * esz), st));
        aoff = buf.as<uint64_t>();
        aqoff = aoff + nq + 1;
        void* scratch = aqoff + nq;  // 8-byte aligned; unused when out_start is given
        aqlen = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + (out_start ? 0 : nq * esz));
        start = out_start ? out_start : scratch;
        return 0;
    }
};

// sas_align_edit over the request of batch B, chained on the stream, where starts or runs are
// asked for (the bytes were validated by the range search when asked for)
static inline int align_winners(const sas_index* x, const MmQueries& B, const AlignReq& r, uint64_t nq, uint32_t k,
                                const ReadOut& o, hipStream_t st, uint32_t flags) {
    if (!o.start && !o.nruns && !o.runs) return 0;
    return sas_align_edit(x, B.qbytes, r.aqoff, r.aqlen, nq, k, r.aoff, o.end, nq, r.start, nullptr, o.nruns, o.runs, st,
                          SAS_DEVICE_PTRS | (flags & SAS_LOCATE_U32));
}
