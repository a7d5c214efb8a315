// pair_path.hpp -- what the paired-end calls share (sas_pairs.hip: sas_map_pairs, the
// fragment-length join; sas_rescue.hip: sas_map_pairs_rescue, the join and a window scan for the
// mate that has no locus): steps 1..3 below (pair_join_batch), the records and the alignments
// (steps 4 and 5, pair_finish) and the argument checks and host-pointer path of both calls
// (pairs_impl).  They are declared here and defined once, with the k_pair_* kernels, in
// sas_pairs.hip; the layout of the join's key is here because k_pair_rescue writes it too.
// Pair i is reads 2i and 2i + 1 of one batch of nq = 2 np reads.
//
//   1. map_select_batch  steps 1..3 of sas_map.hip over the 4 np batch queries (forward read r as
//                     batch query r, its reverse complement as nq + r): the P sorted proposals
//                     and the single-read slots of every (read, strand);
//   2. the loci       a locus is a maximal interval of consecutive ends of one batch query; its
//                     head is the proposal that is no duplicate and does not follow its left
//                     neighbour (k_map_select's two tests).  k_pair_heads counts the heads per
//                     tile of MAP_T proposals, a scan of those counts gives each tile's first
//                     locus, and k_pair_loci, output-centric over the proposals, ranks the heads
//                     inside the tile by a ballot scan and reduces min(dist << 56 | end) per
//                     locus: in the wave by shuffles, in the tile by LDS atomics of one lane per
//                     (wave, locus); a locus inside the tile is written with a plain store, only
//                     the (at most two) loci that cross a tile edge use a 64-bit atomicMin.
//                     k_pair_pack turns the minima into lkey[L] = (batch query << ebits) | e_rep
//                     and ldist[L], ascending by key.  L stays on the device (k_pair_meta: L and
//                     the number LF of forward-strand loci, a prefix of lkey);
//   3. k_pair_join    output-centric over the LF forward loci, two passes.  Reads 2i and 2i + 1
//                     are adjacent batch queries, so the forward loci of both orientations of
//                     pair i are one segment (batch query >> 1).  An item bisects lkey for its
//                     partner window, the reverse-strand loci of the other mate with an end in
//                     [e_x - m_f + min_frag, e_x - m_f + max_frag], and scans it (at most
//                     SAS_PAIR_MAX_SPREAD / 2 + 1 loci).  Pass 1 reduces per pair the least
//                     (sum : 5 | o : 1 | e_x : 41 | e_y - window start : 16) and the number of
//                     proper candidates, pass 2 the number at the pair's least sum; the segmented
//                     reduction is that of step 2, with atomicAdd for the counts.  Integer min and
//                     add only: the result does not depend on the order of arrival;
//   4. k_pair_finalize one thread per pair: the decoded winner (the forward mate's distance is
//                     read back from its locus) or the two single-read winners, every per-read
//                     and per-pair record, and the request of one alignment per read.  Its RESCUE
//                     instantiation (sas_map_pairs_rescue) puts the rescue winner between the two;
//   5. sas_align_edit over those 2 np alignments, chained on the stream (align_winners).
#pragma once
#include "map_path.hpp"

// the pass-1 key of a pair: sum << 58 | o << 57 | e_x << 16 | (e_y - window start)
#define PR_SUM_SHIFT 58
#define PR_O_SHIFT 57
#define PR_EX_SHIFT 16
#define PR_EX_MASK ((1ull << 41) - 1ull)

// The per-read outputs of 2 np reads (map_path.hpp) and the per-pair ones
struct PairOut : ReadOut {
    uint8_t* pflags;
    uint32_t* npairs;
    uint32_t* nbestpairs;
    uint32_t* nrescue;      // sas_map_pairs_rescue alone
};

// What one call asks for.  sas_map_pairs: k_rescue = k and rescue = false
struct PairCall {
    uint32_t k, k_rescue;
    uint64_t max_seed_hits;
    uint32_t min_frag, max_frag;
    uint64_t max_anchors;
    bool rescue;
};

// Steps 1..3: the batch, its loci and the join's slots.  The scratch lives as long as the state
struct PairState {
    MapState ms;
    PoolBuf pslots, meta, toff, lmin, lkey, ldist;
};

// Steps 1..3.  All arrays on the device; Q: the caller's 2 np reads
int pair_join_batch(const sas_index* x, const MmQueries& Q, const PairCall& c, hipStream_t st, uint32_t flags,
                    PairState& ps);

// Steps 4 and 5 behind pair_join_batch.  RESCUE: rmin / rcnt are the rescue's slots (null: it
// found no work) and the alignments are made with k_rescue.  Instantiated in sas_pairs.hip
template <bool RESCUE>
int pair_finish(const sas_index* x, const PairCall& c, PairState& ps, const uint64_t* rmin, const uint64_t* rcnt,
                const PairOut& o, hipStream_t st, uint32_t flags);

// The device path of one call: all arrays on the device; Q: the caller's 2 np reads
typedef int (*PairDevice)(const sas_index* x, const MmQueries& Q, const PairCall& c, const PairOut& o, hipStream_t st,
                          uint32_t flags);

// The argument checks and the host-pointer path of a paired-end call around its device path
int pairs_impl(const char* fn, const sas_index* x, const QueryArgs& q, uint64_t np, const PairCall& c, PairDevice device,
               const PairOut& o, void* stream, uint32_t flags);
