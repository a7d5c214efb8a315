// sas_pairs.hip -- paired-end mapping with a fragment-length join (sas.h: sas_map_pairs,
// sas_map_pairs_fixed).  The steps, their kernels and the argument checks are pair_path.hpp's,
// which sas_rescue.hip shares: the batch, the loci and the join (pair_join_batch), then the
// records and one alignment per read (pair_finish).
#include "pair_path.hpp"

// All arrays on the device; Q: the caller's 2 np reads
static int pairs_device(const sas_index* x, const MmQueries& Q, const PairCall& c, const PairOut& o, hipStream_t st,
                        uint32_t flags) {
    PairState ps;
    TRY(pair_join_batch(x, Q, c, st, flags, ps));
    return pair_finish<false>(x, c, ps, nullptr, nullptr, o, st, flags);
}

extern "C" int sas_map_pairs(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                             uint64_t npairs, uint32_t k, uint64_t max_seed_hits, uint32_t min_frag,
                             uint32_t max_frag, void* out_end, void* out_start, uint8_t* out_dist,
                             uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci, uint8_t* out_nruns,
                             uint16_t* out_runs, uint8_t* out_qflags, uint8_t* out_pflags, uint32_t* out_npairs,
                             uint32_t* out_nbestpairs, void* stream, uint32_t flags) {
    const PairOut o{out_end,   out_start, out_dist,   out_strand, out_nbest,      out_nloci, out_nruns,
                    out_runs,  out_qflags, out_pflags, out_npairs, out_nbestpairs, nullptr};
    const PairCall c{k, k, max_seed_hits, min_frag, max_frag, 0, false};
    return pairs_impl("sas_map_pairs", x, qbytes, true, qoff, qlen, 0, npairs, c, pairs_device, o, stream, flags);
}

extern "C" int sas_map_pairs_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t npairs, uint32_t k,
                                   uint64_t max_seed_hits, uint32_t min_frag, uint32_t max_frag, void* out_end,
                                   void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                                   uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                                   uint8_t* out_pflags, uint32_t* out_npairs, uint32_t* out_nbestpairs, void* stream,
                                   uint32_t flags) {
    const PairOut o{out_end,   out_start, out_dist,   out_strand, out_nbest,      out_nloci, out_nruns,
                    out_runs,  out_qflags, out_pflags, out_npairs, out_nbestpairs, nullptr};
    const PairCall c{k, k, max_seed_hits, min_frag, max_frag, 0, false};
    return pairs_impl("sas_map_pairs_fixed", x, qbytes, false, nullptr, nullptr, m, npairs, c, pairs_device, o, stream,
                      flags);
}
