// build_steps.hpp -- the stages of build_impl (sas_build.hip), each defined in the unit that
// owns its kernels.  A step reads the index's text, SA and the structures built before it,
// and leaves what it builds in the index; on an error the caller frees the index.
#pragma once
#include "common.hpp"

// sas_index.hip
void free_index(sas_index* x);

// build_gen.hip: the ChaCha8 key of ChaCha8Rng::seed_from_u64(seed); random_string(n) drawn
// from it straight into packed text words (zero past n)
struct ChaKey { uint32_t k[8]; };
void gen_key(uint64_t seed, ChaKey* key);
int gen_packed_text(const ChaKey& key, uint64_t n, uint64_t* tw, uint64_t words);

// build_sa.hip: prefix doubling into a device u32[n]
int build_sa_gpu(const uint64_t* tw, uint64_t n, uint32_t* sa_out, uint32_t* rounds_out, bool force_wide);

// sas_build40.hip: the bucketed builder of a packed 40-bit SA (n up to 2^40 as HBM allows).
// sa5: device, 5*n + SAS_SA40_PAD bytes.
int build_sa_gpu40(const uint64_t* tw, uint64_t n, uint8_t* sa5, uint32_t* rounds_out, uint64_t* buckets_out);
// Part builder (sas_build_part): the SA rank range of part `part` of `parts`
// (contiguous 7-mer bins), packed 40-bit; returns the device buffer, the range and
// SA[rank_hi] (n if none).
int build_sa_part40(const uint64_t* tw, uint64_t n, uint32_t part, uint32_t parts, uint8_t** sa5_out,
                    uint64_t* rank_lo, uint64_t* count, uint64_t* next_pos, uint32_t* rounds_out);

// build_lcp.hip.  full = the SA must be a permutation of 0..n (false for a shard's rank range)
int verify_sa(const uint64_t* tw, uint64_t n, const uint8_t* sa, uint32_t w, uint64_t sa_n, bool full);
int build_lcp(sas_index* x);
int build_llcp(sas_index* x);  // after build_lcp

// build_trees.hip.  build_rel: the binary search's pivot blocks, `levels` of them (0: the default)
int build_stree(sas_index* x);
int build_sector(sas_index* x);
int build_quad(sas_index* x, bool compact, uint32_t mode);
int build_rel(sas_index* x, uint32_t levels);

// build_prefix.hip (after build_quad): p chars (0: from sa_n), inl = suffixes per inline entry or 0
int build_prefix(sas_index* x, uint32_t p, uint32_t inl);

// build_tagged.hip: both replace the plain SA
int build_tagged(sas_index* x, uint32_t p);
int build_tag_lines(sas_index* x, uint32_t p);
