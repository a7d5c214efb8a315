// seed_verify.hpp -- what the seed-and-verify calls share (sas_mismatch.hip: Hamming distance,
// sas_edit.hip: edit distance, and the calls built on them: sas_align.hip, sas_map.hip,
// sas_pairs.hip, sas_rescue.hip; sas_match.hip takes the index preconditions), over the call
// scaffolding of call_io.hpp (scratch, scan, the host-pointer path, the query batch MmQueries):
//
//   * device code that the kernels of those files inline: the cut of a query into k + 1 pieces,
//     and the output-centric tiling (csr_tile.hpp) of the candidates (one candidate = one
//     occurrence of one piece) and of the elements of a CSR list (sas_align.hip: alignments,
//     sas_map.hip: the bytes of a ragged batch);
//   * the grid of the helper kernels, and what every verify stage does round its kernel: the
//     read-back of the candidate total, the answer "nothing found", the verify grid, the
//     *_TIMING knob (SeedTiming) and its event pair (SeedTimer);
//   * declared here and defined once in seed_verify.hip: the index preconditions
//     (seed_index_checks), the seed stage up to the candidate offsets (seed_candidates) and the
//     one call path of the calls that return per-query lists in two passes (seed_list_call:
//     sas_locate_mismatch, sas_locate_edit, sas_mems).
#pragma once
#include "call_io.hpp"
#include "csr_tile.hpp"

#include <functional>

#define MM_BLOCK 256
#define MM_T 2048          // candidates per tile
#define MM_PER (MM_T / MM_BLOCK)
#define MM_SLICE 4096      // candidate offsets of a tile staged in LDS (16 KiB)
#define MM_MAX_GRID (1u << 20)
#define MM_MAX_K 15

// b_j: the first char of piece j of a query of m chars cut into kp1 pieces
__device__ __forceinline__ uint32_t mm_piece_start(uint32_t j, uint32_t m, uint32_t kp1) {
    return (uint32_t)(((uint64_t)j * m) / kp1);
}

// The candidates [t0, t0 + n_el) of one tile (n_el <= MM_T), for the whole workgroup of MM_BLOCK
// threads: element e = u MM_BLOCK + tid is occurrence c - coff[pi] of piece pi[u] (its owner in
// the candidate offsets: csr_tile_owners) and lies at text position pv[u] = SA[lo[pi] + c -
// coff[pi]]; ok[u] = 0 for an element past the tile, one that fails the offsets' own bounds or
// one whose rank is no rank of the SA.  All SA reads of a thread are issued before the first is
// used.  `rel` (MM_SLICE words) and `sh_p` (2 words) are LDS; the caller puts a __syncthreads()
// between two tiles.
template <class SA>
__device__ __forceinline__ void mm_tile_candidates(const SA& sa, const uint64_t* __restrict__ coff,
                                                   const uint64_t* __restrict__ lo, uint64_t np, uint64_t n,
                                                   uint64_t t0, uint32_t n_el, uint32_t* rel, uint64_t* sh_p,
                                                   uint64_t (&pi)[MM_PER], uint64_t (&pv)[MM_PER],
                                                   uint32_t (&ok)[MM_PER]) {
    uint64_t rk[MM_PER] = {};
    csr_tile_owners<MM_T, MM_SLICE, MM_BLOCK>(coff, np, t0, n_el, rel, sh_p, pi, ok,
                                              [&](int u, uint64_t c, uint64_t p) {
                                                  rk[u] = lo[p] + (c - coff[p]);
                                                  return csr_in_bounds(coff, p, c) && rk[u] < n;
                                              });
#pragma unroll
    for (int u = 0; u < MM_PER; u++) pv[u] = ok[u] ? sa[rk[u]] : 0;
}

#define AL_BLOCK 256
#define AL_T 1024           // elements per tile
#define AL_PER (AL_T / AL_BLOCK)
#define AL_SLICE 2048       // query offsets of a tile staged in LDS (8 KiB)

// The queries of the elements [t0, t0 + n_el) of one tile of a CSR list (n_el <= AL_T; off: its
// nq + 1 offsets), for the whole workgroup of AL_BLOCK threads: csr_tile_owners at the AL sizes
__device__ __forceinline__ void al_tile_queries(const uint64_t* __restrict__ off, uint64_t nq, uint64_t t0,
                                                uint32_t n_el, uint32_t* rel, uint64_t* sh_p, uint64_t (&qi)[AL_PER],
                                                uint32_t (&ok)[AL_PER]) {
    csr_tile_owners<AL_T, AL_SLICE, AL_BLOCK>(off, nq, t0, n_el, rel, sh_p, qi, ok,
                                              [&](int, uint64_t c, uint64_t q) { return csr_in_bounds(off, q, c); });
}

// The grid of a helper kernel of 256 threads that strides over `count` elements: at most 8
// workgroups per CU, and SAS_TILE_GRID's cap
static inline dim3 seed_grid(const sas_index* x, uint64_t count) {
    return dim3(tile_grid(std::min(grid_for(count), (unsigned)x->num_cus * 8)));
}

// One total of a verify stage (the candidates coff[np], the proposals) read back; synchronises
static inline int seed_read_total(const uint64_t* dev, hipStream_t st, uint64_t* total) {
    HIP_TRY(hipMemcpyAsync(total, dev, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The answer of a batch without a candidate: nq + 1 zero offsets and a zero total (may be null)
static inline int seed_nothing(uint64_t* out_off, uint64_t nq, uint64_t* out_total, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(out_off, 0, (nq + 1) * 8, st));
    if (out_total) HIP_TRY(hipMemsetAsync(out_total, 0, 8, st));
    return 0;
}

// The grid of a verify kernel over C candidates: one workgroup per tile of MM_T, at most
// MM_MAX_GRID (they stride beyond), and SAS_TILE_GRID's cap
static inline dim3 seed_verify_grid(uint64_t C) {
    return dim3((unsigned)tile_grid(std::min<uint64_t>((C + MM_T - 1) / MM_T, MM_MAX_GRID)));
}

// A *_TIMING knob (<env>=1, read at every call: the stages are timed with HIP events, which
// synchronises) and the calling thread's last figures for the extern "C" *_ms getters.  Slot 0:
// the verify kernel and the candidates; slot 1 (sas_locate_edit): the de-duplication, proposals
struct SeedTiming {
    const char* env;
    double ms[2] = {-1.0, -1.0};
    uint64_t count[2] = {0, 0};
    bool on() const {
        const char* e = getenv(env);
        return e && e[0] == '1';
    }
    void reset(uint64_t candidates) {
        ms[0] = ms[1] = -1.0;
        count[0] = candidates;
        count[1] = 0;
    }
    double get(int slot, uint64_t* n) const {
        if (n) *n = count[slot];
        return ms[slot];
    }
};

// The event pair of a SeedTiming knob: nothing happens unless `on`; the events are
// destroyed on every way out.  stop() synchronises and gives the time since the last start()
struct SeedTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    bool on;
    SeedTimer(bool on_, hipStream_t st_) : st(st_), on(on_) {}
    SeedTimer(const SeedTimer&) = delete;
    ~SeedTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int start() {
        if (!on) return 0;
        if (!e0) HIP_TRY(hipEventCreate(&e0));
        if (!e1) HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        return 0;
    }
    int stop(double* ms_out) {
        if (!on) return 0;
        float ms = 0;
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms;
        return 0;
    }
};

// What every call of the family asks of its index, in this order: an index, k <= MM_MAX_K, no
// tagged index, a whole index, a u32 or packed 40-bit SA, SAS_LOCATE_U32 only below 2^32 chars
// and, with `probe`, the range search's own requirements (its error is passed on).  w: the
// call's name, the head of every message
int seed_index_checks(const std::string& w, const sas_index* x, uint32_t k, uint32_t flags, void* stream,
                      bool probe = true);

// A call that returns per-query lists in two passes, as it describes itself to seed_list_call:
// its name, its word in the host-pointer path's labels ("<label> queries"), the words of its
// ENOSPC text (host_list_total) and, where it has one, a check of its own that follows the null test
struct ListCall {
    const char *fn, *label, *noun, *hint;
    std::function<int()> check;
};
// One payload output: `capacity` elements of esz bytes; label: its twin's; required: null is
// refused where the capacity is not 0
struct ListOut {
    void* ptr;
    size_t esz;
    const char* label;
    bool required;
};
// Pass 1, all arrays on the device (out_qflags and out_total may be null): offsets, flags, total;
// the callable keeps the scratch for pass 2.  flags: the call's, SAS_VALIDATE forced on host pointers
typedef std::function<int(const MmQueries& Q, uint64_t* out_off, uint8_t* out_qflags, uint64_t* out_total,
                          hipStream_t st, uint32_t flags)> ListPrepare;
// Pass 2: the first `capacity` elements into the device arrays out[i] of ListOut i
typedef std::function<int(void* const* out, uint64_t capacity, hipStream_t st)> ListScatter;

// Such a call behind its own checks, in this order: the null test ("<fn>: null argument": out_off,
// the queries, a required output, out_total on host pointers), the call's check, hipSetDevice, the
// answer of nq == 0; then on device pointers prepare and scatter, on host pointers the staged queries, the
// twins of out_off and out_qflags, prepare, host_list_total, and for a total above 0 the
// payload's twins of `total` elements, scatter and the copy back
int seed_list_call(const ListCall& c, const sas_index* x, const QueryArgs& q, uint64_t nq, uint64_t* out_off,
                   uint8_t* out_qflags, const ListOut* outs, int nouts, uint64_t capacity, uint64_t* out_total,
                   void* stream, uint32_t flags, const ListPrepare& prepare, const ListScatter& scatter);

// Steps 1 to 4 of sas_mismatch.hip and sas_edit.hip, the scratch of which stays in the state:
// the pieces, their gated SA ranges [lo, hi) and the candidate offsets coff (np + 1; the caller
// reads the candidate total coff[np] back when it needs it)
struct SeedState {
    hipMemPool_t pool = nullptr;
    PoolBuf poff, plen, lohi, coff, qfl, skip;
    uint64_t* lo = nullptr;  // np each
    uint64_t* hi = nullptr;
};

// The three stages of seed_candidates that do not depend on how a query is cut, for a call that
// cuts it otherwise (sas_mems.hip: overlapping windows, one per query offset): the scratch of np
// seeds (poff, plen, lohi, coff; lo and hi set), sas_search_range over the seeds that the caller
// wrote into poff / plen (flags: the call's; SAS_NO_PREFIX_TABLE and SAS_VALIDATE are passed on),
// and sas_locate_offsets on the ranges as the caller's gate left them.  No host read
int seed_alloc(const sas_index* x, uint64_t np, hipStream_t st, SeedState& s);
int seed_ranges(const sas_index* x, const uint8_t* qbytes, uint64_t np, hipStream_t st, uint32_t flags, SeedState& s);
int seed_offsets(const sas_index* x, uint64_t np, hipStream_t st, SeedState& s);

// All arrays on the device.  A query of more than max_m chars gets no seeds and SAS_ED_LONG;
// skip_mask: s.skip gets, per query, a u16 whose bit j says that piece j is no seed; qflags (may
// be null): the per-query flags, SAS_MM_* = SAS_ED_*.  No host read
int seed_candidates(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t max_m,
                    bool skip_mask, uint8_t* qflags, hipStream_t st, uint32_t flags, SeedState& s);
