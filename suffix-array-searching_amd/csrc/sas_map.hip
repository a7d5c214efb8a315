// sas_map.hip -- one record per read on both strands (sas.h: sas_map_edit, sas_map_edit_fixed)
// and the reverse complement it needs (sas_revcomp, sas_revcomp_fixed).  Steps 1..3 and their
// kernels are in map_path.hpp (map_select_batch), shared with sas_pairs.hip.
//
//   1. the batch      forward only: the caller's queries as they are.  Otherwise one scratch batch
//                     of the participating strands, forward as query i and reverse as query nq + i
//                     (reverse alone: query i): k_map_revcomp_fixed, or for ragged queries mm_scan
//                     over qlen, k_map_layout (offsets and lengths of the batch) and k_map_fill
//                     (output-centric over the batch's bytes: a workgroup owns a tile of output
//                     bytes and finds each one's query with al_tile_queries);
//   2. ed_prepare     the seed / verify / sort path of sas_edit.hip, once over that batch: the P
//                     sorted proposals, key = (batch query << ebits) | end, with their distances.
//                     Duplicates are adjacent; the first of a run of equal keys is the end itself;
//   3. k_map_select   output-centric over the sorted proposals, two passes.  A workgroup owns a
//                     tile of MAP_T consecutive proposals; the query of a proposal is in its key,
//                     and its left neighbour in the list tells whether it is a duplicate, the first
//                     end of its query or the first of an interval of consecutive ends, so the
//                     cost per proposal is the same whether 10^7 reads own one end each or one
//                     read owns 10^6.  Pass 1 reduces, per batch query, the minimum of
//                     dist << 56 | end and the number of interval starts; pass 2, with the read's
//                     least distance known from pass 1, the number of starts of intervals at that
//                     distance.  The reduction is segmented: inside the wave by shuffles, inside
//                     the tile by LDS atomics of one lane per (wave, segment) into the segment's
//                     slot (its rank in the tile, from a ballot scan of the segment heads).  A
//                     segment that lies inside the tile is then written with plain stores; only
//                     the (at most two) segments that cross a tile edge use 64-bit atomicMin /
//                     atomicAdd on the slots, which are initialised before the pass.  Integer min
//                     and add: the result does not depend on the order of arrival;
//   4. k_map_finalize one thread per read: the least (dist, strand, end) of the two strands'
//                     slots, the counts summed and clamped to 32 bits, the flags ORed, and the
//                     request of one alignment per read: off = 0 .. nq, the winner's bytes in the
//                     batch as a ragged query, length 0 (no alignment) for an unmapped read;
//   5. sas_align_edit over those nq alignments, chained on the stream.
#include "map_path.hpp"

struct MapFin {
    MmQueries B;            // the batch
    uint64_t nq, n;
    uint32_t strands;
    const uint64_t* kmin;
    const uint64_t* nloci;
    const uint64_t* nbest;
    const uint8_t* efl;     // the batch queries' SAS_ED_* flags
    void* out_end;
    uint8_t* out_dist;
    uint8_t* out_strand;    // may be null, as the three below
    uint32_t* out_nbest;
    uint32_t* out_nloci;
    uint8_t* out_qflags;
    uint64_t* aoff;         // the alignment request: nq + 1 offsets 0 .. nq,
    uint64_t* aqoff;        // the winner's bytes in the batch
    uint32_t* aqlen;        // and their length (0: no alignment)
};

template <bool U32>
__global__ void k_map_finalize(MapFin a) {
    const uint32_t copies = a.strands == (SAS_MAP_FWD | SAS_MAP_REV) ? 2u : 1u;
    GRID_STRIDE(i, a.nq + 1) {
        a.aoff[i] = i;
        if (i == a.nq) continue;
        const MapBest r = map_best_of(i, a.nq, copies, a.strands, a.kmin, a.nloci, a.nbest, a.efl);
        const uint64_t best = r.best;
        const bool mapped = best != MAP_NONE;
        const uint64_t e = mapped ? best & ((1ull << 55) - 1ull) : a.n;
        if (U32) static_cast<uint32_t*>(a.out_end)[i] = (uint32_t)e;
        else static_cast<uint64_t*>(a.out_end)[i] = e;
        a.out_dist[i] = mapped ? (uint8_t)(best >> 56) : (uint8_t)SAS_AL_NONE_DIST;
        if (a.out_strand) a.out_strand[i] = mapped ? (uint8_t)((best >> 55) & 1ull) : 0;
        if (a.out_nbest) a.out_nbest[i] = map_clamp32(r.nbst);
        if (a.out_nloci) a.out_nloci[i] = map_clamp32(r.nl);
        if (a.out_qflags) a.out_qflags[i] = (uint8_t)r.fl;
        a.aqoff[i] = a.B.off(r.bb);
        a.aqlen[i] = mapped ? a.B.len(r.bb) : 0u;
    }
}

struct MapOut {
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

// All arrays on the device; Q: the caller's queries
static int map_device(const sas_index* x, const MmQueries& Q, uint32_t k, uint64_t max_seed_hits, uint32_t strands,
                      const MapOut& o, hipStream_t st, uint32_t flags) {
    const uint64_t nq = Q.nq;
    hipMemPool_t pool;
    TRY(sas_scratch_pool(x, &pool));
    const unsigned cap_grid = (unsigned)x->num_cus * 8;
    const auto grid = [&](uint64_t count) { return dim3(tile_grid(std::min(grid_for(count), cap_grid))); };
    // 1..3. the batch, its sorted proposals, the slots (map_path.hpp)
    MapState ms;
    TRY(map_select_batch(x, Q, k, max_seed_hits, strands, st, flags, ms));
    const MmQueries& B = ms.B;
    // 4. the records and the alignment request
    MmPoolBuf areq;
    const bool align = o.start || o.nruns || o.runs;
    const bool u32 = (flags & SAS_LOCATE_U32) != 0;
    const uint64_t esz = u32 ? 4 : 8;
    TRY(areq.alloc(pool, (nq + 1) * 8 + nq * 8 + nq * 4 + (o.start ? 0 : nq * esz), st));
    MapFin f{};
    f.B = B;
    f.nq = nq;
    f.n = x->n;
    f.strands = strands;
    f.kmin = ms.kmin;
    f.nloci = ms.nloci;
    f.nbest = ms.nbest;
    f.efl = ms.efl.as<uint8_t>();
    f.out_end = o.end;
    f.out_dist = o.dist;
    f.out_strand = o.strand;
    f.out_nbest = o.nbest;
    f.out_nloci = o.nloci;
    f.out_qflags = o.qflags;
    f.aoff = areq.as<uint64_t>();
    f.aqoff = f.aoff + nq + 1;
    void* scratch_start = f.aqoff + nq;                  // 8-byte aligned; unused when out_start is given
    f.aqlen = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch_start) + (o.start ? 0 : nq * esz));
    if (u32) hipLaunchKernelGGL(k_map_finalize<true>, grid(nq + 1), dim3(256), 0, st, f);
    else hipLaunchKernelGGL(k_map_finalize<false>, grid(nq + 1), dim3(256), 0, st, f);
    HIP_TRY(hipGetLastError());
    // 5. one alignment per read (bytes were validated by the range search when asked for)
    if (!align) return 0;
    return sas_align_edit(x, B.qbytes, f.aqoff, f.aqlen, nq, k, f.aoff, o.end, nq, o.start ? o.start : scratch_start,
                          nullptr, o.nruns, o.runs, st, SAS_DEVICE_PTRS | (flags & SAS_LOCATE_U32));
}

static int map_impl(const char* fn, const sas_index* x, const uint8_t* qbytes, bool ragged, const uint64_t* qoff,
                    const uint32_t* qlen, uint32_t m, uint64_t nq, uint32_t k, uint64_t max_seed_hits,
                    uint32_t strands, const MapOut& o, void* stream, uint32_t flags) {
    const std::string w(fn);
    if (strands == 0 || strands > (SAS_MAP_FWD | SAS_MAP_REV))
        SAS_FAIL(EINVAL, w + ": strands must be SAS_MAP_FWD, SAS_MAP_REV or both");
    if (!x) SAS_FAIL(EINVAL, w + ": null index");
    if (k > MM_MAX_K) SAS_FAIL(EINVAL, w + ": k must be 0.." + std::to_string(MM_MAX_K));
    if (x->tag_lines || x->sa_w == 8)
        SAS_FAIL(ENOTSUP, w + ": a tagged index (SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES) is not served");
    if (x->rank_lo != 0 || x->sa_n != x->n)
        SAS_FAIL(ENOTSUP, w + ": needs a whole index (a shard or part holds only a rank range of the SA)");
    if (!x->sa || (x->sa_w != 4 && x->sa_w != 5)) SAS_FAIL(ENOTSUP, w + ": needs a u32 or packed 40-bit SA array");
    if ((flags & SAS_LOCATE_U32) && x->n >= (1ull << 32))
        SAS_FAIL(EINVAL, w + ": SAS_LOCATE_U32 needs a text of n < 2^32 chars");
    // the (batch query, end) sort key of both strands
    if (ed_bits(x->n) + (nq ? ed_bits(2 * nq - 1) : 0) > 64)
        SAS_FAIL(EINVAL, w + ": " + std::to_string(nq) + " reads on two strands and a text of " + std::to_string(x->n) +
                             " chars do not fit the 64-bit (query, end) sort key: split the batch");
    TRY(sas_search_range_fixed(x, nullptr, 1, 0, nullptr, nullptr, stream, flags & SAS_DEVICE_PTRS));
    if (nq == 0) return 0;
    if (!qbytes || (ragged && (!qoff || !qlen)) || !o.end || !o.dist) SAS_FAIL(EINVAL, w + ": null argument");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & SAS_DEVICE_PTRS) {
        const MmQueries Q{qbytes, ragged ? qoff : nullptr, qlen, m, nq};
        return map_device(x, Q, k, max_seed_hits, strands, o, st, flags);
    }
    // host arrays: copy in, the device path, copy out (synchronous; bytes always validated)
    uint64_t span = nq * (uint64_t)m;
    if (ragged) {
        span = 0;
        for (uint64_t i = 0; i < nq; i++) span = std::max(span, qoff[i] + qlen[i]);
    }
    const uint64_t esz = (flags & SAS_LOCATE_U32) ? 4 : 8, stride = 2 * (uint64_t)k + 1;
    DevBuf dq, dqoff, dqlen, dend, dstart, ddist, dstrand, dnbest, dnloci, dnruns, druns, dfl;
    TRY(dq.alloc(span + 64, "map queries"));
    HIP_TRY(hipStreamSynchronize(st));
    if (span) HIP_TRY(hipMemcpy(dq.p, qbytes, span, hipMemcpyHostToDevice));
    if (ragged) {
        TRY(dqoff.alloc(nq * 8, "map query offsets"));
        TRY(dqlen.alloc(nq * 4, "map query lengths"));
        HIP_TRY(hipMemcpy(dqoff.p, qoff, nq * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dqlen.p, qlen, nq * 4, hipMemcpyHostToDevice));
    }
    TRY(dend.alloc(nq * esz, "map ends"));
    TRY(ddist.alloc(nq, "map distances"));
    if (o.start) TRY(dstart.alloc(nq * esz, "map starts"));
    if (o.strand) TRY(dstrand.alloc(nq, "map strands"));
    if (o.nbest) TRY(dnbest.alloc(nq * 4, "map best counts"));
    if (o.nloci) TRY(dnloci.alloc(nq * 4, "map locus counts"));
    if (o.nruns) TRY(dnruns.alloc(nq, "map run counts"));
    if (o.runs) TRY(druns.alloc(nq * stride * 2, "map runs"));
    if (o.qflags) TRY(dfl.alloc(nq, "map query flags"));
    const MmQueries Q{dq.as<uint8_t>(), ragged ? dqoff.as<uint64_t>() : nullptr, dqlen.as<uint32_t>(), m, nq};
    const MapOut d{dend.p, dstart.p, ddist.as<uint8_t>(), dstrand.as<uint8_t>(), dnbest.as<uint32_t>(),
                   dnloci.as<uint32_t>(), dnruns.as<uint8_t>(), druns.as<uint16_t>(), dfl.as<uint8_t>()};
    TRY(map_device(x, Q, k, max_seed_hits, strands, d, st, flags | SAS_VALIDATE));
    HIP_TRY(hipMemcpyAsync(o.end, dend.p, nq * esz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(o.dist, ddist.p, nq, hipMemcpyDeviceToHost, st));
    if (o.start) HIP_TRY(hipMemcpyAsync(o.start, dstart.p, nq * esz, hipMemcpyDeviceToHost, st));
    if (o.strand) HIP_TRY(hipMemcpyAsync(o.strand, dstrand.p, nq, hipMemcpyDeviceToHost, st));
    if (o.nbest) HIP_TRY(hipMemcpyAsync(o.nbest, dnbest.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (o.nloci) HIP_TRY(hipMemcpyAsync(o.nloci, dnloci.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (o.nruns) HIP_TRY(hipMemcpyAsync(o.nruns, dnruns.p, nq, hipMemcpyDeviceToHost, st));
    if (o.runs) HIP_TRY(hipMemcpyAsync(o.runs, druns.p, nq * stride * 2, hipMemcpyDeviceToHost, st));
    if (o.qflags) HIP_TRY(hipMemcpyAsync(o.qflags, dfl.p, nq, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_map_edit(const sas_index* x, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                            uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint32_t strands, void* out_end,
                            void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                            uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                            void* stream, uint32_t flags) {
    const MapOut o{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags};
    return map_impl("sas_map_edit", x, qbytes, true, qoff, qlen, 0, nq, k, max_seed_hits, strands, o, stream, flags);
}

extern "C" int sas_map_edit_fixed(const sas_index* x, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                                  uint64_t max_seed_hits, uint32_t strands, void* out_end, void* out_start,
                                  uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci,
                                  uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags, void* stream,
                                  uint32_t flags) {
    const MapOut o{out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs, out_qflags};
    return map_impl("sas_map_edit_fixed", x, qbytes, false, nullptr, nullptr, m, nq, k, max_seed_hits, strands, o,
                    stream, flags);
}

// Device arrays, on the current device (the call takes no index): scratch from its default pool
static int revcomp_device(const char* fn, const uint8_t* q, const uint64_t* qoff, const uint32_t* qlen, uint32_t m,
                          uint64_t nq, uint8_t* out, uint64_t* out_off, hipStream_t st, bool validate) {
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const unsigned cap_grid = (unsigned)std::max(cus, 1) * 8;
    DevBuf bflag;  // a per-call flag word when it is read back
    if (validate) {
        TRY(bflag.alloc(4, "revcomp flag"));
        HIP_TRY(hipMemsetAsync(bflag.p, 0, 4, st));
    }
    if (qoff) {
        hipMemPool_t pool;
        HIP_TRY(hipDeviceGetDefaultMemPool(&pool, dev));
        TRY(mm_scan(pool, st,
                    rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), MapLenAt{qlen, nq}),
                    out_off, nq + 1));
        // the grid does not wait for the byte total: the tiles are strided over it
        hipLaunchKernelGGL(k_map_fill, dim3(tile_grid(cap_grid)), dim3(AL_BLOCK), 0, st, q, qoff, qlen,
                           nq, out_off, nq, (uint64_t)0, out, bflag.as<uint32_t>());
    } else {
        hipLaunchKernelGGL(k_map_revcomp_fixed, dim3(tile_grid(std::min(grid_for(nq * (uint64_t)m), cap_grid))),
                           dim3(256), 0, st, q, m, nq, out, bflag.as<uint32_t>());
    }
    HIP_TRY(hipGetLastError());
    if (validate) {
        uint32_t hbad = 0;
        HIP_TRY(hipMemcpyAsync(&hbad, bflag.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hbad) SAS_FAIL(EINVAL, std::string(fn) + ": query bytes must be DNA codes 0..3");
    }
    return 0;
}

static int revcomp_impl(const char* fn, const uint8_t* qbytes, bool ragged, const uint64_t* qoff,
                        const uint32_t* qlen, uint32_t m, uint64_t nq, uint8_t* out_bytes, uint64_t* out_off,
                        void* stream, uint32_t flags) {
    const std::string w(fn);
    const bool dev = (flags & SAS_DEVICE_PTRS) != 0;
    if (ragged && !out_off) SAS_FAIL(EINVAL, w + ": null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq == 0) {
        if (ragged) {
            if (dev) HIP_TRY(hipMemsetAsync(out_off, 0, 8, st));
            else out_off[0] = 0;
        }
        return 0;
    }
    if (ragged && (!qoff || !qlen)) SAS_FAIL(EINVAL, w + ": null argument");
    if (dev) {
        if (!qbytes || !out_bytes) SAS_FAIL(EINVAL, w + ": null argument");
        return revcomp_device(fn, qbytes, ragged ? qoff : nullptr, qlen, m, nq, out_bytes, out_off, st,
                              (flags & SAS_VALIDATE) != 0);
    }
    // host arrays: copy in, the kernel, copy out (synchronous; bytes always validated)
    uint64_t span = nq * (uint64_t)m, total = span;
    if (ragged) {
        span = total = 0;
        for (uint64_t i = 0; i < nq; i++) {
            span = std::max(span, qoff[i] + qlen[i]);
            total += qlen[i];
        }
    }
    if (total && (!qbytes || !out_bytes)) SAS_FAIL(EINVAL, w + ": null argument");
    DevBuf dq, dqoff, dqlen, dout, doff;
    TRY(dq.alloc(span + 64, "revcomp queries"));
    TRY(dout.alloc(total + 64, "revcomp output"));
    HIP_TRY(hipStreamSynchronize(st));
    if (span) HIP_TRY(hipMemcpy(dq.p, qbytes, span, hipMemcpyHostToDevice));
    if (ragged) {
        TRY(dqoff.alloc(nq * 8, "revcomp query offsets"));
        TRY(dqlen.alloc(nq * 4, "revcomp query lengths"));
        TRY(doff.alloc((nq + 1) * 8, "revcomp offsets"));
        HIP_TRY(hipMemcpy(dqoff.p, qoff, nq * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dqlen.p, qlen, nq * 4, hipMemcpyHostToDevice));
    }
    TRY(revcomp_device(fn, dq.as<uint8_t>(), ragged ? dqoff.as<uint64_t>() : nullptr, dqlen.as<uint32_t>(), m, nq,
                       dout.as<uint8_t>(), doff.as<uint64_t>(), st, true));
    if (total) HIP_TRY(hipMemcpyAsync(out_bytes, dout.p, total, hipMemcpyDeviceToHost, st));
    if (ragged) HIP_TRY(hipMemcpyAsync(out_off, doff.p, (nq + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sas_revcomp(const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
                           uint8_t* out_bytes, uint64_t* out_off, void* stream, uint32_t flags) {
    return revcomp_impl("sas_revcomp", qbytes, true, qoff, qlen, 0, nq, out_bytes, out_off, stream, flags);
}

extern "C" int sas_revcomp_fixed(const uint8_t* qbytes, uint32_t m, uint64_t nq, uint8_t* out_bytes, void* stream,
                                 uint32_t flags) {
    return revcomp_impl("sas_revcomp_fixed", qbytes, false, nullptr, nullptr, m, nq, out_bytes, nullptr, stream,
                        flags);
}
