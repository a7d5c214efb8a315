/* sas.hpp -- C++17 host-side mirror of the reference's Rust query API over the C ABI
 * (sas.h, sst.h).  Header only; link libsas_amd.so.  The reference is compiled Rust, so the
 * host side above the ABI is compiled C++ with the reference's names and argument meaning:
 *
 *   sas::SaNaive::build(t)                SaNaive::build              sas/sa_search.rs:30-57
 *   sas::binary_search(sa, q, cnt)        binary_search (type F1)     sas/sa_search.rs:98-112, :453
 *   sas::binary_search_batch<B>(sa,qs,cnt) binary_search_batch<B> (F<B>) sas/sa_search.rs:157-196, :454
 *   sas::interpolation_search<16>(sa,q,cnt) interpolation_search<K>   sas/sa_search.rs:376-421
 *   sas::bench / sas::bench_batch         bench / bench_batch         sas/sa_search.rs:423-451
 *   SaNaive::search / search_prefix       Search::search/_prefix      sas/util.rs:29-47
 *   SaNaive::locate / search_between      search_prefix for a whole batch (CSR) / Search::search_range(Range)
 *   SaNaive::match                        longest-prefix match of a whole batch (sas_match; no counterpart)
 *   sas::random_string / random_queries   util.rs:9-26 (ChaCha8Rng::seed_from_u64(31415), main.rs:38)
 *   sas::read_fasta_file                  util.rs:144-169
 *   sst::SortedVec / Eytzinger / STree16 / STree15 / PartitionedSTree16M / DirectMap /
 *   PartitionedSTree16 / 16C / 16L / 16O
 *                                         SearchIndex::new/size/layers + SearchScheme::query
 *                                         sst/lib.rs:30-57, s_tree.rs:72-176, eytzinger.rs, binary_search.rs
 *
 * Every lookup runs on the GPU: host slices go through the library's pinned staging
 * pipeline.  Differences that the GPU makes worth having: `search_many` takes any number of
 * queries (no `array_chunks` remainder is dropped, sas/sa_search.rs:441), and a lower bound
 * of n returns the sentinel position n where the reference reads sa[n] out of bounds.
 *
 * Error behaviour: the reference panics with panic = "abort" (Cargo.toml:12).  Here a
 * non-zero status throws sas::Panic (a std::runtime_error carrying sas_last_error()); left
 * uncaught it terminates the process as the reference's panic does.
 *
 * Every batched call takes an empty batch: no kernel runs and the result vectors are empty, the
 * CSR offsets being {0} (sas.h: nq == 0 writes out_off[0] = 0 and nothing else); stride is still
 * set.  tests/cpp/test_calls.cpp runs each of them against recorded answers.
 */
#ifndef SAS_HPP
#define SAS_HPP

#include <array>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sas.h"
#include "sst.h"

namespace sas {

/* &[u8]: byte codes 0..3 (the reference's Seq = [u8], sas/util.rs:5-6) */
struct Seq {
    const uint8_t* ptr = nullptr;
    size_t len = 0;
    Seq() = default;
    Seq(const uint8_t* p, size_t n) : ptr(p), len(n) {}
    Seq(const std::vector<uint8_t>& v) : ptr(v.data()), len(v.size()) {}  // NOLINT: as &v[..]
    Seq slice(size_t a, size_t b) const { return Seq(ptr + a, b - a); }   // &t[a..b]
    size_t size() const { return len; }
};

struct Panic : std::runtime_error {
    int code;
    Panic(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
    if (rc != 0) throw Panic(rc, std::string("libsas_amd: ") + sas_last_error());
}

enum class Algo : int {
    Plain = SAS_ALGO_PLAIN,
    Lcp = SAS_ALGO_LCP,
    STree = SAS_ALGO_STREE,
    Sector = SAS_ALGO_SECTOR,
    Quad = SAS_ALGO_QUAD,
    Inline = SAS_ALGO_INLINE,
    Llcp = SAS_ALGO_LLCP,
    Prefix = SAS_ALGO_PREFIX,
    Interp = SAS_ALGO_INTERP,
    Tagged = SAS_ALGO_TAGGED,
    StreeLlcp = SAS_ALGO_STREE_LLCP,
    QuadLlcp = SAS_ALGO_QUAD_LLCP,
};

/* build flags of SaNaive::build: the LCP array, the fused quad tree and the p = 16 prefix
 * table with two-suffix inline entries (the fastest lookup at n = 2^30) */
constexpr uint32_t kDefaultBuild = SAS_BUILD_LCP | SAS_BUILD_QUAD | SAS_BUILD_PREFIX | SAS_BUILD_PREFIX_INLINE2;
/* the configs[3] index (long texts, long ragged queries): tagged entries in 128-B bucket
 * lines, no SA array; it answers Algo::Tagged lookups, ranges and sa(rank) */
constexpr uint32_t kLinesBuild = SAS_BUILD_TAGGED | SAS_BUILD_TAG_LINES;

/* GPU-resident replacement for SaNaive<'t> (sas/sa_search.rs:11-19): the packed text, the
 * SA and the search structures live in HBM; the caller keeps its text. */
class SaNaive {
   public:
    /* SaNaive::build(t) (sas/sa_search.rs:30-57): SA built and verified on the GPU */
    static SaNaive build(Seq t, uint32_t flags = kDefaultBuild) {
        sas_index* h = nullptr;
        if (t.len >= 0xFFFFFFFFull) flags &= ~(uint32_t)SAS_BUILD_PREFIX_INLINE2;  // 40-bit SA: rank table
        check(sas_build(t.ptr, t.len, nullptr, 4, flags | SAS_BUILD_VERIFY, &h));
        const Algo a = (flags & SAS_BUILD_TAGGED) ? Algo::Tagged : (flags & SAS_BUILD_PREFIX) ? Algo::Prefix : Algo::Plain;
        return SaNaive(h, t.len, a);
    }
    SaNaive(SaNaive&& o) noexcept : h_(o.h_), n_(o.n_), algo_(o.algo_) { o.h_ = nullptr; }
    SaNaive& operator=(SaNaive&& o) noexcept {
        std::swap(h_, o.h_);
        std::swap(n_, o.n_);
        std::swap(algo_, o.algo_);
        return *this;
    }
    SaNaive(const SaNaive&) = delete;
    SaNaive& operator=(const SaNaive&) = delete;
    ~SaNaive() {
        if (h_) sas_free(h_);
    }

    size_t n() const { return n_; }
    /* the fastest lookup the build flags made possible: Tagged (SAS_BUILD_TAGGED), Prefix
     * (SAS_BUILD_PREFIX), else Plain; Search::search uses it */
    Algo default_algo() const { return algo_; }
    const sas_index* raw() const { return h_; }
    sas_stats stats() const {
        sas_stats s{};
        check(sas_get_stats(h_, &s));
        return s;
    }

    /* the sequence layout (sas_set_layout): seq_start has one more entry than sequences, from 0
     * to n; the segments [seg_lo[i], seg_hi[i]) are the real bases.  An empty seq_start clears
     * it.  No call may be in flight on the index */
    void set_layout(const std::vector<uint64_t>& seq_start, const std::vector<uint64_t>& seg_lo = {},
                    const std::vector<uint64_t>& seg_hi = {}) {
        if (seg_lo.size() != seg_hi.size()) throw std::invalid_argument("set_layout: seg_lo and seg_hi differ in length");
        if (seq_start.size() == 1) throw std::invalid_argument("set_layout: seq_start needs at least two entries");
        check(sas_set_layout(h_, seq_start.data(), seq_start.empty() ? 0 : seq_start.size() - 1, seg_lo.data(),
                             seg_hi.data(), seg_lo.size()));
    }
    /* (sequence id, offset) of each interval [pos[i], pos[i] + span[i]) (no spans: 1 each):
     * SAS_SEQ_NONE and pos[i] itself unless the interval lies inside one segment (sas_translate) */
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> translate(const std::vector<uint64_t>& pos,
                                                                     const std::vector<uint32_t>& span = {}) const {
        if (!span.empty() && span.size() != pos.size()) throw std::invalid_argument("translate: one span per position");
        std::vector<uint32_t> seq(pos.size());
        std::vector<uint64_t> off(pos.size());
        check(sas_translate(h_, pos.data(), span.empty() ? nullptr : span.data(), pos.size(), seq.data(), off.data(),
                            nullptr, 0));
        return {std::move(seq), std::move(off)};
    }

    /* sa[rank] (SaNaive::suffix_at's position, sas/sa_search.rs:79-81) */
    uint64_t sa(uint64_t rank) const {
        uint64_t v = 0;
        check(sas_copy_sa64(h_, rank, 1, &v, 0));
        return v;
    }

    /* one batched lookup of any number of queries; cnt += the reference's probe counter */
    std::vector<size_t> search_many(const std::vector<Seq>& qs, Algo algo, size_t* cnt = nullptr,
                                    uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off(qs.size());
        std::vector<uint32_t> len(qs.size());
        size_t total = 0;
        for (size_t i = 0; i < qs.size(); i++) total += qs[i].len;
        bytes.reserve(total + 64);
        for (size_t i = 0; i < qs.size(); i++) {
            off[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(total + 64, 0);
        std::vector<uint64_t> pos(qs.size());
        std::vector<uint32_t> probes(cnt ? qs.size() : 0);
        if (!qs.empty())
            check(sas_search_batch(h_, bytes.data(), off.data(), len.data(), qs.size(), (int)algo, pos.data(),
                                   cnt ? probes.data() : nullptr, nullptr, flags));
        if (cnt)
            for (uint32_t p : probes) *cnt += p;
        return std::vector<size_t>(pos.begin(), pos.end());
    }

    /* Search::search (sas/util.rs:34): position of the smallest suffix >= q (n if none) */
    size_t search(Seq q) const {
        size_t c = 0;
        return search_many({q}, algo_, &c)[0];
    }

    /* occurrence range: global SA ranks [lo, hi) of the suffixes starting with q */
    std::pair<uint64_t, uint64_t> search_range(Seq q) const {
        const std::vector<uint8_t> b = padded(q);
        const uint64_t off = 0;
        const uint32_t len = (uint32_t)q.len;
        uint64_t lo = 0, hi = 0;
        check(sas_search_range(h_, b.data(), &off, &len, 1, &lo, &hi, nullptr, 0));
        return {lo, hi};
    }

    /* occurrence ranges of many queries in one call (the staged host pipeline) */
    std::vector<std::pair<uint64_t, uint64_t>> search_ranges(const std::vector<Seq>& qs, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off(qs.size()), lo(qs.size()), hi(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            off[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        if (!qs.empty())
            check(sas_search_range(h_, bytes.data(), off.data(), len.data(), qs.size(), lo.data(), hi.data(), nullptr,
                                   flags));
        std::vector<std::pair<uint64_t, uint64_t>> r(qs.size());
        for (size_t i = 0; i < qs.size(); i++) r[i] = {lo[i], hi[i]};
        return r;
    }

    /* Search::search_prefix (sas/util.rs:36-40, unimplemented!() upstream): every text
     * position where q occurs, in SA order */
    std::vector<size_t> search_prefix(Seq q) const {
        const auto r = search_range(q);
        std::vector<uint64_t> v(r.second - r.first);
        if (!v.empty()) check(sas_copy_sa64(h_, r.first, v.size(), v.data(), 0));
        return std::vector<size_t>(v.begin(), v.end());
    }

    /* CSR result of locate: query k's positions are pos[off[k] .. off[k+1]), in SA order */
    struct Located {
        std::vector<uint64_t> off, pos;
    };

    /* search_prefix for any number of queries in one call (sas_locate: range search, offsets
     * and the ragged expansion on the GPU, one copy back); max_per_query caps each query's
     * positions at its first max_per_query in SA order (0: no cap).  locate({}) is off = {0} and no
     * position */
    Located locate(const std::vector<Seq>& qs, uint64_t max_per_query = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Located r;
        r.off.assign(qs.size() + 1, 0);
        uint64_t total = 0;
        /* the sizing call (ENOSPC unless nothing occurs), then the real one */
        const int rc = sas_locate(h_, bytes.data(), qoff.data(), len.data(), qs.size(), max_per_query, r.off.data(),
                                  nullptr, 0, &total, nullptr, 0);
        if (rc != ENOSPC) check(rc);
        r.pos.resize(total);
        if (total)
            check(sas_locate(h_, bytes.data(), qoff.data(), len.data(), qs.size(), max_per_query, r.off.data(),
                             r.pos.data(), total, &total, nullptr, 0));
        return r;
    }

    /* longest-prefix match of query k: q[0 .. len) is the longest prefix that occurs in the text,
     * pos one position where it does (n when len == 0), [lo, hi) the SA ranks of every suffix
     * that starts with it */
    struct Matched {
        std::vector<uint32_t> len;
        std::vector<uint64_t> pos, lo, hi;
    };

    /* how much of each query occurs, and where, in one call (sas_match); ranges = false leaves
     * lo / hi empty (no tree needed) */
    Matched match(const std::vector<Seq>& qs, bool ranges = true, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Matched r;
        r.len.assign(qs.size(), 0);
        r.pos.assign(qs.size(), 0);
        if (ranges) {
            r.lo.assign(qs.size(), 0);
            r.hi.assign(qs.size(), 0);
        }
        if (!qs.empty())
            check(sas_match(h_, bytes.data(), qoff.data(), len.data(), qs.size(), r.len.data(), r.pos.data(),
                            ranges ? r.lo.data() : nullptr, ranges ? r.hi.data() : nullptr, nullptr, flags));
        return r;
    }

    /* CSR result of locate_mismatch: query k's alignments are pos[off[k] .. off[k+1]) with their
     * Hamming distances in dist, ordered by (reporting piece, SA rank); qflags[k] is a mask of
     * SAS_MM_TRUNCATED and SAS_MM_SHORT */
    struct Mismatched {
        std::vector<uint64_t> off, pos;
        std::vector<uint8_t> dist, qflags;
    };

    /* every alignment of every query with at most k substituted chars, in one call
     * (sas_locate_mismatch: seed and verify on the GPU); a seed that occurs more than
     * max_seed_hits times is skipped (0: no limit) */
    Mismatched locate_mismatch(const std::vector<Seq>& qs, uint32_t k, uint64_t max_seed_hits = 0,
                               uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Mismatched r;
        r.off.assign(qs.size() + 1, 0);
        r.qflags.assign(qs.size(), 0);
        uint64_t total = 0;
        /* the sizing call (ENOSPC unless nothing aligns), then the real one */
        const int rc = sas_locate_mismatch(h_, bytes.data(), qoff.data(), len.data(), qs.size(), k, max_seed_hits,
                                           r.off.data(), nullptr, nullptr, r.qflags.data(), 0, &total, nullptr, flags);
        if (rc != ENOSPC) check(rc);
        r.pos.resize(total);
        r.dist.resize(total);
        if (total)
            check(sas_locate_mismatch(h_, bytes.data(), qoff.data(), len.data(), qs.size(), k, max_seed_hits,
                                      r.off.data(), r.pos.data(), r.dist.data(), r.qflags.data(), total, &total,
                                      nullptr, flags));
        return r;
    }

    /* CSR result of mems: query k's maximal exact matches are the entries off[k] .. off[k+1]),
     * query[qpos .. qpos + len) = text[tpos .. tpos + len), ordered by (qpos, SA rank of tpos);
     * qflags[k] is a mask of SAS_MEM_TRUNCATED and SAS_MEM_SHORT */
    struct Mems {
        std::vector<uint64_t> off, tpos;
        std::vector<uint32_t> qpos, len;
        std::vector<uint8_t> qflags;
    };

    /* every maximal exact match of at least min_len chars of every query, in one call (sas_mems:
     * seed and extend on the GPU); a query offset whose first min_len chars occur more than
     * max_hits times is skipped (0: no limit); flags: SAS_MEM_UNIQUE keeps the matches whose
     * string occurs once in the text */
    Mems mems(const std::vector<Seq>& qs, uint32_t min_len, uint64_t max_hits = 0, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Mems r;
        r.off.assign(qs.size() + 1, 0);
        r.qflags.assign(qs.size(), 0);
        uint64_t total = 0;
        /* the sizing call (ENOSPC unless nothing matches), then the real one */
        const int rc = sas_mems(h_, bytes.data(), qoff.data(), len.data(), qs.size(), min_len, max_hits, r.off.data(),
                                nullptr, nullptr, nullptr, r.qflags.data(), 0, &total, nullptr, flags);
        if (rc != ENOSPC) check(rc);
        r.qpos.resize(total);
        r.tpos.resize(total);
        r.len.resize(total);
        if (total)
            check(sas_mems(h_, bytes.data(), qoff.data(), len.data(), qs.size(), min_len, max_hits, r.off.data(),
                           r.qpos.data(), r.tpos.data(), r.len.data(), r.qflags.data(), total, &total, nullptr, flags));
        return r;
    }

    /* CSR result of locate_edit: query k's end positions are end[off[k] .. off[k+1]), ascending,
     * with D(e) (the least edit distance of the query to a text substring ending at e) in dist;
     * qflags[k] is a mask of SAS_ED_TRUNCATED, SAS_ED_SHORT and SAS_ED_LONG */
    struct Edited {
        std::vector<uint64_t> off, end;
        std::vector<uint8_t> dist, qflags;
    };

    /* every end position of every query within edit distance k (substitutions, insertions and
     * deletions), in one call (sas_locate_edit: seed and verify on the GPU); a seed that occurs
     * more than max_seed_hits times is skipped (0: no limit) */
    Edited locate_edit(const std::vector<Seq>& qs, uint32_t k, uint64_t max_seed_hits = 0, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Edited r;
        r.off.assign(qs.size() + 1, 0);
        r.qflags.assign(qs.size(), 0);
        uint64_t total = 0;
        /* the sizing call (ENOSPC unless nothing is within k), then the real one */
        const int rc = sas_locate_edit(h_, bytes.data(), qoff.data(), len.data(), qs.size(), k, max_seed_hits,
                                       r.off.data(), nullptr, nullptr, r.qflags.data(), 0, &total, nullptr, flags);
        if (rc != ENOSPC) check(rc);
        r.end.resize(total);
        r.dist.resize(total);
        if (total)
            check(sas_locate_edit(h_, bytes.data(), qoff.data(), len.data(), qs.size(), k, max_seed_hits,
                                  r.off.data(), r.end.data(), r.dist.data(), r.qflags.data(), total, &total, nullptr,
                                  flags));
        return r;
    }

    /* Result of align_edit, one entry per end of an Edited: start[a] is the largest s with
     * ed(query, t[s .. end[a])) = dist[a], the least distance of any start; the script from
     * (0, s) is runs[a * stride .. a * stride + nruns[a]), each run (len << 2) | op with op one of
     * SAS_AL_EQ, SAS_AL_X, SAS_AL_INS and SAS_AL_DEL; stride = 2k + 1, unused slots are 0.  An end
     * without an alignment within k has start = n, dist = SAS_AL_NONE_DIST and nruns = 0 */
    struct Aligned {
        std::vector<uint64_t> start;
        std::vector<uint8_t> dist, nruns;
        std::vector<uint16_t> runs;
        size_t stride = 1;
    };

    /* where the alignment of every end of `e` (locate_edit of the same queries) starts, and its
     * edit script, in one call (sas_align_edit: a banded pass and a walk per end on the GPU) */
    Aligned align_edit(const std::vector<Seq>& qs, uint32_t k, const Edited& e, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Aligned r;
        const size_t na = e.end.size();
        r.stride = 2 * (size_t)k + 1;
        r.start.assign(na, n_);
        r.dist.assign(na, (uint8_t)SAS_AL_NONE_DIST);
        r.nruns.assign(na, 0);
        r.runs.assign(na * r.stride, 0);
        if (na)
            check(sas_align_edit(h_, bytes.data(), qoff.data(), len.data(), qs.size(), k, e.off.data(), e.end.data(),
                                 na, r.start.data(), r.dist.data(), r.nruns.data(), r.runs.data(), nullptr, flags));
        return r;
    }

    /* Result of map_edit, one record per read: the best alignment on the selected strands
     * (strand 1: the read's reverse complement against t[start .. end)), n_best / n_loci = the
     * equally good and all places (n_best == 1 && n_loci == 1: the unique mapping), the script as
     * in Aligned, qflags = SAS_ED_* of the strands.  An unmapped read has end = start = n,
     * dist = SAS_AL_NONE_DIST and n_best = 0 */
    struct Mapped {
        std::vector<uint64_t> end, start;
        std::vector<uint8_t> dist, strand, nruns, qflags;
        std::vector<uint32_t> n_best, n_loci;
        std::vector<uint16_t> runs;
        size_t stride = 1;
    };

    /* read mapping in one call (sas_map_edit): every read's best alignment within k edits on both
     * strands (strands: SAS_MAP_FWD | SAS_MAP_REV), its script and how many places are as good */
    Mapped map_edit(const std::vector<Seq>& qs, uint32_t k, uint64_t max_seed_hits = 0,
                    uint32_t strands = SAS_MAP_FWD | SAS_MAP_REV, uint32_t flags = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        Mapped r;
        const size_t nq = qs.size();
        r.stride = 2 * (size_t)k + 1;
        r.end.assign(nq, n_);
        r.start.assign(nq, n_);
        r.dist.assign(nq, (uint8_t)SAS_AL_NONE_DIST);
        r.strand.assign(nq, 0);
        r.nruns.assign(nq, 0);
        r.qflags.assign(nq, 0);
        r.n_best.assign(nq, 0);
        r.n_loci.assign(nq, 0);
        r.runs.assign(nq * r.stride, 0);
        check(sas_map_edit(h_, bytes.data(), qoff.data(), len.data(), nq, k, max_seed_hits, strands, r.end.data(),
                           r.start.data(), r.dist.data(), r.strand.data(), r.n_best.data(), r.n_loci.data(),
                           r.nruns.data(), r.runs.data(), r.qflags.data(), nullptr, flags));
        return r;
    }

    /* Result of map_pairs: Mapped's fields, one entry per read (pair i = reads 2i and 2i + 1), and
     * per pair pflags (SAS_PAIR_PROPER), n_pairs = the proper candidates and n_best_pairs = those
     * of the least summed distance */
    struct MappedPairs : Mapped {
        std::vector<uint8_t> pflags;
        std::vector<uint32_t> n_pairs, n_best_pairs;
    };

    /* paired-end mapping in one call (sas_map_pairs): qs holds the pairs interleaved, mate 1 then
     * mate 2 (an odd number of reads throws std::invalid_argument); a pair with a forward / reverse
     * placement whose fragment length is in [min_frag, max_frag] gets that placement, every other
     * read its own map_edit record */
    MappedPairs map_pairs(const std::vector<Seq>& qs, uint32_t k, uint32_t min_frag, uint32_t max_frag,
                          uint64_t max_seed_hits = 0, uint32_t flags = 0) const {
        if (qs.size() % 2) throw std::invalid_argument("map_pairs: an odd number of reads");
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        MappedPairs r;
        const size_t nq = qs.size(), np = nq / 2;
        r.stride = 2 * (size_t)k + 1;
        r.end.assign(nq, n_);
        r.start.assign(nq, n_);
        r.dist.assign(nq, (uint8_t)SAS_AL_NONE_DIST);
        r.strand.assign(nq, 0);
        r.nruns.assign(nq, 0);
        r.qflags.assign(nq, 0);
        r.n_best.assign(nq, 0);
        r.n_loci.assign(nq, 0);
        r.runs.assign(nq * r.stride, 0);
        r.pflags.assign(np, 0);
        r.n_pairs.assign(np, 0);
        r.n_best_pairs.assign(np, 0);
        check(sas_map_pairs(h_, bytes.data(), qoff.data(), len.data(), np, k, max_seed_hits, min_frag, max_frag,
                            r.end.data(), r.start.data(), r.dist.data(), r.strand.data(), r.n_best.data(),
                            r.n_loci.data(), r.nruns.data(), r.runs.data(), r.qflags.data(), r.pflags.data(),
                            r.n_pairs.data(), r.n_best_pairs.data(), nullptr, flags));
        return r;
    }

    /* Result of map_pairs_rescue: MappedPairs' fields (pflags also SAS_PAIR_RESCUED and
     * SAS_PAIR_RESCUE_SKIPPED, qflags also SAS_MAP_RESCUED, stride = 2 k_rescue + 1) and per pair
     * n_rescue = the runs of candidate ends in its anchors' windows */
    struct MappedPairsRescue : MappedPairs {
        std::vector<uint32_t> n_rescue;
    };

    /* map_pairs with mate rescue (sas_map_pairs_rescue): a pair without a proper placement and with
     * at most max_anchors loci (0: no rescue) has the fragment window of each locus scanned for the
     * other mate within k_rescue >= k edits, with no seeds */
    MappedPairsRescue map_pairs_rescue(const std::vector<Seq>& qs, uint32_t k, uint32_t k_rescue, uint32_t min_frag,
                                       uint32_t max_frag, uint64_t max_anchors, uint64_t max_seed_hits = 0,
                                       uint32_t flags = 0) const {
        if (qs.size() % 2) throw std::invalid_argument("map_pairs_rescue: an odd number of reads");
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> qoff(qs.size());
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); i++) {
            qoff[i] = bytes.size();
            len[i] = (uint32_t)qs[i].len;
            bytes.insert(bytes.end(), qs[i].ptr, qs[i].ptr + qs[i].len);
        }
        bytes.resize(bytes.size() + 64, 0);
        MappedPairsRescue r;
        const size_t nq = qs.size(), np = nq / 2;
        r.stride = 2 * (size_t)k_rescue + 1;
        r.end.assign(nq, n_);
        r.start.assign(nq, n_);
        r.dist.assign(nq, (uint8_t)SAS_AL_NONE_DIST);
        r.strand.assign(nq, 0);
        r.nruns.assign(nq, 0);
        r.qflags.assign(nq, 0);
        r.n_best.assign(nq, 0);
        r.n_loci.assign(nq, 0);
        r.runs.assign(nq * r.stride, 0);
        r.pflags.assign(np, 0);
        r.n_pairs.assign(np, 0);
        r.n_best_pairs.assign(np, 0);
        r.n_rescue.assign(np, 0);
        check(sas_map_pairs_rescue(h_, bytes.data(), qoff.data(), len.data(), np, k, k_rescue, max_seed_hits, min_frag,
                                   max_frag, max_anchors, r.end.data(), r.start.data(), r.dist.data(),
                                   r.strand.data(), r.n_best.data(), r.n_loci.data(), r.nruns.data(), r.runs.data(),
                                   r.qflags.data(), r.pflags.data(), r.n_pairs.data(), r.n_best_pairs.data(),
                                   r.n_rescue.data(), nullptr, flags));
        return r;
    }

    /* Search::search_range over a Range<&Seq> (sas/util.rs:41-46, unimplemented!() upstream):
     * the positions of the suffixes s with a <= s < b, in SA order.  One range on host
     * pointers: two lower bounds and one sas_copy_sa64; batches of ranges are
     * sas_locate_offsets + sas_locate_fill, which take device pointers */
    std::vector<size_t> search_between(Seq a, Seq b) const {
        const auto r = search_ranges({a, b});
        const uint64_t lo = r[0].first, hi = r[1].first;
        std::vector<uint64_t> v(hi > lo ? hi - lo : 0);
        if (!v.empty()) check(sas_copy_sa64(h_, lo, v.size(), v.data(), 0));
        return std::vector<size_t>(v.begin(), v.end());
    }

   private:
    SaNaive(sas_index* h, size_t n, Algo a) : h_(h), n_(n), algo_(a) {}
    static std::vector<uint8_t> padded(Seq q) {
        std::vector<uint8_t> b(q.ptr, q.ptr + q.len);
        b.resize(q.len + 64, 0);
        return b;
    }
    sas_index* h_ = nullptr;
    size_t n_ = 0;
    Algo algo_ = Algo::Prefix;
};

/* type F1 (sas/sa_search.rs:453): binary_search (:98-112), the canonical lookup: the
 * position of the lower bound of q under slice order; cnt counts loop iterations */
inline size_t binary_search(const SaNaive& sa, Seq q, size_t& cnt) { return sa.search_many({q}, Algo::Plain, &cnt)[0]; }

/* the same positions from the fastest GPU structure (PREFIX: the prefix table made live);
 * cnt counts as binary_search's does from the table's range (1 + iterations) */
inline size_t prefix_search(const SaNaive& sa, Seq q, size_t& cnt) { return sa.search_many({q}, Algo::Prefix, &cnt)[0]; }

/* interpolation_search<K> (sas/sa_search.rs:376-421), K = 16 as main.rs:97 runs it */
template <size_t K = 16>
inline size_t interpolation_search(const SaNaive& sa, Seq q, size_t& cnt) {
    static_assert(K == 16, "the GPU kernel restates interpolation_search<16>");
    return sa.search_many({q}, Algo::Interp, &cnt)[0];
}

/* type F<B> (sas/sa_search.rs:454): binary_search_batch<B> (:157-196) */
template <size_t B>
inline std::array<size_t, B> binary_search_batch(const SaNaive& sa, const std::array<Seq, B>& qs, size_t& cnt) {
    const auto v = sa.search_many(std::vector<Seq>(qs.begin(), qs.end()), Algo::Plain, &cnt);
    std::array<size_t, B> out{};
    for (size_t i = 0; i < B; i++) out[i] = v[i];
    return out;
}

using F1 = size_t (*)(const SaNaive&, Seq, size_t&);

/* bench (sas/sa_search.rs:423-436): time f over the queries, print name, total, per query,
 * per probe, probes per query to stderr; returns the elapsed seconds */
inline double bench(const SaNaive& sa, const std::vector<Seq>& queries, const char* name, F1 f) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t cnt = 0;
    for (const Seq& q : queries) f(sa, q, cnt);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "%-20s: %8.2fs %6.0fns %6.0fns %5.2f\n", name, s, s * 1e9 / queries.size(),
                 s * 1e9 / (cnt ? cnt : 1), (double)cnt / queries.size());
    return s;
}

/* bench_batch (sas/sa_search.rs:438-451), except that the whole query list is one GPU
 * batch (the reference's array_chunks::<B> drops the remainder) */
inline double bench_batch(const SaNaive& sa, const std::vector<Seq>& queries, const char* name,
                          Algo algo = Algo::Prefix) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t cnt = 0;
    sa.search_many(queries, algo, &cnt);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "%-20s: %8.2fs %6.0fns %6.0fns %5.2f\n", name, s, s * 1e9 / queries.size(),
                 s * 1e9 / (cnt ? cnt : 1), (double)cnt / queries.size());
    return s;
}

/* the script in runs[a * stride .. a * stride + nruns[a]) as a string such as "17=1X14=" */
inline std::string cigar(const std::vector<uint16_t>& runs, const std::vector<uint8_t>& nruns, size_t stride, size_t a) {
    std::string s;
    for (size_t i = 0; i < nruns[a]; i++) {
        const uint16_t run = runs[a * stride + i];
        s += std::to_string(run >> 2);
        s += "=XID"[run & 3u];
    }
    return s;
}

/* the script of alignment a of an Aligned as a string such as "17=1X14=": = a match, X a
 * substitution, I a query char that the text lacks, D a text char that the query lacks */
inline std::string cigar(const SaNaive::Aligned& r, size_t a) { return cigar(r.runs, r.nruns, r.stride, a); }

/* the script of read a of a Mapped, MappedPairs or MappedPairsRescue, against the strand it was
 * placed on ("" for an unmapped read) */
inline std::string cigar(const SaNaive::Mapped& r, size_t a) { return cigar(r.runs, r.nruns, r.stride, a); }

/* random_string (sas/util.rs:9-15) with ChaCha8Rng::seed_from_u64(seed) */
inline std::vector<uint8_t> random_string(size_t n, uint64_t seed = 31415) {
    std::vector<uint8_t> t(n);
    if (n) check(sas_gen_text(seed, n, t.data(), 0));
    return t;
}

/* random_queries (sas/util.rs:18-26): substrings t[i..i+len], i < n - margin, len in
 * [len_lo, len_hi); the ChaCha8 stream continues after the text's n words */
inline std::vector<Seq> random_queries(Seq t, size_t nq, uint64_t seed = 31415, uint32_t len_lo = 30,
                                       uint32_t len_hi = 100, uint64_t margin = 200) {
    std::vector<uint64_t> off(nq);
    std::vector<uint32_t> len(nq);
    if (nq) check(sas_gen_queries(seed, t.len, t.len, nq, margin, len_lo, len_hi, off.data(), len.data(), nullptr));
    std::vector<Seq> qs(nq);
    for (size_t i = 0; i < nq; i++) qs[i] = t.slice(off[i], off[i] + len[i]);
    return qs;
}

/* read_fasta_file (sas/util.rs:144-169): A/C/G/T/a/c/g/t -> 0..3, every other byte -> 0 */
inline std::vector<uint8_t> read_fasta_file(const std::string& path) {
    uint64_t n = 0;
    check(sas_read_fasta(path.c_str(), nullptr, 0, &n));
    std::vector<uint8_t> v(n);
    check(sas_read_fasta(path.c_str(), v.data(), n, &n));
    v.resize(n);
    return v;
}

}  // namespace sas

namespace sst {

using sas::check;

/* SearchIndex (sst/lib.rs:30-48) over sorted u32 keys: new / size / layers, and query
 * (SearchScheme::query, :55-57): the first key >= q for every query (u32::MAX if none for
 * Eytzinger and SortedVec, as upstream; the S-trees need the MAX sentinel the reference's
 * tests push, sst/s_tree.rs:864) */
class SearchIndex {
   public:
    SearchIndex(SearchIndex&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    SearchIndex& operator=(SearchIndex&& o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    SearchIndex(const SearchIndex&) = delete;
    ~SearchIndex() {
        if (h_) sst_free(h_);
    }
    size_t size() const { return (size_t)sst_size(h_); }
    size_t layers() const { return (size_t)sst_layers(h_); }
    std::vector<uint32_t> query(const std::vector<uint32_t>& qs) const {
        std::vector<uint32_t> out(qs.size());
        if (!qs.empty()) check(sst_query(h_, qs.data(), qs.size(), out.data(), nullptr, nullptr, 0));
        return out;
    }
    uint32_t query_one(uint32_t q) const { return query({q})[0]; }
    /* the leaf slot of each answer (the rank the SA use of the tree needs) */
    std::vector<uint64_t> ranks(const std::vector<uint32_t>& qs) const {
        std::vector<uint32_t> v(qs.size());
        std::vector<uint64_t> r(qs.size());
        if (!qs.empty()) check(sst_query(h_, qs.data(), qs.size(), v.data(), r.data(), nullptr, 0));
        return r;
    }

   protected:
    static sst_index* make(const std::vector<uint32_t>& vals, int layout, uint32_t flags) {
        sst_index* h = nullptr;
        check(sst_build(vals.data(), vals.size(), layout, flags, &h));
        return h;
    }
    explicit SearchIndex(sst_index* h) : h_(h) {}
    sst_index* h_ = nullptr;
};

struct SortedVec : SearchIndex {  // sst/binary_search.rs:8-49
    static SortedVec new_(const std::vector<uint32_t>& v) { return SortedVec(make(v, SST_SORTED, 0)); }
    using SearchIndex::SearchIndex;
};
struct Eytzinger : SearchIndex {  // sst/eytzinger.rs:9-180
    static Eytzinger new_(const std::vector<uint32_t>& v) { return Eytzinger(make(v, SST_EYTZINGER, 0)); }
    using SearchIndex::SearchIndex;
};
template <int LAYOUT>
struct STree : SearchIndex {  // sst/s_tree.rs:14-20: STree16 = STree<16,16>, STree15 = STree<15,16>
    /* SearchIndex::new = new_params(vals, false, false, false) (s_tree.rs:48-50) */
    static STree new_(const std::vector<uint32_t>& v) { return new_params(v, false, false, false); }
    /* STree::new_params (s_tree.rs:72-176) */
    static STree new_params(const std::vector<uint32_t>& v, bool left_max, bool reverse, bool full) {
        const uint32_t f = (left_max ? SST_LEFT_MAX : 0) | (reverse ? SST_REVERSE : 0) | (full ? SST_FULL : 0);
        return STree(make(v, LAYOUT, f));
    }
    using SearchIndex::SearchIndex;
};
using STree16 = STree<SST_STREE16>;
using STree15 = STree<SST_STREE15>;
struct PartitionedSTree16M : SearchIndex {  // sst/partitioned_s_tree.rs:98
    static PartitionedSTree16M new_(const std::vector<uint32_t>& v, uint32_t b) {
        return PartitionedSTree16M(make(v, SST_PARTITIONED_MAP, SST_PART_BITS(b)));
    }
    using SearchIndex::SearchIndex;
};
/* PartitionedSTree<16,16,Tp>::new(vals, b) for Tp = Simple, Compact, L1, Overlapping
   (sst/partitioned_s_tree.rs:86-94 type aliases; values only: the leaves are padded) */
template <int LAYOUT>
struct PartitionedSTree : SearchIndex {
    static PartitionedSTree new_(const std::vector<uint32_t>& v, uint32_t b) {
        return PartitionedSTree(make(v, LAYOUT, SST_PART_BITS(b)));
    }
    using SearchIndex::SearchIndex;
};
using PartitionedSTree16 = PartitionedSTree<SST_PARTITIONED>;
using PartitionedSTree16C = PartitionedSTree<SST_PARTITIONED_COMPACT>;
using PartitionedSTree16L = PartitionedSTree<SST_PARTITIONED_L1>;
using PartitionedSTree16O = PartitionedSTree<SST_PARTITIONED_OVERLAP>;
struct DirectMap : SearchIndex {  // the prefix map taken to its limit (sst.h SST_DIRECT_MAP)
    static DirectMap new_(const std::vector<uint32_t>& v) { return DirectMap(make(v, SST_DIRECT_MAP, 0)); }
    using SearchIndex::SearchIndex;
};

}  // namespace sst

#endif /* SAS_HPP */
