/*
 * sas.h -- C ABI of the MI355X suffix-array search engine (libsas_amd.so).
 *
 * Drop-in boundary for the reference's Rust SA query API
 * (RagnarGrootKoerkamp/suffix-array-searching, sas/ = suffix-array-searching/src):
 *
 *   sas_build          replaces SaNaive::build(t: &Seq) -> SaNaive      sas/sa_search.rs:30-57
 *                      and Search::build                                  sas/util.rs:31
 *   sas_search_batch   replaces the batch type F<B>                       sas/sa_search.rs:454
 *                        fn(&SaNaive, [&[u8]; B], &mut usize) -> [usize; B]
 *                      and the single-query type F1                       sas/sa_search.rs:453
 *                        fn(&SaNaive, &[u8], &mut usize) -> usize   (nq = 1)
 *                      Semantics of every algo = binary_search            sas/sa_search.rs:98-112
 *                        position SA[lower_bound(q)] under Rust slice order.
 *   sas_search_fixed   the same for a contiguous block of fixed-length queries
 *   sas_gen_text       random_string(n, ChaCha8Rng::seed_from_u64(seed))  sas/util.rs:9-15, sas/main.rs:38
 *   sas_gen_queries    random_queries(t, q, rng)                          sas/util.rs:18-26
 *
 * Conventions (no C++ exceptions cross this ABI; sas/Cargo.toml panics instead):
 *   - every function returns 0 on success or a positive errno value
 *     (EINVAL bad argument, ENOMEM device memory, ENOTSUP unsupported size,
 *     EIO HIP runtime failure); sas_last_error() gives a thread-local message.
 *   - text and query bytes are DNA codes 0..3 (the reference's random_string
 *     and FASTA loader only produce these, sas/util.rs:9-15,144-169).
 *   - a query above every suffix gets the sentinel position n (the reference
 *     reads sa[n] out of bounds there).
 *   - pointers are host pointers unless SAS_DEVICE_PTRS is set, in which case
 *     every input/output array of the call is device (HBM) memory.
 *   - a built index is immutable and thread-safe; concurrent searches on
 *     different streams are allowed.
 */
#ifndef SAS_H
#define SAS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sas_index sas_index;

/* flags */
#define SAS_DEVICE_PTRS   (1u << 0)  /* all array arguments are device pointers          */
#define SAS_BUILD_LCP     (1u << 1)  /* also build the LCP array (Kasai semantics)       */
#define SAS_BUILD_STREE   (1u << 2)  /* also build the S-tree over 16-char SA keys       */
#define SAS_BUILD_VERIFY  (1u << 3)  /* run the range + adjacency + permutation check on
                                        the whole SA, a caller's at its own width: see
                                        sas_verify                                        */
#define SAS_NO_LDS_TOP    (1u << 4)  /* search: do not serve the top levels from LDS     */
#define SAS_VALIDATE      (1u << 5)  /* search: reject query bytes > 3 (synchronises)    */
#define SAS_ROUTE_PACKED  (1u << 26)  /* sas_route_pack(_cap): write each query as one 2-bit
                                         packed word (m <= 32, 8 B per send slot, the
                                         sas_search_packed format) instead of its m bytes */
#define SAS_NO_PREFIX_TABLE (1u << 25) /* sas_search_range: use the tree descents even when
                                        the index has a prefix table                      */
#define SAS_QUERIES_ARE_SLICES (1u << 28) /* sas_search_batch, SAS_ALGO_TAGGED, device pointers:
                                        query k is the slice t[qoff[k] .. qoff[k] + qlen[k])
                                        of the indexed text itself (the reference's borrowed
                                        &t[i..i+len] queries, sas/util.rs:18-26); qbytes is
                                        ignored (may be NULL), the chars come from the index's
                                        packed text, and a lookup whose candidate suffix is
                                        the query's own start skips its text compare.  The
                                        call checks every slice lies inside the text (EINVAL)
                                        and synchronises on the stream to do so            */
#define SAS_RANGE_NO_INLINE (1u << 27) /* sas_search_range(_fixed): on a two/four-suffix inline
                                        prefix table, bisect both bounds from the table's rank
                                        range instead of testing the inline slots first     */
#define SAS_LOCATE_U32    (1u << 29) /* sas_locate*: out_pos holds u32 positions instead of u64
                                        (EINVAL for a text of n >= 2^32 chars)              */
#define SAS_LOCATE_NO_PARTITION (1u << 30) /* sas_locate*, sas_locate_fill: no partition pre-pass; each
                                        workgroup bisects out_off for its tiles' first queries
                                        itself (the same result; an A/B hook)               */
#define SAS_PREFIX_RANGE  (1u << 24) /* search, PLAIN / LCP: start binary_search from the
                                        prefix table's range of q's first p chars, as the
                                        reference's binary_search does (sas/sa_search.rs:
                                        98-101); needs SAS_BUILD_PREFIX                    */
#define SAS_BUILD_WIDE    (1u << 6)  /* build: use the n >= 2^31 two-pass doubling rounds
                                        at any n (test hook for that path)               */
#define SAS_BUILD_SECTOR  (1u << 7)  /* also build the sector tree (SAS_ALGO_SECTOR)     */
#define SAS_BUILD_SA40    (1u << 8)  /* store the SA as packed 40-bit entries and use the
                                        bucketed 64-bit builder at any n (automatic for
                                        n >= 2^32 - 64; test hook below that)             */
#define SAS_BUILD_QUAD    (1u << 9)  /* also build the quad tree (SAS_ALGO_QUAD)         */
#define SAS_BUILD_QUAD_COMPACT (1u << 10) /* build the quad tree with key-only leaves: 8 B
                                        per suffix (eight 32-char keys per 64-B leaf) instead
                                        of 16, SA values read from the SA array.  Fits next to
                                        a 40-bit SA at n = 2^34 in one GPU's HBM.  Implies
                                        SAS_BUILD_QUAD                                     */
#define SAS_BUILD_QUAD_ABS (1u << 11) /* quad tree inner nodes in the absolute layout: 16 u32
                                        16-char separators, 17-ary                        */
#define SAS_BUILD_QUAD_REL (1u << 12) /* quad tree inner nodes in the prefix-relative layout:
                                        the node's shared d-char prefix + 30 u16 separators
                                        over the next 8 chars, 31-ary.  Neither flag: the
                                        layout with fewer levels larger than the 256 MiB
                                        Infinity Cache (absolute on a tie; n = 2^30 builds
                                        absolute, n = 2^34 compact builds relative)        */
#define SAS_BUILD_PREFIX  (1u << 14) /* also build the prefix table for SAS_ALGO_PREFIX (the
                                        reference's fill_prefix_table, sas/sa_search.rs:59-95):
                                        u32[4^p + 1], entry x = first SA rank whose p-char
                                        key is >= x.  p = SAS_BUILD_PREFIX_P(p) (1..17) or,
                                        if 0, ceil(log4(n)) + 1 capped at 16 (16 at n = 2^30:
                                        16 GiB).  Needs SAS_BUILD_QUAD.  u32 entries, or
                                        packed 40-bit ones beside a 40-bit SA             */
#define SAS_BUILD_PREFIX_INLINE (1u << 15) /* the prefix table with 16-B entries: the first
                                        suffix of each key's range inlined as {32-char key,
                                        rank, SA}, so a lookup answered by that suffix is
                                        one read.  Fused quad leaves, u32 SA only         */
#define SAS_BUILD_PREFIX_INLINE2 (1u << 21) /* the prefix table with 32-B entries: the first
                                        TWO suffixes of each key's range (ranks r, r + 1)
                                        inlined, read by a lane pair as one request       */
#define SAS_BUILD_PREFIX_INLINE4 (1u << 22) /* 64-B entries: the first FOUR suffixes of each
                                        range, read by a 4-lane group as one request      */
#define SAS_BUILD_PREFIX_P(p) ((uint32_t)(p) << 16)  /* bits 16..20: prefix chars       */
#define SAS_BUILD_TAGGED  (1u << 23) /* store the SA as 8-B tagged entries {SA 40 bits | the
                                        suffix's chars [p, p+12) in the high 24 bits} plus a
                                        u64 bucket table over the first p chars {first rank
                                        40 bits | rank count 24 bits} (the reference's prefix
                                        table, sas/sa_search.rs:59-95, live) for
                                        SAS_ALGO_TAGGED: an entry holds a suffix's (p+12)-char
                                        key AND its position, so a lookup is the bucket
                                        entry, one window of consecutive entries and (for
                                        m > p + 12) one text window.  p = SAS_BUILD_PREFIX_P
                                        or ceil(log4 n) capped at 16 (16 at n = 2^34: 32 GiB
                                        table beside 128 GiB of entries).  The entries
                                        replace the SA (sa_width 8).  Combines with LCP;
                                        not with the trees, LLCP or SAS_BUILD_PREFIX*  */
#define SAS_BUILD_TOP2_LEVELS(L) ((uint32_t)(L) << 27) /* bits 27..31: depth L (1..31) of
                                        the binary-search pivots (PLAIN / LCP / LLCP / INLINE):
                                        prefix-relative blocks of up to 4 levels (32 B each:
                                        the lcp P of the block's bounds and the 8 chars after
                                        P of 15 pivots); levels 1-15 (72.5 KiB) are staged in
                                        each workgroup's LDS, the rest cost one request per
                                        block instead of an SA word and a text window per
                                        level.  L is rounded up to the 4-level grid past the
                                        LDS levels (19, 23, 27, 31).  0 = the default, 27
                                        levels (273 MiB); 31 levels cost 4.3 GiB at n = 2^30.
                                        Clamped to the iteration count; results never depend
                                        on L                                               */
#define SAS_BUILD_TAG_LINES (1u << 24) /* with SAS_BUILD_TAGGED: the tagged entries as one
                                        128-B line per p-char bucket {overflow offset 40 bits
                                        | count 24 bits, the 20 entries of ranks first ..
                                        first + 19 as 48-bit {SA | tag} split into u16 high and
                                        u32 low halves} (slots past the bucket's count hold the
                                        next buckets' first suffixes, so the line ends with
                                        the answer to "every suffix of the bucket is < q") plus
                                        an overflow array with ranks first + 20 .. first + count
                                        of the larger buckets, the buckets' first ranks and a
                                        second text copy 64 B off the 128-B line grid.  A
                                        lookup reads its line as one request of an 8-lane
                                        group: bucket and first entries together.  p =
                                        SAS_BUILD_PREFIX_P or ceil(log4 n) - 2 (15 at n = 2^34:
                                        128 GiB of lines, ~16 suffixes each).  No SA array:
                                        TAGGED lookups, ranges and sas_copy_sa64          */
#define SAS_BUILD_LLCP    (1u << 13) /* also build the Manber-Myers accelerant for
                                        SAS_ALGO_LLCP: per SA rank m, one 16-B entry
                                        {SA[m] 40 bits, Llcp 12 bits, Rlcp 12 bits, 16 chars
                                        of SA[m] after each} of the binary-search interval
                                        whose mid is m, derived from the LCP array (built
                                        too).  16 B per suffix                           */

/* search algorithms; all return bit-identical positions */
enum sas_algo {
    SAS_ALGO_PLAIN = 0, /* lockstep lower-bound binary search over SA (A6/A9)              */
    SAS_ALGO_LCP   = 1, /* same probes, Manber-Myers mlr LCP skipping of known chars (A21) */
    SAS_ALGO_STREE = 2, /* S-tree over 16-char SA keys + exact tail search (K2+K3)         */
    SAS_ALGO_SECTOR = 3, /* sector tree: 32-B nodes (one HBM sector), 9-ary on 16-char keys,
                           leaves fuse (32-char key, SA value) pairs: no text/SA reads for m<=32 */
    SAS_ALGO_QUAD = 4,  /* quad tree: 4 lanes per query load each 64-B node in one request;
                           31-ary on the 8 chars after each node's shared prefix (17-ary on
                           16-char keys with SAS_BUILD_QUAD_ABS), leaves = 4 fused (32-char
                           key, SA) entries                                                  */
    SAS_ALGO_INLINE = 5, /* PLAIN's probe sequence (binary_search_batch) over the quad tree's
                           fused (32-char key, SA) entries: one 16-B read per probe instead of
                           an SA word + text words ("inlining values", todo.org:18-19)     */
    SAS_ALGO_LLCP = 6,  /* PLAIN's probe sequence with Manber-Myers LLCP/RLCP skipping: a probe
                           reads one 16-B {SA, Llcp, Rlcp, chars} entry and decides from the
                           lcp values alone unless they tie llcp/rlcp; a tie compares the
                           entry's 16 chars before any text (needs SAS_BUILD_LLCP; the LCP
                           array at work, A21)                                              */
    SAS_ALGO_PREFIX = 7, /* prefix table lookup (the rank range of q's first p chars, one 8-B
                           read; sas/sa_search.rs:59-95) + binary search over that range on
                           the quad tree's leaf entries: ~2 memory requests per lookup
                           (needs SAS_BUILD_PREFIX)                                          */
    SAS_ALGO_INTERP = 8, /* interpolation_search<16> (sas/sa_search.rs:376-421): the mid is
                           interpolated from string_value<16> of the bounds and the query
                           (sas/util.rs:76-117), clamped to [1/16, 15/16] of the range, exact
                           compares; out_probes = its cnt.  Reads the fused quad leaves'
                           {32-char key, SA} entries when built (one request per probe),
                           else SA + text.  With SAS_PREFIX_RANGE it starts from the prefix
                           table's range.  n < 2^32 (the reference asserts r_val * r fits a
                           usize, :389-392); ENOTSUP above                                   */
    SAS_ALGO_TAGGED = 9, /* bucket table + tagged SA entries (needs SAS_BUILD_TAGGED): the
                           configs[3] shape's lookup, ~4-5 memory requests for a long query  */
    SAS_ALGO_STREE_LLCP = 10, /* configs[2]'s combination: the STREE descent over the 16-char SA keys
                           (LDS-staged top layers) gives the run of suffixes sharing q's key,
                           then Manber-Myers LLCP skipping finishes inside it (the LLCP entries'
                           binary-search tree walked from its root, mids outside the run decided
                           with no read); needs SAS_BUILD_STREE and SAS_BUILD_LLCP          */
    SAS_ALGO_QUAD_LLCP = 11 /* configs[2] as one kernel: QUAD's descent over the fused 32-char
                           keys (LDS-staged top layers); a query the routed leaf does not settle
                           (q's 32-char key shared by several suffixes: long queries on
                           repetitive text) continues with LLCP skipping inside the run of
                           suffixes sharing its key, whose far end comes from where the path of
                           the next 16-char key parts from q's.  m <= 32: QUAD itself.  Needs
                           SAS_BUILD_QUAD with fused leaves in the absolute layout (the default
                           below 2^31 suffixes; SAS_BUILD_QUAD_ABS) and SAS_BUILD_LLCP        */
};

typedef struct sas_stats {
    uint64_t n;              /* text length (chars)                               */
    uint64_t text_bytes;     /* packed 2-bit text in HBM                          */
    uint64_t sa_bytes;       /* suffix array (sa_width bytes per entry)           */
    uint64_t lcp_bytes;      /* LCP array (u32), 0 if not built                   */
    uint64_t stree_bytes;    /* S-tree incl. 16-char key leaves, 0 if not built   */
    uint32_t stree_layers;   /* S-tree height (layers incl. leaves)               */
    uint32_t stree_lds_layers; /* layers served from LDS                          */
    uint32_t top_levels;     /* binary-search levels served from LDS (15, fewer for a
                                shallow search)                                       */
    uint32_t iterations;     /* ilog2(n)+1 lockstep iterations (sa_search.rs:171) */
    uint64_t build_sa_ns;    /* wall time of the SA construction (0 if supplied)  */
    uint64_t build_total_ns; /* wall time of sas_build                            */
    uint32_t sa_rounds;      /* prefix-doubling rounds after the 32-char sort     */
    uint32_t sa_width;       /* bytes per stored SA entry: 4 (u32) or 5 (40-bit)  */
    uint64_t rank_lo;        /* global SA rank of this index's first entry         */
    uint64_t sa_entries;     /* SA entries held (n, or a shard's rank range)       */
    uint64_t next_pos;       /* SA[rank_lo + sa_entries] (n if none)               */
    uint64_t sector_bytes;   /* sector tree (inner nodes + fused leaves), 0 if not built */
    uint32_t sector_layers;  /* sector tree height incl. the leaf layer           */
    uint32_t sector_lds_layers; /* its layers served from LDS                     */
    uint64_t quad_bytes;     /* quad tree (inner nodes + leaves), 0 if not built   */
    uint32_t quad_layers;    /* quad tree height incl. the leaf layer              */
    uint32_t quad_lds_layers; /* its layers served from LDS                       */
    uint32_t quad_entry_bytes; /* quad leaf bytes per suffix: 16 (fused key + SA),
                                  8 (SAS_BUILD_QUAD_COMPACT), 0 if not built        */
    uint32_t quad_fan;       /* quad inner-node fan-out: 31 (prefix-relative nodes) or
                                17 (SAS_BUILD_QUAD_ABS), 0 if not built              */
    uint32_t top2_levels;    /* binary-search levels whose pivots come from LDS or the
                                prefix-relative blocks (PLAIN/LCP/LLCP/INLINE)       */
    uint64_t llcp_bytes;     /* SAS_BUILD_LLCP entries (16 B per suffix), 0 if not built */
    uint64_t prefix_bytes;   /* SAS_BUILD_PREFIX table, 0 if not built                */
    uint32_t prefix_chars;   /* its p (chars per table key)                           */
    uint32_t tag_chars;      /* SAS_BUILD_TAGGED: p of the bucket table (0 if not built);
                                sa_width is then 8 (tagged entries)                   */
    uint64_t tag_table_bytes; /* SAS_BUILD_TAGGED bucket table, (4^p + 1) x 8 B       */
    uint64_t index_bytes;    /* every HBM array of the index together (text, SA or tagged
                                entries, LCP, LLCP, trees, tables, top2)              */
    uint32_t tag_line_slots; /* SAS_BUILD_TAG_LINES: entries per 128-B bucket line (20), else 0;
                                tag_table_bytes is then the lines and the first-rank
                                table, sa_bytes the overflow                          */
    uint32_t tag_line_tag_bits; /* SAS_BUILD_TAG_LINES: tag bits of a line entry (48 minus
                                the SA bits: 16 below n = 2^32, 13 at n = 2^34)       */
    uint64_t tag_overflow_entries; /* SAS_BUILD_TAG_LINES: entries in the overflow array */
    uint64_t text2_bytes;    /* SAS_BUILD_TAG_LINES: the second packed-text copy (64 B off
                                the 128-B line grid, so a tie's compare reads one line) */
    uint64_t top2_bytes;     /* 0 since round 4: every pivot level is in the rel blocks */
    uint32_t rel_levels;     /* the prefix-relative pivot blocks: the levels they reach
                                (the pivot depth rounded up to 4-level blocks past the
                                15 LDS levels, clamped to the iterations; 0 if none) */
    uint32_t rel_pad;        /* 0 */
    uint64_t rel_bytes;      /* their array: one 32-B block {lcp of the block's bounds, the
                                8 chars after it of each of 15 pivots} per 4-level subtree
                                (16 B for a shorter one), the LDS levels' first    */
    uint64_t prefix_key_lo;  /* SAS_BUILD_PREFIX: the first p-char key the table holds an entry
                                for: 0 for a whole index; for a part / shard (a contiguous SA
                                rank range) the key of its first suffix                */
    uint64_t prefix_entries; /* its entries: 4^p + 1 for a whole index; for a part, its first
                                suffix's key .. its last one's + 2 (1/8 of the keys each at 8
                                parts of a random text); prefix_bytes = entries x entry bytes */
} sas_stats;

const char* sas_last_error(void);

/* Build an index over text[0..n).  sa_or_null: caller's suffix array with
 * sa_width = 4 (u32, n < 2^32), 5 (packed 40-bit little-endian) or 8 (u64),
 * or NULL to construct it on the GPU (prefix doubling on 32-char packed keys).
 * n < 2^32 - 64 keeps a u32 SA; larger n (up to 2^40, as HBM allows) or
 * SAS_BUILD_SA40 store a packed 40-bit SA, built by the bucketed builder
 * (32-char-key buckets sorted one at a time, then doubling rounds over the
 * tied suffixes only).  The library copies everything into HBM. */
int sas_build(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width,
              uint32_t flags, sas_index** out);
int sas_free(sas_index* index);

/* Sharded-text mode: the index holds only global SA ranks
 * [rank_lo, rank_hi) (the packed text stays whole: compares need any suffix).
 * sa_or_null is the FULL suffix array, or NULL to construct it here.  A
 * search on a shard returns SA[global lower bound] when that rank lies in
 * (rank_lo, rank_hi], i.e. for every query routed to it by sas_route. */
int sas_build_shard(const uint8_t* text, uint64_t n, const void* sa_or_null, int sa_width,
                    uint64_t rank_lo, uint64_t rank_hi, uint32_t flags, sas_index** out);

/* Sharded-text mode without any whole-SA step: part `part` of `parts` builds ONLY
 * its own SA rank range, so the text size is not capped by one GPU's memory for
 * a full SA.  Every part takes the same contiguous range of
 * 7-char-prefix bins from the text's histogram (balanced to bin granularity, so
 * the range is chosen by the library: sas_get_stats -> rank_lo, sa_entries,
 * next_pos), ties on 32-char keys are resolved inside the part by text windows.
 * The SA is stored 40-bit.  ENOTSUP for a text whose repeated prefixes exceed
 * 2^21 chars (use sas_build_shard), EINVAL for an empty part. */
int sas_build_part(const uint8_t* text, uint64_t n, uint32_t part, uint32_t parts, uint32_t flags,
                   sas_index** out);

/* sas_build / sas_build_part over the text random_string(n) draws from
 * ChaCha8Rng::seed_from_u64(seed) (sas/util.rs:9-15, sas/main.rs:38 -- the same
 * chars sas_gen_text writes), generated on the GPU straight into the index's 2-bit
 * packed text: no n-byte copy exists on the host or the device (a sharded rank of
 * configs[4] holds the whole text packed, n/4 bytes, and never its bytes).  Replaces
 * `SaNaive::build(&random_string(n))` of sas/main.rs:53-65. */
int sas_build_gen(uint64_t seed, uint64_t n, uint32_t flags, sas_index** out);
int sas_build_part_gen(uint64_t seed, uint64_t n, uint32_t part, uint32_t parts, uint32_t flags,
                       sas_index** out);

/* Query routing for the sharded mode: out_shard[k] = number of splitter
 * suffixes (text positions splitter_pos[0..nsplit), in increasing suffix
 * order: the first suffix of shards 1..W-1) that are < query k.  Fixed-length
 * queries qbytes[k*m .. (k+1)*m).  Device pointers with SAS_DEVICE_PTRS. */
int sas_route(const sas_index* index, const uint64_t* splitter_pos, uint32_t nsplit,
              const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t* out_shard,
              void* stream, uint32_t flags);

/* sas_route for ragged queries: query k = qbytes[qoff[k] .. qoff[k] + qlen[k]). */
int sas_route_batch(const sas_index* index, const uint64_t* splitter_pos, uint32_t nsplit,
                    const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
                    uint32_t* out_shard, void* stream, uint32_t flags);

/* One sharded step's send side, fused on the GPU (device pointers only,
 * SAS_DEVICE_PTRS): route each fixed-length query (as sas_route), group the
 * queries by destination shard (counting sort) and copy their bytes into
 * out_send, bucket after bucket.  out_counts[w] = queries for shard w
 * (w < nsplit + 1); out_slot[k] = send position of query k, so the positions
 * that come back in send order are gathered with it.  Order inside a bucket is
 * unspecified. */
int sas_route_pack(const sas_index* index, const uint64_t* splitter_pos, uint32_t nsplit,
                   const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t* out_counts,
                   uint8_t* out_send, uint64_t* out_slot, void* stream, uint32_t flags);

/* (SAS_ROUTE_PACKED in flags: out_send holds one u64 packed word per slot.) */
/* sas_route_pack with fixed-capacity buckets: bucket w owns send slots [w*cap, (w+1)*cap)
 * (out_send holds (nsplit + 1) * cap * m bytes), so every rank's all-to-all uses equal splits
 * and needs no host-side counts.  out_counts[w] is the true count; a query past its bucket's
 * cap is not copied and its out_slot is (nsplit + 1) * cap - 1: the caller checks
 * out_counts[w] <= cap on the device and redoes an overflowing step exactly.  Send slots a
 * bucket does not fill keep their old bytes.  EINVAL if cap == 0.  One pass over the
 * queries: out_counts is zeroed and accumulated on the stream. */
int sas_route_pack_cap(const sas_index* index, const uint64_t* splitter_pos, uint32_t nsplit,
                       const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t cap, uint64_t* out_counts,
                       uint8_t* out_send, uint64_t* out_slot, void* stream, uint32_t flags);

/* The sharded step's receive side (device pointers only, SAS_DEVICE_PTRS): out[k] =
 * back[slot[k]], the positions that came back in send-slot order put in query order; with
 * overflow non-null, *overflow is set to 1 (never cleared) when some counts[w] > cap,
 * w < nparts (the out_counts of sas_route_pack_cap), so a caller can defer that check. */
int sas_shard_gather(const sas_index* index, const uint64_t* back, const uint64_t* slot, uint64_t nq,
                     const uint64_t* counts, uint32_t nparts, uint64_t cap, uint64_t* out,
                     uint32_t* overflow, void* stream, uint32_t flags);

/* The sharded step's local lookup over the received slots (device pointers only,
 * SAS_DEVICE_PTRS): slot b*cap + j (b < nbuckets, j < cap) holds a query iff
 * j < counts[b] (the counts each source rank sent, e.g. sas_route_pack_cap's out_counts
 * after a count exchange); only those slots are searched and written, the others are
 * skipped without a read.  queries: m bytes per slot, or with SAS_ROUTE_PACKED one u64
 * 2-bit word per slot (SAS_ALGO_PREFIX, m <= 32).  Algorithms: PLAIN, LCP, LLCP, PREFIX,
 * and QUAD for m <= 32 (ENOTSUP otherwise: search every slot with sas_search_fixed).
 * EINVAL if nbuckets * cap >= 2^32.  Asynchronous on `stream`. */
int sas_search_buckets(const sas_index* index, const void* queries, uint32_t m, uint32_t nbuckets,
                       uint64_t cap, const uint64_t* counts, int algo, uint64_t* out_pos, void* stream,
                       uint32_t flags);

/* The source hash the library was built from (the Makefile's sha256 over csrc/ and
 * include/, 16 hex digits): profiles record it, so counters collected on one build are
 * never attached to another. */
const char* sas_source_hash(void);

int sas_get_stats(const sas_index* index, sas_stats* out);

/* Copy the suffix array / LCP array out (dst host or device per flags).
 * sas_copy_sa needs a u32 SA (sa_width 4, EINVAL otherwise); sas_copy_sa64
 * copies global ranks [start, start+count) of either width as u64.  LCP values
 * are u32 (capped at 2^32-1). */
int sas_copy_sa(const sas_index* index, uint32_t* dst, uint64_t count, uint32_t flags);
int sas_copy_sa64(const sas_index* index, uint64_t start, uint64_t count, uint64_t* dst, uint32_t flags);
int sas_copy_lcp(const sas_index* index, uint32_t* dst, uint64_t count, uint32_t flags);

/* 2-bit packed fixed-length queries, m <= 32: word i holds query i's chars, the first in
 * bits 63..62, zero padded (how the reference packs DNA for its interpolation search,
 * string_value<K>, sas/util.rs:76-117).  A lookup then reads 8 B of query instead of m.
 * sas_pack_queries: device pointers (SAS_DEVICE_PTRS: a kernel on `stream`) or host arrays
 * (packed on the host's worker pool, AVX2 or BMI2 where the CPU has them); EINVAL on codes > 3.
 * sas_search_packed: SAS_ALGO_PREFIX only; host or device pointers per flags. */
int sas_pack_queries(const uint8_t* qbytes, uint32_t m, uint64_t nq, uint64_t* out_words, void* stream,
                     uint32_t flags);
int sas_search_packed(const sas_index* index, const uint64_t* qwords, uint32_t m, uint64_t nq, int algo,
                      uint64_t* out_pos, uint32_t* out_probes, void* stream, uint32_t flags);

/* Substrings of the indexed text as byte codes 0..3: out[out_off[i] .. out_off[i] + len[i])
 * = text[pos[i] .. pos[i] + len[i]) (0 past the text end), from the index's packed copy,
 * so a caller can drop its own byte copy of a large text after sas_build.  Device
 * pointers only (SAS_DEVICE_PTRS), stream-ordered on `stream`. */
int sas_extract(const sas_index* index, const uint64_t* pos, const uint32_t* len, const uint64_t* out_off,
                uint64_t count, uint8_t* out, void* stream, uint32_t flags);

/* GPU check of the SA (SAS_BUILD_VERIFY at build, sas_verify on a built index).  In this order,
 * each EINVAL with its message:
 *   1. every entry is < n                        "suffix array holds an entry >= n"
 *   2. the suffixes of adjacent ranks strictly increase, whole suffixes compared, a proper
 *      prefix before the longer one (the reference's build assertion, sas/sa_search.rs:36-38)
 *                                                "suffix array not sorted: ..."
 *   3. (whole indexes) every position occurs     "suffix array is not a permutation of 0..n"
 * n strictly increasing suffixes with starts < n are pairwise distinct, hence a permutation:
 * once 1 and 2 pass on a whole index, 3 cannot fail, and no caller should wait for its message.
 * SAS_BUILD_VERIFY checks the whole array, a shard's too (sas_build_shard: all n entries of
 * the caller's array, before the rank range is cut out), and a caller's array at the caller's
 * own width: a u64 or packed 40-bit entry >= n fails check 1 even where the index's narrower
 * entry would drop its high bits.  Without the flag nothing about a caller's array is promised:
 * an entry >= n then makes the build read outside the text.
 * sas_verify checks what the index holds: a shard's held ranks only (checks 1 and 2 on
 * [rank_lo, rank_lo + sa_entries), not the pair across either edge), so a fault of the caller's
 * array outside them goes unseen.  ENOTSUP for a bucket-line index (SAS_BUILD_TAG_LINES holds
 * no SA array: verify at build).  Returns 0 if valid. */
int sas_verify(const sas_index* index);

/* Ragged batch: query k = qbytes[qoff[k] .. qoff[k] + qlen[k]).
 * out_pos[k] = SA[lower_bound(q_k)] (or n).  out_probes (optional): for PLAIN, LCP,
 * LLCP and INTERP the number of probes of query k, the reference's `cnt` counter
 * (sas/sa_search.rs:104,178); for the tree algorithms the memory reads of the lookup
 * (tree nodes and leaves; STREE_LLCP / QUAD_LLCP: + the LLCP entries read, QUAD_LLCP: + the
 * text compare of the leaf's candidate), which have no reference counterpart.
 * stream: hipStream_t or NULL.
 * With host pointers the call is synchronous; with SAS_DEVICE_PTRS it is
 * asynchronous on `stream`. */
int sas_search_batch(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff,
                     const uint32_t* qlen, uint64_t nq, int algo, uint64_t* out_pos,
                     uint32_t* out_probes, void* stream, uint32_t flags);

/* Fixed-length batch: query k = qbytes[k*m .. (k+1)*m). */
int sas_search_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                     int algo, uint64_t* out_pos, uint32_t* out_probes, void* stream,
                     uint32_t flags);

/* Occurrence ranges (Search::search_prefix / search_range, sas/util.rs:36-46,
 * declared but unimplemented!() in the reference): global SA ranks
 * [out_lo[k], out_hi[k]) of the suffixes that start with query k; the count
 * is out_hi - out_lo and the positions are SA[out_lo .. out_hi)
 * (sas_copy_sa_range).  Needs SAS_BUILD_TAGGED, SAS_BUILD_QUAD or SAS_BUILD_SECTOR: the
 * tagged index uses its bucket table; otherwise the prefix table when built beside the quad
 * tree (unless SAS_NO_PREFIX_TABLE), else the quad tree, else the sector tree.  On a
 * two/four-suffix inline prefix table a query's lane group tests both bounds on the entry's
 * slots first (one request answers most queries); bounds not found there are bisected in
 * lock step.  No probe counts are reported (the reference has no range search to count
 * against).  Ragged queries as in sas_search_batch. */
int sas_search_range(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff,
                     const uint32_t* qlen, uint64_t nq, uint64_t* out_lo, uint64_t* out_hi,
                     void* stream, uint32_t flags);
/* sas_search_range for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_search_range_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                           uint64_t* out_lo, uint64_t* out_hi, void* stream, uint32_t flags);
/* Copy SA[start .. start+count) (global ranks) out: the text positions of a range. */
int sas_copy_sa_range(const sas_index* index, uint64_t start, uint64_t count, uint32_t* dst,
                      uint32_t flags);

/* Batched locate: every occurrence position of every query, in CSR form.  out_off[0..nq]
 * (u64) are the offsets, out_off[nq] the total; the positions of query k are
 * out_pos[out_off[k] .. out_off[k+1]) in SA rank order (the order of search_prefix), as u64,
 * or as u32 with SAS_LOCATE_U32.  Every SA storage is served: u32, packed 40-bit, tagged
 * entries and SAS_BUILD_TAG_LINES (there each rank costs a binary search over the buckets'
 * first ranks: correct, not tuned).
 *
 * sas_locate_offsets (device pointers only, asynchronous on `stream`):
 *   cnt[k] = ranks in both [lo[k], hi[k]) and [rank_lo, rank_lo + sa_entries) (hi < lo: none), capped at
 *   max_per_query unless that is 0; out_off = exclusive scan of cnt.  A shard or part counts
 *   only the ranks it holds, so the union over shards is the whole answer; the reference's
 *   search_range(Range<&Seq>) is lo = range(a).lo, hi = range(b).lo.
 * sas_locate_fill (device pointers only, asynchronous, no host synchronisation):
 *   out_pos[out_off[k] + j] = SA[max(lo[k], rank_lo) + j] for j < out_off[k+1] - out_off[k]
 *   and out_off[k] + j < capacity; nothing at or past `capacity` is written.  The grid is
 *   sized from `capacity` (the host never reads the total): the caller checks
 *   out_off[nq] <= capacity afterwards, the contract of sas_route_pack_cap.  lo / out_off are
 *   those given to / written by sas_locate_offsets on the same index.
 * sas_locate / sas_locate_fixed: sas_search_range(_fixed) (same index requirements, same
 *   query validation), then offsets, then fill.  With SAS_DEVICE_PTRS: asynchronous, scratch
 *   from the index's stream-ordered pool, out_total (device, may be NULL) = out_off[nq].
 *   With host pointers: synchronous; *out_total is always set and out_off always filled; if
 *   the total exceeds `capacity` nothing is copied to out_pos and the call returns ENOSPC
 *   (out_pos == NULL, capacity == 0 is the sizing call). */
int sas_locate_offsets(const sas_index* index, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                       uint64_t max_per_query, uint64_t* out_off, void* stream, uint32_t flags);
int sas_locate_fill(const sas_index* index, const uint64_t* lo, const uint64_t* out_off, uint64_t nq,
                    void* out_pos, uint64_t capacity, void* stream, uint32_t flags);
int sas_locate(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
               uint64_t nq, uint64_t max_per_query, uint64_t* out_off, void* out_pos, uint64_t capacity,
               uint64_t* out_total, void* stream, uint32_t flags);
int sas_locate_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                     uint64_t max_per_query, uint64_t* out_off, void* out_pos, uint64_t capacity,
                     uint64_t* out_total, void* stream, uint32_t flags);

/* Longest-prefix match: how much of each query occurs in the text, and where.  With lb = the
 * number of suffixes < q (the rank the searches use), a = lcp(q, t[SA[lb-1]..]) (0 if
 * lb == 0) and b = lcp(q, t[SA[lb]..]) (0 if lb == n), lcps capped by both lengths:
 *   out_len[k] = max(a, b), the length of the longest prefix of query k that occurs anywhere
 *                in the text (it is always an lcp with one of those two neighbours);
 *   out_pos[k] = a text position where that prefix occurs: SA[lb] if lb < n and b == len, else
 *                SA[lb-1]; n when len == 0;
 *   [out_lo[k], out_hi[k]) = the SA ranks of every suffix that starts with q[0 .. len), what
 *                sas_search_range returns for that prefix ([0, n) when len == 0).
 * out_pos, out_lo and out_hi may each be NULL.  One lower-bound search per query that keeps
 * the exact lcps of its bounds, started from the prefix table's range when the index has one
 * and the query has at least p chars (SAS_NO_PREFIX_TABLE: always from [0, n), an A/B and
 * test hook); the ranges are one sas_search_range over the same bytes with out_len as the
 * lengths.  Needs a whole index (no shard, no part) with a u32 or packed 40-bit SA array;
 * SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES indexes return ENOTSUP.  out_lo / out_hi also need
 * what sas_search_range needs (its error is returned otherwise).  With SAS_DEVICE_PTRS:
 * asynchronous on `stream`, scratch from the index's stream-ordered pool; SAS_VALIDATE
 * rejects query bytes > 3 (synchronises).  With host pointers: synchronous, bytes always
 * validated.  Ragged queries may overlap in qbytes.
 *
 * sas_match_stats, the matching statistics of a pattern: query i = pattern[i .. min(i +
 * max_len, plen)) for every i in [0, plen); the outputs have plen entries. */
int sas_match(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
              uint64_t nq, uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi,
              void* stream, uint32_t flags);
/* sas_match for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_match_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq,
                    uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi,
                    void* stream, uint32_t flags);
int sas_match_stats(const sas_index* index, const uint8_t* pattern, uint64_t plen, uint32_t max_len,
                    uint32_t* out_len, uint64_t* out_pos, uint64_t* out_lo, uint64_t* out_hi,
                    void* stream, uint32_t flags);

/* k-mismatch locate (Hamming distance): every alignment of every query with at most k
 * substituted chars, by seed and verify.  An alignment of a query q of m chars is a text
 * position s with s + m <= n; its distance is the number of j < m with q[j] != t[s + j] (an
 * alignment never runs past the text end: the padding behind the text matches nothing).
 * The query is cut into k + 1 pieces, piece j = chars [b_j, b_{j+1}) with b_j = floor(j m /
 * (k + 1)); an alignment of distance <= k matches at least one piece exactly, so the
 * occurrences of the pieces (one sas_search_range over all of them) are the candidates, and
 * one kernel verifies them against the packed text, 32 chars per XOR and popcount.
 *   - a piece that occurs more than max_seed_hits times in the text (its whole SA range;
 *     max_seed_hits == 0: no limit) is skipped as a seed and its query flagged
 *     SAS_MM_TRUNCATED;
 *   - a query with m <= k (the empty query at every k) has no k + 1 non-empty pieces: it gets
 *     no result and the flag SAS_MM_SHORT;
 *   - the answer of a query is every alignment of distance <= k at which at least one
 *     non-skipped piece matches exactly: for an unflagged query the complete k-mismatch
 *     answer.  Each alignment is reported once, by the first non-skipped piece that matches
 *     exactly there, and a query's results are ordered by (that piece, the SA rank of its
 *     occurrence).  With k == 0 and max_seed_hits == 0 the positions of a non-empty query are
 *     sas_locate's, in its order.
 * Results in CSR form as sas_locate gives them: out_off[0..nq] (u64), out_pos (u64, or u32
 * with SAS_LOCATE_U32), out_dist (one byte per position: its distance; may be NULL) and
 * out_qflags (one byte per query: SAS_MM_*; may be NULL).  k is 0..15 (EINVAL above).  Flags:
 * SAS_DEVICE_PTRS, SAS_LOCATE_U32, SAS_VALIDATE, SAS_NO_PREFIX_TABLE.  Needs what
 * sas_search_range needs (its error is returned otherwise) on a whole index (no shard, no
 * part) with a u32 or packed 40-bit SA array; SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES indexes
 * return ENOTSUP.
 * With host pointers: synchronous, bytes always validated; *out_total is always set, out_off
 * and out_qflags always filled; if the total exceeds `capacity` nothing is copied to out_pos /
 * out_dist and the call returns ENOSPC (out_pos == NULL, capacity == 0 is the sizing call).
 * With SAS_DEVICE_PTRS: scratch from the index's stream-ordered pool; nothing at or past
 * `capacity` is written; out_total (device, may be NULL) = out_off[nq], which the caller
 * checks against `capacity` afterwards.  The call synchronises on `stream` ONCE, to read
 * the number of candidates (the occurrences of all seeds) back to the host: it sizes the
 * candidate scratch and the grids.  Nothing else synchronises unless SAS_VALIDATE is set. */
#define SAS_MM_TRUNCATED 1u /* out_qflags: a seed was skipped (more than max_seed_hits hits) */
#define SAS_MM_SHORT     2u /* out_qflags: m <= k, no result                                  */
int sas_locate_mismatch(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                        uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off, void* out_pos,
                        uint8_t* out_dist, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total,
                        void* stream, uint32_t flags);
/* sas_locate_mismatch for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_locate_mismatch_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                              uint64_t max_seed_hits, uint64_t* out_off, void* out_pos, uint8_t* out_dist,
                              uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream,
                              uint32_t flags);
/* Timing helper for benches: with SAS_MM_TIMING=1 in the environment every sas_locate_mismatch*
 * call times its verify kernel with HIP events (and synchronises to do so); this returns the
 * calling thread's last figure in ms (< 0: none) and the candidates it verified. */
double sas_locate_mismatch_verify_ms(uint64_t* candidates);

/* k-difference locate (unit-cost edit distance: a substitution, an insertion and a deletion
 * cost 1 each): Sellers' problem, by seed and verify.  For a query q of m chars and the text
 * t of n chars let D(e) = min over 0 <= s <= e of ed(q, t[s .. e)), defined for every end
 * position e in [0, n].  Nothing behind the text end takes part: the zero padding of the
 * packed text is not text.  The k-difference answer of q is every e with D(e) <= k, each
 * reported once with its distance D(e), in ascending order of e.  The neighbouring ends of
 * one alignment are all reported: an exact occurrence ending at e also gives e - j and e + j
 * with distance j for every j <= k, wherever nothing better ends there.  Where an alignment
 * starts and its edit script are not reported.
 * The query is cut as for sas_locate_mismatch, into k + 1 pieces, piece j = chars [b_j,
 * b_{j+1}) with b_j = floor(j m / (k + 1)).  An alignment with at most k edits leaves one piece
 * untouched, which then occurs exactly at some text position pv; with s0 = pv - b_j (signed)
 * the alignment ends in [s0 + m - k, s0 + m + k].  Every occurrence of a piece (one
 * sas_search_range over all pieces) is a candidate, and one kernel runs Myers' bit-vector
 * algorithm, free start, over the window t[max(0, s0 - 2k) .. min(n, s0 + m + k)) of each: every
 * alignment of cost <= k that ends in the candidate's interval starts inside that window, so
 * D(e) capped at k + 1 is the same whichever candidate computes it.  The ends that several
 * candidates propose are sorted and reported once.
 *   - a piece that occurs more than max_seed_hits times in the text (max_seed_hits == 0: no
 *     limit) is skipped as a seed and its query flagged SAS_ED_TRUNCATED; the query's answer
 *     is then exactly {e : D(e) <= k and some occurrence pv of a non-skipped piece j has
 *     |e - (pv - b_j + m)| <= k};
 *   - a query with m <= k (the empty query at every k) gets no result and SAS_ED_SHORT;
 *   - a query with m > SAS_ED_MAX_M gets no result, no seeds and SAS_ED_LONG (a per-query
 *     flag, so that one long query does not fail a ragged batch);
 *   - an unflagged query gets the complete k-difference answer.
 * Results in CSR form: out_off[0..nq] (u64), out_end (u64, or u32 with SAS_LOCATE_U32, which
 * needs n < 2^32: EINVAL otherwise), out_dist (one byte per end: D(e); may be NULL) and
 * out_qflags (one byte per query: SAS_ED_*; may be NULL).  k is 0..15 (EINVAL above).  Flags:
 * SAS_DEVICE_PTRS, SAS_LOCATE_U32, SAS_VALIDATE, SAS_NO_PREFIX_TABLE.  Needs what
 * sas_search_range needs (its error is returned otherwise) on a whole index (no shard, no
 * part) with a u32 or packed 40-bit SA array; SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES indexes
 * return ENOTSUP.  The proposals are sorted by a 64-bit key (query, end): if the bits of nq - 1
 * and of n together exceed 64 the call returns EINVAL and asks to split the batch.
 * With host pointers: synchronous, bytes always validated; *out_total is always set, out_off
 * and out_qflags always filled; if the total exceeds `capacity` nothing is copied to out_end /
 * out_dist and the call returns ENOSPC (out_end == NULL, capacity == 0 is the sizing call).
 * With SAS_DEVICE_PTRS: scratch from the index's stream-ordered pool; nothing at or past
 * `capacity` is written; out_total (device, may be NULL) = out_off[nq], which the caller
 * checks against `capacity` afterwards.  The call synchronises on `stream` TWICE: to read the
 * number of candidates (the occurrences of all seeds; it sizes the candidate scratch and the
 * grids) and the number of proposed ends (it sizes the sort).  Nothing else synchronises
 * unless SAS_VALIDATE is set. */
#define SAS_ED_TRUNCATED 1u /* out_qflags: a seed was skipped (more than max_seed_hits hits) */
#define SAS_ED_SHORT     2u /* out_qflags: m <= k, no result                                  */
#define SAS_ED_LONG      4u /* out_qflags: m > SAS_ED_MAX_M, no result                        */
#define SAS_ED_MAX_M     256u
int sas_locate_edit(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                    uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint64_t* out_off, void* out_end,
                    uint8_t* out_dist, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total,
                    void* stream, uint32_t flags);
/* sas_locate_edit for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_locate_edit_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                          uint64_t max_seed_hits, uint64_t* out_off, void* out_end, uint8_t* out_dist,
                          uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream,
                          uint32_t flags);
/* Timing helpers for benches: with SAS_ED_TIMING=1 in the environment every sas_locate_edit*
 * call times its verify kernel, and the de-duplication from the first proposal written to the
 * offsets, with HIP events (and synchronises to do so); these return the calling thread's last
 * figures in ms (< 0: none), with the candidates verified and the ends proposed. */
double sas_locate_edit_verify_ms(uint64_t* candidates);
double sas_locate_edit_dedup_ms(uint64_t* proposals);
/* Maximal exact matches (MEMs) of every query, by seed and extend: the first step for a query
 * that shares only stretches with the text (a long read, a contig, another assembly; MUMmer's
 * -maxmatch).  For a query p of m chars, the text t of n chars and min_len = L >= 1, a match is a
 * triple (i, j, len) with len >= L, i + len <= m, j + len <= n and p[i .. i + len) = t[j .. j +
 * len).  It is maximal when both hold:
 *   - left:  i = 0, or j = 0, or p[i - 1] != t[j - 1];
 *   - right: i + len = m, or j + len = n, or p[i + len] != t[j + len].
 * Nothing behind the text end takes part: the zero padding of the packed text is code 0 = 'A' and
 * never extends a match.  Equivalently, the MEMs are the maximal runs of `true` of length >= L on
 * the diagonals of the m x n matrix [p[i] = t[j]].
 * Every MEM starts with an occurrence of the window p[i .. i + L), so the windows of all query
 * offsets i <= m - L go through one sas_search_range, and one kernel takes every occurrence of
 * every window: it drops those that extend to the left (one text char, one query byte) and
 * extends the others to the right, 32 chars a step.  There is no bound on m other than u32.
 *   - max_hits: if it is not 0, a query offset i whose window occurs more than max_hits times in
 *     the text (its whole SA range) is skipped and the query flagged SAS_MEM_TRUNCATED; its
 *     answer is exactly the MEMs (i, j, len) whose offset i was not skipped.  0: no limit;
 *   - a query with m < L (the empty one included) gets no result and SAS_MEM_SHORT;
 *   - SAS_MEM_UNIQUE (a call flag): only MEMs whose string t[j .. j + len) occurs exactly once in
 *     the indexed text are reported (MUMmer's -mumreference).  It is decided from the SA
 *     neighbours of the occurrence's rank r, text against text: unique iff lcp(t[SA[r - 1] ..],
 *     t[j ..]) < len and lcp(t[SA[r + 1] ..], t[j ..]) < len, the lcps capped at the text end, a
 *     neighbour that does not exist counting as smaller.  No LCP array is needed;
 *   - with a sequence layout set (sas_set_layout) each segment is a text of its own, as for the
 *     approximate calls: an occurrence [j, j + L) that does not lie inside one segment is no
 *     candidate, and in both maximality rules the segment's lo and hi take the place of 0 and n.
 *     max_hits and SAS_MEM_UNIQUE keep counting occurrences in the whole indexed text.  Without a
 *     layout the call runs a kernel without these tests; a layout of one segment [0, n) gives
 *     the same bytes;
 *   - the reverse-complement strand is not searched: pass sas_revcomp's output as a second batch.
 * Results in CSR form, as sas_locate_mismatch gives them: out_off[0..nq] (u64) and per match
 * out_qpos (u32: i), out_tpos (u64, or u32 with SAS_LOCATE_U32, which needs n < 2^32: EINVAL
 * otherwise: j) and out_len (u32); out_qflags is one byte per query (SAS_MEM_*; may be NULL).
 * Inside a query the matches are ordered by ascending i, then by ascending SA rank of the suffix
 * t[j ..].  min_len == 0 is EINVAL (checked before the index).  Flags: SAS_DEVICE_PTRS,
 * SAS_LOCATE_U32, SAS_VALIDATE, SAS_NO_PREFIX_TABLE, SAS_MEM_UNIQUE.  Needs what sas_search_range
 * needs (its error is returned otherwise) on a whole index (no shard, no part) with a u32 or
 * packed 40-bit SA array; SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES indexes return ENOTSUP.
 * With host pointers: synchronous, bytes always validated (those of short queries too);
 * *out_total is always set, out_off and out_qflags always filled; if the total exceeds
 * `capacity` nothing is copied to out_qpos / out_tpos / out_len and the call returns ENOSPC
 * (all three NULL, capacity == 0 is the sizing call).  With SAS_DEVICE_PTRS: scratch from the
 * index's stream-ordered pool (36 B per window and 24 B per candidate; a ragged batch 8 B per
 * window more); nothing at or past `capacity` is written; out_total (device, may be NULL) =
 * out_off[nq], which the caller checks against `capacity` afterwards.  nq == 0 writes
 * out_off[0] = 0.  sas_mems_fixed synchronises on `stream` ONCE, to read the number of
 * candidates (the occurrences of all windows that were not skipped) back to the host: it sizes
 * the candidate scratch and the grid.  sas_mems synchronises once more before that, to read the
 * number of windows of its ragged batch.  Nothing else synchronises unless SAS_VALIDATE is set. */
#define SAS_MEM_TRUNCATED 1u /* out_qflags: a query offset was skipped (more than max_hits hits) */
#define SAS_MEM_SHORT     2u /* out_qflags: m < min_len, no result                                */
#define SAS_MEM_UNIQUE    (1u << 1) /* sas_mems*: only matches whose string occurs once in the text */
int sas_mems(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
             uint32_t min_len, uint64_t max_hits, uint64_t* out_off, uint32_t* out_qpos, void* out_tpos,
             uint32_t* out_len, uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream,
             uint32_t flags);
/* sas_mems for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_mems_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t min_len,
                   uint64_t max_hits, uint64_t* out_off, uint32_t* out_qpos, void* out_tpos, uint32_t* out_len,
                   uint8_t* out_qflags, uint64_t capacity, uint64_t* out_total, void* stream, uint32_t flags);
/* Timing helper for benches: with SAS_MEM_TIMING=1 in the environment every sas_mems* call times
 * its verify kernel with HIP events (and synchronises to do so); this returns the calling
 * thread's last figure in ms (< 0: none) and the candidates it verified. */
double sas_mems_verify_ms(uint64_t* candidates);
/* Debug helper for tests: SAS_TILE_GRID=g in the environment (read at every call) caps at g
 * workgroups the grids of the tiled kernels of sas_locate*, sas_locate_mismatch*,
 * sas_locate_edit*, sas_mems*, sas_align_edit*, sas_map_edit*, sas_map_pairs*, sas_map_pairs_rescue* and
 * sas_revcomp*, so a small batch takes the tile loops of a large one; results do not depend on
 * it.  It only lowers a grid.  This returns the cap in force, 0 for none (unset, empty or not positive). */
uint32_t sas_tile_grid_cap(void);

/* Where an approximate match starts and its edit script, for ends that sas_locate_edit*
 * reported (or any other ends).  For a query q of m chars, an end e in [0, n] and a bound k in
 * 0..15 (EINVAL above):
 *   - w0 = max(0, e - m - k);
 *   - for 0 <= i <= m and w0 <= j <= e, R[i][j] = ed(q[i .. m), t[j .. e)), the unit-cost edit
 *     distance of the query suffix and the text slice;
 *   - d = min over j of R[0][j].  Whenever D(e) <= k this is D(e) itself: an alignment of cost
 *     <= k that ends at e cannot start before e - m - k.
 * Reported per alignment:
 *   - start: s = the largest j with R[0][j] = d, the shortest text substring that reaches the
 *     distance;
 *   - script: walk forward from (i, j) = (0, s) until (m, e); at each cell the first rule that
 *     applies:
 *       1. i < m, j < e and R[i+1][j+1] + (q[i] != t[j]) == R[i][j]: emit SAS_AL_EQ if the chars
 *          are equal, else SAS_AL_X; both advance;
 *       2. j < e and R[i][j+1] + 1 == R[i][j]: emit SAS_AL_DEL (a text char that the query
 *          lacks); j advances;
 *       3. otherwise emit SAS_AL_INS (a query char that the text lacks); i advances.
 *     The script is run-length encoded as runs of equal ops, each (len << 2) | op in a uint16_t;
 *     it has at most 2k + 1 runs, because at most k ops are not SAS_AL_EQ;
 *   - no alignment: start = n, dist = SAS_AL_NONE_DIST, nruns = 0 and all run slots 0, when
 *     m == 0, m > SAS_ED_MAX_M, e > n or d > k.
 * The rule is deterministic and independent of how it is computed.  Nothing outside t[w0 .. e)
 * takes part: neither a char before w0 nor the zero padding behind the text.
 * off[0..nq] (u64) and end[] (u64, or u32 with SAS_LOCATE_U32) are what sas_locate_edit* wrote:
 * alignment a belongs to the query i with off[i] <= a < off[i+1].  out_start (u64, or u32 with
 * SAS_LOCATE_U32, which needs n < 2^32: EINVAL otherwise), out_dist, out_nruns (one byte each)
 * and out_runs[a * (2k + 1) + r] are written for every a < min(na, off[nq]); run slots that are
 * not used are written as 0; nothing at or past that bound is touched.  out_dist, out_nruns and
 * out_runs may each be NULL.  EINVAL for a null index and, when na > 0, for a null off, end or
 * out_start.  Flags: SAS_DEVICE_PTRS, SAS_LOCATE_U32, SAS_VALIDATE.
 * The call reads only the packed text, never the SA: every index is served, shards and parts
 * (their text is whole) and SAS_BUILD_TAGGED / SAS_BUILD_TAG_LINES indexes (they keep the text)
 * included.
 * With SAS_DEVICE_PTRS the call is asynchronous on `stream` and synchronises nowhere (the grid
 * and the scratch, from the index's stream-ordered pool, are sized from na), so it chains behind
 * sas_locate_edit on the same stream; SAS_VALIDATE rejects query bytes > 3 and synchronises to
 * do so.  With host pointers: synchronous, bytes always validated. */
#define SAS_AL_EQ  0u /* run ops: (len << 2) | op in a uint16_t; len <= m + k < 2^14 */
#define SAS_AL_X   1u
#define SAS_AL_INS 2u /* query char absent from the text */
#define SAS_AL_DEL 3u /* text char absent from the query */
#define SAS_AL_NONE_DIST 255u
int sas_align_edit(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                   uint64_t nq, uint32_t k, const uint64_t* off, const void* end, uint64_t na,
                   void* out_start, uint8_t* out_dist, uint8_t* out_nruns, uint16_t* out_runs,
                   void* stream, uint32_t flags);
/* sas_align_edit for fixed-length queries qbytes[k*m .. (k+1)*m). */
int sas_align_edit_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                         const uint64_t* off, const void* end, uint64_t na, void* out_start,
                         uint8_t* out_dist, uint8_t* out_nruns, uint16_t* out_runs, void* stream,
                         uint32_t flags);

/* Reverse complement of DNA queries: rc(q)[j] = q[m - 1 - j] ^ 3 for a query of m chars (the codes
 * are A C G T = 0 1 2 3, so the complement of c is c ^ 3).  sas_revcomp writes the reverse
 * complements of the ragged queries back to back in query order, and out_off[0 .. nq] (u64) = the
 * exclusive sum of qlen: ragged inputs may overlap in qbytes, so their offsets cannot be reused.
 * sas_revcomp_fixed writes query i at out_bytes[i m].  The calls take no index; with
 * SAS_DEVICE_PTRS they run on the current device, asynchronous on `stream`.  Anyone who wants every
 * hit of sas_locate_edit / sas_locate_mismatch on both strands needs them.  Flags: SAS_DEVICE_PTRS
 * and SAS_VALIDATE (rejects bytes > 3, synchronises); host pointers: synchronous, bytes always
 * validated.  nq == 0 writes out_off[0] = 0 and nothing else. */
int sas_revcomp(const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen, uint64_t nq,
                uint8_t* out_bytes, uint64_t* out_off, void* stream, uint32_t flags);
int sas_revcomp_fixed(const uint8_t* qbytes, uint32_t m, uint64_t nq, uint8_t* out_bytes, void* stream,
                      uint32_t flags);

/* Read mapping: the best alignment of every read on both strands, one fixed-size record per read.
 * For read i with the query q of m chars, a bound k in 0..15 (EINVAL above) and max_seed_hits:
 *   - q_0 = q and q_1 = rc(q);
 *   - A_s is the answer that sas_locate_edit defines for q_s with the same k and max_seed_hits: a
 *     list of (e, D) ascending in e, empty for a SAS_ED_SHORT or SAS_ED_LONG query, reduced in
 *     the way documented there when a seed is skipped;
 *   - `strands` is a bit mask, SAS_MAP_FWD, SAS_MAP_REV or both (EINVAL otherwise): only the
 *     selected strands take part, and everything below is a pure function of their A_s.
 * Reported per read:
 *   - best: the least triple (D, s, e) over all ends of all participating strands, in
 *     lexicographic order: the least distance, then forward before reverse, then the smallest
 *     end.  It gives out_dist, out_strand and out_end.  The end is a text coordinate on either
 *     strand: the reverse-strand alignment is that of rc(q) against t[start .. end), as SAM
 *     reports it;
 *   - n_best: the number of maximal intervals e, e + 1, e + 2, ... of consecutive ends, all in A_s
 *     of one strand and all at the distance out_dist, summed over the strands.  Two occurrences
 *     two chars apart count as two; one occurrence never counts twice.  A read that equals its
 *     own reverse complement counts each place once per strand;
 *   - n_loci: the number of maximal intervals of consecutive reported ends, of any distance <= k,
 *     summed over the strands.  As |D(e + 1) - D(e)| <= 1 these are the valleys of D below k + 1.
 *     n_best == 1 && n_loci == 1 is the unique mapping.  Both counts are accumulated in 64 bits
 *     and written clamped at UINT32_MAX;
 *   - out_start, out_nruns, out_runs (2k + 1 slots per read): exactly what sas_align_edit defines
 *     for (q_strand, end, k): the largest start that reaches the distance, its tie rule, its runs;
 *   - out_qflags: the OR of the SAS_ED_* flags of the participating strands;
 *   - no end on any participating strand: end = start = n, dist = SAS_AL_NONE_DIST, strand = 0,
 *     n_best = n_loci = 0, nruns = 0, every run slot 0.
 * Every output has one entry per read (out_end / out_start u64, or u32 with SAS_LOCATE_U32, which
 * needs n < 2^32: EINVAL otherwise): there is no capacity, no sizing call and no ENOSPC.  out_start,
 * out_strand, out_nbest, out_nloci, out_nruns, out_runs and out_qflags may each be NULL; out_end
 * and out_dist are required when nq > 0.  nq == 0 writes nothing.  Flags: SAS_DEVICE_PTRS,
 * SAS_LOCATE_U32, SAS_VALIDATE, SAS_NO_PREFIX_TABLE.  The index requirements and their errors are
 * those of sas_locate_edit (ENOTSUP for shards, parts and tagged indexes); the reads of both
 * strands are one batch of the seed-and-verify path, so EINVAL when the bits of 2 nq - 1 and of n
 * together exceed the 64-bit sort key.  Only each read's winner is aligned, one alignment per read.
 * With SAS_DEVICE_PTRS: scratch from the index's stream-ordered pool; the call synchronises on
 * `stream` where sas_locate_edit does, twice (the candidates and the proposed ends of the whole
 * batch), and, for ragged queries with the reverse strand selected, once more before them, to
 * size the batch's bytes from the sum of qlen (sas_map_edit_fixed and SAS_MAP_FWD alone: never).
 * Nothing else synchronises unless SAS_VALIDATE is set.  With host pointers: synchronous, bytes
 * always validated. */
#define SAS_MAP_FWD 1u /* strands: the read as given             */
#define SAS_MAP_REV 2u /* strands: the read's reverse complement */
int sas_map_edit(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                 uint64_t nq, uint32_t k, uint64_t max_seed_hits, uint32_t strands, void* out_end,
                 void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                 uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                 void* stream, uint32_t flags);
/* sas_map_edit for fixed-length reads qbytes[k*m .. (k+1)*m). */
int sas_map_edit_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t nq, uint32_t k,
                       uint64_t max_seed_hits, uint32_t strands, void* out_end, void* out_start,
                       uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci,
                       uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags, void* stream,
                       uint32_t flags);

/* Paired-end mapping: the reads of a pair placed together, by a join of their ends on the fragment
 * length.  One batch of 2 np reads, interleaved as in an interleaved FASTQ: pair i is read 2i
 * (mate 1) and read 2i + 1 (mate 2); the query arguments are those of sas_map_edit / _fixed with
 * nq = 2 np.  k is 0..15 (EINVAL above), max_seed_hits as there, min_frag <= max_frag.
 *   - answers: for read r, A_0(r) and A_1(r) are exactly sas_map_edit's: the sas_locate_edit answer
 *     of the read and of its reverse complement for the same k and max_seed_hits, empty for a
 *     SAS_ED_SHORT or SAS_ED_LONG read, reduced as documented there when a seed is skipped;
 *   - loci: a locus of (r, s) is a maximal interval e, e + 1, e + 2, ... of consecutive ends in
 *     A_s(r), the intervals n_loci counts.  Its representative is the least (D, e) in it, in
 *     lexicographic order;
 *   - candidates: the orientation is forward / reverse (the Illumina paired-end library) and is
 *     fixed.  For orientation o in {0, 1} the forward mate is f = 2i + o and the reverse mate is
 *     v = 2i + 1 - o; a candidate is (x, y), x a locus of (f, 0) and y a locus of (v, 1), with the
 *     representatives (D_x, e_x) and (D_y, e_y);
 *   - fragment length: F = e_y - e_x + m_f in signed 64-bit arithmetic, m_f the forward mate's
 *     length: the template length with the forward mate's start taken as e_x - m_f.  The true one,
 *     end_v - start_f of the outputs, differs from it by at most k; using ends alone keeps the join
 *     a pure function of the A_s.  The candidate is proper iff min_frag <= F <= max_frag.
 * Reported per pair (np entries each):
 *   - out_npairs: the number of proper candidates over both orientations;
 *   - out_nbestpairs: the number of those with the least sum D_x + D_y;
 *   - out_pflags: bit SAS_PAIR_PROPER is set iff n_pairs > 0.
 *     Both counts are accumulated in 64 bits and written clamped at UINT32_MAX;
 *   - the best pair is the least (D_x + D_y, o, e_x, e_y), in lexicographic order.
 * Reported per read (2 np entries each, in the layout of sas_map_edit's outputs):
 *   - in a proper pair read f gets end = e_x, dist = D_x, strand = 0 and read v gets end = e_y,
 *     dist = D_y, strand = 1; out_start, out_nruns and the 2k + 1 run slots are sas_align_edit's
 *     for (q_strand, end, k);
 *   - in a pair that is not proper both reads get exactly the record sas_map_edit gives them with
 *     strands = SAS_MAP_FWD | SAS_MAP_REV (an unmapped read the unmapped record defined there);
 *   - out_nbest, out_nloci and out_qflags are always sas_map_edit's single-read values, proper or
 *     not.
 * max_frag - min_frag above SAS_PAIR_MAX_SPREAD, or min_frag > max_frag, is EINVAL, checked before
 * the index: a forward locus's partners lie in a window of spread + 1 end positions, loci are at
 * least 2 apart, so the window holds at most spread / 2 + 1 of them, which bounds one work item's
 * scan (and lets the join's key hold e_y relative to the window in 16 bits).  The index
 * requirements and their errors are sas_map_edit's (ENOTSUP for shards, parts and tagged
 * indexes); the two mates on two strands are one batch of the seed-and-verify path, so EINVAL
 * when the bits of 4 np - 1 and of n together exceed the 64-bit sort key.  np == 0 writes
 * nothing.  out_end and out_dist are required, every other output may be NULL.  Flags:
 * SAS_DEVICE_PTRS, SAS_LOCATE_U32, SAS_VALIDATE, SAS_NO_PREFIX_TABLE.  Other orientations (FF,
 * RF), the rescue of a mate that has no end within k (sas_map_pairs_rescue below), a mapping quality
 * and SAM text are not part of the call.
 * With SAS_DEVICE_PTRS the call synchronises on `stream` where sas_map_edit on the same reads
 * does, and nowhere else: the loci scratch and the join's grids are sized from the number of
 * proposed ends, which the host holds already, and the number of loci stays on the device.  With
 * host pointers: synchronous, bytes always validated. */
#define SAS_PAIR_PROPER 1u /* out_pflags: some candidate has its fragment length in the window */
#define SAS_PAIR_MAX_SPREAD 65535u
int sas_map_pairs(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                  uint64_t npairs, uint32_t k, uint64_t max_seed_hits, uint32_t min_frag, uint32_t max_frag,
                  void* out_end, void* out_start, uint8_t* out_dist, uint8_t* out_strand,
                  uint32_t* out_nbest, uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs,
                  uint8_t* out_qflags, uint8_t* out_pflags, uint32_t* out_npairs, uint32_t* out_nbestpairs,
                  void* stream, uint32_t flags);
/* sas_map_pairs for fixed-length reads qbytes[k*m .. (k+1)*m). */
int sas_map_pairs_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t npairs, uint32_t k,
                        uint64_t max_seed_hits, uint32_t min_frag, uint32_t max_frag, void* out_end,
                        void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                        uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                        uint8_t* out_pflags, uint32_t* out_npairs, uint32_t* out_nbestpairs, void* stream,
                        uint32_t flags);

/* Paired-end mapping with mate rescue: sas_map_pairs, and for a pair that it leaves without a
 * proper candidate a direct scan, with no seeds, of the window in which the fragment length puts
 * the other mate.  A mate loses its loci when its seeds are skipped by max_seed_hits (it lies in a
 * repeat) or when it carries more than k edits; its partner usually maps, and says where to look.
 * The arguments are sas_map_pairs' with k_rescue behind k, max_anchors behind max_frag and
 * out_nrescue (per pair, may be NULL) behind out_nbestpairs.  Everything below is a pure function
 * of D of sas_locate_edit's text (the full-text Sellers D(e) of a query) and of sas_map_pairs'
 * own definitions for the same k, max_seed_hits, min_frag and max_frag.
 *   - bounds: k <= k_rescue <= 15 (EINVAL otherwise, checked with the window, before the index);
 *     every other argument check, index requirement and error is sas_map_pairs';
 *   - alignments: out_start, out_nruns and out_runs of every read are sas_align_edit's for
 *     (q_strand, end, k_rescue), with a run stride of 2 k_rescue + 1.  For an end with D(e) <= k
 *     that is the start and the script it gives with k: the larger bound only adds smaller
 *     starts to the window w0 .. e, the reported start is the largest that reaches the distance,
 *     and R does not depend on the window;
 *   - eligible: pair i is eligible iff its n_pairs under sas_map_pairs is 0, max_anchors > 0 and
 *     1 <= A(i) <= max_anchors, A(i) the number of loci of reads 2i and 2i + 1 over both strands
 *     (the unclamped 64-bit sum of their two n_loci).  A pair with n_pairs = 0, max_anchors > 0
 *     and A(i) > max_anchors gets SAS_PAIR_RESCUE_SKIPPED.  max_anchors = 0 switches rescue off:
 *     with k_rescue = k the outputs are then byte for byte sas_map_pairs', and out_nrescue is 0;
 *   - anchors: every locus of an eligible pair is an anchor: a locus of (a, s) with the
 *     representative (D_a, e_a); b is the other read of the pair, m_b its length.  An anchor is
 *     skipped when m_b <= k_rescue or m_b > SAS_ED_MAX_M.  The partner is searched on strand 1 - s,
 *     with q_b when s = 1 and with rc(q_b) when s = 0, by the D of that query: no seeds, no
 *     max_seed_hits.
 *       s = 0 (the anchor is the forward mate, f = a and v = b): the window is W = [e_a - m_a +
 *         min_frag, e_a - m_a + max_frag] cut to [0, n]; the candidates are the e_y in W with
 *         D(e_y) <= k_rescue; e_x = e_a and D_x = D_a;
 *       s = 1 (the anchor is the reverse mate, v = a and f = b): W = [e_a + m_b - max_frag,
 *         e_a + m_b - min_frag] cut to [0, n]; the candidates are the e_x in W with D(e_x) <=
 *         k_rescue; e_y = e_a and D_y = D_a.
 *     In both cases F = e_y - e_x + m_f lies in [min_frag, max_frag] and o = f - 2i, as in
 *     sas_map_pairs;
 *   - the best candidate is the least (D_x + D_y, o, e_x, e_y) over all anchors.  A candidate of a
 *     forward anchor and one of a reverse anchor never coincide in (o, e_x, e_y): both ends would
 *     be locus representatives with F in the window, and the pair would be proper.  So the 64-bit
 *     key of the join orders the candidates of both sides as it is;
 *   - out_nrescue[i]: the sum over the pair's anchors of the number of maximal intervals of
 *     consecutive candidate ends inside that anchor's window, accumulated in 64 bits and clamped
 *     at UINT32_MAX; 0 for every pair that is not eligible;
 *   - a pair with at least one candidate is rescued: SAS_PAIR_RESCUED in out_pflags; the anchor
 *     read gets end = e_a, dist = D_a, strand = s; the other read gets the candidate's end, its D
 *     (which may exceed k), strand 1 - s and SAS_MAP_RESCUED in out_qflags; both are re-aligned
 *     as stated above;
 *   - SAS_PAIR_PROPER, out_npairs, out_nbestpairs, out_nbest, out_nloci, the other out_qflags
 *     bits and every record of a pair that is proper or not rescued stay what sas_map_pairs
 *     defines.
 * One work item of the scan takes SAS_RESCUE_CHUNK consecutive ends of one anchor's window (and
 * the m_b + k_rescue + 1 columns before them), so a window of spread + 1 ends is ceil((spread + 1)
 * / SAS_RESCUE_CHUNK) items.  With SAS_DEVICE_PTRS the call synchronises exactly where
 * sas_map_pairs does: the anchor count stays on the device, the scratch is sized from the number
 * of proposed ends and the scan's grid is capped and strides over the count.  With host pointers:
 * synchronous, bytes always validated. */
#define SAS_PAIR_RESCUED        2u /* out_pflags: placed by a window scan from an anchor            */
#define SAS_PAIR_RESCUE_SKIPPED 4u /* out_pflags: no proper candidate, more than max_anchors loci  */
#define SAS_MAP_RESCUED         8u /* out_qflags: this read's end comes from the window scan        */
#define SAS_RESCUE_CHUNK 128u      /* window ends per work item of the scan                         */
int sas_map_pairs_rescue(const sas_index* index, const uint8_t* qbytes, const uint64_t* qoff, const uint32_t* qlen,
                         uint64_t npairs, uint32_t k, uint32_t k_rescue, uint64_t max_seed_hits,
                         uint32_t min_frag, uint32_t max_frag, uint64_t max_anchors, void* out_end,
                         void* out_start, uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest,
                         uint32_t* out_nloci, uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags,
                         uint8_t* out_pflags, uint32_t* out_npairs, uint32_t* out_nbestpairs,
                         uint32_t* out_nrescue, void* stream, uint32_t flags);
/* sas_map_pairs_rescue for fixed-length reads qbytes[k*m .. (k+1)*m). */
int sas_map_pairs_rescue_fixed(const sas_index* index, const uint8_t* qbytes, uint32_t m, uint64_t npairs,
                               uint32_t k, uint32_t k_rescue, uint64_t max_seed_hits, uint32_t min_frag,
                               uint32_t max_frag, uint64_t max_anchors, void* out_end, void* out_start,
                               uint8_t* out_dist, uint8_t* out_strand, uint32_t* out_nbest, uint32_t* out_nloci,
                               uint8_t* out_nruns, uint16_t* out_runs, uint8_t* out_qflags, uint8_t* out_pflags,
                               uint32_t* out_npairs, uint32_t* out_nbestpairs, uint32_t* out_nrescue,
                               void* stream, uint32_t flags);

/* Timing helper for benches: run `reps` back-to-back fixed-length searches on
 * device buffers and report the average duration of the search kernel itself
 * (HIP events on `stream`) in *kernel_ns and of the whole call in *call_ns. */
int sas_time_fixed(const sas_index* index, const uint8_t* d_qbytes, uint32_t m, uint64_t nq,
                   int algo, uint64_t* d_out_pos, int reps, void* stream, uint32_t flags,
                   double* kernel_ns, double* call_ns);

/* Generators (bit-exact restatements of the reference's seeded inputs). */
int sas_gen_text(uint64_t seed, uint64_t n, uint8_t* out, uint32_t flags);
/* Offsets i = gen_range(0..n - margin) and lengths gen_range(len_lo..len_hi)
 * (fixed when len_hi == len_lo + 1), continuing the ChaCha8 stream at
 * keystream word `word_pos` (= n after sas_gen_text).  Host arrays only.
 * Returns the next free keystream word through *next_word (may be NULL). */
int sas_gen_queries(uint64_t seed, uint64_t word_pos, uint64_t n, uint64_t nq, uint64_t margin,
                    uint32_t len_lo, uint32_t len_hi, uint64_t* off, uint32_t* len,
                    uint64_t* next_word);

/* One process, several GPUs (SURVEY §8b sas_build_multi).  mode
 * SAS_MULTI_REPLICATE: every device builds the whole index (sas_build) and a
 * batch is cut into contiguous query chunks, one per device, run concurrently.
 * SAS_MULTI_SHARD: device g builds only part g of the SA rank space
 * (sas_build_part, balanced to 7-char-prefix bins); queries are routed on the
 * first device against the parts' first suffixes (sas_route_batch) and each part
 * answers its own.  Results are identical to one sas_build index.  `devices`
 * lists ngpu device ordinals (repeats allowed: several parts on one GPU).  Host
 * pointers only; the text stays with the caller.  The one-process-per-GPU path
 * over RCCL is bench.py --mode shard / sas_amd.shard. */
typedef struct sas_multi sas_multi;
#define SAS_MULTI_REPLICATE 0
#define SAS_MULTI_SHARD     1
int sas_build_multi(const uint8_t* text, uint64_t n, const int* devices, int ngpu, int mode,
                    uint32_t flags, sas_multi** out);
int sas_multi_free(sas_multi* multi);
int sas_multi_parts(const sas_multi* multi);
int sas_multi_get_stats(const sas_multi* multi, int part, sas_stats* out);
/* Ragged batch as sas_search_batch (synchronous, host pointers). */
int sas_search_multi(const sas_multi* multi, const uint8_t* qbytes, const uint64_t* qoff,
                     const uint32_t* qlen, uint64_t nq, int algo, uint64_t* out_pos, uint32_t flags);

/* Real-data inputs.
 * sas_read_fasta: read_fasta_file (sas/util.rs:144-169) -- records concatenated,
 * A/C/G/T/a/c/g/t -> 0..3; FASTA and FASTQ, no gzip.  The text alone does not say where a
 * record starts nor which chars were no base (they are stored as code 0):
 * sas_read_fasta_layout below reads the same bytes together with the sequence layout that
 * keeps approximate matches inside one record and out of the gaps.
 * out == NULL -> only *len is computed (size the buffer, then call again). */
int sas_read_fasta(const char* path, uint8_t* out, uint64_t cap, uint64_t* len);

/* The sequence layout: a side table on a built index that says where the sequences of the text
 * start and which stretches of it are real bases.  It is set after the build and changes neither
 * the text, the SA nor any exact lookup.
 *   - sequences: seq_start[0 .. nseq] is non-decreasing with seq_start[0] = 0 and seq_start[nseq]
 *     = n; sequence i is the text [seq_start[i], seq_start[i + 1]) and may be empty (FASTA has
 *     empty records, and the ids stay aligned with the names).  The sequence of an end position
 *     e >= 1 is the largest i with seq_start[i] < e.  nseq < 2^32 - 1;
 *   - segments, the stretches of real bases: seg_lo[i] < seg_hi[i] <= seg_lo[i + 1], seg_hi[i] <= n,
 *     and no seq_start value lies strictly inside (seg_lo[i], seg_hi[i]): a segment lies inside
 *     one sequence.  nseg may be 0 (everything is masked).  A position in no segment is a gap.
 *     The segment of an end e is the one with lo < e <= hi.
 * sas_check_layout (host only, no device call) returns EINVAL on anything else, with a
 * sas_last_error message that names the offending entry.  sas_set_layout (host pointers) calls it
 * first, copies the three arrays to the device and synchronises the device before it swaps them
 * in; nseq == 0 clears the layout.  THE CALLER MUST HAVE NO CALL IN FLIGHT ON THE INDEX when it
 * sets or clears the layout: a set index is no longer immutable at that moment.  Any index may
 * carry a layout, shards, parts and tagged indexes included (sas_align_edit and sas_translate
 * serve them).  sas_get_layout is the query (sas_stats keeps its size): the counts, and with
 * non-null arrays (nseq + 1, nseg and nseg entries) the values; nseq = 0: no layout.
 *
 * With a layout set, each segment is a text of its own for the approximate calls; with none they
 * run exactly as before, and a layout of one sequence and one segment [0, n) gives the same bytes:
 *   - sas_locate_mismatch*: an alignment [s, s + m) is reported only if it lies inside one segment;
 *   - sas_locate_edit*: D_L(e) = min over s of ed(q, t[s .. e)) with [s, e) inside one segment,
 *     undefined (nothing is reported) for an e in no segment; the unflagged answer is {e : D_L(e)
 *     <= k}, the union over the segments of the no-layout answer on t[lo .. hi) as a text of its
 *     own, shifted by lo.  The seed gate is unchanged (max_seed_hits counts the SA occurrences in
 *     the whole text); a seed occurrence that is not inside one segment is no candidate; for a
 *     SAS_ED_TRUNCATED query "some occurrence pv of a non-skipped piece" is restricted to the
 *     occurrences in the segment of e;
 *   - sas_align_edit*: w0 = max(lo of e's segment, e - m - k); an end in no segment gets the
 *     "no alignment" record;
 *   - sas_map_edit*: its reduction over the constrained ends of both strands; n_best and n_loci
 *     keep their run definitions;
 *   - sas_map_pairs*: the loci are those of the constrained answers, and a candidate is proper
 *     only if both of its ends have the same sequence.  Sequence, not segment: mates legitimately
 *     span a gap inside one scaffold;
 *   - sas_map_pairs_rescue*: the window W of partner ends is intersected with the anchor's
 *     sequence i, (seq_start[i], seq_start[i + 1]]; the scanned distance is D_L, so an end in no
 *     segment is no candidate and breaks a run of candidate ends like any other end that is none;
 *     the window's first end, a run head, is the first end of the intersected window;
 *   - the exact calls (sas_search*, sas_search_range*, sas_locate*, sas_match*) are index lookups
 *     and ignore the layout: filter their positions with sas_translate.
 *
 * sas_translate: text positions back to (sequence, offset).  For the interval [pos[i], pos[i] +
 * span[i]) (span_or_null == NULL: every span is 1; a span of 0 counts as 1): out_seq[i] = the
 * sequence id if the interval lies inside one segment, else SAS_SEQ_NONE; out_off[i] = pos[i] -
 * seq_start[id], or pos[i] itself beside SAS_SEQ_NONE.  pos and out_off are u64, or u32 with
 * SAS_LOCATE_U32 (as sas_locate* wrote them; EINVAL for n >= 2^32); span and out_seq are u32.
 * With SAS_DEVICE_PTRS the call is asynchronous on `stream` and reads nothing back; with host
 * pointers it is synchronous.  EINVAL for an index without a layout. */
#define SAS_SEQ_NONE 0xFFFFFFFFu
int sas_check_layout(uint64_t n, const uint64_t* seq_start, uint64_t nseq,
                     const uint64_t* seg_lo, const uint64_t* seg_hi, uint64_t nseg);
int sas_set_layout(sas_index* index, const uint64_t* seq_start, uint64_t nseq,
                   const uint64_t* seg_lo, const uint64_t* seg_hi, uint64_t nseg);
int sas_get_layout(const sas_index* index, uint64_t* nseq, uint64_t* nseg,
                   uint64_t* seq_start, uint64_t* seg_lo, uint64_t* seg_hi);
int sas_translate(const sas_index* index, const void* pos, const uint32_t* span_or_null, uint64_t count,
                  uint32_t* out_seq, void* out_off, void* stream, uint32_t flags);
/* sas_read_fasta_layout: the text of sas_read_fasta, byte for byte (an SA built from it stays
 * valid), with its layout: one sequence per record, FASTA or FASTQ (seq_start gets nseq + 1
 * entries; seq_cap counts entries), a segment per maximal run of ACGTacgt inside a record, and
 * in `names` each header's first word, NUL-terminated, in record order.  Every array may be NULL:
 * it is then not written, and *len, *nseq, *nseg and *names_len (may be NULL) are still set, so a
 * call with all of them NULL sizes the buffers.  ENOMEM when a non-null array is too small. */
int sas_read_fasta_layout(const char* path, uint8_t* out, uint64_t cap, uint64_t* len,
                          uint64_t* seq_start, uint64_t seq_cap, uint64_t* nseq,
                          uint64_t* seg_lo, uint64_t* seg_hi, uint64_t seg_cap, uint64_t* nseg,
                          char* names, uint64_t names_cap, uint64_t* names_len);
/* sas_kmer_keys: the --human u32 keys of sst/bin/bench.rs:58-76 for the S-tree:
 * out[j] = packed chars [j, j+k) & i32::MAX, j < min(n, limit+k-1) - (k-1),
 * out[0] = i32::MAX.  out == NULL -> only *count.  k in 1..16. */
int sas_kmer_keys(const uint8_t* text, uint64_t n, uint32_t k, uint64_t limit, uint32_t* out,
                  uint64_t* count, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* SAS_H */
