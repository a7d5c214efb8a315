"""Host-side mirror of the reference's suffix-array query API (sas/sa_search.rs).

    SaNaive.build(t)                      <- SaNaive::build            sas/sa_search.rs:30-57
    binary_search(sa, q, cnt)             <- binary_search (type F1)    sas/sa_search.rs:98-112, :453
    binary_search_batch(sa, qs, cnt)      <- binary_search_batch<B>     sas/sa_search.rs:157-196, :454
    SaNaive.search_batch(queries, algo)   <- bench_batch driver         sas/sa_search.rs:437-451
    random_string / random_queries        <- sas/util.rs:9-26 (ChaCha8Rng::seed_from_u64, sas/main.rs:38)

Every call runs on the GPU through libsas_amd.so.  `cnt` is the reference's
`&mut usize` probe counter: pass a `Counter` and it is incremented by the number
of suffix comparisons the query made.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._io import HOST, Side, as_u8 as _as_u8, is_cuda as _is_cuda, ptr as _ptr, queries as _queries, sized
from ._lib import check, lib


@dataclass
class Counter:
    """Stands in for the reference's `cnt: &mut usize` argument."""
    value: int = 0


# the mapping records: (field, one entry per "read" or per "pair", kind, a column per run).  Mapped
# is sas_map_edit's record, MappedPairs (sas_map_pairs) adds three fields per pair, MappedPairsRescue
# (sas_map_pairs_rescue) one more; the C calls take the outputs in this order.
_RECORD = (("end", "read", "pos", False), ("start", "read", "pos", False), ("dist", "read", "u8", False),
           ("strand", "read", "u8", False), ("n_best", "read", "u32", False), ("n_loci", "read", "u32", False),
           ("nruns", "read", "u8", False), ("runs", "read", "u16", True), ("qflags", "read", "u8", False),
           ("pflags", "pair", "u8", False), ("n_pairs", "pair", "u32", False), ("n_best_pairs", "pair", "u32", False),
           ("n_rescue", "pair", "u32", False))
Mapped = namedtuple("Mapped", [f[0] for f in _RECORD[:9]])
MappedPairs = namedtuple("MappedPairs", [f[0] for f in _RECORD[:12]])
MappedPairsRescue = namedtuple("MappedPairsRescue", [f[0] for f in _RECORD])


def _run_cols(k) -> int:
    """Columns of a `runs` output: an alignment within k edits has at most 2k + 1 runs."""
    return 2 * int(k) + 1


def _record(rec, side: Side, nq: int, k):
    """The outputs of a mapping call on `side`, uninitialised: nq reads (nq / 2 pairs), scripts of
    up to k edits."""
    return rec(*(side.new(kind, (nq if per == "read" else nq // 2,) + ((_run_cols(k),) if runs else ()))
                 for _, per, kind, runs in _RECORD[:len(rec._fields)]))


def _prefix_flags(prefix, quad, n: int, inline: bool = False) -> int:
    """prefix=None: build the prefix table (SAS_BUILD_PREFIX, p chosen by the library)
    whenever a quad tree is built and n < 2^32 - 1; False: never; an int: that p.
    inline: 1 (or True): 16-B entries inlining each range's first suffix
    (SAS_BUILD_PREFIX_INLINE); 2 / 4: 32-B / 64-B entries with its first two / four
    (_INLINE2 / _INLINE4)."""
    if prefix is None:
        prefix = bool(quad) and n < 0xFFFFFFFF
    if prefix is False:
        return 0
    f = _lib.SAS_BUILD_PREFIX | ({1: _lib.SAS_BUILD_PREFIX_INLINE, 2: _lib.SAS_BUILD_PREFIX_INLINE2,
                                    4: _lib.SAS_BUILD_PREFIX_INLINE4}.get(int(inline), 0))
    if prefix is True:
        return f
    return f | _lib.SAS_BUILD_PREFIX_P(int(prefix))


def _quad_flags(quad) -> int:
    """True: fused leaves; "compact": key-only leaves.  The inner-node layout is picked
    by the library (SAS_BUILD_QUAD_ABS / _REL in sas.h) unless a suffix forces it:
    "abs" / "rel" (fused) or "compact-abs" / "compact-rel"."""
    if quad is False:
        return 0
    if quad is True:
        quad = "fused"
    if not isinstance(quad, str):
        raise ValueError(f"quad must be a bool or a string, not {quad!r}")
    leaves, _, layout = quad.partition("-") if quad.startswith("compact") else ("fused", "", quad)
    if layout == "fused":
        layout = ""
    flags = {"fused": _lib.SAS_BUILD_QUAD, "compact": _lib.SAS_BUILD_QUAD_COMPACT}.get(leaves)
    lay = {"": 0, "abs": _lib.SAS_BUILD_QUAD_ABS, "rel": _lib.SAS_BUILD_QUAD_REL}.get(layout)
    if flags is None or lay is None:
        raise ValueError(f"quad must be True, False, 'compact', 'abs', 'rel', 'compact-abs' or "
                         f"'compact-rel', not {quad!r}")
    return flags | lay


def _build_flags(n: int, flags: int = 0, *, lcp, stree, sector, quad, llcp, prefix, prefix_inline=False,
                 prefix_n: int | None = None, verify=False, sa40=False, top2_levels: int = 0) -> int:
    """The SAS_BUILD_* flags of the structures asked for, ORed into `flags`.  Every builder passes
    its own defaults; llcp None: only while n < 2^31; prefix None: _prefix_flags' default for a
    table over prefix_n suffixes (None: n)."""
    if llcp is None:
        llcp = n < (1 << 31)
    flags |= (_lib.SAS_BUILD_LCP if lcp else 0) | (_lib.SAS_BUILD_STREE if stree else 0)
    flags |= (_lib.SAS_BUILD_LLCP if llcp else 0) | (_lib.SAS_BUILD_SECTOR if sector else 0)
    flags |= (_lib.SAS_BUILD_VERIFY if verify else 0) | (_lib.SAS_BUILD_SA40 if sa40 else 0)
    flags |= _lib.SAS_BUILD_TOP2_LEVELS(top2_levels) | _quad_flags(quad)
    return flags | _prefix_flags(prefix, quad, n if prefix_n is None else prefix_n, prefix_inline)


class SaNaive:
    """GPU-resident suffix-array index: 2-bit packed text, u32 SA, optional LCP
    array and S-tree over 16-char SA keys, all in HBM."""

    def __init__(self, handle, n):
        self._h = handle
        self.n = n  # text length
        self.sa_n = self.stats()["sa_entries"]  # SA entries held (n, or a shard's rank range)
        self.rank_lo = self.stats()["rank_lo"]
        self.next_pos = self.stats()["next_pos"]  # SA value of the rank after this index's range
        self._device = None  # the GPU the index was built on (the current one at build time)
        try:
            import torch
            if torch.cuda.is_available():
                self._device = torch.cuda.current_device()
        except ImportError:
            pass

    @classmethod
    def build(cls, t, sa=None, lcp: bool = True, stree: bool | None = None, verify: bool = False,
              rank_range: tuple[int, int] | None = None, flags: int = 0, sector: bool | None = None,
              sa40: bool = False, quad: bool | str | None = None, llcp: bool | None = None,
              prefix: bool | int | None = None, prefix_inline: bool | int = False,
              tagged: bool | int = False, top2_levels: int = 0, tag_lines: bool = False) -> "SaNaive":
        """Index over t.  rank_range=(lo, hi): sharded-text mode, hold only global SA
        ranks [lo, hi) (sas_build_shard); `sa` is then the FULL suffix array or None
        (u32 or u64 array).  sa40: store a packed 40-bit SA and use the bucketed
        builder even when n < 2^32 (automatic above).  quad="compact": key-only quad
        leaves (8 B per suffix, SA values read from the SA array; SAS_BUILD_QUAD_COMPACT).
        llcp: the Manber-Myers Llcp/Rlcp entries for algo="llcp" (SAS_BUILD_LLCP, 16 B
        per suffix, implies the LCP array); None = only while n < 2^31 (<= 32 GiB).  prefix: the prefix table for algo="prefix"
        (SAS_BUILD_PREFIX; None = whenever quad is built and n < 2^32 - 1, an int = its
        p chars); prefix_inline: 16-B entries that inline each range's first suffix
        (True / 1: SAS_BUILD_PREFIX_INLINE) or 32-B ones with its first two (2:
        SAS_BUILD_PREFIX_INLINE2); fused quad leaves, u32 SA.  tagged: the SA as 8-B tagged
        entries + a bucket table over the first p chars (SAS_BUILD_TAGGED; True = p chosen by
        the library, an int = that p) for algo="tagged"; it replaces the SA and leaves out the
        trees, LLCP and the prefix tables (their defaults turn off).  top2_levels: depth of
        the binary-search pivots (SAS_BUILD_TOP2_LEVELS, rounded up to 4-level prefix-relative
        blocks past the 15 LDS levels; 0 = the library default, 27 levels, 273 MiB; 30 -> all
        31 levels of n = 2^30, 4.3 GiB).
        tag_lines (with tagged): the tagged entries as 128-B bucket lines + an overflow array
        (SAS_BUILD_TAG_LINES; p = ceil(log4 n) - 2 unless tagged gives it): one request gives a
        lookup its bucket and first 20 entries; algo="tagged" only, no SA array."""
        t = _as_u8(t)
        dev = _is_cuda(t)
        n = int(t.numel() if dev else len(t))
        if tagged is not False:
            stree, sector, quad, prefix = bool(stree), bool(sector), quad or False, prefix or False
            llcp = bool(llcp)
            flags |= _lib.SAS_BUILD_TAGGED | (0 if tagged is True else _lib.SAS_BUILD_PREFIX_P(int(tagged)))
            flags |= _lib.SAS_BUILD_TAG_LINES if tag_lines else 0
            lcp = lcp and not tag_lines  # a bucket-line index serves TAGGED only: no LCP array
        flags = _build_flags(n, flags | (_lib.SAS_DEVICE_PTRS if dev else 0), lcp=lcp,
                             stree=True if stree is None else stree, sector=True if sector is None else sector,
                             quad=True if quad is None else quad, llcp=llcp, prefix=prefix,
                             prefix_inline=prefix_inline,
                             prefix_n=None if rank_range is None else rank_range[1] - rank_range[0], verify=verify,
                             sa40=sa40, top2_levels=top2_levels)
        sa_w = 4
        if sa is not None:
            if dev != _is_cuda(sa):
                raise ValueError("text and sa must both be host or both be device arrays")
            if not dev:
                sa = np.asarray(sa)
                sa = np.ascontiguousarray(sa, np.uint64 if sa.dtype.itemsize == 8 else np.uint32)
            sa_w = sa.element_size() if dev else sa.dtype.itemsize
        h = C.c_void_p()
        if rank_range is None:
            check(lib().sas_build(_ptr(t), n, _ptr(sa), sa_w, flags, C.byref(h)))
        else:
            check(lib().sas_build_shard(_ptr(t), n, _ptr(sa), sa_w, int(rank_range[0]), int(rank_range[1]), flags,
                                        C.byref(h)))
        return cls(h, n)

    @classmethod
    def build_part(cls, t, part: int, parts: int, lcp: bool = True, stree: bool = True, verify: bool = False,
                   flags: int = 0, sector: bool = True, quad: bool | str = True, llcp: bool | None = None,
                   prefix: bool | int | None = None, prefix_inline: bool | int = False,
                   top2_levels: int = 0) -> "SaNaive":
        """Sharded-text index that builds ONLY its own SA rank range (sas_build_part):
        part `part` of `parts` contiguous 7-char-prefix bin ranges.  The range is
        chosen by the library (stats: rank_lo, sa_entries, next_pos).  prefix_inline as in
        build (inline tables need n < 2^32 beside the part's 40-bit SA)."""
        t = _as_u8(t)
        dev = _is_cuda(t)
        n = int(t.numel() if dev else len(t))
        flags = _build_flags(n, flags | (_lib.SAS_DEVICE_PTRS if dev else 0), lcp=lcp, stree=stree, sector=sector,
                             quad=quad, llcp=llcp, prefix=prefix, prefix_inline=prefix_inline, verify=verify,
                             top2_levels=top2_levels)
        h = C.c_void_p()
        check(lib().sas_build_part(_ptr(t), n, int(part), int(parts), flags, C.byref(h)))
        return cls(h, n)

    @classmethod
    def build_gen(cls, n: int, seed: int = 31415, part: int | None = None, parts: int | None = None,
                  flags: int = 0, **kw) -> "SaNaive":
        """The index over random_string(n, seed) (sas/util.rs:9-15) generated on the GPU
        straight into the packed text (sas_build_gen / sas_build_part_gen): no n-byte text
        exists anywhere.  part/parts: a build_part index; the keyword flags are build's
        (lcp, stree, sector, quad, llcp, prefix, prefix_inline, top2_levels, verify)."""
        structures = dict(lcp=True, stree=True, sector=True, quad=True, llcp=None, prefix=None, prefix_inline=False,
                          verify=False, top2_levels=0)
        if set(kw) - set(structures):
            raise TypeError(f"build_gen: unexpected {sorted(set(kw) - set(structures))}")
        flags = _build_flags(n, flags, **{**structures, **kw})
        h = C.c_void_p()
        if part is None:
            check(lib().sas_build_gen(seed, n, flags, C.byref(h)))
        else:
            check(lib().sas_build_part_gen(seed, n, int(part), int(parts), flags, C.byref(h)))
        return cls(h, n)

    @classmethod
    def build_part_gen(cls, n: int, seed: int = 31415, part: int = 0, parts: int = 1, **kw) -> "SaNaive":
        """build_part over random_string(n, seed) generated on the GPU (sas_build_part_gen)."""
        return cls.build_gen(n, seed=seed, part=part, parts=parts, **kw)

    def free(self):
        if self._h:
            lib().sas_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # -- introspection (Index<usize> for SaNaive, sas/sa_search.rs:21-27)
    def stats(self) -> dict:
        s = _lib.SasStats()
        check(lib().sas_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def suffix_array(self, count: int | None = None, start: int = 0) -> np.ndarray:
        """Local SA entries [start, start+count): u32 for a u32 index, u64 for a 40-bit one."""
        count = self.sa_n - start if count is None else count
        if self.stats()["sa_width"] == 4 and start == 0:
            out = HOST.new("u32", count)
            check(lib().sas_copy_sa(self._h, _ptr(out), count, 0))
            return out
        out = HOST.new("u64", count)
        check(lib().sas_copy_sa64(self._h, self.rank_lo + start, count, _ptr(out), 0))
        return out

    # -- the sequence layout (sas.h: sas_set_layout): each segment is a text of its own for the
    #    approximate calls; exact lookups ignore it
    def set_layout(self, seq_start=None, seg_lo=(), seg_hi=()):
        """Set the index's sequence layout from host arrays (sas_set_layout: seq_start has one more
        entry than sequences, from 0 to n; the segments [seg_lo[i], seg_hi[i]) are the real bases),
        or clear it with seq_start=None.  No call may be in flight on the index."""
        if seq_start is None:
            check(lib().sas_set_layout(self._h, None, 0, None, None, 0))
            return
        s = np.ascontiguousarray(seq_start, np.uint64)
        lo, hi = np.ascontiguousarray(seg_lo, np.uint64), np.ascontiguousarray(seg_hi, np.uint64)
        if len(s) < 2 or len(lo) != len(hi):
            raise ValueError("set_layout: seq_start needs at least two entries, seg_lo and seg_hi equal lengths")
        check(lib().sas_set_layout(self._h, s.ctypes.data, len(s) - 1, lo.ctypes.data if len(lo) else None,
                                   hi.ctypes.data if len(hi) else None, len(lo)))

    def layout(self):
        """(seq_start, seg_lo, seg_hi) as numpy uint64 arrays (sas_get_layout), or None without one."""
        nseq, nseg = C.c_uint64(0), C.c_uint64(0)
        check(lib().sas_get_layout(self._h, C.byref(nseq), C.byref(nseg), None, None, None))
        if nseq.value == 0:
            return None
        s, lo, hi = HOST.new("u64", nseq.value + 1), HOST.new("u64", nseg.value), HOST.new("u64", nseg.value)
        check(lib().sas_get_layout(self._h, None, None, _ptr(s), _ptr(lo), _ptr(hi)))
        return s, lo, hi

    def translate(self, pos, span=None, u32: bool = False, stream=None):
        """Text positions to (sequence id, offset in it) (sas_translate): the id is SAS_SEQ_NONE, and
        the offset the position itself, unless [pos, pos + span) (span None: 1) lies inside one
        segment.  torch CUDA tensors (pos int64, or int32 with u32; span int32) -> CUDA tensors
        (int32 ids holding the u32 bits, offsets in pos's dtype), asynchronous; numpy -> numpy."""
        side = Side(pos, stream, u32)
        if side.dev:
            dt = side.dtype("pos")
            if pos.dtype != dt or (span is not None and (not _is_cuda(span) or span.dtype != side.dtype("u32"))):
                raise ValueError(f"translate: pos must be a CUDA {dt} tensor and span a CUDA int32 tensor")
            pos = pos.contiguous()
            span = None if span is None else span.contiguous()
        else:
            pos = np.ascontiguousarray(pos, side.dtype("pos"))
            span = None if span is None else np.ascontiguousarray(span, np.uint32)
        cnt = side.count(pos)
        if span is not None and side.count(span) != cnt:
            raise ValueError("translate: one span per position")
        seq, off = side.new("u32", cnt), side.new("pos", cnt)
        check(lib().sas_translate(self._h, _ptr(pos), _ptr(span), cnt, _ptr(seq), _ptr(off), side.stream,
                                  side.flags))
        return seq, off

    def lcp_array(self) -> np.ndarray:
        out = HOST.new("u32", self.sa_n)
        check(lib().sas_copy_lcp(self._h, _ptr(out), self.sa_n, 0))
        return out

    def extract(self, pos, lens, out_off, out, stream=None):
        """Text substrings as byte codes from the index's packed text (sas_extract):
        out[out_off[i] : out_off[i] + lens[i]] = text[pos[i] : pos[i] + lens[i]].
        torch CUDA tensors (int64 pos / out_off, int32 lens, uint8 out), async."""
        side = Side(out, stream)
        check(lib().sas_extract(self._h, _ptr(pos), _ptr(lens), _ptr(out_off), int(pos.numel()), _ptr(out), side.stream,
                                side.flags))
        return out

    @staticmethod
    def pack_queries(qbytes, m: int, stream=None):
        """2-bit packed fixed-length queries (sas_pack_queries; m <= 32): torch CUDA
        uint8 in -> torch CUDA int64 words out (first char in bits 63..62); numpy uint8 in
        -> numpy uint64 out, packed on the host."""
        side = Side(qbytes, stream)
        qbytes = _as_u8(qbytes)
        nq = side.count(qbytes) // m if m else 0
        out = side.new("u64", nq)
        check(lib().sas_pack_queries(_ptr(qbytes), m, nq, _ptr(out), side.stream, side.flags))
        return out

    def search_packed(self, qwords, m: int, algo: str = "prefix", probes: bool = False, out=None, stream=None):
        """Lookups of packed fixed-length queries (sas_search_packed): numpy uint64 in ->
        numpy out; torch CUDA in -> torch CUDA out (async)."""
        side = Side(qwords, stream)
        if not side.dev:
            qwords = np.ascontiguousarray(qwords, np.uint64)
        nq = side.count(qwords)
        if out is None or not side.dev:  # `out` is for device calls; a host call returns a new array
            out = side.new("u64", nq)
        pr = side.new("u32" if probes else None, nq)
        check(lib().sas_search_packed(self._h, _ptr(qwords), m, nq, _lib.ALGOS[algo], _ptr(out), _ptr(pr),
                                      side.stream, side.flags))
        return (out, pr) if probes else out

    def search_buckets(self, queries, m: int, cap: int, counts, algo: str = "prefix", out=None, stream=None):
        """The sharded step's local lookup (sas_search_buckets): `queries` holds
        counts.numel() buckets of `cap` slots (uint8, m bytes a slot, or int64 2-bit words
        for PREFIX with m <= 32), bucket b's first counts[b] slots are queries; only those
        are searched and written into `out` (int64, one per slot).  torch CUDA tensors."""
        dev = queries.device
        for name, tns in (("queries", queries), ("counts", counts)) + ((("out", out),) if out is not None else ()):
            if not tns.is_cuda or tns.device != dev:
                raise ValueError(f"search_buckets: {name} must be a CUDA tensor on {dev}, not {tns.device}")
        side = Side(queries, stream)
        i64 = side.dtype("u64")
        nb = int(counts.numel())
        packed = queries.dtype == i64
        need = nb * cap * (1 if packed else m)
        if counts.dtype != i64 or not counts.is_contiguous() or queries.numel() < need or \
                not queries.is_contiguous() or (not packed and queries.dtype != side.dtype("u8")):
            raise ValueError("search_buckets: int64 counts, and uint8 bytes or int64 words for every slot")
        if out is None:
            out = side.new("u64", nb * cap)
        if out.dtype != i64 or out.numel() < nb * cap:
            raise ValueError("search_buckets: int64 out of one entry per slot")
        check(lib().sas_search_buckets(self._h, _ptr(queries), m, nb, int(cap), _ptr(counts), _lib.ALGOS[algo],
                                       _ptr(out), side.stream, (_lib.SAS_ROUTE_PACKED if packed else 0) | side.flags))
        return out

    def route(self, splitter_pos, qbytes, m: int, stream=None):
        """Sharded mode: shard id of each fixed-length query = number of splitter
        suffixes < q (sas_route).  numpy in -> numpy out; CUDA in -> CUDA out."""
        side = Side(qbytes, stream)
        if not side.dev:
            qbytes, splitter_pos = _as_u8(qbytes), np.ascontiguousarray(splitter_pos, np.uint64)
        nq, nsplit = side.count(qbytes) // m, side.count(splitter_pos)
        out = side.new("u32", nq)
        check(lib().sas_route(self._h, _ptr(splitter_pos) if nsplit else None, nsplit, _ptr(qbytes), m, nq, _ptr(out),
                              side.stream, side.flags))
        return out

    def route_pack(self, splitter_pos, qbytes, m: int, stream=None, cap: int | None = None, send=None,
                   packed: bool = False):
        """Send side of one sharded step, fused on the GPU (sas_route_pack): CUDA
        tensors in -> (counts int64 [W], send uint8 [nq*m] grouped by shard,
        slot int64 [nq] = send position of each query).  cap: fixed-capacity buckets
        (sas_route_pack_cap): send holds W*cap slots, bucket w at slots [w*cap, ...), and
        counts > cap on the device marks an overflow.  packed (m <= 32, SAS_ROUTE_PACKED):
        each slot is the query's 8-B 2-bit word (send is int64) instead of its m bytes.
        `send` may be passed in (reused)."""
        side = Side(qbytes, stream)
        nq = qbytes.numel() // m
        W = splitter_pos.numel() + 1
        counts = side.new("u64", W)
        slots = W * cap if cap else nq
        size = slots if packed else slots * m
        kind = "u64" if packed else "u8"
        if send is None or send.numel() < max(size, 1) or send.dtype != side.dtype(kind):
            send = side.new(kind, max(size, 1), 0)
        slot = side.new("u64", max(nq, 1))
        fn, caps = (lib().sas_route_pack_cap, (int(cap),)) if cap else (lib().sas_route_pack, ())
        check(fn(self._h, _ptr(splitter_pos) if W > 1 else None, W - 1, _ptr(qbytes), m, nq, *caps, _ptr(counts),
                 _ptr(send), _ptr(slot), side.stream, (_lib.SAS_ROUTE_PACKED if packed else 0) | side.flags))
        return counts, send[:size], slot[:nq]

    def shard_gather(self, back, slot, out=None, counts=None, cap: int = 0, overflow=None, stream=None):
        """Receive side of one sharded step (sas_shard_gather): out[k] = back[slot[k]]; with
        `overflow` (an int32 CUDA tensor of 1, never cleared here) it is set to 1 when some
        counts[w] > cap."""
        side = Side(slot, stream)
        nq = slot.numel()
        if out is None:
            out = side.new("u64", nq)
        i64 = side.dtype("u64")
        if out.numel() < nq or out.dtype != i64 or back.dtype != i64 or slot.dtype != i64:
            raise ValueError("shard_gather: int64 back/slot/out, out of at least len(slot)")
        if overflow is not None and (counts is None or overflow.dtype != side.dtype("u32")):
            raise ValueError("shard_gather: overflow needs counts and an int32 flag")
        check(lib().sas_shard_gather(self._h, _ptr(back), _ptr(slot), nq, _ptr(counts),
                                     counts.numel() if counts is not None else 0, int(cap), _ptr(out), _ptr(overflow),
                                     side.stream, side.flags))
        return out[:nq]

    def verify(self):
        check(lib().sas_verify(self._h))

    # -- searching
    def search_fixed(self, qbytes, m: int, algo: str = "plain", probes: bool = False, stream=None,
                     out=None, flags: int = 0):
        """Fixed-length queries, query k = qbytes[k*m:(k+1)*m].  Host numpy in ->
        numpy out (synchronous); torch CUDA in -> CUDA out (async on `stream`)."""
        return self._search(_queries(qbytes, None, None, m, stream), algo, probes, out, flags)

    def search_batch(self, qbytes, qoff, qlen, algo: str = "plain", probes: bool = False, stream=None,
                     out=None, flags: int = 0):
        """Ragged queries, query k = qbytes[qoff[k] : qoff[k] + qlen[k]]."""
        return self._search(_queries(qbytes, qoff, qlen, 0, stream), algo, probes, out, flags)

    def search_slices(self, qoff, qlen, algo: str = "tagged", probes: bool = False, stream=None, out=None,
                      flags: int = 0):
        """Queries that are slices of the indexed text, t[qoff[k] : qoff[k] + qlen[k]] (the
        reference's borrowed &t[i..i+len] queries; SAS_QUERIES_ARE_SLICES): torch CUDA int64
        offsets / int32 lengths in, no query bytes -> torch CUDA positions out."""
        side = Side(qoff, stream)
        if not (side.dev and _is_cuda(qlen)):
            raise ValueError("search_slices: torch CUDA qoff / qlen")
        if qoff.dtype != side.dtype("u64") or qlen.dtype != side.dtype("u32") or not qoff.is_contiguous() or \
                not qlen.is_contiguous() or qoff.numel() != qlen.numel():
            raise ValueError("search_slices: contiguous int64 qoff and int32 qlen of the same length")
        nq = side.count(qoff)
        return self._search((side, nq, (None, _ptr(qoff), _ptr(qlen), nq), ""), algo, probes, out,
                            flags | _lib.SAS_QUERIES_ARE_SLICES)

    def _search(self, q, algo, probes, out, flags):
        side, nq, lead, suffix = q
        if out is None:
            out = side.new("u64", nq)
        elif not side.dev:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous
                    and len(out) >= nq):
                raise ValueError("out: a C-contiguous numpy uint64 array of at least nq entries")
            out = out[:nq]
        pr = side.new("u32", nq) if probes else None
        fn = lib().sas_search_fixed if suffix else lib().sas_search_batch
        check(fn(self._h, *lead, _lib.ALGOS[algo], _ptr(out), _ptr(pr), side.stream, flags | side.flags))
        return (out, pr) if probes else out

    def search(self, queries, algo: str = "plain", probes: bool = False):
        """List of byte strings / arrays -> positions (host)."""
        qs = [_as_u8(q) for q in queries]
        lens = np.array([len(q) for q in qs], np.uint32)
        off = np.zeros(len(qs), np.uint64)
        if len(qs):
            off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        buf = np.concatenate(qs + [np.zeros(64, np.uint8)]) if qs else np.zeros(64, np.uint8)
        return self.search_batch(buf, off, lens, algo=algo, probes=probes)

    def search_range(self, qbytes, qoff, qlen, stream=None, flags: int = 0):
        """Occurrence ranges (Search::search_prefix, sas/util.rs:36-40): global SA
        ranks (lo, hi) of the suffixes starting with each query; count = hi - lo."""
        return self._search_range(_queries(qbytes, qoff, qlen, 0, stream), flags)

    def search_range_fixed(self, qbytes, m: int, stream=None, flags: int = 0):
        """search_range for fixed-length queries qbytes[k*m .. (k+1)*m) (sas_search_range_fixed)."""
        return self._search_range(_queries(qbytes, None, None, m, stream, what="search_range"), flags)

    def _search_range(self, q, flags):
        side, nq, lead, suffix = q
        lo, hi = side.new("u64", nq), side.new("u64", nq)
        # ranks, not text positions: a side that carries u32 positions passes no SAS_LOCATE_U32 here
        check(getattr(lib(), "sas_search_range" + suffix)(self._h, *lead, _ptr(lo), _ptr(hi), side.stream,
                                                          flags | (side.flags & _lib.SAS_DEVICE_PTRS)))
        return lo, hi

    def search_prefix(self, q) -> np.ndarray:
        """All text positions where q occurs (Search::search_prefix, sas/util.rs:36-40)."""
        q = _as_u8(q)
        buf = np.concatenate([q, np.zeros(64, np.uint8)])
        lo, hi = self.search_range(buf, np.zeros(1, np.uint64), np.array([len(q)], np.uint32))
        cnt = int(hi[0] - lo[0])
        if self.stats()["sa_width"] != 4:
            out = HOST.new("u64", cnt)
            check(lib().sas_copy_sa64(self._h, int(lo[0]), cnt, _ptr(out), 0))
            return out
        out = HOST.new("u32", cnt)
        check(lib().sas_copy_sa_range(self._h, int(lo[0]), cnt, _ptr(out), 0))
        return out

    # -- batched locate: every occurrence position of every query (sas_locate*)
    def locate_ranges(self, lo, hi, max_per_query: int = 0, out=None, capacity: int | None = None,
                      u32: bool = False, stream=None, flags: int = 0):
        """Positions of the SA rank ranges [lo[k], hi[k]) this index holds, in CSR form
        (sas_locate_offsets + sas_locate_fill): torch CUDA int64 lo / hi in -> (off, pos), off
        int64 [nq + 1], query k's positions pos[off[k] : off[k + 1]] in SA rank order (int64, or
        with u32 int32 holding the u32 bit patterns).  max_per_query caps each query's count
        (0: no cap).  Without out / capacity the total is read back once (off[nq].item()) to
        size pos; with `out` (a tensor to fill) or `capacity` nothing synchronises, pos is the
        whole buffer, nothing at or past its capacity is written and the caller checks
        off[nq] <= capacity.  A shard emits only the ranks it holds."""
        side = Side(lo, stream, u32)
        if not (side.dev and _is_cuda(hi)) or lo.dtype != side.dtype("u64") or hi.dtype != side.dtype("u64") or \
                lo.numel() != hi.numel() or not lo.is_contiguous() or not hi.is_contiguous():
            raise ValueError("locate_ranges: contiguous torch CUDA int64 lo and hi of the same length")
        nq = side.count(lo)
        off = side.new("u64", nq + 1)
        check(lib().sas_locate_offsets(self._h, _ptr(lo), _ptr(hi), nq, int(max_per_query), _ptr(off), side.stream,
                                       _lib.SAS_DEVICE_PTRS))

        def fill(bufs, cap, _):
            return lib().sas_locate_fill(self._h, _ptr(lo), _ptr(off), nq, _ptr(bufs[0]), int(cap), side.stream,
                                         flags | side.flags)
        (pos,), _ = sized(side, "locate_ranges", fill, off, nq, out=out, capacity=capacity, sizing=False)
        return off, pos

    def _locate(self, q, max_per_query, out, capacity, flags):
        side, nq, lead, suffix = q
        if side.dev and out is None and capacity is None:  # ranges, offsets, one read of the total, fill
            lo, hi = self._search_range(q, flags)
            return self.locate_ranges(lo, hi, max_per_query, u32=side.u32, stream=side.stream,
                                      flags=flags & _lib.SAS_LOCATE_NO_PARTITION)
        fn = getattr(lib(), "sas_locate" + suffix)
        off = side.new("u64", nq + 1)

        def call(bufs, cap, total):
            return fn(self._h, *lead, int(max_per_query), _ptr(off), _ptr(bufs[0]), int(cap), total, side.stream,
                      flags | side.flags)
        (pos,), _ = sized(side, "locate", call, off, nq, out=out, capacity=capacity)
        return off, pos

    def locate(self, qbytes, qoff, qlen, max_per_query: int = 0, u32: bool = False, stream=None, out=None,
               capacity: int | None = None, flags: int = 0):
        """Every occurrence position of every ragged query qbytes[qoff[k] : qoff[k] + qlen[k]]
        in one call (sas_locate): (off, pos) in CSR form as locate_ranges gives them.  numpy in
        -> numpy out (a sizing call, then the real one); torch CUDA in -> CUDA out, async when
        out / capacity is given (otherwise the total is read back once)."""
        return self._locate(_queries(qbytes, qoff, qlen, 0, stream, u32), max_per_query, out, capacity, flags)

    def locate_fixed(self, qbytes, m: int, max_per_query: int = 0, u32: bool = False, stream=None, out=None,
                     capacity: int | None = None, flags: int = 0):
        """locate for fixed-length queries qbytes[k*m : (k+1)*m] (sas_locate_fixed)."""
        return self._locate(_queries(qbytes, None, None, m, stream, u32, "locate"), max_per_query, out, capacity,
                            flags)

    def locate_between(self, a, b) -> np.ndarray:
        """Positions of the suffixes s with a <= s < b, in SA order (Search::search_range over a
        Range<&Seq>, sas/util.rs:41-46): the ranks from range(a).lo to range(b).lo."""
        import torch
        a, b = _as_u8(a), _as_u8(b)
        buf = np.concatenate([a, b, np.zeros(64, np.uint8)])
        lo, _ = self.search_range(buf, np.array([0, len(a)], np.uint64), np.array([len(a), len(b)], np.uint32))
        dev = torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())
        dlo = torch.tensor([int(lo[0])], dtype=torch.int64, device=dev)
        dhi = torch.tensor([int(lo[1])], dtype=torch.int64, device=dev)
        _, pos = self.locate_ranges(dlo, dhi)
        return pos.cpu().numpy().astype(np.uint64)

    # -- longest-prefix match and matching statistics (sas_match*)
    def _match(self, fn, side, nq, lead, ranges, flags):
        ln, pos = side.new("u32", nq), side.new("u64", nq)
        lo, hi = side.new("u64" if ranges else None, nq), side.new("u64" if ranges else None, nq)
        check(fn(self._h, *lead, _ptr(ln), _ptr(pos), _ptr(lo), _ptr(hi), side.stream, flags | side.flags))
        return (ln, pos, lo, hi) if ranges else (ln, pos)

    def match(self, qbytes, qoff, qlen, ranges: bool = True, stream=None, flags: int = 0):
        """Longest-prefix match of ragged queries qbytes[qoff[k] : qoff[k] + qlen[k]] (sas_match):
        (len, pos) or with ranges (len, pos, lo, hi).  len[k] is the length of the longest prefix
        of query k that occurs in the text, pos[k] a position where it occurs (n when len is 0),
        [lo[k], hi[k]) the SA ranks of every suffix starting with that prefix.  numpy in -> numpy
        out (uint32 len, uint64 others; synchronous); torch CUDA in (uint8 bytes, int64 qoff,
        int32 qlen) -> CUDA out (int32 len, int64 others; async on `stream`)."""
        side, nq, lead, _ = _queries(qbytes, qoff, qlen, 0, stream)
        return self._match(lib().sas_match, side, nq, lead, ranges, flags)

    def match_fixed(self, qbytes, m: int, ranges: bool = True, stream=None, flags: int = 0):
        """match for fixed-length queries qbytes[k*m : (k+1)*m] (sas_match_fixed)."""
        side, nq, lead, _ = _queries(qbytes, None, None, m, stream, what="match")
        return self._match(lib().sas_match_fixed, side, nq, lead, ranges, flags)

    def match_stats(self, pattern, max_len: int, ranges: bool = True, stream=None, flags: int = 0):
        """Matching statistics of `pattern` (sas_match_stats): match of the queries
        pattern[i : min(i + max_len, len(pattern))] for every i, one entry per pattern char."""
        side = Side(pattern, stream)
        pattern = _as_u8(pattern)
        plen = side.count(pattern)
        return self._match(lib().sas_match_stats, side, plen, (_ptr(pattern), plen, int(max_len)), ranges, flags)

    # -- k-mismatch and k-difference locate (sas_locate_mismatch*, sas_locate_edit*: one contract)
    def _locate_mismatch(self, fn, q, k, max_seed_hits, dist, out, capacity, flags):
        side, nq, lead, suffix = q
        f = getattr(lib(), fn + suffix)
        off, qfl = side.new("u64", nq + 1), side.new("u8", nq)

        def call(bufs, cap, total):
            return f(self._h, *lead, int(k), int(max_seed_hits), _ptr(off), _ptr(bufs[0]), _ptr(bufs[1]), _ptr(qfl),
                     int(cap), total, side.stream, flags | side.flags)
        (pos, dst), _ = sized(side, fn[4:], call, off, nq, ("pos", "u8" if dist else None), out, capacity)
        return off, pos, dst, qfl

    def locate_mismatch(self, qbytes, qoff, qlen, k: int, max_seed_hits: int = 0, u32: bool = False,
                        dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """Every alignment of every ragged query qbytes[qoff[i] : qoff[i] + qlen[i]] with at most
        k substituted chars (sas_locate_mismatch): (off, pos, dist, qflags).  Query i's alignments
        are pos[off[i] : off[i + 1]], dist their Hamming distances (None with dist=False), qflags[i]
        a mask of SAS_MM_TRUNCATED (a seed occurred more than max_seed_hits times and was skipped;
        0: no limit) and SAS_MM_SHORT (len <= k: no result).  numpy in -> numpy out (a sizing
        call, then the real one); torch CUDA in -> CUDA out: with out / capacity one call that
        writes nothing at or past the capacity (the caller checks off[nq]), otherwise a sizing
        call first."""
        return self._locate_mismatch("sas_locate_mismatch", _queries(qbytes, qoff, qlen, 0, stream, u32), k,
                                     max_seed_hits, dist, out, capacity, flags)

    def locate_mismatch_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, u32: bool = False,
                              dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """locate_mismatch for fixed-length queries qbytes[i*m : (i+1)*m] (sas_locate_mismatch_fixed)."""
        q = _queries(qbytes, None, None, m, stream, u32, "locate_mismatch")
        return self._locate_mismatch("sas_locate_mismatch", q, k, max_seed_hits, dist, out, capacity, flags)

    # -- maximal exact matches (sas_mems*)
    def _mems(self, q, min_len, max_hits, unique, out, capacity, flags):
        side, nq, lead, suffix = q
        f = getattr(lib(), "sas_mems" + suffix)
        off, qfl = side.new("u64", nq + 1), side.new("u8", nq)
        flags |= _lib.SAS_MEM_UNIQUE if unique else 0

        def call(bufs, cap, total):
            return f(self._h, *lead, int(min_len), int(max_hits), _ptr(off), _ptr(bufs[1]), _ptr(bufs[0]),
                     _ptr(bufs[2]), _ptr(qfl), int(cap), total, side.stream, flags | side.flags)
        (tpos, qpos, ln), _ = sized(side, "mems" + suffix, call, off, nq, ("pos", "u32", "u32"), out, capacity)
        return off, qpos, tpos, ln, qfl

    def mems(self, qbytes, qoff, qlen, min_len: int, max_hits: int = 0, unique: bool = False, u32: bool = False,
             stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """Every maximal exact match of at least min_len chars between every ragged query
        qbytes[qoff[k] : qoff[k] + qlen[k]] and the text (sas_mems): (off, qpos, tpos, len, qflags).
        Query k's matches are the entries off[k] : off[k + 1]: query[qpos : qpos + len] ==
        text[tpos : tpos + len], extendable neither to the left nor to the right, ordered by qpos,
        then by the SA rank of tpos.  qflags[k] is a mask of SAS_MEM_TRUNCATED (a query offset whose
        first min_len chars occur more than max_hits times was skipped; 0: no limit) and
        SAS_MEM_SHORT (len < min_len: no result).  unique: only matches whose string occurs once in
        the text.  numpy in -> numpy out (a sizing call, then the real one); torch CUDA in -> CUDA
        out: with out (the tpos buffer) / capacity one call that writes nothing at or past the
        capacity (the caller checks off[nq]), otherwise a sizing call first."""
        return self._mems(_queries(qbytes, qoff, qlen, 0, stream, u32), min_len, max_hits, unique, out, capacity,
                          flags)

    def mems_fixed(self, qbytes, m: int, min_len: int, max_hits: int = 0, unique: bool = False, u32: bool = False,
                   stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """mems for fixed-length queries qbytes[k*m : (k+1)*m] (sas_mems_fixed)."""
        return self._mems(_queries(qbytes, None, None, m, stream, u32, "mems"), min_len, max_hits, unique, out,
                          capacity, flags)

    def locate_edit(self, qbytes, qoff, qlen, k: int, max_seed_hits: int = 0, u32: bool = False,
                    dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """Every end position of every ragged query qbytes[qoff[i] : qoff[i] + qlen[i]] within edit
        distance k (sas_locate_edit, Sellers' problem): (off, end, dist, qflags).  With D(e) = the
        least unit-cost edit distance between query i and a text substring that ends at e, query
        i's ends are end[off[i] : off[i + 1]], every e in [0, n] with D(e) <= k in ascending order;
        dist holds D(e) (None with dist=False).  The neighbouring ends of one alignment are all
        reported; where an alignment starts is not.  qflags[i] is a mask of SAS_ED_TRUNCATED (a
        seed occurred more than max_seed_hits times and was skipped; 0: no limit), SAS_ED_SHORT
        (len <= k: no result) and SAS_ED_LONG (len > 256: no result).  numpy in -> numpy out (a
        sizing call, then the real one); torch CUDA in -> CUDA out: with out / capacity one call
        that writes nothing at or past the capacity (the caller checks off[nq]), otherwise a
        sizing call first."""
        return self._locate_mismatch("sas_locate_edit", _queries(qbytes, qoff, qlen, 0, stream, u32), k,
                                     max_seed_hits, dist, out, capacity, flags)

    def locate_edit_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, u32: bool = False,
                          dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """locate_edit for fixed-length queries qbytes[i*m : (i+1)*m] (sas_locate_edit_fixed)."""
        return self._locate_mismatch("sas_locate_edit", _queries(qbytes, None, None, m, stream, u32, "locate_edit"), k,
                                     max_seed_hits, dist, out, capacity, flags)

    # -- alignment start and edit script of each reported end (sas_align_edit*)
    def _align_edit(self, q, k, off, end, flags):
        side, nq, lead, suffix = q
        if side.dev:
            dt = side.dtype("pos")
            if not (_is_cuda(off) and _is_cuda(end)) or off.dtype != side.dtype("u64") or end.dtype != dt:
                raise ValueError(f"align_edit: off must be a CUDA int64 tensor and end a CUDA {dt} tensor")
            off, end = off.contiguous(), end.contiguous()
        else:
            off, end = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(end, side.dtype("pos"))
        na = side.count(end)
        # an alignment past off[nq] is not written: it reads as "none"
        start, dist = side.new("pos", na, self.n), side.new("u8", na, _lib.SAS_AL_NONE_DIST)
        nruns, runs = side.new("u8", na, 0), side.new("u16", (na, _run_cols(k)), 0)
        check(getattr(lib(), "sas_align_edit" + suffix)(self._h, *lead, int(k), _ptr(off), _ptr(end), na, _ptr(start),
                                                        _ptr(dist), _ptr(nruns), _ptr(runs), side.stream,
                                                        flags | side.flags))
        return start, dist, nruns, runs

    def align_edit(self, qbytes, qoff, qlen, k: int, off, end, u32: bool = False, flags: int = 0, stream=None):
        """Where each reported end's alignment starts, and its edit script (sas_align_edit):
        (start, dist, nruns, runs) for the ends end[off[i] : off[i + 1]] of the ragged queries
        qbytes[qoff[i] : qoff[i] + qlen[i]], as locate_edit returned them (u32: end and start hold
        32-bit positions).  start[a] is the largest s with ed(query, t[s : end[a]]) = dist[a], the
        least distance of any start; runs[a, :nruns[a]] is the run-length encoded script from
        (0, s), each run (len << 2) | op with op one of SAS_AL_EQ, SAS_AL_X, SAS_AL_INS (a query
        char that the text lacks) and SAS_AL_DEL (a text char that the query lacks); runs has
        2k + 1 columns, the unused ones 0 (sas_amd.cigar prints a row).  An end without an
        alignment within k has start = n, dist = 255 and nruns = 0.  numpy in -> numpy out; torch
        CUDA in -> CUDA out (runs as int16), asynchronous on the stream, no host read."""
        return self._align_edit(_queries(qbytes, qoff, qlen, 0, stream, u32), k, off, end, flags)

    def align_edit_fixed(self, qbytes, m: int, k: int, off, end, u32: bool = False, flags: int = 0, stream=None):
        """align_edit for fixed-length queries qbytes[i*m : (i+1)*m] (sas_align_edit_fixed)."""
        return self._align_edit(_queries(qbytes, None, None, m, stream, u32, "align_edit"), k, off, end, flags)

    # -- read mapping: the best alignment per read on both strands (sas_map_edit*)
    def _map(self, rec, fn, q, args, k_runs, flags):
        """One mapping call: the record `rec` of outputs with scripts of up to k_runs edits, the entry
        point fn (+ "_fixed") and its scalar arguments between the queries and the outputs."""
        side, nq, lead, suffix = q
        r = _record(rec, side, nq, k_runs)
        check(getattr(lib(), fn + suffix)(self._h, *lead, *map(int, args), *map(_ptr, r), side.stream,
                                          flags | side.flags))
        return r

    def map_edit(self, qbytes, qoff, qlen, k: int, max_seed_hits: int = 0, strands: int = 3, u32: bool = False,
                 flags: int = 0, stream=None):
        """Read mapping (sas_map_edit): one record per ragged read qbytes[qoff[i] : qoff[i] + qlen[i]],
        the named tuple Mapped(end, start, dist, strand, n_best, n_loci, nruns, runs, qflags).  Over
        the ends locate_edit defines for the read (strand 0) and for its reverse complement (strand 1)
        at the same k and max_seed_hits, the best is the least (dist, strand, end); the strand-1
        alignment is that of the reverse complement against t[start : end].  n_best counts the
        maximal runs of consecutive ends at the best distance, n_loci those of any distance <= k,
        both summed over the strands (n_best == 1 and n_loci == 1: the unique mapping); start, nruns
        and runs (2k + 1 columns) are align_edit's for the winner; qflags is the OR of the strands'
        SAS_ED_* flags.  strands: 1 forward only, 2 reverse only, 3 both.  An unmapped read has
        end = start = n, dist = 255, strand = 0 and zero counts and runs.  numpy in -> numpy out;
        torch CUDA in -> CUDA out (n_best / n_loci as int32, runs as int16 bit patterns)."""
        return self._map(Mapped, "sas_map_edit", _queries(qbytes, qoff, qlen, 0, stream, u32),
                         (k, max_seed_hits, strands), k, flags)

    def map_edit_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, strands: int = 3, u32: bool = False,
                       flags: int = 0, stream=None):
        """map_edit for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_edit_fixed)."""
        return self._map(Mapped, "sas_map_edit", _queries(qbytes, None, None, m, stream, u32, "map_edit"),
                         (k, max_seed_hits, strands), k, flags)

    # -- paired-end mapping: the mates of a pair placed together (sas_map_pairs*)
    def map_pairs(self, qbytes, qoff, qlen, k: int, min_frag: int, max_frag: int, max_seed_hits: int = 0,
                  u32: bool = False, flags: int = 0, stream=None):
        """Paired-end mapping (sas_map_pairs): the ragged reads come interleaved, pair i = reads 2i
        (mate 1) and 2i + 1 (mate 2); an odd number of reads raises ValueError.  Returns the named
        tuple MappedPairs(end, start, dist, strand, n_best, n_loci, nruns, runs, qflags, pflags,
        n_pairs, n_best_pairs): the first nine as map_edit's, one entry per read, the last three one
        entry per pair.  A candidate is a locus (a maximal run of consecutive ends, represented by
        its least (dist, end)) of one mate on the forward strand with one of the other mate on the
        reverse strand; it is proper when min_frag <= e_rev - e_fwd + len(forward mate) <= max_frag
        (max_frag - min_frag <= 65535).  n_pairs counts the proper candidates, n_best_pairs those of
        the least summed distance, pflags bit 0 (SAS_PAIR_PROPER) says there is one.  In a proper
        pair both reads get the best candidate's ends (the least (sum, orientation, forward end,
        reverse end)), strands 0 / 1 and align_edit's start and runs for them; otherwise each read
        keeps map_edit's own record.  n_best, n_loci and qflags are always map_edit's.  numpy in ->
        numpy out; torch CUDA in -> CUDA out (counts as int32, runs as int16 bit patterns)."""
        return self._map(MappedPairs, "sas_map_pairs", _queries(qbytes, qoff, qlen, 0, stream, u32, pairs=True),
                         (k, max_seed_hits, min_frag, max_frag), k, flags)

    def map_pairs_fixed(self, qbytes, m: int, k: int, min_frag: int, max_frag: int, max_seed_hits: int = 0,
                        u32: bool = False, flags: int = 0, stream=None):
        """map_pairs for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_pairs_fixed)."""
        return self._map(MappedPairs, "sas_map_pairs",
                         _queries(qbytes, None, None, m, stream, u32, "map_pairs", pairs=True),
                         (k, max_seed_hits, min_frag, max_frag), k, flags)

    # -- paired-end mapping with mate rescue (sas_map_pairs_rescue*)
    def map_pairs_rescue(self, qbytes, qoff, qlen, k: int, k_rescue: int, min_frag: int, max_frag: int,
                         max_anchors: int, max_seed_hits: int = 0, u32: bool = False, flags: int = 0, stream=None):
        """map_pairs with mate rescue (sas_map_pairs_rescue).  A pair without a proper candidate and
        with 1 .. max_anchors loci over both mates and strands (max_anchors = 0: no rescue) has the
        fragment window of every locus scanned, with no seeds, for the other mate on the opposite
        strand within k_rescue >= k edits.  Returns the named tuple MappedPairsRescue: MappedPairs'
        fields and n_rescue, per pair the runs of candidate ends in its anchors' windows.  A rescued
        pair has SAS_PAIR_RESCUED in pflags, the anchor read its locus, the other read the best
        candidate's end, its distance (which may exceed k) and SAS_MAP_RESCUED in qflags; a pair
        with more than max_anchors loci has SAS_PAIR_RESCUE_SKIPPED.  runs has 2 k_rescue + 1 slots
        per read; everything else is map_pairs'."""
        return self._map(MappedPairsRescue, "sas_map_pairs_rescue",
                         _queries(qbytes, qoff, qlen, 0, stream, u32, pairs=True),
                         (k, k_rescue, max_seed_hits, min_frag, max_frag, max_anchors), k_rescue, flags)

    def map_pairs_rescue_fixed(self, qbytes, m: int, k: int, k_rescue: int, min_frag: int, max_frag: int,
                               max_anchors: int, max_seed_hits: int = 0, u32: bool = False, flags: int = 0,
                               stream=None):
        """map_pairs_rescue for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_pairs_rescue_fixed)."""
        return self._map(MappedPairsRescue, "sas_map_pairs_rescue",
                         _queries(qbytes, None, None, m, stream, u32, "map_pairs_rescue", pairs=True),
                         (k, k_rescue, max_seed_hits, min_frag, max_frag, max_anchors), k_rescue, flags)

    def time_fixed(self, d_qbytes, m: int, nq: int, d_out, algo="plain", reps=1, stream=None, flags=0):
        """Average (kernel_ns, call_ns) of `reps` back-to-back searches on device buffers."""
        kn, cn = C.c_double(0), C.c_double(0)
        check(lib().sas_time_fixed(self._h, _ptr(d_qbytes), m, nq, _lib.ALGOS[algo], _ptr(d_out), reps, stream,
                                   flags, C.byref(kn), C.byref(cn)))
        return kn.value, cn.value


def cigar(runs_row, nruns) -> str:
    """The script of one alignment of SaNaive.align_edit as a string such as "17=1X14=": the first
    `nruns` runs of the row, = a match, X a substitution, I a query char that the text lacks, D
    a text char that the query lacks."""
    row = runs_row.cpu().numpy() if hasattr(runs_row, "cpu") else np.asarray(runs_row)
    return "".join(f"{int(r) >> 2}{'=XID'[int(r) & 3]}" for r in row[:int(nruns)].astype(np.int64) & 0xFFFF)


def revcomp(qbytes, qoff=None, qlen=None, m: int | None = None, stream=None, flags: int = 0):
    """Reverse complements of DNA queries, rc(q)[j] = q[len - 1 - j] ^ 3 (sas_revcomp): for ragged
    queries qbytes[qoff[i] : qoff[i] + qlen[i]] (which may overlap) -> (bytes, off), the reverse
    complements back to back in query order and off = the exclusive sum of qlen (nq + 1 entries);
    with m, for fixed-length queries qbytes[i*m : (i+1)*m] -> bytes, query i at i*m
    (sas_revcomp_fixed).  numpy in -> numpy out (bytes validated); torch CUDA in -> CUDA out, on
    the current stream of the tensor's device."""
    side, nq, lead, suffix = _queries(qbytes, None if m is not None else qoff, qlen, m, stream,
                                      what="revcomp without m")
    with side.guard():
        if suffix:
            out = side.new("u8", nq * lead[1])
            check(lib().sas_revcomp_fixed(*lead, _ptr(out), side.stream, flags | side.flags))
            return out
        qlen = side.keep[2]
        total = (int(qlen.sum()) if nq else 0) if side.dev else int(qlen.astype(np.uint64).sum())
        out, off = side.new("u8", total), side.new("u64", nq + 1)
        check(lib().sas_revcomp(*lead, _ptr(out), _ptr(off), side.stream, flags | side.flags))
        return out, off


def binary_search(sa: SaNaive, q, cnt: Counter | None = None) -> int:
    """sas/sa_search.rs:98-112 -- position of the first suffix >= q (n if none)."""
    pos, pr = sa.search([q], algo="plain", probes=True)
    if cnt is not None:
        cnt.value += int(pr[0])
    return int(pos[0])


def binary_search_batch(sa: SaNaive, qs, cnt: Counter | None = None, algo: str = "plain") -> list[int]:
    """sas/sa_search.rs:157-196 -- B queries at once (any B; no remainder is dropped)."""
    pos, pr = sa.search(list(qs), algo=algo, probes=True)
    if cnt is not None:
        cnt.value += int(pr.sum())
    return [int(p) for p in pos]


# ---------------------------------------------------------------- generators
def random_string(n: int, seed: int = 31415, device=None):
    """sas/util.rs:9-15 with ChaCha8Rng::seed_from_u64(seed): bit-exact stream."""
    if device is not None:
        import torch
        out = torch.empty(n, dtype=torch.uint8, device=device)
        check(lib().sas_gen_text(seed, n, out.data_ptr(), _lib.SAS_DEVICE_PTRS))
        return out
    out = HOST.new("u8", n)
    check(lib().sas_gen_text(seed, n, _ptr(out), 0))
    return out


def random_queries(n: int, nq: int, seed: int = 31415, word_pos: int | None = None, margin: int = 200,
                   len_lo: int = 30, len_hi: int = 100):
    """sas/util.rs:18-26 -> (offsets u64, lengths u32, next keystream word).  The
    stream continues after the text's n words unless word_pos is given."""
    off, ln = HOST.new("u64", nq), HOST.new("u32", nq)
    nxt = C.c_uint64(0)
    check(lib().sas_gen_queries(seed, n if word_pos is None else word_pos, n, nq, margin, len_lo, len_hi,
                                _ptr(off), _ptr(ln), C.byref(nxt)))
    return off, ln, nxt.value


# ---------------------------------------------------------------- real data
def read_fasta_file(path: str) -> np.ndarray:
    """sas/util.rs:144-169: concatenated record sequences as codes 0..3 (others -> 0)."""
    n = C.c_uint64(0)
    check(lib().sas_read_fasta(path.encode(), None, 0, C.byref(n)))
    out = HOST.new("u8", n.value)
    check(lib().sas_read_fasta(path.encode(), _ptr(out), n.value, C.byref(n)))
    return out


# sas_amd.read_fasta_layout: the text, and what SaNaive.set_layout takes
FastaLayout = namedtuple("FastaLayout", "text seq_start seg_lo seg_hi names")


def read_fasta_layout(path: str) -> FastaLayout:
    """sas_read_fasta_layout: read_fasta_file's bytes, the start of every record (seq_start, one
    more entry than records), the maximal runs of ACGTacgt as segments [seg_lo, seg_hi) and the
    first word of every header."""
    L = lib()
    n, nseq, nseg, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    p = path.encode()
    check(L.sas_read_fasta_layout(p, None, 0, C.byref(n), None, 0, C.byref(nseq), None, None, 0, C.byref(nseg),
                                  None, 0, C.byref(nl)))
    out, starts = HOST.new("u8", n.value), HOST.new("u64", nseq.value + 1)
    lo, hi = HOST.new("u64", nseg.value), HOST.new("u64", nseg.value)
    names = C.create_string_buffer(max(nl.value, 1))
    check(L.sas_read_fasta_layout(p, _ptr(out), n.value, C.byref(n), _ptr(starts), len(starts), C.byref(nseq),
                                  _ptr(lo), _ptr(hi), nseg.value, C.byref(nseg), C.cast(names, C.c_void_p), nl.value,
                                  C.byref(nl)))
    words = names.raw[: nl.value].split(b"\0")[:-1] if nl.value else []
    return FastaLayout(out, starts, lo, hi, [w.decode() for w in words])


def _u64(x):
    return np.ascontiguousarray(x, np.uint64)


def check_layout(n: int, seq_start, seg_lo, seg_hi) -> None:
    """sas_check_layout (no device call): raises SasError (EINVAL) naming the entry that breaks a
    rule of sas.h's sequence layout."""
    s, lo, hi = _u64(seq_start), _u64(seg_lo), _u64(seg_hi)
    if len(lo) != len(hi):
        raise ValueError("seg_lo and seg_hi differ in length")
    check(lib().sas_check_layout(int(n), s.ctypes.data if len(s) else None, max(len(s), 1) - 1,
                                 lo.ctypes.data if len(lo) else None, hi.ctypes.data if len(hi) else None, len(lo)))


def kmer_keys(t, k: int = 16, limit: int | None = None) -> np.ndarray:
    """sst/bin/bench.rs:58-76 (--human): u32 k-mer keys & i32::MAX, vals[0] = MAX."""
    t = _as_u8(t)
    n = len(t)
    limit = n if limit is None else limit
    cnt = C.c_uint64(0)
    check(lib().sas_kmer_keys(_ptr(t), n, k, limit, None, C.byref(cnt), 0))
    out = HOST.new("u32", cnt.value)
    check(lib().sas_kmer_keys(_ptr(t), n, k, limit, _ptr(out), C.byref(cnt), 0))
    return out
