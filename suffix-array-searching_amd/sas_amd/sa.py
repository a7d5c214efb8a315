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
import errno
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, lib


@dataclass
class Counter:
    """Stands in for the reference's `cnt: &mut usize` argument."""
    value: int = 0


# one record per read of SaNaive.map_edit (sas_map_edit)
Mapped = namedtuple("Mapped", "end start dist strand n_best n_loci nruns runs qflags")
# SaNaive.map_pairs (sas_map_pairs): Mapped's fields per read, then three per pair
MappedPairs = namedtuple("MappedPairs", Mapped._fields + ("pflags", "n_pairs", "n_best_pairs"))
# SaNaive.map_pairs_rescue (sas_map_pairs_rescue): MappedPairs' fields, then one more per pair
MappedPairsRescue = namedtuple("MappedPairsRescue", MappedPairs._fields + ("n_rescue",))


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _ptr(x):
    if x is None:
        return None
    if _is_cuda(x) or hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data


def _as_u8(x):
    if _is_cuda(x):
        return x
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, np.uint8)


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
        n = int(t.numel() if _is_cuda(t) else len(t))
        if tagged is not False:
            stree, sector, quad, prefix = bool(stree), bool(sector), quad or False, prefix or False
            llcp = bool(llcp)
            flags |= _lib.SAS_BUILD_TAGGED | (0 if tagged is True else _lib.SAS_BUILD_PREFIX_P(int(tagged)))
            flags |= _lib.SAS_BUILD_TAG_LINES if tag_lines else 0
            lcp = lcp and not tag_lines  # a bucket-line index serves TAGGED only: no LCP array
        stree = True if stree is None else stree
        sector = True if sector is None else sector
        quad = True if quad is None else quad
        flags |= (_lib.SAS_BUILD_LCP if lcp else 0) | (_lib.SAS_BUILD_STREE if stree else 0)
        if llcp is None:
            llcp = n < (1 << 31)
        flags |= _lib.SAS_BUILD_LLCP if llcp else 0
        flags |= (_lib.SAS_BUILD_VERIFY if verify else 0) | (_lib.SAS_BUILD_SECTOR if sector else 0)
        flags |= _lib.SAS_BUILD_SA40 if sa40 else 0
        flags |= _lib.SAS_BUILD_TOP2_LEVELS(top2_levels)
        flags |= _quad_flags(quad) | _prefix_flags(prefix, quad, n if rank_range is None else rank_range[1] - rank_range[0],
                                                   prefix_inline)
        sa_ptr, sa_w = None, 4
        if sa is not None:
            if _is_cuda(t) != _is_cuda(sa):
                raise ValueError("text and sa must both be host or both be device arrays")
            if not _is_cuda(sa):
                sa = np.asarray(sa)
                sa = np.ascontiguousarray(sa, np.uint64 if sa.dtype.itemsize == 8 else np.uint32)
                sa_w = sa.dtype.itemsize
            else:
                sa_w = sa.element_size()
            sa_ptr = _ptr(sa)
        if _is_cuda(t):
            flags |= _lib.SAS_DEVICE_PTRS
        h = C.c_void_p()
        if rank_range is None:
            check(lib().sas_build(_ptr(t), n, sa_ptr, sa_w, flags, C.byref(h)))
        else:
            check(lib().sas_build_shard(_ptr(t), n, sa_ptr, sa_w, int(rank_range[0]), int(rank_range[1]), flags,
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
        n = int(t.numel() if _is_cuda(t) else len(t))
        flags |= (_lib.SAS_BUILD_LCP if lcp else 0) | (_lib.SAS_BUILD_STREE if stree else 0)
        flags |= (_lib.SAS_BUILD_VERIFY if verify else 0) | (_lib.SAS_BUILD_SECTOR if sector else 0)
        llcp = (n < (1 << 31)) if llcp is None else llcp
        flags |= _quad_flags(quad) | (_lib.SAS_BUILD_LLCP if llcp else 0) | _prefix_flags(prefix, quad, n, prefix_inline)
        flags |= _lib.SAS_BUILD_TOP2_LEVELS(top2_levels)
        if _is_cuda(t):
            flags |= _lib.SAS_DEVICE_PTRS
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
        lcp, stree = kw.pop("lcp", True), kw.pop("stree", True)
        sector, quad = kw.pop("sector", True), kw.pop("quad", True)
        verify, top2 = kw.pop("verify", False), kw.pop("top2_levels", 0)
        prefix, inline = kw.pop("prefix", None), kw.pop("prefix_inline", False)
        llcp = kw.pop("llcp", None)
        if kw:
            raise TypeError(f"build_gen: unexpected {sorted(kw)}")
        llcp = (n < (1 << 31)) if llcp is None else llcp
        flags |= (_lib.SAS_BUILD_LCP if lcp else 0) | (_lib.SAS_BUILD_STREE if stree else 0)
        flags |= (_lib.SAS_BUILD_VERIFY if verify else 0) | (_lib.SAS_BUILD_SECTOR if sector else 0)
        flags |= _quad_flags(quad) | (_lib.SAS_BUILD_LLCP if llcp else 0) | _prefix_flags(prefix, quad, n, inline)
        flags |= _lib.SAS_BUILD_TOP2_LEVELS(top2)
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
            out = np.zeros(max(count, 1), np.uint32)
            check(lib().sas_copy_sa(self._h, out.ctypes.data, count, 0))
            return out[:count]
        out = np.zeros(max(count, 1), np.uint64)
        check(lib().sas_copy_sa64(self._h, self.rank_lo + start, count, out.ctypes.data, 0))
        return out[:count]

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
        s = np.zeros(nseq.value + 1, np.uint64)
        lo, hi = np.zeros(max(nseg.value, 1), np.uint64), np.zeros(max(nseg.value, 1), np.uint64)
        check(lib().sas_get_layout(self._h, None, None, s.ctypes.data, lo.ctypes.data, hi.ctypes.data))
        return s, lo[: nseg.value], hi[: nseg.value]

    def translate(self, pos, span=None, u32: bool = False, stream=None):
        """Text positions to (sequence id, offset in it) (sas_translate): the id is SAS_SEQ_NONE, and
        the offset the position itself, unless [pos, pos + span) (span None: 1) lies inside one
        segment.  torch CUDA tensors (pos int64, or int32 with u32; span int32) -> CUDA tensors
        (int32 ids holding the u32 bits, offsets in pos's dtype), asynchronous; numpy -> numpy."""
        L = lib()
        if _is_cuda(pos):
            import torch
            dt = torch.int32 if u32 else torch.int64
            if pos.dtype != dt or (span is not None and (not _is_cuda(span) or span.dtype != torch.int32)):
                raise ValueError(f"translate: pos must be a CUDA {dt} tensor and span a CUDA int32 tensor")
            pos = pos.contiguous()
            span = None if span is None else span.contiguous()
            cnt = int(pos.numel())
            if span is not None and int(span.numel()) != cnt:
                raise ValueError("translate: one span per position")
            seq = torch.empty(cnt, dtype=torch.int32, device=pos.device)
            off = torch.empty(cnt, dtype=dt, device=pos.device)
            st = stream if stream is not None else torch.cuda.current_stream(pos.device).cuda_stream
            check(L.sas_translate(self._h, _ptr(pos), _ptr(span), cnt, _ptr(seq), _ptr(off), st,
                                  _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)))
            return seq, off
        pos = np.ascontiguousarray(pos, np.uint32 if u32 else np.uint64)
        span = None if span is None else np.ascontiguousarray(span, np.uint32)
        if span is not None and len(span) != len(pos):
            raise ValueError("translate: one span per position")
        seq = np.zeros(len(pos), np.uint32)
        off = np.zeros(len(pos), pos.dtype)
        check(L.sas_translate(self._h, _ptr(pos), _ptr(span), len(pos), _ptr(seq), _ptr(off), stream,
                              _lib.SAS_LOCATE_U32 if u32 else 0))
        return seq, off

    def lcp_array(self) -> np.ndarray:
        out = np.zeros(self.sa_n, np.uint32)
        check(lib().sas_copy_lcp(self._h, out.ctypes.data, self.sa_n, 0))
        return out

    def extract(self, pos, lens, out_off, out, stream=None):
        """Text substrings as byte codes from the index's packed text (sas_extract):
        out[out_off[i] : out_off[i] + lens[i]] = text[pos[i] : pos[i] + lens[i]].
        torch CUDA tensors (int64 pos / out_off, int32 lens, uint8 out), async."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
        check(lib().sas_extract(self._h, _ptr(pos), _ptr(lens), _ptr(out_off), int(pos.numel()), _ptr(out), st,
                                _lib.SAS_DEVICE_PTRS))
        return out

    @staticmethod
    def pack_queries(qbytes, m: int, stream=None):
        """2-bit packed fixed-length queries (sas_pack_queries; m <= 32): torch CUDA
        uint8 in -> torch CUDA int64 words out (first char in bits 63..62); numpy uint8 in
        -> numpy uint64 out, packed on the host."""
        if not _is_cuda(qbytes):
            qbytes = _as_u8(qbytes)
            nq = len(qbytes) // m if m else 0
            out = np.zeros(max(nq, 1), np.uint64)
            check(lib().sas_pack_queries(_ptr(qbytes), m, nq, _ptr(out), None, 0))
            return out[:nq]
        import torch
        nq = qbytes.numel() // m if m else 0
        out = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
        st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
        check(lib().sas_pack_queries(_ptr(qbytes), m, nq, _ptr(out), st, _lib.SAS_DEVICE_PTRS))
        return out

    def search_packed(self, qwords, m: int, algo: str = "prefix", probes: bool = False, out=None, stream=None):
        """Lookups of packed fixed-length queries (sas_search_packed): numpy uint64 in ->
        numpy out; torch CUDA in -> torch CUDA out (async)."""
        if _is_cuda(qwords):
            import torch
            nq = qwords.numel()
            out = torch.empty(nq, dtype=torch.int64, device=qwords.device) if out is None else out
            pr = torch.empty(nq, dtype=torch.int32, device=qwords.device) if probes else None
            st = stream if stream is not None else torch.cuda.current_stream(qwords.device).cuda_stream
            check(lib().sas_search_packed(self._h, _ptr(qwords), m, nq, _lib.ALGOS[algo], _ptr(out),
                                          _ptr(pr) if probes else None, st, _lib.SAS_DEVICE_PTRS))
            return (out, pr) if probes else out
        qwords = np.ascontiguousarray(qwords, np.uint64)
        nq = len(qwords)
        out = np.zeros(max(nq, 1), np.uint64)
        pr = np.zeros(max(nq, 1), np.uint32) if probes else None
        check(lib().sas_search_packed(self._h, qwords.ctypes.data, m, nq, _lib.ALGOS[algo], out.ctypes.data,
                                      pr.ctypes.data if probes else None, None, 0))
        return (out[:nq], pr[:nq]) if probes else out[:nq]

    def search_buckets(self, queries, m: int, cap: int, counts, algo: str = "prefix", out=None, stream=None):
        """The sharded step's local lookup (sas_search_buckets): `queries` holds
        counts.numel() buckets of `cap` slots (uint8, m bytes a slot, or int64 2-bit words
        for PREFIX with m <= 32), bucket b's first counts[b] slots are queries; only those
        are searched and written into `out` (int64, one per slot).  torch CUDA tensors."""
        import torch
        dev = queries.device
        for name, tns in (("queries", queries), ("counts", counts)) + ((("out", out),) if out is not None else ()):
            if not tns.is_cuda or tns.device != dev:
                raise ValueError(f"search_buckets: {name} must be a CUDA tensor on {dev}, not {tns.device}")
        nb = int(counts.numel())
        packed = queries.dtype == torch.int64
        need = nb * cap * (1 if packed else m)
        if counts.dtype != torch.int64 or not counts.is_contiguous() or queries.numel() < need or \
                not queries.is_contiguous() or (not packed and queries.dtype != torch.uint8):
            raise ValueError("search_buckets: int64 counts, and uint8 bytes or int64 words for every slot")
        if out is None:
            out = torch.empty(nb * cap, dtype=torch.int64, device=queries.device)
        if out.dtype != torch.int64 or out.numel() < nb * cap:
            raise ValueError("search_buckets: int64 out of one entry per slot")
        st = stream if stream is not None else torch.cuda.current_stream(queries.device).cuda_stream
        fl = _lib.SAS_DEVICE_PTRS | (_lib.SAS_ROUTE_PACKED if packed else 0)
        check(lib().sas_search_buckets(self._h, _ptr(queries), m, nb, int(cap), _ptr(counts), _lib.ALGOS[algo],
                                       _ptr(out), st, fl))
        return out

    def route(self, splitter_pos, qbytes, m: int, stream=None):
        """Sharded mode: shard id of each fixed-length query = number of splitter
        suffixes < q (sas_route).  numpy in -> numpy out; CUDA in -> CUDA out."""
        if _is_cuda(qbytes):
            import torch
            nq = qbytes.numel() // m
            out = torch.empty(nq, dtype=torch.int32, device=qbytes.device)
            st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
            check(lib().sas_route(self._h, splitter_pos.data_ptr(), splitter_pos.numel(), qbytes.data_ptr(), m, nq,
                                  out.data_ptr(), st, _lib.SAS_DEVICE_PTRS))
            return out
        qbytes = _as_u8(qbytes)
        sp = np.ascontiguousarray(splitter_pos, np.uint64)
        nq = len(qbytes) // m
        out = np.zeros(max(nq, 1), np.uint32)
        check(lib().sas_route(self._h, sp.ctypes.data if len(sp) else None, len(sp), qbytes.ctypes.data, m, nq,
                              out.ctypes.data, stream, 0))
        return out[:nq]

    def route_pack(self, splitter_pos, qbytes, m: int, stream=None, cap: int | None = None, send=None,
                   packed: bool = False):
        """Send side of one sharded step, fused on the GPU (sas_route_pack): CUDA
        tensors in -> (counts int64 [W], send uint8 [nq*m] grouped by shard,
        slot int64 [nq] = send position of each query).  cap: fixed-capacity buckets
        (sas_route_pack_cap): send holds W*cap slots, bucket w at slots [w*cap, ...), and
        counts > cap on the device marks an overflow.  packed (m <= 32, SAS_ROUTE_PACKED):
        each slot is the query's 8-B 2-bit word (send is int64) instead of its m bytes.
        `send` may be passed in (reused)."""
        import torch
        nq = qbytes.numel() // m
        W = splitter_pos.numel() + 1
        counts = torch.empty(W, dtype=torch.int64, device=qbytes.device)
        slots = W * cap if cap else nq
        size = slots if packed else slots * m
        dt = torch.int64 if packed else torch.uint8
        if send is None or send.numel() < max(size, 1) or send.dtype != dt:
            send = torch.zeros(max(size, 1), dtype=dt, device=qbytes.device)
        slot = torch.empty(max(nq, 1), dtype=torch.int64, device=qbytes.device)
        st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
        sp = splitter_pos.data_ptr() if W > 1 else None
        fl = _lib.SAS_DEVICE_PTRS | (_lib.SAS_ROUTE_PACKED if packed else 0)
        if cap:
            check(lib().sas_route_pack_cap(self._h, sp, W - 1, qbytes.data_ptr(), m, nq, int(cap), counts.data_ptr(),
                                           send.data_ptr(), slot.data_ptr(), st, fl))
        else:
            check(lib().sas_route_pack(self._h, sp, W - 1, qbytes.data_ptr(), m, nq, counts.data_ptr(),
                                       send.data_ptr(), slot.data_ptr(), st, fl))
        return counts, send[:size], slot[:nq]

    def shard_gather(self, back, slot, out=None, counts=None, cap: int = 0, overflow=None, stream=None):
        """Receive side of one sharded step (sas_shard_gather): out[k] = back[slot[k]]; with
        `overflow` (an int32 CUDA tensor of 1, never cleared here) it is set to 1 when some
        counts[w] > cap."""
        import torch
        nq = slot.numel()
        if out is None:
            out = torch.empty(nq, dtype=torch.int64, device=slot.device)
        if out.numel() < nq or out.dtype != torch.int64 or back.dtype != torch.int64 or slot.dtype != torch.int64:
            raise ValueError("shard_gather: int64 back/slot/out, out of at least len(slot)")
        if overflow is not None and (counts is None or overflow.dtype != torch.int32):
            raise ValueError("shard_gather: overflow needs counts and an int32 flag")
        st = stream if stream is not None else torch.cuda.current_stream(slot.device).cuda_stream
        check(lib().sas_shard_gather(self._h, back.data_ptr(), slot.data_ptr(), nq,
                                     counts.data_ptr() if counts is not None else None,
                                     counts.numel() if counts is not None else 0, int(cap), out.data_ptr(),
                                     overflow.data_ptr() if overflow is not None else None, st,
                                     _lib.SAS_DEVICE_PTRS))
        return out[:nq]

    def verify(self):
        check(lib().sas_verify(self._h))

    # -- searching
    def search_fixed(self, qbytes, m: int, algo: str = "plain", probes: bool = False, stream=None,
                     out=None, flags: int = 0):
        """Fixed-length queries, query k = qbytes[k*m:(k+1)*m].  Host numpy in ->
        numpy out (synchronous); torch CUDA in -> CUDA out (async on `stream`)."""
        dev = _is_cuda(qbytes)
        nq = (qbytes.numel() if dev else len(qbytes)) // max(m, 1) if m else 0
        if m == 0:
            raise ValueError("use search_batch for empty queries")
        return self._run(qbytes, None, None, m, nq, algo, probes, stream, out, flags, dev)

    def search_batch(self, qbytes, qoff, qlen, algo: str = "plain", probes: bool = False, stream=None,
                     out=None, flags: int = 0):
        """Ragged queries, query k = qbytes[qoff[k] : qoff[k] + qlen[k]]."""
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._run(qbytes, qoff, qlen, 0, nq, algo, probes, stream, out, flags, dev)

    def search_slices(self, qoff, qlen, algo: str = "tagged", probes: bool = False, stream=None, out=None,
                      flags: int = 0):
        """Queries that are slices of the indexed text, t[qoff[k] : qoff[k] + qlen[k]] (the
        reference's borrowed &t[i..i+len] queries; SAS_QUERIES_ARE_SLICES): torch CUDA int64
        offsets / int32 lengths in, no query bytes -> torch CUDA positions out."""
        import torch
        if not (_is_cuda(qoff) and _is_cuda(qlen)):
            raise ValueError("search_slices: torch CUDA qoff / qlen")
        if qoff.dtype != torch.int64 or qlen.dtype != torch.int32 or not qoff.is_contiguous() or \
                not qlen.is_contiguous() or qoff.numel() != qlen.numel():
            raise ValueError("search_slices: contiguous int64 qoff and int32 qlen of the same length")
        nq = int(qoff.numel())
        if out is None:
            out = torch.empty(nq, dtype=torch.int64, device=qoff.device)
        pr = torch.empty(nq, dtype=torch.int32, device=qoff.device) if probes else None
        st = stream if stream is not None else torch.cuda.current_stream(qoff.device).cuda_stream
        check(lib().sas_search_batch(self._h, None, _ptr(qoff), _ptr(qlen), nq, _lib.ALGOS[algo], _ptr(out),
                                     _ptr(pr), st, flags | _lib.SAS_DEVICE_PTRS | _lib.SAS_QUERIES_ARE_SLICES))
        return (out, pr) if probes else out

    def _run(self, qbytes, qoff, qlen, m, nq, algo, probes, stream, out, flags, dev):
        a = _lib.ALGOS[algo]
        if dev:
            import torch
            if out is None:
                out = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
            pr = torch.empty(nq, dtype=torch.int32, device=qbytes.device) if probes else None
            st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
            flags |= _lib.SAS_DEVICE_PTRS
        else:
            qbytes = _as_u8(qbytes)
            if out is None:
                out = np.zeros(max(nq, 1), np.uint64)
            elif not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous
                      and len(out) >= nq):
                raise ValueError("out: a C-contiguous numpy uint64 array of at least nq entries")
            pr = np.zeros(max(nq, 1), np.uint32) if probes else None
            st = stream
        if qoff is None:
            rc = lib().sas_search_fixed(self._h, _ptr(qbytes), m, nq, a, _ptr(out), _ptr(pr), st, flags)
        else:
            rc = lib().sas_search_batch(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, a, _ptr(out), _ptr(pr),
                                        st, flags)
        check(rc)
        if not dev:
            out, pr = out[:nq], (pr[:nq] if pr is not None else None)
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
        dev = _is_cuda(qbytes)
        if dev:
            import torch
            nq = qoff.numel()
            lo = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
            hi = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
            st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
            flags |= _lib.SAS_DEVICE_PTRS
        else:
            qbytes = _as_u8(qbytes)
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
            nq = len(qoff)
            lo = np.zeros(max(nq, 1), np.uint64)
            hi = np.zeros(max(nq, 1), np.uint64)
            st = stream
        check(lib().sas_search_range(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, _ptr(lo), _ptr(hi), st,
                                     flags))
        return (lo, hi) if dev else (lo[:nq], hi[:nq])

    def search_range_fixed(self, qbytes, m: int, stream=None, flags: int = 0):
        """search_range for fixed-length queries qbytes[k*m .. (k+1)*m) (sas_search_range_fixed)."""
        dev = _is_cuda(qbytes)
        nq = qbytes.numel() // m if dev else len(qbytes) // m
        if dev:
            import torch
            lo = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
            hi = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
            st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
            flags |= _lib.SAS_DEVICE_PTRS
        else:
            qbytes = _as_u8(qbytes)
            lo = np.zeros(max(nq, 1), np.uint64)
            hi = np.zeros(max(nq, 1), np.uint64)
            st = stream
        check(lib().sas_search_range_fixed(self._h, _ptr(qbytes), m, nq, _ptr(lo), _ptr(hi), st, flags))
        return (lo, hi) if dev else (lo[:nq], hi[:nq])

    def search_prefix(self, q) -> np.ndarray:
        """All text positions where q occurs (Search::search_prefix, sas/util.rs:36-40)."""
        q = _as_u8(q)
        buf = np.concatenate([q, np.zeros(64, np.uint8)])
        lo, hi = self.search_range(buf, np.zeros(1, np.uint64), np.array([len(q)], np.uint32))
        cnt = int(hi[0] - lo[0])
        if self.stats()["sa_width"] != 4:
            out = np.zeros(max(cnt, 1), np.uint64)
            check(lib().sas_copy_sa64(self._h, int(lo[0]), cnt, out.ctypes.data, 0))
            return out[:cnt]
        out = np.zeros(max(cnt, 1), np.uint32)
        check(lib().sas_copy_sa_range(self._h, int(lo[0]), cnt, out.ctypes.data, 0))
        return out[:cnt]

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
        import torch
        if not (_is_cuda(lo) and _is_cuda(hi)) or lo.dtype != torch.int64 or hi.dtype != torch.int64 or \
                lo.numel() != hi.numel() or not lo.is_contiguous() or not hi.is_contiguous():
            raise ValueError("locate_ranges: contiguous torch CUDA int64 lo and hi of the same length")
        nq = int(lo.numel())
        dt = torch.int32 if u32 else torch.int64
        fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
        st = stream if stream is not None else torch.cuda.current_stream(lo.device).cuda_stream
        off = torch.empty(nq + 1, dtype=torch.int64, device=lo.device)
        check(lib().sas_locate_offsets(self._h, _ptr(lo), _ptr(hi), nq, int(max_per_query), _ptr(off), st,
                                       _lib.SAS_DEVICE_PTRS))
        total = None
        if out is None:
            if capacity is None:
                capacity = total = int(off[nq].item())
            out = torch.empty(max(int(capacity), 1), dtype=dt, device=lo.device)
        else:
            if not _is_cuda(out) or out.dtype != dt or not out.is_contiguous():
                raise ValueError(f"locate_ranges: out must be a contiguous CUDA {dt} tensor")
            capacity = out.numel() if capacity is None else capacity
            if capacity > out.numel():
                raise ValueError("locate_ranges: capacity exceeds out")
        check(lib().sas_locate_fill(self._h, _ptr(lo), _ptr(off), nq, _ptr(out), int(capacity), st, fl))
        return off, (out[:total] if total is not None else out)

    def _locate(self, qbytes, qoff, qlen, m, nq, max_per_query, u32, stream, out, capacity, flags):
        if _is_cuda(qbytes):
            import torch
            if out is None and capacity is None:  # ranges, offsets, one read of the total, fill
                lo, hi = (self.search_range(qbytes, qoff, qlen, stream=stream, flags=flags) if qoff is not None
                          else self.search_range_fixed(qbytes, m, stream=stream, flags=flags))
                return self.locate_ranges(lo, hi, max_per_query, u32=u32, stream=stream,
                                          flags=flags & _lib.SAS_LOCATE_NO_PARTITION)
            dt = torch.int32 if u32 else torch.int64
            if out is None:
                out = torch.empty(max(int(capacity), 1), dtype=dt, device=qbytes.device)
            elif not _is_cuda(out) or out.dtype != dt or not out.is_contiguous():
                raise ValueError(f"locate: out must be a contiguous CUDA {dt} tensor")
            capacity = out.numel() if capacity is None else capacity
            if capacity > out.numel():
                raise ValueError("locate: capacity exceeds out")
            off = torch.empty(nq + 1, dtype=torch.int64, device=qbytes.device)
            st = stream if stream is not None else torch.cuda.current_stream(qbytes.device).cuda_stream
            fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
            if qoff is not None:
                rc = lib().sas_locate(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, int(max_per_query),
                                      _ptr(off), _ptr(out), int(capacity), None, st, fl)
            else:
                rc = lib().sas_locate_fixed(self._h, _ptr(qbytes), m, nq, int(max_per_query), _ptr(off), _ptr(out),
                                            int(capacity), None, st, fl)
            check(rc)
            return off, out
        qbytes = _as_u8(qbytes)
        fl = flags | (_lib.SAS_LOCATE_U32 if u32 else 0)
        off = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)

        def call(pos, cap):
            if qoff is not None:
                return lib().sas_locate(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, int(max_per_query),
                                        _ptr(off), _ptr(pos), cap, C.byref(total), stream, fl)
            return lib().sas_locate_fixed(self._h, _ptr(qbytes), m, nq, int(max_per_query), _ptr(off), _ptr(pos),
                                          cap, C.byref(total), stream, fl)

        rc = call(None, 0)  # the sizing call: ENOSPC unless nothing occurs
        if rc not in (0, errno.ENOSPC):
            check(rc)
        pos = np.zeros(max(total.value, 1), np.uint32 if u32 else np.uint64)
        if total.value:
            check(call(pos, total.value))
        return off, pos[:total.value]

    def locate(self, qbytes, qoff, qlen, max_per_query: int = 0, u32: bool = False, stream=None, out=None,
               capacity: int | None = None, flags: int = 0):
        """Every occurrence position of every ragged query qbytes[qoff[k] : qoff[k] + qlen[k]]
        in one call (sas_locate): (off, pos) in CSR form as locate_ranges gives them.  numpy in
        -> numpy out (a sizing call, then the real one); torch CUDA in -> CUDA out, async when
        out / capacity is given (otherwise the total is read back once)."""
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._locate(qbytes, qoff, qlen, 0, nq, max_per_query, u32, stream, out, capacity, flags)

    def locate_fixed(self, qbytes, m: int, max_per_query: int = 0, u32: bool = False, stream=None, out=None,
                     capacity: int | None = None, flags: int = 0):
        """locate for fixed-length queries qbytes[k*m : (k+1)*m] (sas_locate_fixed)."""
        if m <= 0:
            raise ValueError("use locate for empty queries")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._locate(qbytes, None, None, m, nq, max_per_query, u32, stream, out, capacity, flags)

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
    def _match(self, kind, qbytes, qoff, qlen, m, nq, ranges, stream, flags):
        dev = _is_cuda(qbytes)
        if dev:
            import torch
            d = qbytes.device
            ln = torch.empty(nq, dtype=torch.int32, device=d)
            pos = torch.empty(nq, dtype=torch.int64, device=d)
            lo = torch.empty(nq, dtype=torch.int64, device=d) if ranges else None
            hi = torch.empty(nq, dtype=torch.int64, device=d) if ranges else None
            st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
            flags |= _lib.SAS_DEVICE_PTRS
        else:
            qbytes = _as_u8(qbytes)
            ln = np.zeros(max(nq, 1), np.uint32)
            pos = np.zeros(max(nq, 1), np.uint64)
            lo = np.zeros(max(nq, 1), np.uint64) if ranges else None
            hi = np.zeros(max(nq, 1), np.uint64) if ranges else None
            st = stream
        outs = (_ptr(ln), _ptr(pos), _ptr(lo), _ptr(hi), st, flags)
        if kind == "ragged":
            rc = lib().sas_match(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, *outs)
        elif kind == "fixed":
            rc = lib().sas_match_fixed(self._h, _ptr(qbytes), m, nq, *outs)
        else:
            rc = lib().sas_match_stats(self._h, _ptr(qbytes), nq, m, *outs)
        check(rc)
        res = (ln, pos, lo, hi) if ranges else (ln, pos)
        return res if dev else tuple(r[:nq] for r in res)

    def match(self, qbytes, qoff, qlen, ranges: bool = True, stream=None, flags: int = 0):
        """Longest-prefix match of ragged queries qbytes[qoff[k] : qoff[k] + qlen[k]] (sas_match):
        (len, pos) or with ranges (len, pos, lo, hi).  len[k] is the length of the longest prefix
        of query k that occurs in the text, pos[k] a position where it occurs (n when len is 0),
        [lo[k], hi[k]) the SA ranks of every suffix starting with that prefix.  numpy in -> numpy
        out (uint32 len, uint64 others; synchronous); torch CUDA in (uint8 bytes, int64 qoff,
        int32 qlen) -> CUDA out (int32 len, int64 others; async on `stream`)."""
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._match("ragged", qbytes, qoff, qlen, 0, nq, ranges, stream, flags)

    def match_fixed(self, qbytes, m: int, ranges: bool = True, stream=None, flags: int = 0):
        """match for fixed-length queries qbytes[k*m : (k+1)*m] (sas_match_fixed)."""
        if m <= 0:
            raise ValueError("use match for empty queries")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._match("fixed", qbytes, None, None, int(m), nq, ranges, stream, flags)

    def match_stats(self, pattern, max_len: int, ranges: bool = True, stream=None, flags: int = 0):
        """Matching statistics of `pattern` (sas_match_stats): match of the queries
        pattern[i : min(i + max_len, len(pattern))] for every i, one entry per pattern char."""
        plen = int(pattern.numel() if _is_cuda(pattern) else len(pattern))
        return self._match("stats", pattern, None, None, int(max_len), plen, ranges, stream, flags)

    # -- k-mismatch and k-difference locate (sas_locate_mismatch*, sas_locate_edit*: one contract)
    def _locate_mismatch(self, qbytes, qoff, qlen, m, nq, k, max_seed_hits, u32, dist, stream, out, capacity, flags,
                         fn="sas_locate_mismatch"):
        L = lib()
        ragged_fn, fixed_fn = getattr(L, fn), getattr(L, fn + "_fixed")

        def call(off, pos, dst, qfl, cap, total, st, fl):
            tail = (int(k), int(max_seed_hits), _ptr(off), _ptr(pos), _ptr(dst), _ptr(qfl), int(cap), total, st, fl)
            if qoff is not None:
                return ragged_fn(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, *tail)
            return fixed_fn(self._h, _ptr(qbytes), m, nq, *tail)

        if _is_cuda(qbytes):
            import torch
            d = qbytes.device
            dt = torch.int32 if u32 else torch.int64
            st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
            fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
            off = torch.empty(nq + 1, dtype=torch.int64, device=d)
            qfl = torch.empty(nq, dtype=torch.uint8, device=d)
            total = None
            if out is None and capacity is None:  # a sizing call, one read of the total, the real call
                check(call(off, None, None, qfl, 0, None, st, fl))
                capacity = total = int(off[nq].item())
            if out is None:
                out = torch.empty(max(int(capacity), 1), dtype=dt, device=d)
            elif not _is_cuda(out) or out.dtype != dt or not out.is_contiguous():
                raise ValueError(f"{fn[4:]}: out must be a contiguous CUDA {dt} tensor")
            capacity = out.numel() if capacity is None else capacity
            if capacity > out.numel():
                raise ValueError(f"{fn[4:]}: capacity exceeds out")
            dst = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=d) if dist else None
            if total != 0:
                check(call(off, out, dst, qfl, capacity, None, st, fl))
            if total is not None:
                out, dst = out[:total], (dst[:total] if dist else None)
            return off, out, dst, qfl
        qbytes = _as_u8(qbytes)
        fl = flags | (_lib.SAS_LOCATE_U32 if u32 else 0)
        off = np.zeros(nq + 1, np.uint64)
        qfl = np.zeros(max(nq, 1), np.uint8)
        total = C.c_uint64(0)
        rc = call(off, None, None, qfl, 0, C.byref(total), stream, fl)  # the sizing call
        if rc not in (0, errno.ENOSPC):
            check(rc)
        pos = np.zeros(max(total.value, 1), np.uint32 if u32 else np.uint64)
        dst = np.zeros(max(total.value, 1), np.uint8) if dist else None
        if total.value:
            check(call(off, pos, dst, qfl, total.value, C.byref(total), stream, fl))
        return off, pos[:total.value], (dst[:total.value] if dist else None), qfl[:nq]

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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._locate_mismatch(qbytes, qoff, qlen, 0, nq, k, max_seed_hits, u32, dist, stream, out, capacity,
                                     flags)

    def locate_mismatch_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, u32: bool = False,
                              dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """locate_mismatch for fixed-length queries qbytes[i*m : (i+1)*m] (sas_locate_mismatch_fixed)."""
        if m <= 0:
            raise ValueError("use locate_mismatch for empty queries")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._locate_mismatch(qbytes, None, None, int(m), nq, k, max_seed_hits, u32, dist, stream, out,
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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._locate_mismatch(qbytes, qoff, qlen, 0, nq, k, max_seed_hits, u32, dist, stream, out, capacity,
                                     flags, fn="sas_locate_edit")

    def locate_edit_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, u32: bool = False,
                          dist: bool = True, stream=None, out=None, capacity: int | None = None, flags: int = 0):
        """locate_edit for fixed-length queries qbytes[i*m : (i+1)*m] (sas_locate_edit_fixed)."""
        if m <= 0:
            raise ValueError("use locate_edit for empty queries")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._locate_mismatch(qbytes, None, None, int(m), nq, k, max_seed_hits, u32, dist, stream, out,
                                     capacity, flags, fn="sas_locate_edit")

    # -- alignment start and edit script of each reported end (sas_align_edit*)
    def _align_edit(self, qbytes, qoff, qlen, m, nq, k, off, end, u32, stream, flags):
        L = lib()
        k = int(k)
        stride = 2 * k + 1

        def call(na, start, dist, nruns, runs, st, fl):
            tail = (k, _ptr(off), _ptr(end), int(na), _ptr(start), _ptr(dist), _ptr(nruns), _ptr(runs), st, fl)
            if qoff is not None:
                return L.sas_align_edit(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, *tail)
            return L.sas_align_edit_fixed(self._h, _ptr(qbytes), m, nq, *tail)

        if _is_cuda(qbytes):
            import torch
            d = qbytes.device
            dt = torch.int32 if u32 else torch.int64
            if not (_is_cuda(off) and _is_cuda(end)) or off.dtype != torch.int64 or end.dtype != dt:
                raise ValueError(f"align_edit: off must be a CUDA int64 tensor and end a CUDA {dt} tensor")
            off, end = off.contiguous(), end.contiguous()
            na = int(end.numel())
            st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
            fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
            # an alignment past off[nq] is not written: it reads as "none"
            start = torch.full((na,), self.n, dtype=dt, device=d)
            dist = torch.full((na,), _lib.SAS_AL_NONE_DIST, dtype=torch.uint8, device=d)
            nruns = torch.zeros(na, dtype=torch.uint8, device=d)
            runs = torch.zeros((na, stride), dtype=torch.int16, device=d)
            check(call(na, start, dist, nruns, runs, st, fl))
            return start, dist, nruns, runs
        qbytes = _as_u8(qbytes)
        off = np.ascontiguousarray(off, np.uint64)
        end = np.ascontiguousarray(end, np.uint32 if u32 else np.uint64)
        na = len(end)
        fl = flags | (_lib.SAS_LOCATE_U32 if u32 else 0)
        start = np.full(na, self.n, np.uint32 if u32 else np.uint64)
        dist = np.full(na, _lib.SAS_AL_NONE_DIST, np.uint8)
        nruns = np.zeros(na, np.uint8)
        runs = np.zeros((na, stride), np.uint16)
        check(call(na, start, dist, nruns, runs, stream, fl))
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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._align_edit(qbytes, qoff, qlen, 0, nq, k, off, end, u32, stream, flags)

    def align_edit_fixed(self, qbytes, m: int, k: int, off, end, u32: bool = False, flags: int = 0, stream=None):
        """align_edit for fixed-length queries qbytes[i*m : (i+1)*m] (sas_align_edit_fixed)."""
        if m <= 0:
            raise ValueError("use align_edit for empty queries")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._align_edit(qbytes, None, None, int(m), nq, k, off, end, u32, stream, flags)

    # -- read mapping: the best alignment per read on both strands (sas_map_edit*)
    def _map_edit(self, qbytes, qoff, qlen, m, nq, k, max_seed_hits, strands, u32, stream, flags):
        L = lib()
        k = int(k)
        stride = 2 * k + 1

        def call(r, st, fl):
            tail = (k, int(max_seed_hits), int(strands), _ptr(r.end), _ptr(r.start), _ptr(r.dist), _ptr(r.strand),
                    _ptr(r.n_best), _ptr(r.n_loci), _ptr(r.nruns), _ptr(r.runs), _ptr(r.qflags), st, fl)
            if qoff is not None:
                return L.sas_map_edit(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, *tail)
            return L.sas_map_edit_fixed(self._h, _ptr(qbytes), m, nq, *tail)

        if _is_cuda(qbytes):
            import torch
            d = qbytes.device
            dt = torch.int32 if u32 else torch.int64
            st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
            fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)

            def new(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=d)
            r = Mapped(new(nq, dt), new(nq, dt), new(nq, torch.uint8), new(nq, torch.uint8), new(nq, torch.int32),
                       new(nq, torch.int32), new(nq, torch.uint8), new((nq, stride), torch.int16),
                       new(nq, torch.uint8))
            check(call(r, st, fl))
            return r
        qbytes = _as_u8(qbytes)
        pt = np.uint32 if u32 else np.uint64
        r = Mapped(np.empty(nq, pt), np.empty(nq, pt), np.empty(nq, np.uint8), np.empty(nq, np.uint8),
                   np.empty(nq, np.uint32), np.empty(nq, np.uint32), np.empty(nq, np.uint8),
                   np.empty((nq, stride), np.uint16), np.empty(nq, np.uint8))
        check(call(r, stream, flags | (_lib.SAS_LOCATE_U32 if u32 else 0)))
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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._map_edit(qbytes, qoff, qlen, 0, nq, k, max_seed_hits, strands, u32, stream, flags)

    def map_edit_fixed(self, qbytes, m: int, k: int, max_seed_hits: int = 0, strands: int = 3, u32: bool = False,
                       flags: int = 0, stream=None):
        """map_edit for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_edit_fixed)."""
        if m <= 0:
            raise ValueError("use map_edit for empty reads")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._map_edit(qbytes, None, None, int(m), nq, k, max_seed_hits, strands, u32, stream, flags)

    # -- paired-end mapping: the mates of a pair placed together (sas_map_pairs*)
    def _map_pairs(self, qbytes, qoff, qlen, m, nq, k, min_frag, max_frag, max_seed_hits, u32, stream, flags,
                   rescue=None):
        """rescue: None (sas_map_pairs*) or (k_rescue, max_anchors) (sas_map_pairs_rescue*)."""
        if nq % 2:
            raise ValueError(f"paired reads come interleaved, mate 1 then mate 2: {nq} reads is an odd number")
        L = lib()
        k = int(k)
        np_, stride = nq // 2, 2 * (k if rescue is None else int(rescue[0])) + 1
        Rec = MappedPairs if rescue is None else MappedPairsRescue

        def call(r, st, fl):
            ptrs = tuple(_ptr(v) for v in r) + (st, fl)
            if rescue is None:
                tail = (k, int(max_seed_hits), int(min_frag), int(max_frag)) + ptrs
                ragged, fixed = L.sas_map_pairs, L.sas_map_pairs_fixed
            else:
                tail = (k, int(rescue[0]), int(max_seed_hits), int(min_frag), int(max_frag), int(rescue[1])) + ptrs
                ragged, fixed = L.sas_map_pairs_rescue, L.sas_map_pairs_rescue_fixed
            if qoff is not None:
                return ragged(self._h, _ptr(qbytes), _ptr(qoff), _ptr(qlen), np_, *tail)
            return fixed(self._h, _ptr(qbytes), m, np_, *tail)

        if _is_cuda(qbytes):
            import torch
            d = qbytes.device
            dt = torch.int32 if u32 else torch.int64
            st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
            fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)

            def new(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=d)
            r = Rec(new(nq, dt), new(nq, dt), new(nq, torch.uint8), new(nq, torch.uint8),
                    new(nq, torch.int32), new(nq, torch.int32), new(nq, torch.uint8),
                    new((nq, stride), torch.int16), new(nq, torch.uint8), new(np_, torch.uint8),
                    new(np_, torch.int32), new(np_, torch.int32),
                    *([] if rescue is None else [new(np_, torch.int32)]))
            check(call(r, st, fl))
            return r
        qbytes = _as_u8(qbytes)
        pt = np.uint32 if u32 else np.uint64
        r = Rec(np.empty(nq, pt), np.empty(nq, pt), np.empty(nq, np.uint8), np.empty(nq, np.uint8),
                np.empty(nq, np.uint32), np.empty(nq, np.uint32), np.empty(nq, np.uint8),
                np.empty((nq, stride), np.uint16), np.empty(nq, np.uint8), np.empty(np_, np.uint8),
                np.empty(np_, np.uint32), np.empty(np_, np.uint32),
                *([] if rescue is None else [np.empty(np_, np.uint32)]))
        check(call(r, stream, flags | (_lib.SAS_LOCATE_U32 if u32 else 0)))
        return r

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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._map_pairs(qbytes, qoff, qlen, 0, nq, k, min_frag, max_frag, max_seed_hits, u32, stream, flags)

    def map_pairs_fixed(self, qbytes, m: int, k: int, min_frag: int, max_frag: int, max_seed_hits: int = 0,
                        u32: bool = False, flags: int = 0, stream=None):
        """map_pairs for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_pairs_fixed)."""
        if m <= 0:
            raise ValueError("use map_pairs for empty reads")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._map_pairs(qbytes, None, None, int(m), nq, k, min_frag, max_frag, max_seed_hits, u32, stream,
                               flags)

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
        dev = _is_cuda(qbytes)
        if not dev:
            qoff = np.ascontiguousarray(qoff, np.uint64)
            qlen = np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if dev else len(qoff))
        return self._map_pairs(qbytes, qoff, qlen, 0, nq, k, min_frag, max_frag, max_seed_hits, u32, stream, flags,
                               rescue=(k_rescue, max_anchors))

    def map_pairs_rescue_fixed(self, qbytes, m: int, k: int, k_rescue: int, min_frag: int, max_frag: int,
                               max_anchors: int, max_seed_hits: int = 0, u32: bool = False, flags: int = 0,
                               stream=None):
        """map_pairs_rescue for fixed-length reads qbytes[i*m : (i+1)*m] (sas_map_pairs_rescue_fixed)."""
        if m <= 0:
            raise ValueError("use map_pairs_rescue for empty reads")
        nq = (qbytes.numel() if _is_cuda(qbytes) else len(qbytes)) // m
        return self._map_pairs(qbytes, None, None, int(m), nq, k, min_frag, max_frag, max_seed_hits, u32, stream,
                               flags, rescue=(k_rescue, max_anchors))

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
    L = lib()
    dev = _is_cuda(qbytes)
    if dev:
        import torch
        d = qbytes.device
        st = stream if stream is not None else torch.cuda.current_stream(d).cuda_stream
        fl = flags | _lib.SAS_DEVICE_PTRS
        with torch.cuda.device(d):
            if m is not None:
                nq = qbytes.numel() // int(m)
                out = torch.empty(nq * int(m), dtype=torch.uint8, device=d)
                check(L.sas_revcomp_fixed(_ptr(qbytes), int(m), nq, _ptr(out), st, fl))
                return out
            nq = int(qoff.numel())
            out = torch.empty(int(qlen.sum()) if nq else 0, dtype=torch.uint8, device=d)
            off = torch.empty(nq + 1, dtype=torch.int64, device=d)
            check(L.sas_revcomp(_ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, _ptr(out), _ptr(off), st, fl))
            return out, off
    qbytes = _as_u8(qbytes)
    if m is not None:
        nq = len(qbytes) // int(m)
        out = np.empty(nq * int(m), np.uint8)
        check(L.sas_revcomp_fixed(_ptr(qbytes), int(m), nq, _ptr(out), stream, flags))
        return out
    qoff = np.ascontiguousarray(qoff, np.uint64)
    qlen = np.ascontiguousarray(qlen, np.uint32)
    nq = len(qoff)
    out = np.empty(int(qlen.astype(np.uint64).sum()), np.uint8)
    off = np.empty(nq + 1, np.uint64)
    check(L.sas_revcomp(_ptr(qbytes), _ptr(qoff), _ptr(qlen), nq, _ptr(out), _ptr(off), stream, flags))
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
    out = np.zeros(max(n, 1), np.uint8)
    check(lib().sas_gen_text(seed, n, out.ctypes.data, 0))
    return out[:n]


def random_queries(n: int, nq: int, seed: int = 31415, word_pos: int | None = None, margin: int = 200,
                   len_lo: int = 30, len_hi: int = 100):
    """sas/util.rs:18-26 -> (offsets u64, lengths u32, next keystream word).  The
    stream continues after the text's n words unless word_pos is given."""
    off = np.zeros(max(nq, 1), np.uint64)
    ln = np.zeros(max(nq, 1), np.uint32)
    nxt = C.c_uint64(0)
    check(lib().sas_gen_queries(seed, n if word_pos is None else word_pos, n, nq, margin, len_lo, len_hi,
                                off.ctypes.data, ln.ctypes.data, C.byref(nxt)))
    return off[:nq], ln[:nq], nxt.value


# ---------------------------------------------------------------- real data
def read_fasta_file(path: str) -> np.ndarray:
    """sas/util.rs:144-169: concatenated record sequences as codes 0..3 (others -> 0)."""
    n = C.c_uint64(0)
    check(lib().sas_read_fasta(path.encode(), None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), np.uint8)
    check(lib().sas_read_fasta(path.encode(), out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


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
    out = np.zeros(max(n.value, 1), np.uint8)
    starts = np.zeros(nseq.value + 1, np.uint64)
    lo, hi = np.zeros(max(nseg.value, 1), np.uint64), np.zeros(max(nseg.value, 1), np.uint64)
    names = C.create_string_buffer(max(nl.value, 1))
    check(L.sas_read_fasta_layout(p, out.ctypes.data, n.value, C.byref(n), starts.ctypes.data, len(starts),
                                  C.byref(nseq), lo.ctypes.data, hi.ctypes.data, nseg.value, C.byref(nseg),
                                  C.cast(names, C.c_void_p), nl.value, C.byref(nl)))
    words = names.raw[: nl.value].split(b"\0")[:-1] if nl.value else []
    return FastaLayout(out[: n.value], starts, lo[: nseg.value], hi[: nseg.value], [w.decode() for w in words])


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
    check(lib().sas_kmer_keys(t.ctypes.data, n, k, limit, None, C.byref(cnt), 0))
    out = np.zeros(max(cnt.value, 1), np.uint32)
    check(lib().sas_kmer_keys(t.ctypes.data, n, k, limit, out.ctypes.data, C.byref(cnt), 0))
    return out[: cnt.value]
