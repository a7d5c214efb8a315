"""The sequence layout on the CPU (no kernel is launched): the symbols, sas_check_layout's rules, the
reader sas_read_fasta_layout against a Python restatement, the numpy reference of the layout
semantics that tests/test_gpu_layout.py compares the GPU with, checked here against plain loops,
and tests/cpp/layout_host_check.cpp, a program of its own built with the host sanitizers.

The reference is the existing restatements (EBrute, MBrute, align_ref_sel, map_ref) applied to each
segment as a text of its own and shifted by the segment's lo; the seed gate alone counts
occurrences in the whole text, as sas.h says."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from sas_amd import _lib
from test_align_host import NONE_DIST, align_ref_sel, ed_loops
from test_gpu_edit import LONG, MAX_M, SHORT, TRUNCATED, EBrute
from test_map_host import map_ref, revcomp_ref
from test_pairs_host import FIELDS as PAIR_FIELDS, loci_reps, pairs_ref_all
from test_rescue_host import FIELDS as RESCUE_FIELDS, anchors_of, rescue_ref_all, window_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "layout_host_check.cpp")
SEQ_NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- the reference
class Layout:
    """seq_start (nseq + 1 entries), seg_lo, seg_hi as int64 arrays."""

    def __init__(self, seq_start, seg_lo, seg_hi):
        self.seq_start = np.asarray(seq_start, np.int64)
        self.lo, self.hi = np.asarray(seg_lo, np.int64), np.asarray(seg_hi, np.int64)
        self.n = int(self.seq_start[-1])
        for a in (self.seq_start, self.lo, self.hi):
            a.setflags(write=False)

    def seg_of_pos(self, p):
        """the segment with lo <= p < hi, or -1"""
        g = int(np.searchsorted(self.lo, p, side="right")) - 1
        return g if g >= 0 and p < self.hi[g] else -1

    def seg_of_end(self, e):
        """the segment with lo < e <= hi, or -1"""
        return self.seg_of_pos(e - 1) if e >= 1 else -1

    def seq_of_end(self, e):
        """the largest i with seq_start[i] < e"""
        return int(np.searchsorted(self.seq_start, e, side="left")) - 1

    def inside(self, s, e):
        """[s, e) lies inside one segment"""
        g = self.seg_of_pos(s)
        return g >= 0 and e <= self.hi[g]

    def translate(self, pos, span):
        """sas_translate: (sequence id, offset) of [pos, pos + max(span, 1))."""
        span = max(int(span), 1)
        if self.inside(pos, pos + span):
            i = self.seq_of_end(pos + 1)
            return i, pos - int(self.seq_start[i])
        return SEQ_NONE, pos


class LBrute:
    """The layout semantics of sas.h over a text: one EBrute per segment, one over the whole text
    for the seed gate."""

    def __init__(self, t, lay):
        self.t, self.lay, self.n = t, lay, len(t)
        self.whole = EBrute(t)
        self.subs = [EBrute(t[lo:hi]) for lo, hi in zip(lay.lo, lay.hi)]

    def edit(self, q, k, max_hits):
        """(ends, distances, flags) of sas_locate_edit with the layout set."""
        m = len(q)
        if m <= k:
            return [], [], SHORT
        if m > MAX_M:
            return [], [], LONG
        b = [j * m // (k + 1) for j in range(k + 2)]
        pieces = [q[b[j]:b[j + 1]].tobytes() for j in range(k + 1)]
        skipped = [bool(max_hits) and len(self.whole.occurrences(p)) > max_hits for p in pieces]
        flags = TRUNCATED if any(skipped) else 0
        ends, dist = [], []
        for lo, sub in zip(self.lay.lo, self.subs):
            ns = sub.n
            near = np.zeros(ns + 2, np.int64)
            for j in range(k + 1):
                if skipped[j]:
                    continue
                c = np.array(sub.occurrences(pieces[j]), np.int64) - b[j] + m  # occurrences inside the segment
                l, h = np.maximum(c - k, 0), np.minimum(c + k, ns) + 1
                ok = l < h
                np.add.at(near, l[ok], 1)
                np.add.at(near, h[ok], -1)
            near = np.cumsum(near)[:ns + 1]
            if not near.any():
                continue
            D = sub.rows([q])[0]
            es = np.flatnonzero((D <= k) & (near > 0))
            ends += (es + int(lo)).tolist()
            dist += D[es].tolist()
        return ends, dist, flags

    def mismatch(self, mb, q, k, max_hits):
        """sas_locate_mismatch with the layout set, from the whole-text answer of MBrute mb: the
        alignments inside one segment, in the same order."""
        pos, dist, flags, _ = mb.answer(q, k, max_hits)
        keep = [i for i, s in enumerate(pos) if self.lay.inside(s, s + len(q))]
        return [pos[i] for i in keep], [dist[i] for i in keep], flags

    def align(self, qs, qi, end, k, sel):
        """align_ref_sel per segment: (start, dist, nruns, runs) of the alignments sel."""
        stride = 2 * k + 1
        start = np.full(len(sel), self.n, np.int64)
        dist = np.full(len(sel), NONE_DIST, np.int64)
        nruns = np.zeros(len(sel), np.int64)
        runs = np.zeros((len(sel), stride), np.int64)
        by_seg = {}
        for x, a in enumerate(sel):
            g = self.lay.seg_of_end(int(end[a])) if int(end[a]) <= self.n else -1
            if g >= 0:
                by_seg.setdefault(g, []).append(x)
        for g, xs in by_seg.items():
            lo, hi = int(self.lay.lo[g]), int(self.lay.hi[g])
            shifted = np.asarray(end, np.int64) - lo
            s, d, nr, rr = align_ref_sel(self.t[lo:hi], qs, qi, shifted, k, [sel[x] for x in xs])
            has = d != NONE_DIST
            start[xs] = np.where(has, s + lo, self.n)
            dist[xs], nruns[xs], runs[xs] = d, nr, rr
        return start, dist, nruns, runs

    def answers(self, qs, k, max_hits):
        """(A_0, A_1): the constrained answers of every read and of its reverse complement."""
        return ([self.edit(q, k, max_hits) for q in qs], [self.edit(revcomp_ref(q), k, max_hits) for q in qs])

    def d_l(self, q):
        """D_L(e) for e in [0, n]; 999 where it is undefined (an end in no segment)."""
        D = np.full(self.n + 1, 999, np.int64)
        for lo, hi, sub in zip(self.lay.lo, self.lay.hi, self.subs):
            D[lo + 1:hi + 1] = sub.rows([np.asarray(q, np.uint8)])[0][1:]
        return D

    def pairs(self, qs, k, max_hits, min_frag, max_frag, k_align=None, A=None):
        """sas_map_pairs' records with the layout set: test_pairs_host's pairs_ref_all with the sequence
        condition added (a candidate is proper only if both ends have the same sequence), every
        candidate on its own, over the constrained answers; alignments in the band of k_align."""
        k_align = k if k_align is None else k_align
        A = self.answers(qs, k, max_hits) if A is None else A
        out = self.map(qs, k_align, max_hits, 3, A=A)
        nq = len(qs)
        out.update(n_pairs=np.zeros(nq // 2, np.int64), n_best_pairs=np.zeros(nq // 2, np.int64))
        chosen, sel = list(qs), []
        for i in range(nq // 2):
            cands = []
            for o in (0, 1):
                f, v = 2 * i + o, 2 * i + 1 - o
                dx, ex = loci_reps(A[0][f][0], A[0][f][1])
                dy, ey = loci_reps(A[1][v][0], A[1][v][1])
                for x in range(len(ex)):
                    for y in range(len(ey)):
                        F = int(ey[y]) - int(ex[x]) + len(qs[f])
                        if min_frag <= F <= max_frag and self.lay.seq_of_end(int(ex[x])) == self.lay.seq_of_end(int(ey[y])):
                            cands.append((int(dx[x] + dy[y]), o, int(ex[x]), int(ey[y]), int(dx[x]), int(dy[y])))
            if not cands:
                continue
            best = min(cands)
            out["n_pairs"][i] = len(cands)
            out["n_best_pairs"][i] = sum(c[0] == best[0] for c in cands)
            _, o, ex, ey, dx, dy = best
            f, v = 2 * i + o, 2 * i + 1 - o
            out["end"][f], out["dist"][f], out["strand"][f] = ex, dx, 0
            out["end"][v], out["dist"][v], out["strand"][v] = ey, dy, 1
            chosen[v] = revcomp_ref(qs[v])
            sel += [f, v]
        out["pflags"] = (out["n_pairs"] > 0).astype(np.int64)
        self._realign(out, chosen, sel, k_align)
        return out

    def _realign(self, out, chosen, sel, k_align):
        if sel:
            sel = np.array(sorted(sel))
            start, dist, nruns, runs = self.align(chosen, np.arange(len(chosen)), out["end"], k_align, sel)
            assert np.array_equal(dist, out["dist"][sel])  # the alignment's distance is D_L(e)
            out["start"][sel], out["nruns"][sel], out["runs"][sel] = start, nruns, runs

    def rescue(self, qs, k, k_rescue, max_hits, min_frag, max_frag, max_anchors):
        """sas_map_pairs_rescue's records with the layout set: test_rescue_host's rescue_ref_all with
        the window of partner ends cut to the anchor's sequence (seq_start[i], seq_start[i + 1]] and
        D_L as the scanned distance."""
        A = self.answers(qs, k, max_hits)
        out = self.pairs(qs, k, max_hits, min_frag, max_frag, k_align=k_rescue, A=A)
        nq = len(qs)
        out["n_rescue"] = np.zeros(nq // 2, np.int64)
        chosen, sel = [None] * nq, []
        for i in range(nq // 2):
            anchors = anchors_of(A, i) if out["n_pairs"][i] == 0 and max_anchors > 0 else []
            if len(anchors) > max_anchors:
                out["pflags"][i] |= 4
                continue
            runs, best = 0, None
            for a, s, d_a, e_a in anchors:
                b = a ^ 1
                m_a, m_b = len(qs[a]), len(qs[b])
                if m_b <= k_rescue or m_b > MAX_M:
                    continue
                lo, hi = window_of(self.n, s, e_a, m_a, m_b, min_frag, max_frag)
                sq = self.lay.seq_of_end(e_a)
                lo, hi = max(lo, int(self.lay.seq_start[sq]) + 1), min(hi, int(self.lay.seq_start[sq + 1]))
                if lo > hi:
                    continue
                D = self.d_l(qs[b] if s == 1 else revcomp_ref(qs[b]))[lo:hi + 1]
                cand = D <= k_rescue
                runs += int((cand & ~np.concatenate([[False], cand[:-1]])).sum())
                ends = lo + np.flatnonzero(cand)
                if len(ends) == 0:
                    continue
                j = np.lexsort((ends, D[cand]))[0]
                dd, ee = int(D[cand][j]), int(ends[j])
                c = (d_a + dd, a - 2 * i, e_a, ee, d_a, dd, 0) if s == 0 else (d_a + dd, b - 2 * i, ee, e_a, dd, d_a, 1)
                best = c if best is None or c[:4] < best[:4] else best
            out["n_rescue"][i] = runs
            if best is None:
                continue
            _, o, ex, ey, dx, dy, s = best
            f, v = 2 * i + o, 2 * i + 1 - o
            out["pflags"][i] |= 2
            out["end"][f], out["dist"][f], out["strand"][f] = ex, dx, 0
            out["end"][v], out["dist"][v], out["strand"][v] = ey, dy, 1
            out["qflags"][v if s == 0 else f] |= 8
            chosen[f], chosen[v] = qs[f], revcomp_ref(qs[v])
            sel += [f, v]
        self._realign(out, chosen, sel, k_rescue)
        return out

    def map(self, qs, k, max_hits, strands, A=None):
        """sas_map_edit's records with the layout set: map_ref over the constrained answers (A: those
        of another k, for the rescue's wider alignment band), then the constrained alignment of each
        winner."""
        nq, stride = len(qs), 2 * k + 1
        A0, A1 = self.answers(qs, k, max_hits) if A is None else A
        rec = np.array([map_ref(self.n, a0, a1, strands) for a0, a1 in zip(A0, A1)], np.int64).reshape(nq, 6)
        out = dict(end=rec[:, 0], dist=rec[:, 1], strand=rec[:, 2], n_best=rec[:, 3], n_loci=rec[:, 4],
                   qflags=rec[:, 5], start=np.full(nq, self.n, np.int64), nruns=np.zeros(nq, np.int64),
                   runs=np.zeros((nq, stride), np.int64))
        chosen = [revcomp_ref(q) if s else q for q, s in zip(qs, out["strand"])]
        sel = np.flatnonzero(out["dist"] != NONE_DIST)
        if len(sel):
            start, dist, nruns, runs = self.align(chosen, np.arange(nq), out["end"], k, sel)
            assert np.array_equal(dist, out["dist"][sel])
            out["start"][sel], out["nruns"][sel], out["runs"][sel] = start, nruns, runs
        return out

    def translate(self, pos, span):
        return self.lay.translate(pos, span)


# ---------------------------------------------------------------- symbols and argument checks
U64, U32, VP = C.c_uint64, C.c_uint32, C.c_void_p
P64 = C.POINTER(C.c_uint64)
SIGNATURES = {
    "sas_check_layout": [U64, VP, U64, VP, VP, U64],
    "sas_set_layout": [VP, VP, U64, VP, VP, U64],
    "sas_get_layout": [VP, P64, P64, VP, VP, VP],
    "sas_translate": [VP, VP, VP, U64, VP, VP, VP, U32],
    "sas_read_fasta_layout": [C.c_char_p, VP, U64, P64, VP, U64, P64, VP, VP, U64, P64, VP, U64, P64],
}


def test_symbols_declared_exported_and_bound():
    import sas_amd
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name)
        assert list(getattr(L, name).argtypes) == sig, name
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    assert "#define SAS_SEQ_NONE 0xFFFFFFFFu" in src and _lib.SAS_SEQ_NONE == SEQ_NONE
    assert "NO CALL IN FLIGHT" in src and "ignore the layout" in src and "sas_translate" in src
    for name in ("set_layout", "layout", "translate"):
        assert callable(getattr(sas_amd.SaNaive, name))
    assert callable(sas_amd.read_fasta_layout) and callable(sas_amd.check_layout)
    hpp = open(os.path.join(REPO, "include", "sas.hpp")).read()
    assert "void set_layout(" in hpp and "translate(" in hpp


def test_null_index_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(4, np.uint64)
    p = a.ctypes.data
    n1, n2 = C.c_uint64(0), C.c_uint64(0)
    for rc in (L.sas_set_layout(None, p, 1, None, None, 0),
               L.sas_get_layout(None, C.byref(n1), C.byref(n2), None, None, None),
               L.sas_translate(None, p, None, 1, p, p, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()


def test_check_layout_accepts():
    import sas_amd
    sas_amd.check_layout(20, [0, 10, 10, 20], [2, 12], [8, 18])   # an empty sequence
    sas_amd.check_layout(20, [0, 10, 20], [2, 5, 10], [5, 10, 20])  # adjacent segments, also across a start
    sas_amd.check_layout(20, [0, 20], [], [])                      # nseg == 0: everything is masked
    sas_amd.check_layout(0, [0, 0], [], [])                        # the empty text
    sas_amd.check_layout(20, [0, 20], [0], [20])                   # the identity


@pytest.mark.parametrize("what,n,starts,lo,hi,word", [
    ("seq_start[0] != 0", 20, [1, 10, 20], [2], [8], "seq_start[0]"),
    ("last start != n", 20, [0, 10, 19], [2], [8], "seq_start[2]"),
    ("decreasing starts", 20, [0, 12, 11, 20], [2], [8], "seq_start[2]"),
    ("an empty segment", 20, [0, 10, 20], [2, 12], [2, 18], "segment 0"),
    ("overlapping segments", 20, [0, 10, 20], [2, 7], [8, 9], "segment 1"),
    ("a segment across a sequence start", 20, [0, 10, 20], [2, 9], [8, 11], "seq_start[1]"),
    ("hi > n", 20, [0, 10, 20], [2, 12], [8, 21], "segment 1"),
])
def test_check_layout_refuses(what, n, starts, lo, hi, word):
    import sas_amd
    with pytest.raises(sas_amd.SasError) as ei:
        sas_amd.check_layout(n, starts, lo, hi)
    assert ei.value.code == errno.EINVAL and word in str(ei.value), what


# ---------------------------------------------------------------- the reader
RECORDS = [  # (header, sequence lines)
    ("chrA first record", ["NNNacgtACGT", "ACGNNNNACG", "TTNACGT", "GGNN"]),   # leading, inner, single inner, trailing N
    ("empty", []),
    ("chrC\tx y", ["ACGTRYKMacgt", "TTTT"]),                                    # IUPAC codes are gaps too
]
CODE = {c: i for i, c in enumerate("ACGT")}


def restate(records):
    """What the reader must give: text codes, seq_start, segments, names."""
    text, starts, lo, hi, names = [], [0], [], [], []
    for header, lines in records:
        names.append(header.split()[0])
        run = None
        for ch in "".join(lines):
            base = ch.upper() in CODE
            if base and run is None:
                run = len(text)
            if not base and run is not None:
                lo.append(run)
                hi.append(len(text))
                run = None
            text.append(CODE.get(ch.upper(), 0))
        if run is not None:
            lo.append(run)
            hi.append(len(text))
        starts.append(len(text))
    return np.array(text, np.uint8), starts, lo, hi, names


def write_fasta(path, records, eol):
    with open(path, "wb") as f:
        for header, lines in records:
            f.write((">" + header + eol).encode())
            for ln in lines:
                f.write((ln + eol).encode())


def write_fastq(path, records, eol):
    with open(path, "wb") as f:
        for header, lines in records:
            s = "".join(lines)
            f.write(("@" + header + eol + s + eol + "+" + eol + "I" * len(s) + eol).encode())


@pytest.mark.parametrize("fmt,eol", [("fasta", "\n"), ("fasta", "\r\n"), ("fastq", "\n"), ("fastq", "\r\n")])
def test_reader_against_restatement(tmp_path, fmt, eol):
    import sas_amd
    path = str(tmp_path / ("x." + fmt))
    (write_fasta if fmt == "fasta" else write_fastq)(path, RECORDS, eol)
    text, starts, lo, hi, names = restate(RECORDS)
    assert len(lo) == 5 and text[0] == 0 and lo[0] == 3  # the leading N run is text, and no segment
    got = sas_amd.read_fasta_layout(path)
    assert np.array_equal(got.text, sas_amd.read_fasta_file(path))  # the bytes of sas_read_fasta
    assert np.array_equal(got.text, text)
    assert got.seq_start.tolist() == starts and got.names == names
    assert got.seg_lo.tolist() == lo and got.seg_hi.tolist() == hi
    assert starts[1] == starts[2]  # the empty record keeps its id
    sas_amd.check_layout(len(text), got.seq_start, got.seg_lo, got.seg_hi)
    # a buffer that is too small is refused
    L = _lib.lib()
    n, ns, ng = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    small = np.zeros(2, np.uint64)
    rc = L.sas_read_fasta_layout(path.encode(), None, 0, C.byref(n), small.ctypes.data, 2, C.byref(ns), None, None, 0,
                                 C.byref(ng), None, 0, None)
    assert rc == errno.ENOMEM


# ---------------------------------------------------------------- the reference against plain loops
def small_case():
    """300 chars: two sequences, the first with a one-char gap, the second with a leading gap."""
    t = O.random_string(300, seed=21).copy()
    lay = Layout([0, 150, 300], [0, 61, 170], [60, 150, 300])
    t[60] = 0
    t[150:170] = 0
    return t, lay


def d_l_loops(t, lay, q, k):
    """{e: D_L(e)} for D_L(e) <= k: the least ed(q, t[s:e]) over the s with [s, e) inside one segment,
    every pair (s, e) on its own (only starts within m + k of the end can reach k)."""
    out = {}
    m = len(q)
    for lo, hi in zip(lay.lo.tolist(), lay.hi.tolist()):
        for e in range(lo + 1, hi + 1):
            best = min(ed_loops(q.tolist(), t[s:e].tolist()) for s in range(max(lo, e - m - k), e + 1))
            if best <= k:
                out[e] = best
    return out


def test_reference_agrees_with_plain_loops():
    t, lay = small_case()
    lb = LBrute(t, lay)
    rng = np.random.default_rng(5)
    qs = [t[50:60], t[55:65], t[61:71], t[145:155], t[150:160], t[170:180], t[169:179], t[290:300],
          np.zeros(10, np.uint8), np.concatenate([t[100:104], t[105:111]]), np.concatenate([[3], t[61:70]]).astype(np.uint8)]
    qs += [rng.integers(0, 4, 10).astype(np.uint8) for _ in range(3)]
    differs = 0
    for q in qs:
        q = np.asarray(q, np.uint8)
        for k in (0, 1, 2):
            ends, dist, fl = lb.edit(q, k, 0)
            assert fl == 0 and dict(zip(ends, dist)) == d_l_loops(t, lay, q, k), (q, k)
            assert ends == sorted(ends)
            differs += dict(zip(ends, dist)) != lb.whole.full(q, k)
            # every reported end aligns inside its segment, at its distance, and the script is one of that cost
            if ends:
                s, d, nr, rr = lb.align([q], np.zeros(len(ends), np.int64), np.array(ends), k, list(range(len(ends))))
                assert d.tolist() == dist
                for a, e in enumerate(ends):
                    assert lay.inside(int(s[a]), e) and ed_loops(q.tolist(), t[int(s[a]):e].tolist()) == dist[a]
    assert differs >= 8  # the layout changes the answer of the planted queries
    # ends in no segment get no alignment
    s, d, nr, rr = lb.align([qs[0]], np.zeros(3, np.int64), np.array([0, 61, 160]), 2, [0, 1, 2])
    assert d.tolist() == [NONE_DIST] * 3 and s.tolist() == [300] * 3
    # translate
    assert lb.translate(59, 1) == (0, 59) and lb.translate(60, 1) == (SEQ_NONE, 60)
    assert lb.translate(59, 2) == (SEQ_NONE, 59) and lb.translate(170, 0) == (1, 20)
    assert lb.translate(149, 1) == (0, 149) and lb.translate(149, 2) == (SEQ_NONE, 149)
    assert lb.translate(300, 1) == (SEQ_NONE, 300)


def test_pair_references_against_the_existing_ones():
    """Under the identity layout LBrute.pairs and LBrute.rescue are test_pairs_host's and
    test_rescue_host's references field for field; a sequence start between two mates, and nothing
    else, takes their proper pair away, and the rescue does not look across it either."""
    t = O.random_string(1200, seed=33)
    rng = np.random.default_rng(9)
    m, k, kr, frag = 24, 1, 3, (50, 400)
    qs = []
    for s, gap, ed1, ed2 in ((100, 200, 0, 0), (500, 250, 1, 0), (300, 150, 0, 3), (700, 300, 3, 0), (40, 900, 0, 0)):
        a, b = t[s:s + m].copy(), revcomp_ref(t[s + gap - m:s + gap]).copy()
        for q, ne in ((a, ed1), (b, ed2)):
            for p in rng.choice(m, ne, replace=False):
                q[p] ^= 1 + int(rng.integers(0, 3))
        qs += [a, b]
    qs += [t[900:900 + m], t[10:10 + m]]  # no reverse mate at all
    br = EBrute(t)
    A_f, A_r = br.answers(qs, k, 0), br.answers([revcomp_ref(q) for q in qs], k, 0)
    want_p = pairs_ref_all(t, qs, k, A_f, A_r, *frag)
    want_r = rescue_ref_all(t, qs, k, kr, A_f, A_r, *frag, 4)
    ident = LBrute(t, Layout([0, 1200], [0], [1200]))
    got_p, got_r = ident.pairs(qs, k, 0, *frag), ident.rescue(qs, k, kr, 0, *frag, 4)
    for f in PAIR_FIELDS:
        assert np.array_equal(got_p[f], want_p[f]), f
    for f in RESCUE_FIELDS:
        assert np.array_equal(got_r[f], want_r[f]), f
    assert want_p["n_pairs"][:2].tolist() == [1, 1] and (want_r["pflags"][2:4] & 2).all()  # proper, and rescued
    # a sequence start at 200: between the mates of pair 0 and inside the window of nothing else
    cut = LBrute(t, Layout([0, 200, 1200], [0, 200], [200, 1200]))
    cp, cr = cut.pairs(qs, k, 0, *frag), cut.rescue(qs, k, kr, 0, *frag, 4)
    assert cp["n_pairs"].tolist() == [0] + want_p["n_pairs"][1:].tolist()
    assert cr["pflags"][0] == 0 and cr["n_rescue"][0] == 0 and np.array_equal(cr["pflags"][1:], want_r["pflags"][1:])
    for f in ("end", "dist", "strand"):  # both mates still map, each on its own
        assert np.array_equal(cp[f][2:], want_p[f][2:]) and (cp["dist"][:2] == 0).all()


# ---------------------------------------------------------------- the host code under the sanitizers
def test_layout_host_check_under_sanitizers(tmp_path):
    """layout.hpp's bisects against linear scans, sas_check_layout's rules and the reader, in a program
    of its own built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    fasta = str(tmp_path / "x.fa")
    write_fasta(fasta, RECORDS, "\r\n")
    exe = tmp_path / "layout_host_check"
    inc = [a for d in ("/opt/rocm/include",) if os.path.isdir(d) for a in ("-I", d)]
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-D__HIP_PLATFORM_AMD__", *inc, SRC, "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), fasta], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "layout host ok" in r.stdout
    text, starts, lo, hi, names = restate(RECORDS)
    want = "reader len %d nseq %d nseg %d names_len %d" % (len(text), len(starts) - 1, len(lo),
                                                          sum(len(x) + 1 for x in names))
    assert want in r.stdout, r.stdout
