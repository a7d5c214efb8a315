"""CPU checks behind tests/test_gpu_tiles.py (no kernel is launched): the cases that module runs under
SAS_TILE_GRID hold what they are there for, asserted from the brute force alone -- enough tiles of
each kernel's tile size that a capped grid takes the tile loop several times per workgroup, and,
for the sparse case, CSR offsets whose slice of one tile does not fit the LDS stage, so the
kernels bisect global memory.  sas_tile_grid_cap is declared, exported and bound, and follows the
variable.

The cases and their references are built here once per process (functools.lru_cache) and shared
with the GPU module; every array handed out is read-only."""
import ctypes as C
import functools
import os
import types

import numpy as np

from sas_amd import _lib
from test_align_host import NONE_DIST, align_ref_sel
from test_gpu_edit import MAX_M, TEXTS, EBrute, edited, expected, make_queries, make_text
from test_gpu_locate import N as LOC_N, synthetic_cases as locate_cases
from test_gpu_map import Case as MapCase
from test_gpu_match import pack
from test_gpu_mismatch import MBrute
from test_gpu_pairs import Case as PairCase
from test_map_host import intervals, map_ref_all, revcomp_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernels' tile sizes and LDS stages (csrc/seed_verify.hpp, map_path.hpp, sas_locate.hip)
MM_T, AL_T, MAP_T, LOC_T = 2048, 1024, 2048, 2048
MM_SLICE, AL_SLICE = 4096, 2048
GRIDS = ("1", "3")
MIN_TILES = 2 * 3 + 1  # under the widest cap every workgroup still takes more than two tiles
TILE_RUNS = (("period7", 1), ("random", 3))  # (text, k) of the tile-loop cases
PAIR_RUNS = (("selfrc", 1, (100, 700)), ("random", 3, (0, 400)))
ALIGN_ALL, ALIGN_SAMPLE = 5000, 3000
SPARSE = dict(text="random", nq=6000, m=24, k=1, every=10, empties=4096, seed=77)


def tiles(total, T):
    return (int(total) + T - 1) // T


def span(off, T):
    """Over all aligned tiles [t0, min(t0 + T, total)) of the CSR offsets off (total = off[-1]): the
    largest p1 - p0 + 1, p0 and p1 the last entries with off[p] <= the tile's first and last
    element.  The tiled kernels stage off[p0 .. p1] in LDS when that many entries fit."""
    off = np.asarray(off, np.int64)
    total = int(off[-1])
    if total == 0:
        return 0
    t0 = np.arange(0, total, T, dtype=np.int64)
    t1 = np.minimum(t0 + T, total) - 1
    p0 = np.searchsorted(off, t0, side="right") - 1
    p1 = np.searchsorted(off, t1, side="right") - 1
    return int((p1 - p0 + 1).max())


def csr(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def piece_counts(count, qs, k, max_m=None):
    """Candidates per piece of every query (sas.h: piece j = chars [j m / (k + 1), (j + 1) m / (k + 1)),
    no seed cap): the occurrences of the piece, none for a query of m <= k or m > max_m."""
    out = np.zeros(len(qs) * (k + 1), np.int64)
    for i, q in enumerate(qs):
        m = len(q)
        if m <= k or (max_m is not None and m > max_m):
            continue
        for j in range(k + 1):
            out[i * (k + 1) + j] = count(q[j * m // (k + 1):(j + 1) * m // (k + 1)].tobytes())
    return out


class Brute(EBrute):
    """EBrute that keeps the answers of a list of queries: expected() and the map references ask for
    the same ones."""

    def __init__(self, t):
        super().__init__(t)
        self._ans = {}

    def answers(self, qs, k, max_hits):
        key = (id(qs), k, max_hits)
        if key not in self._ans:
            self._ans[key] = (qs, super().answers(qs, k, max_hits))
        return self._ans[key][1]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def mismatch_expected(mb, qs, k):
    ans = [mb.answer(q, k, 0) for q in qs]
    exp = dict(off=csr([len(a[0]) for a in ans]), pos=np.array([p for a in ans for p in a[0]], np.int64),
               dist=np.array([d for a in ans for d in a[1]], np.int64),
               qflags=np.array([a[2] for a in ans], np.int64), cand=int(sum(a[3] for a in ans)))
    frozen(*(v for v in exp.values() if isinstance(v, np.ndarray)))
    return exp


class EditCase:
    """The queries of tests/test_gpu_edit.py for one (text, k), or any other list of them: the brute
    force's k-difference answer, its k-mismatch answer on demand, and the alignments of its ends
    with the fields that test_gpu_align's structure() and compare() read."""

    def __init__(self, t, qs, k):
        self.t, self.n, self.k, self.qs = t, len(t), k, qs
        self.br = Brute(t)
        self.qb, self.qoff, self.qlen = pack(qs)
        self.exp = expected(self.br, qs, k, 0)
        self.off, self.end, self.dist = self.exp["off"], self.exp["end"], self.exp["dist"]
        self.na = len(self.end)
        self.qi = np.searchsorted(self.off, np.arange(self.na), side="right") - 1
        self.pieces = piece_counts(lambda p: len(self.br.occurrences(p)), qs, k, MAX_M)
        frozen(self.qb, self.qoff, self.qlen, self.qi, self.pieces)

    @functools.cached_property
    def mm(self):
        """(expected, candidates per piece) of sas_locate_mismatch: no query is too long for it"""
        mb = MBrute(self.t)
        pieces = piece_counts(mb.count, self.qs, self.k)
        frozen(pieces)
        return mismatch_expected(mb, self.qs, self.k), pieces

    @functools.cached_property
    def sel(self):
        """the alignments compared bit for bit: all, or each query's first and last and a sample"""
        if self.na <= ALIGN_ALL:
            sel = np.arange(self.na)
        else:
            cnt = np.diff(self.off)
            edge = np.concatenate([self.off[:-1][cnt > 0], self.off[1:][cnt > 0] - 1])
            sel = np.unique(np.concatenate([edge, np.random.default_rng(77).choice(self.na, ALIGN_SAMPLE, False)]))
        frozen(sel)
        return sel

    @functools.cached_property
    def ref(self):
        ref = align_ref_sel(self.t, self.qs, self.qi, self.end, self.k, self.sel)
        frozen(*ref)
        return ref


@functools.lru_cache(maxsize=None)
def edit_case(name, k):
    t = make_text(name)
    qs, _ = make_queries(t, k, 2000 + 10 * TEXTS.index(name) + k)
    return EditCase(t, qs, k)


@functools.lru_cache(maxsize=None)
def map_case(name, k):
    return MapCase(name, k, 0)


@functools.lru_cache(maxsize=None)
def pair_case(name, k):
    return PairCase(name, k, 0)


def proposals(c, strands):
    """Sorted proposals of the select and loci kernels: the brute force counts every end once per
    candidate that proposes it (info["prop"]), over the strands of the mask."""
    return sum(a[3]["prop"] for s in (0, 1) if (strands >> s) & 1 for a in c.A[s])


@functools.lru_cache(maxsize=None)
def sparse_case():
    """6000 reads of 24 chars on the random text, k = 1: every tenth is a text slice with at most one
    edit, the rest are random and occur nowhere, so most pieces have no candidate and most reads
    no answer.  `e` is the batch of the ragged map call: every second text slice reverse-complemented
    and 4096 empty reads in the middle; its reads, both strands' answers and the reference records."""
    p = SPARSE
    t = make_text(p["text"])
    n, m, k = len(t), p["m"], p["k"]
    rng = np.random.default_rng(p["seed"])
    kinds = ("sub", "ins", "del")
    qs = []
    for i in range(p["nq"]):
        q = rng.integers(0, 4, m).astype(np.uint8)
        if i % p["every"] == 0:
            ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20)))
                   for _ in range(int(rng.integers(0, k + 1)))]
            ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
            s = int(rng.integers(0, n - ln + 1))
            q = edited(rng, t[s:s + ln], ops)
            assert len(q) == m
        qs.append(q)
    c = EditCase(t, qs, k)
    half = p["nq"] // 2
    empty = [np.zeros(0, np.uint8) for _ in range(p["empties"])]
    rcs = [revcomp_ref(q) for q in qs]
    fwd, rev = c.br.answers(qs, k, 0), c.br.answers(rcs, k, 0)
    # the map batch: every second text slice reverse-complemented (its two answers change places)
    flip = [i % (2 * p["every"]) == p["every"] for i in range(p["nq"])]
    mqs = [rcs[i] if f else qs[i] for i, f in enumerate(flip)]
    A = [[(rev if f else fwd)[i] for i, f in enumerate(flip)], [(fwd if f else rev)[i] for i, f in enumerate(flip)]]
    none = c.br.answer(empty[0], k, 0)
    eqs = mqs[:half] + empty + mqs[half:]
    A = [a[:half] + [none] * len(empty) + a[half:] for a in A]
    e = types.SimpleNamespace(k=k, mh=0, qs=eqs, A=A)
    e.qb, e.qoff, e.qlen = pack(eqs)
    e.ref = {3: map_ref_all(t, eqs, k, A[0], A[1], 3)}
    e.rc = np.concatenate([revcomp_ref(q) for q in eqs])
    frozen(e.qb, e.qoff, e.qlen, e.rc, *e.ref[3].values())
    c.e = e
    return c


def test_span():
    assert span([0, 0], 4) == 0
    assert span([0, 5], 4) == 1 and span([0, 4, 8], 4) == 1
    assert span([0, 3, 5], 4) == 2  # tile [0, 4) holds elements of both
    assert span([0, 1, 1, 1, 1, 2], 4) == 5  # entries without an element in between are part of the slice
    assert span([0, 0, 0, 7, 7], 4) == 1  # leading and trailing ones are not: p0 is the last entry <= t0
    assert span(np.arange(0, 101), 10) == 10 and span(np.arange(0, 101) * 3, 10) == 4


def test_tile_loop_cases_have_tiles_to_loop_over():
    """Every call of the tile-loop table runs at least 2 g + 1 tiles of its kernel for g = 3."""
    fig = {}
    for name, k in TILE_RUNS:
        c = edit_case(name, k)
        assert c.pieces.sum() == c.exp["cand"]  # the two counts of the brute force agree
        fig[(name, k)] = dict(edit=tiles(c.pieces.sum(), MM_T), mismatch=tiles(c.mm[1].sum(), MM_T),
                              align=tiles(c.na, AL_T))
        assert c.mm[1].sum() == c.mm[0]["cand"]
        for m in (64, 129):  # the fixed-length calls: their own candidates
            sel = [i for i, q in enumerate(c.qs) if len(q) == m]
            cand = sum(c.pieces[i * (k + 1):(i + 1) * (k + 1)].sum() for i in sel)
            fig[(name, k)]["edit m=%d" % m] = tiles(cand, MM_T)
        mc = map_case(name, k)
        fig[(name, k)].update({"select 3": tiles(proposals(mc, 3), MAP_T), "select 2": tiles(proposals(mc, 2), MAP_T),
                               "map bytes": tiles(2 * int(mc.qlen.sum()), AL_T)})
    for name, k, w in PAIR_RUNS:
        pc = pair_case(name, k)
        fwd = sum(intervals(np.asarray(a[0])) for a in pc.A[0])  # forward-strand loci: the join's elements
        fig[("pairs", name, k)] = {"loci": tiles(proposals(pc, 3), MAP_T), "join": tiles(fwd, MAP_T)}
    lc = {name: tiles(np.where(hi > lo, np.minimum(hi, LOC_N) - np.minimum(lo, LOC_N), 0).sum(), LOC_T)
          for name, (lo, hi) in locate_cases().items()}
    fig["locate"] = {name: nt for name, nt in lc.items() if nt >= MIN_TILES}
    assert len(fig["locate"]) >= 4, lc  # the others are there for their edges: empty, reversed, clipped
    print("tiles per call:", fig)
    for key, f in fig.items():
        for what, nt in f.items():
            if not what.startswith("edit m="):
                assert nt >= MIN_TILES, (key, what, nt)
    # the fixed-length calls are there for the kernels of 1 and 4 words of rows: on period7 they loop too
    assert all(fig[("period7", 1)]["edit m=%d" % m] >= 2 for m in (64, 129)), fig[("period7", 1)]


def test_sparse_case_overflows_the_lds_stage():
    """The sparse case's offsets: one tile's slice of them is larger than the kernels' LDS stage."""
    c = sparse_case()
    e = c.e
    k = c.k
    assert c.pieces.sum() == c.exp["cand"] and c.mm[1].sum() == c.mm[0]["cand"]
    fig = dict(
        candidates=int(c.pieces.sum()), pieces=len(c.pieces), ends=c.na,
        cand_span=span(csr(c.pieces), MM_T), mm_cand_span=span(csr(c.mm[1]), MM_T), answer_span=span(c.off, AL_T),
        byte_span=span(csr(np.concatenate([e.qlen, e.qlen]).astype(np.int64)), AL_T),
        revcomp_span=span(csr(e.qlen.astype(np.int64)), AL_T))
    # inside map_edit: the candidates of both strands' batch, and one alignment per mapped read
    both = np.concatenate([piece_counts(lambda p: len(c.br.occurrences(p)), e.qs, k, MAX_M),
                           piece_counts(lambda p: len(c.br.occurrences(p)), [revcomp_ref(q) for q in e.qs], k, MAX_M)])
    fig["map_cand_span"] = span(csr(both), MM_T)
    fig["map_align_span"] = span(csr(e.ref[3]["dist"] != NONE_DIST), AL_T)
    print("sparse case:", fig)
    assert fig["cand_span"] > MM_SLICE and fig["mm_cand_span"] > MM_SLICE   # locate_edit, locate_mismatch
    assert fig["answer_span"] > AL_SLICE                                    # align_edit
    assert fig["byte_span"] > AL_SLICE and fig["revcomp_span"] > AL_SLICE   # k_map_fill: map_edit, revcomp
    assert fig["map_cand_span"] > MM_SLICE and fig["map_align_span"] > AL_SLICE
    # it is sparse and not empty: reads with an answer on either side of the empties, most without one
    cnt = np.diff(c.off)
    half = SPARSE["nq"] // 2
    assert (cnt[:half] > 0).any() and (cnt[half:] > 0).any() and (cnt == 0).sum() > 5 * (cnt > 0).sum()
    mapped = e.ref[3]["dist"] != NONE_DIST
    assert mapped.sum() >= (cnt > 0).sum() and (e.ref[3]["strand"][mapped] == 1).any() and len(c.mm[0]["pos"]) > 300
    assert (e.qlen[half:half + SPARSE["empties"]] == 0).all() and e.qlen[half - 1] and e.qlen[half + SPARSE["empties"]]
    # none of the suite's other edit cases gets there: the gap this case closes
    for name, kk in TILE_RUNS:
        d = edit_case(name, kk)
        assert span(csr(d.pieces), MM_T) <= MM_SLICE and span(d.off, AL_T) <= AL_SLICE, (name, kk)


def test_symbol_declared_exported_and_bound(monkeypatch):
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    assert "sas_tile_grid_cap" in declared and hasattr(raw, "sas_tile_grid_cap")
    assert list(L.sas_tile_grid_cap.argtypes) == [] and L.sas_tile_grid_cap.restype == C.c_uint32
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    assert "uint32_t sas_tile_grid_cap(void);" in src and "SAS_TILE_GRID" in src
    # read at every call; unset, empty, zero, negative and no number are no cap
    monkeypatch.delenv("SAS_TILE_GRID", raising=False)
    assert L.sas_tile_grid_cap() == 0
    for v, cap in (("1", 1), ("3", 3), ("", 0), ("0", 0), ("-2", 0), ("x", 0), ("4096", 4096),
                   ("99999999999", 0xFFFFFFFF)):
        monkeypatch.setenv("SAS_TILE_GRID", v)
        assert L.sas_tile_grid_cap() == cap, v
    monkeypatch.delenv("SAS_TILE_GRID")
    assert L.sas_tile_grid_cap() == 0
