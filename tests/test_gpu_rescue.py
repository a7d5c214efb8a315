"""Paired-end mapping with mate rescue (sas_map_pairs_rescue / sas_map_pairs_rescue_fixed and their
Python mirrors) against the numpy restatement of sas.h's definition (tests/test_rescue_host.py:
rescue_ref_all over the brute force's answers and its full Sellers rows), bit for bit.  The pairs
are made by construction: a mate with more edits than the seeds bear beside a clean partner, on
either strand and in either slot; fragments across the boundary of `selfrc`, whose periodic part
loses every seed to max_seed_hits; windows cut at both text ends; partners of every word count;
candidate runs over a chunk edge of the scan; anchor counts at and above max_anchors."""
import errno

import numpy as np
import pytest

from sas_amd import _lib
from test_gpu_edit import BUILDS, EBrute, edited, make_text as edit_text
from test_gpu_match import pack
from test_gpu_pairs import CANARY, SELFRC_N, cu, dev_call as pairs_dev_call, make_text as pairs_text
from test_map_host import intervals, map_ref_all, revcomp_ref
from test_pairs_host import FIELDS as PAIR_FIELDS_ALL
from test_rescue_host import FIELDS, PROPER, RESCUED, Rows, SKIPPED, anchors_of, categories, rescue_ref_all, window_of

pytestmark = pytest.mark.gpu

CHUNK = _lib.SAS_RESCUE_CHUNK
# (text, k, k_rescue, max_seed_hits)
RUNS = [("random", 1, 1, 0), ("random", 1, 3, 0), ("random", 0, 15, 0), ("random", 3, 3, 0),
        ("tiny", 1, 1, 0), ("tiny", 1, 3, 0), ("tiny", 0, 15, 0), ("tiny", 3, 3, 0),
        ("selfrc", 1, 1, 3099), ("selfrc", 1, 2, 3099)]
# the last window has three chunks of ends, the third ragged
WINDOWS = [(0, 400), (150, 151), (60, 60 + 2 * CHUNK + 41)]
WHOLE = ("quad_p8", "sa40", "quad_notable")
MAX_ANCHORS = 4
PARTNER_MS = (257, 64, 65, 128, 256)
# the categories (tests/test_rescue_host.py: categories) that the first window of a run must hold
ALL = {"fwd_anchor", "rev_anchor", "beyond_k", "truncated", "skipped", "nothing", "runs2"}
NEEDS = {
    ("random", 1, 1, 0): {"skipped", "nothing"},                       # k_rescue = k, no seed skipped: a
    ("random", 3, 3, 0): {"skipped", "nothing"},                       # candidate is a locus's end off its window
    ("random", 1, 3, 0): ALL - {"truncated"},
    ("random", 0, 15, 0): ALL - {"truncated"},
    ("tiny", 1, 1, 0): {"skipped"},                                    # 40 chars: every window holds the text
    ("tiny", 3, 3, 0): {"skipped"},
    ("tiny", 1, 3, 0): {"fwd_anchor", "rev_anchor", "beyond_k", "skipped"},
    ("tiny", 0, 15, 0): {"fwd_anchor", "rev_anchor", "beyond_k", "skipped"},
    ("selfrc", 1, 1, 3099): ALL - {"beyond_k"},
    ("selfrc", 1, 2, 3099): ALL,
}


def make_text(name):
    return pairs_text(name) if name == "selfrc" else edit_text(name)


def make_pairs(t, name, k, kr, mh, seed):
    """The interleaved reads of one run.  A fragment t[s .. s + L) gives mate 1 = t[s .. s + m1) and
    mate 2 = rc(t[s + L - m2 .. s + L)), each with its own number of edits; `swap` puts them in the
    other slots."""
    rng = np.random.default_rng(seed)
    n = len(t)
    kinds = ("sub", "ins", "del")
    br = EBrute(t)
    reads = []

    def cut(s, m, edits, only=None):
        """a read of m chars: the text slice at s (cut to the text) of the length that the edits turn into m"""
        ops = [(only or kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(edits)]
        ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
        s = min(max(s, 0), max(n - ln, 0))
        q = edited(rng, t[s:s + ln], ops) if 1 <= ln <= n - s else t[s:s + m]
        return q if len(q) == m else t[s:s + m].copy()

    def put(a, b, swap=None):
        swap = (len(reads) // 2) % 2 if swap is None else swap
        reads.extend([b, a] if swap else [a, b])

    def frag(L, m1, m2, e1=0, e2=0, s=None, swap=None, s0=0, s1=n, only=None):
        L = min(max(L, m1, m2, 1), s1 - s0)
        s = s0 + int(rng.integers(0, s1 - s0 - L + 1)) if s is None else s
        put(cut(s, m1, e1, only), revcomp_ref(cut(s + L - m2, m2, e2, only)), swap)

    def rnd(m):
        return rng.integers(0, 4, m).astype(np.uint8)

    heavy = sorted({k + 1, kr}) if kr > k else [k]   # more edits than the seeds bear, where there is room
    if name == "tiny":
        for m in (kr + 4, 12, 16):
            for e in heavy:
                for swap in (0, 1):
                    frag(int(rng.integers(m, 30)), m, m, e, 0, swap=swap)    # reverse anchor
                    frag(int(rng.integers(m, 30)), m, m, 0, e, swap=swap)    # forward anchor
            frag(25, m, m)                                                   # proper
            put(cut(3, m, 0), rnd(m))                                        # nothing to find
            put(rnd(m), rnd(m))                                              # no locus at all
        for m in (k + 1, k + 2, kr, kr + 1):                                 # short mates: many loci, short partners
            if m:
                frag(20, m, 12)
                frag(20, 12, m)
        for m in (k + 2, k + 3):                                             # many loci and no proper candidate
            put(cut(5, m, 0), rnd(12))
            put(rnd(12), revcomp_ref(cut(9, m, 0)))
        return reads
    lo_t, hi_t = (SELFRC_N, n) if name == "selfrc" else (0, n)               # where a read maps in one place
    ms = (20, 33) if name == "selfrc" else (33, 64, 65, 100, 128)
    ms = tuple(m for m in ms if m > 2 * kr + 2)
    for m in ms:
        for e in heavy:
            for swap in (0, 1):
                frag(int(rng.integers(160, 380)), m, m, e, 0, swap=swap, s0=lo_t, s1=hi_t)   # reverse anchor
                frag(int(rng.integers(160, 380)), m, m, 0, e, swap=swap, s0=lo_t, s1=hi_t)   # forward anchor
        # the fragment length at every bound of every window, the heavy mate on either side
        for b in sorted({b for w in WINDOWS for b in w}):
            for L in (b - 1, b, b + 1):
                if m <= L:
                    frag(L, m, m, heavy[0], 0, s0=lo_t, s1=hi_t)
                    frag(L, m, m, 0, heavy[-1], s0=lo_t, s1=hi_t)
        for _ in range(2):
            frag(int(rng.integers(160, 380)), m, m, s0=lo_t, s1=hi_t)        # proper
            frag(int(rng.integers(160, 380)), m, m, k, k, s0=lo_t, s1=hi_t)
        # both mates map, no proper candidate: anchors on both sides
        frag(int(rng.integers(700, 900)), m, m, s0=lo_t, s1=hi_t)            # too long a fragment
        s = lo_t + int(rng.integers(0, hi_t - lo_t - 400))
        put(cut(s, m, 0), cut(s + 200, m, 0))                                # both from one strand
        put(revcomp_ref(cut(s, m, 0)), cut(s + 200, m, 0))                   # facing outwards
        put(cut(s, m, 0), rnd(max(m, 24)))                                   # nothing to find
        put(rnd(max(m, 24)), revcomp_ref(cut(s, m, 0)))
        put(rnd(max(m, 24)), rnd(max(m, 24)))                                # no locus at all
        # windows cut at 0 (reverse anchor near the text's start) and at n (forward anchor at its end)
        # (selfrc begins with its periodic part, where no read maps in few places)
        for L in (m + 5, 170):
            if name != "selfrc":
                frag(L, m, m, heavy[-1], 0, s=0)
            frag(L, m, m, 0, heavy[-1], s=n - L)
        put(cut(n - m, m, 0), rnd(40))         # (150, 151): the forward anchor's window starts behind n
        put(rnd(40), cut(n - m, m, 0))
    anchor_m = 40 if name != "selfrc" else 30
    for m in PARTNER_MS:                       # every word count of the partner, and one too long
        for swap in (0, 1):
            frag(300, anchor_m, m, 0, heavy[-1], swap=swap, s0=lo_t, s1=hi_t)
            frag(300, m, anchor_m, heavy[-1], 0, swap=swap, s0=lo_t, s1=hi_t)
    for m in sorted({0, k, k + 1, kr, kr + 1} - {0 if name == "selfrc" else -1}):   # partners at the short bound
        frag(200, anchor_m, m, s0=lo_t, s1=hi_t)
        frag(200, m, anchor_m, s0=lo_t, s1=hi_t)
    if kr > k:
        # a candidate run over a chunk edge: a partner with k + 1 substitutions whose valley of ends
        # is centred RS_CHUNK ends behind the window's first, for the forward and the reverse anchor
        for w in (WINDOWS[0], WINDOWS[2]):
            for m in (33, 100) if name != "selfrc" else (30,):
                frag(w[0] + CHUNK, m, m, 0, k + 1, s0=lo_t, s1=hi_t, only="sub")
                frag(w[1] - CHUNK, m, m, k + 1, 0, s0=lo_t, s1=hi_t, only="sub")
        # short heavy partners: several candidate runs in one window
        for m in (kr + 3, kr + 5):
            for _ in range(3):
                frag(int(rng.integers(160, 380)), anchor_m, m, 0, k + 1, s0=lo_t, s1=hi_t)
                frag(int(rng.integers(160, 380)), m, anchor_m, k + 1, 0, s0=lo_t, s1=hi_t)
    if name == "selfrc":
        # across the boundary: the forward mate in the periodic part loses every seed (TRUNCATED, no
        # locus), the reverse mate in the tail is the anchor and the window is full of candidates
        for L in (170, 230, 390):
            for swap in (0, 1):
                frag(L, 20, 30, swap=swap, s=SELFRC_N - L + 60)
        for j in range(10):   # the window at every phase of the period: in some a run of ends lies over a chunk edge
            frag(200 + j, 20, 30, s=SELFRC_N - 140)
        # a forward anchor at the tail's start whose reverse mate, ending 10 chars behind its start, lies
        # half in the periodic part (that seed is skipped) and has a substitution in the other half
        for swap in (0, 1):
            x = t[SELFRC_N - 10:SELFRC_N + 10].copy()
            x[15] = (x[15] + 1) & 3
            put(t[SELFRC_N:SELFRC_N + 20].copy(), revcomp_ref(x), swap)
        for _ in range(4):                                                   # no locus at all
            frag(int(rng.integers(160, 380)), 20, 20, s0=0, s1=SELFRC_N)
    # short mates that occur in many places, beside a partner without a locus: anchor counts around
    # MAX_ANCHORS, one pair exactly at it and one just above it
    want = {MAX_ANCHORS: 2, MAX_ANCHORS + 1: 2}
    for _ in range(4000):
        if not any(want.values()):
            break
        m = int(rng.integers(k + 4, 3 * k + 10))
        s = lo_t + int(rng.integers(0, hi_t - lo_t - 400))
        a = cut(s, m, 0)
        loci = sum(intervals(br.answer(q, k, mh)[0]) for q in (a, revcomp_ref(a)))
        if want.get(loci, 0):
            b = revcomp_ref(cut(s + 250, 40, heavy[-1] if kr > k else k + 1))
            if not any(br.answer(q, k, mh)[0] for q in (b, revcomp_ref(b))):
                want[loci] -= 1
                put(a, b)
    assert not any(want.values()), (name, k, kr, want)
    assert len(reads) % 2 == 0
    return reads


class Case:
    """One run: the interleaved reads, the brute force's answers on both strands, the single-read
    records aligned with k_rescue and per window the reference.  Computed once, read-only, shared by
    every test."""

    def __init__(self, name, k, kr, mh):
        self.name, self.k, self.kr, self.mh = name, k, kr, mh
        self.t = make_text(name)
        self.n = len(self.t)
        br = EBrute(self.t)
        self.rows = Rows(br)
        self.qs = make_pairs(self.t, name, k, kr, mh, 7000 + RUNS.index((name, k, kr, mh)))
        self.rcs = [revcomp_ref(q) for q in self.qs]
        self.qb, self.qoff, self.qlen = pack(self.qs)
        self.A = (br.answers(self.qs, k, mh), br.answers(self.rcs, k, mh))
        self.single = map_ref_all(self.t, self.qs, kr, self.A[0], self.A[1], 3)
        self._ref = {}
        for v in (self.qb, self.qoff, self.qlen) + tuple(self.single.values()):
            v.setflags(write=False)

    def ref(self, w, anchors=MAX_ANCHORS):
        if (w, anchors) not in self._ref:
            r = rescue_ref_all(self.t, self.qs, self.k, self.kr, self.A[0], self.A[1], w[0], w[1], anchors,
                               rows=self.rows, base=self.single)
            for v in r.values():
                v.setflags(write=False)
            self._ref[(w, anchors)] = r
        return self._ref[(w, anchors)]


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name, k, kr, mh=0):
        if (name, k, kr, mh) not in made:
            made[(name, k, kr, mh)] = Case(name, k, kr, mh)
        return made[(name, k, kr, mh)]
    return get


def dev_call(torch, idx, c, w, anchors=MAX_ANCHORS, u32=False, skip=(), flags=0, fixed=None, kr=None):
    """sas_map_pairs_rescue on device pointers (fixed = (bytes, m): sas_map_pairs_rescue_fixed) into
    buffers with 64 canary elements behind every output; the outputs named in `skip` are passed as
    NULL.  Returns a dict of int64 arrays (None for a skipped output) and checks the canaries."""
    k, kr = c.k, c.kr if kr is None else kr
    stride = 2 * kr + 1
    nq = len(c.qoff) if fixed is None else len(fixed[0]) // fixed[1]
    npairs = nq // 2
    pt = torch.int32 if u32 else torch.int64
    shape = dict(end=(nq, pt), start=(nq, pt), dist=(nq, torch.uint8), strand=(nq, torch.uint8),
                 n_best=(nq, torch.int32), n_loci=(nq, torch.int32), nruns=(nq, torch.uint8),
                 runs=(nq * stride, torch.int16), qflags=(nq, torch.uint8), pflags=(npairs, torch.uint8),
                 n_pairs=(npairs, torch.int32), n_best_pairs=(npairs, torch.int32), n_rescue=(npairs, torch.int32))
    buf = {f: torch.full((cnt + CANARY,), 77, dtype=dt, device="cuda") for f, (cnt, dt) in shape.items()}
    ptr = [None if f in skip else buf[f].data_ptr() for f in FIELDS]
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    L = _lib.lib()
    if fixed is None:
        dq, do, dl = cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32)
        _lib.check(L.sas_map_pairs_rescue(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), npairs, k, kr, c.mh,
                                          w[0], w[1], anchors, *ptr, st, fl))
    else:
        dq = cu(torch, fixed[0], np.uint8)
        _lib.check(L.sas_map_pairs_rescue_fixed(idx._h, dq.data_ptr(), fixed[1], npairs, k, kr, c.mh, w[0], w[1],
                                                anchors, *ptr, st, fl))
    torch.cuda.synchronize()
    out = {}
    for f, (cnt, _) in shape.items():
        assert (buf[f][0 if f in skip else cnt:] == 77).all(), (f, "canary")
        out[f] = None if f in skip else buf[f][:cnt].cpu().numpy().astype(np.int64)
    if out["runs"] is not None:
        out["runs"] = (out["runs"] & 0xFFFF).reshape(nq, stride)
    for f in ("n_best", "n_loci", "n_pairs", "n_best_pairs", "n_rescue"):
        if out[f] is not None:
            out[f] &= 0xFFFFFFFF
    return out


def as_dict(rec):
    """A MappedPairsRescue tuple (numpy or torch) as int64 arrays."""
    out = {f: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64) for f, v in zip(FIELDS, rec)}
    out["runs"] &= 0xFFFF
    for f in ("n_best", "n_loci", "n_pairs", "n_best_pairs", "n_rescue"):
        out[f] &= 0xFFFFFFFF
    return out


def same(got, ref, what, reads=None, fields=FIELDS):
    """Every field that was asked for equals the reference; reads: the rows of a selection of
    reads (whole pairs, in order)."""
    pairs = None if reads is None else reads[0::2] // 2
    for f in fields:
        if got[f] is None:
            continue
        rows = reads if f in FIELDS[:9] else pairs
        r = ref[f] if rows is None else ref[f][rows]
        bad = np.flatnonzero((got[f] != r).reshape(len(r), -1).any(1))
        assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:5]], r[bad[:5]])


def scan_shapes(c, w, anchors=MAX_ANCHORS):
    """From the reference alone: the work items of the scan (chunks that hold an end), and whether
    some candidate run crosses the chunk edge RS_CHUNK ends behind a window's unclipped first end."""
    ref = c.ref(w, anchors)
    items, over_edge = 0, False
    for i in np.flatnonzero(((ref["pflags"] & (PROPER | SKIPPED)) == 0)):
        for a, s, _, e_a in anchors_of(c.A, i):
            m_a, m_b = len(c.qs[a]), len(c.qs[a ^ 1])
            if m_b <= c.kr or m_b > 256:
                continue
            first = e_a - m_a + w[0] if s == 0 else e_a + m_b - w[1]
            lo, hi = window_of(c.n, s, e_a, m_a, m_b, w[0], w[1])
            if lo > hi:
                continue
            items += (hi - first) // CHUNK - (lo - first) // CHUNK + 1
            e = first + CHUNK
            if lo < e <= hi:
                D = c.rows(c.qs[a ^ 1] if s == 1 else revcomp_ref(c.qs[a ^ 1]))
                over_edge |= bool(D[e - 1] <= c.kr and D[e] <= c.kr)
    return items, over_edge


def test_cases_hold_every_shape_that_matters(cases):
    """From the brute force and the reference alone, before any GPU call."""
    for run in RUNS:
        name, k, kr, mh = run
        c = cases(*run)
        lens = c.qlen.astype(np.int64)
        ref = c.ref(WINDOWS[0])
        cat = categories(ref, k)
        have = {f for f, v in cat.items() if v.any()}
        assert NEEDS[run] <= have, (run, {f: int(v.sum()) for f, v in cat.items()})
        assert (ref["pflags"] & PROPER).any() and (c.single["dist"][0::2] == 255)[c.single["dist"][1::2] == 255].any()
        if name == "tiny":
            continue
        for side in (lens[0::2], lens[1::2]):
            assert set(PARTNER_MS) <= set(side.tolist()), run
        both_map = ((ref["pflags"] & PROPER) == 0) & (c.single["dist"][0::2] != 255) & (c.single["dist"][1::2] != 255)
        assert both_map.any(), run
        # the anchor counts at and just above the bound, with no proper candidate
        A = np.array([len(anchors_of(c.A, i)) for i in range(len(lens) // 2)])
        improper = (ref["pflags"] & PROPER) == 0
        assert (A[improper] == MAX_ANCHORS).any() and (A[improper] == MAX_ANCHORS + 1).any(), run
        assert ((ref["pflags"] & SKIPPED) != 0)[improper & (A == MAX_ANCHORS + 1)].all()
        assert not (ref["pflags"] & SKIPPED)[A <= MAX_ANCHORS].any()
        # windows cut at both text ends and an empty one (the narrow window of a forward anchor at n)
        cut0 = cutn = empty = False
        for w in WINDOWS:
            r = c.ref(w)
            for i in np.flatnonzero((r["pflags"] & (PROPER | SKIPPED)) == 0):
                for a, s, _, e_a in anchors_of(c.A, i):
                    m_a, m_b = len(c.qs[a]), len(c.qs[a ^ 1])
                    first = e_a - m_a + w[0] if s == 0 else e_a + m_b - w[1]
                    lo, hi = window_of(c.n, s, e_a, m_a, m_b, w[0], w[1])
                    cut0 |= first < 0 <= hi
                    cutn |= lo <= c.n < first + w[1] - w[0]
                    empty |= lo > hi
        assert (cut0 or name == "selfrc") and cutn and empty, (run, cut0, cutn, empty)
        for w in (WINDOWS[0], WINDOWS[2]):
            items, over_edge = scan_shapes(c, w)
            assert items >= 3 * 64, (run, w, items)
            assert over_edge or kr == k, (run, w)
        if kr > k:   # some rescued mate is beyond k in every window
            assert all(categories(c.ref(w), k)["beyond_k"].any() for w in WINDOWS), run


@pytest.mark.parametrize("build", WHOLE)
@pytest.mark.parametrize("name,k,kr,mh", RUNS)
def test_rescue_equals_reference(sas, cases, name, k, kr, mh, build):
    import torch
    c = cases(name, k, kr, mh)
    for w in WINDOWS:
        c.ref(w)   # the reference stands before the GPU is asked
    idx = sas.SaNaive.build(c.t, **BUILDS[build])
    for w in WINDOWS:
        what = (name, k, kr, mh, build, w)
        same(dev_call(torch, idx, c, w), c.ref(w), what + ("device",))
        if w == WINDOWS[0] and build == "quad_p8":
            host = idx.map_pairs_rescue(c.qb, c.qoff, c.qlen, k, kr, w[0], w[1], MAX_ANCHORS, max_seed_hits=mh)
            assert host.end.dtype == np.uint64 and host.runs.dtype == np.uint16 and host.n_rescue.dtype == np.uint32
            assert host.runs.shape == (len(c.qs), 2 * kr + 1)
            same(as_dict(host), c.ref(w), what + ("host",))


@pytest.mark.parametrize("name,k,mh", [("random", 1, 0), ("random", 3, 0), ("selfrc", 1, 3099)])
def test_rescue_off_is_map_pairs(sas, cases, name, k, mh):
    """max_anchors = 0 and k_rescue = k: every shared output equals sas_map_pairs' on the same reads,
    on device and on host pointers, and n_rescue is 0."""
    import torch
    c = cases(name, k, k, mh)
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    for w in WINDOWS[:2]:
        plain = pairs_dev_call(torch, idx, c, w)
        got = dev_call(torch, idx, c, w, anchors=0)
        for f in PAIR_FIELDS_ALL:
            assert np.array_equal(got[f], plain[f]), (name, k, w, f)
        assert not got["n_rescue"].any()
        same(got, c.ref(w, 0), (name, k, w, "reference"))
    w = WINDOWS[0]
    hp = idx.map_pairs(c.qb, c.qoff, c.qlen, k, w[0], w[1], max_seed_hits=mh)
    hr = idx.map_pairs_rescue(c.qb, c.qoff, c.qlen, k, k, w[0], w[1], 0, max_seed_hits=mh)
    for f, a, b in zip(PAIR_FIELDS_ALL, hp, hr):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, k, f)
    assert not hr.n_rescue.any()


def test_call_forms(sas, cases):
    import torch
    c = cases("random", 1, 3)
    k, kr, w = c.k, c.kr, WINDOWS[0]
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    full = dev_call(torch, idx, c, w)
    same(full, c.ref(w), "device")
    # u32 against u64; the search without the prefix table; validated bytes
    same(dev_call(torch, idx, c, w, u32=True), full, "u32")
    same(dev_call(torch, idx, c, w, flags=_lib.SAS_NO_PREFIX_TABLE), full, "no table")
    same(dev_call(torch, idx, c, w, flags=_lib.SAS_VALIDATE), full, "validated")
    # another bound on the anchors: fewer pairs are eligible
    same(dev_call(torch, idx, c, w, anchors=1), c.ref(w, 1), "one anchor")
    # the Python mirror: device tensors and host arrays, u64 and u32
    dargs = (cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32), k, kr, w[0], w[1],
             MAX_ANCHORS)
    mir = idx.map_pairs_rescue(*dargs)
    torch.cuda.synchronize()
    assert mir.end.dtype == torch.int64 and mir.runs.shape == (len(c.qs), 2 * kr + 1) and mir.dist.is_cuda
    assert mir.n_rescue.shape == (len(c.qs) // 2,) and type(mir) is sas.MappedPairsRescue
    same(as_dict(mir), full, "mirror")
    host = idx.map_pairs_rescue(c.qb, c.qoff, c.qlen, k, kr, w[0], w[1], MAX_ANCHORS, u32=True)
    assert host.end.dtype == np.uint32 and host.start.dtype == np.uint32
    same(as_dict(host), full, "host u32")
    with pytest.raises(ValueError):
        idx.map_pairs_rescue(c.qb, c.qoff[:-1], c.qlen[:-1], k, kr, w[0], w[1], MAX_ANCHORS)
    with pytest.raises(ValueError):
        idx.map_pairs_rescue_fixed(c.qb[:96], 32, k, kr, w[0], w[1], MAX_ANCHORS)
    # each optional output NULL in turn (its buffer stays untouched), and all of them at once
    optional = ("start", "strand", "n_best", "n_loci", "nruns", "runs", "qflags", "pflags", "n_pairs", "n_best_pairs",
                "n_rescue")
    for skip in [(f,) for f in optional] + [optional]:
        got = dev_call(torch, idx, c, w, skip=skip, u32=len(skip) == 1 and skip[0] in ("start", "runs"))
        assert all((got[f] is None) == (f in skip) for f in FIELDS)
        same(got, full, skip)
    # the required outputs
    L = _lib.lib()
    npairs = len(c.qs) // 2
    end, dist = np.zeros(2 * npairs, np.uint64), np.zeros(2 * npairs, np.uint8)
    p = (c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data)
    nulls = (None,) * 11
    _lib.check(L.sas_map_pairs_rescue(idx._h, *p, npairs, k, kr, 0, w[0], w[1], MAX_ANCHORS, end.ctypes.data, None,
                                      dist.ctypes.data, *nulls, 0))
    assert np.array_equal(end.astype(np.int64), full["end"]) and np.array_equal(dist.astype(np.int64), full["dist"])
    for e_, d_ in ((None, dist.ctypes.data), (end.ctypes.data, None)):
        assert L.sas_map_pairs_rescue(idx._h, *p, npairs, k, kr, 0, w[0], w[1], MAX_ANCHORS, e_, None, d_, *nulls,
                                      0) == errno.EINVAL
    # bytes > 3: host pointers always validate, device pointers with SAS_VALIDATE
    badq = c.qb.copy()
    badq[int(c.qoff[2])] = 4
    assert c.qlen[2] > 0
    with pytest.raises(sas.SasError) as e:
        idx.map_pairs_rescue(badq, c.qoff, c.qlen, k, kr, w[0], w[1], MAX_ANCHORS)
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.map_pairs_rescue(cu(torch, badq, np.uint8), *dargs[1:], flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL


def test_fixed_length_agrees_with_ragged(sas, cases):
    import torch
    for run in (("random", 1, 3, 0), ("selfrc", 1, 2, 3099)):
        c = cases(*run)
        k, kr, w = c.k, c.kr, WINDOWS[0]
        idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
        lens = c.qlen.astype(np.int64)
        seen = 0
        for m in (20, 30, 33, 64, 65, 100, 128, 256, 257):
            pairs = np.flatnonzero((lens[0::2] == m) & (lens[1::2] == m))
            if len(pairs) == 0:
                continue
            seen += 1
            reads = np.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)
            fb = np.concatenate([c.qs[i] for i in reads])
            for u32 in (False, True):
                got = dev_call(torch, idx, c, w, u32=u32, fixed=(fb, m))
                same(got, c.ref(w), run + (m, u32, "device"), reads=reads)
            host = idx.map_pairs_rescue_fixed(fb, m, k, kr, w[0], w[1], MAX_ANCHORS, max_seed_hits=c.mh)
            same(as_dict(host), c.ref(w), run + (m, "host"), reads=reads)
            dev = idx.map_pairs_rescue_fixed(cu(torch, fb, np.uint8), m, k, kr, w[0], w[1], MAX_ANCHORS,
                                             max_seed_hits=c.mh, u32=True)
            torch.cuda.synchronize()
            assert dev.end.dtype == torch.int32 and dev.runs.shape == (len(reads), 2 * kr + 1)
            same(as_dict(dev), c.ref(w), run + (m, "mirror"), reads=reads)
        assert seen >= 2, run
    # the word counts of the fixed-length kernels: rescued pairs of 64, 65 .. 128 and 129 .. 256 chars
    c = cases("random", 1, 3)
    ref = c.ref(WINDOWS[0])
    lens = c.qlen.astype(np.int64)
    for m in (64, 65, 100, 128):
        pairs = np.flatnonzero((lens[0::2] == m) & (lens[1::2] == m))
        assert (ref["pflags"][pairs] & RESCUED).any(), m


def test_errors(sas, cases):
    c = cases("random", 1, 3)
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    for k, kr, lo, hi in ((16, 16, 0, 400), (1, 0, 0, 400), (1, 16, 0, 400), (1, 3, 0, 65536), (1, 3, 401, 400)):
        with pytest.raises(sas.SasError) as e:
            idx.map_pairs_rescue(c.qb, c.qoff, c.qlen, k, kr, lo, hi, MAX_ANCHORS)
        assert e.value.code == errno.EINVAL, (k, kr, lo, hi)
        with pytest.raises(sas.SasError) as e:
            idx.map_pairs_rescue_fixed(c.qb[:128], 32, k, kr, lo, hi, MAX_ANCHORS)
        assert e.value.code == errno.EINVAL, (k, kr, lo, hi)
    tagged = sas.SaNaive.build(c.t, lcp=False, tagged=True)
    with pytest.raises(sas.SasError) as e:
        tagged.map_pairs_rescue(c.qb, c.qoff, c.qlen, 1, 3, 0, 400, MAX_ANCHORS)
    assert e.value.code == errno.ENOTSUP
    # np = 0 writes nothing and returns 0
    end, dist = np.full(4, 7, np.uint64), np.full(4, 7, np.uint8)
    assert _lib.lib().sas_map_pairs_rescue(idx._h, None, None, None, 0, 1, 3, 0, 0, 400, MAX_ANCHORS, end.ctypes.data,
                                           None, dist.ctypes.data, *((None,) * 11), 0) == 0
    assert (end == 7).all() and (dist == 7).all()
    empty = idx.map_pairs_rescue(c.qb, c.qoff[:0], c.qlen[:0], 1, 3, 0, 400, MAX_ANCHORS)
    assert [len(v) for v in empty] == [0] * 13


@pytest.mark.parametrize("g", ("1", "2"))
def test_scan_tile_loop(sas, cases, g, monkeypatch):
    """SAS_TILE_GRID caps the scan's grid at g workgroups of 256 lanes, so the (at least 3 x 64) work
    items are taken in several strides of the grid; the results are those of the run without a cap."""
    import torch
    from test_gpu_tiles import tile_grid
    for run in (("random", 1, 3, 0), ("random", 0, 15, 0)):
        c = cases(*run)
        for w in (WINDOWS[0], WINDOWS[2]):
            assert scan_shapes(c, w)[0] > 256 * int(g), (run, w)
        idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
        for w in (WINDOWS[0], WINDOWS[2]):
            free = dev_call(torch, idx, c, w)
            with tile_grid(monkeypatch, g):
                capped = dev_call(torch, idx, c, w)
            same(capped, free, run + (w, g))
            same(capped, c.ref(w), run + (w, g, "reference"))
