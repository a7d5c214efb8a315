"""Paired-end mapping (sas_map_pairs / sas_map_pairs_fixed and their Python mirrors) against the
numpy restatement of sas.h's definition (tests/test_pairs_host.py: pairs_ref_all over the brute
force's answers for each read and its reverse complement), bit for bit.  Pairs are cut from the
texts of tests/test_gpu_edit.py and from `selfrc`, a text that is its own reverse complement, the
only repetitive one here on which a proper pair exists at all."""
import errno
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_edit import BARE, BUILDS, EBrute, edited, make_text as edit_text
from test_gpu_map import as_dict as map_as_dict
from test_gpu_match import pack
from test_map_host import FIELDS as MAP_FIELDS, intervals, map_ref_all, revcomp_ref
from test_pairs_host import FIELDS, PAIR_FIELDS, categories, loci_reps, pairs_ref_all

pytestmark = pytest.mark.gpu

# (text, k, max_seed_hits); the last two skip seeds
RUNS = [("tiny", 0, 0), ("tiny", 1, 0), ("tiny", 2, 0), ("tiny", 3, 0), ("random", 1, 0), ("random", 3, 0),
        ("random", 15, 0), ("zero_tail", 3, 0), ("zeros", 3, 0), ("selfrc", 1, 0), ("selfrc", 3, 0),
        ("random", 2, 20), ("selfrc", 1, 3099)]
# the fragment windows of each text; the first is the one its shape assertions are made for
WINDOWS = {"selfrc": [(100, 700), (0, 400), (150, 151)]}
DEFAULT_WINDOWS = [(0, 400), (150, 151)]
WHOLE = ("quad_p8", "sa40", "quad_notable")
JOIN_TILE = 2048  # forward loci per workgroup tile of the join kernel
LOCI_TILE = 2048  # proposals per workgroup tile of the loci compaction
LENGTHS = (0, 8, 32, 63, 64, 65, 128, 256, 257)
CANARY = 64
SELFRC_N = 31000  # with the tail below 2^15 chars: the brute force keeps its rows in int16
SELFRC_PAIRS = 24
SELFRC_TAIL = 1500


def make_text(name):
    if name == "selfrc":
        # period 10 and equal to its own reverse complement: a read cut from it has a locus every 10
        # chars on both strands.  A random tail behind it carries the pairs that map in one place
        a = np.array([0, 2, 1, 1, 3], np.uint8)
        unit = np.concatenate([a, revcomp_ref(a)])
        return np.concatenate([np.tile(unit, SELFRC_N // len(unit)), O.random_string(SELFRC_TAIL, seed=14)])
    return edit_text(name)


def windows_of(name):
    return WINDOWS.get(name, DEFAULT_WINDOWS)


def make_pairs(t, name, k, seed):
    """The interleaved reads of one run: fragments t[s .. s + L) with mate 1 = edited(t[s .. s + m1))
    and mate 2 = rc(edited(t[s + L - m2 .. s + L))), up to k edits each, every second pair swapped."""
    rng = np.random.default_rng(seed)
    n = len(t)
    kinds = ("sub", "ins", "del")
    wins = windows_of(name)
    lo, hi = wins[0]
    reads = []

    def cut(s, m):
        ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20)))
               for _ in range(int(rng.integers(0, k + 1)))]
        if m > n:
            return rng.integers(0, 4, m).astype(np.uint8)
        # a read of m chars: a text slice of the length that the edits turn into m
        ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
        q = edited(rng, t[s:s + ln], ops) if 1 <= ln <= n - s else t[s:s + m]
        return q if len(q) == m else t[s:s + m].copy()

    def frag(L, m1, m2, kind="proper", s0=0, s1=n):
        """a fragment of L chars inside t[s0 .. s1)"""
        L = min(max(L, m1, m2, 1), s1 - s0)
        s = s0 + int(rng.integers(0, s1 - s0 - L + 1))
        a, b = cut(s, m1), revcomp_ref(cut(max(s + L - m2, 0), m2))
        if kind == "same":        # both mates from the same strand
            b = revcomp_ref(b)
        elif kind == "random":    # one random mate
            b = rng.integers(0, 4, max(m2, 24)).astype(np.uint8)
        elif kind == "outward":   # the mates face away from each other: F = m1 + m2 - L
            a, b = revcomp_ref(a), revcomp_ref(b)
        reads.extend([b, a] if (len(reads) // 2) % 2 else [a, b])

    if name == "selfrc":
        for _ in range(SELFRC_PAIRS):
            frag(int(rng.integers(lo, hi + 1)), 20, 20, s1=SELFRC_N)
        ms = (20, 33)
        frag = functools.partial(frag, s0=SELFRC_N)  # everything else from the random tail
    elif name == "tiny":
        ms = (k + 4, 9, 12)
    else:
        ms = (max(20, 3 * k + 8), 33, 64, 100)
    for m in ms:
        for _ in range(3):
            frag(int(rng.integers(max(lo, 150), hi + 1)), m, m)
        # just outside and just inside every bound of every window
        for b in sorted({b for w in wins for b in w}):
            for L in sorted({b - 1, b + 1, b - 1 - k, b - 1 + k, b + 1 - k, b + 1 + k}):
                if m <= L <= n:
                    frag(L, m, m)
        for kind in ("same", "random", "outward"):
            frag(int(rng.integers(max(lo, 150), hi + 1)), m, m, kind)
            frag(3 * m, m, m, kind)
    for m in LENGTHS:  # in both mate slots
        L = int(rng.integers(max(lo, 150), hi + 1))
        frag(L, m, 30)
        frag(L, m, 30)
        frag(L, m, m)
    if name != "selfrc":
        for m in (k + 1, k + 2, k + 3, 4 * k + 4, 5 * k + 4):  # short mates that occur in many places
            for _ in range(10 if m > k + 3 else 6):
                frag(int(rng.integers(10, 40)), m, m)
    assert len(reads) % 2 == 0
    return reads


class Case:
    """One (text, k, max_seed_hits) run: the interleaved reads, the brute force's answers on both
    strands, the single-read records and per window the reference.  Computed once, read-only,
    shared by every test."""

    def __init__(self, name, k, mh):
        self.name, self.k, self.mh = name, k, mh
        self.t = make_text(name)
        self.n = len(self.t)
        br = EBrute(self.t)
        self.qs = make_pairs(self.t, name, k, 4000 + 10 * RUNS.index((name, k, mh)) + k)
        self.rcs = [revcomp_ref(q) for q in self.qs]
        self.qb, self.qoff, self.qlen = pack(self.qs)
        self.A = (br.answers(self.qs, k, mh), br.answers(self.rcs, k, mh))
        self.single = map_ref_all(self.t, self.qs, k, self.A[0], self.A[1], 3)
        self.windows = windows_of(name)
        self._ref = {}
        for v in (self.qb, self.qoff, self.qlen) + tuple(self.single.values()):
            v.setflags(write=False)

    def ref(self, w):
        if w not in self._ref:
            r = pairs_ref_all(self.t, self.qs, self.k, self.A[0], self.A[1], w[0], w[1], base=self.single)
            for v in r.values():
                v.setflags(write=False)
            self._ref[w] = r
        return self._ref[w]


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name, k, mh=0):
        if (name, k, mh) not in made:
            made[(name, k, mh)] = Case(name, k, mh)
        return made[(name, k, mh)]
    return get


def cu(torch, a, dtype):
    """A device copy (the fixtures' arrays are read-only)."""
    return torch.from_numpy(np.array(a, dtype)).cuda()


def dev_call(torch, idx, c, w, u32=False, skip=(), flags=0, fixed=None):
    """sas_map_pairs on device pointers (fixed = (bytes, m): sas_map_pairs_fixed) into buffers with
    64 canary elements behind every output; the outputs named in `skip` are passed as NULL.
    Returns a dict of int64 arrays (None for a skipped output) and checks the canaries."""
    from sas_amd import _lib
    k = c.k
    stride = 2 * k + 1
    nq = len(c.qoff) if fixed is None else len(fixed[0]) // fixed[1]
    npairs = nq // 2
    pt = torch.int32 if u32 else torch.int64
    shape = dict(end=(nq, pt), start=(nq, pt), dist=(nq, torch.uint8), strand=(nq, torch.uint8),
                 n_best=(nq, torch.int32), n_loci=(nq, torch.int32), nruns=(nq, torch.uint8),
                 runs=(nq * stride, torch.int16), qflags=(nq, torch.uint8), pflags=(npairs, torch.uint8),
                 n_pairs=(npairs, torch.int32), n_best_pairs=(npairs, torch.int32))
    buf = {f: torch.full((cnt + CANARY,), 77, dtype=dt, device="cuda") for f, (cnt, dt) in shape.items()}
    ptr = [None if f in skip else buf[f].data_ptr() for f in FIELDS]
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    L = _lib.lib()
    if fixed is None:
        dq, do, dl = cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32)
        _lib.check(L.sas_map_pairs(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), npairs, k, c.mh, w[0], w[1],
                                   *ptr, st, fl))
    else:
        dq = cu(torch, fixed[0], np.uint8)
        _lib.check(L.sas_map_pairs_fixed(idx._h, dq.data_ptr(), fixed[1], npairs, k, c.mh, w[0], w[1], *ptr, st, fl))
    torch.cuda.synchronize()
    out = {}
    for f, (cnt, _) in shape.items():
        assert (buf[f][0 if f in skip else cnt:] == 77).all(), (f, "canary")
        out[f] = None if f in skip else buf[f][:cnt].cpu().numpy().astype(np.int64)
    if out["runs"] is not None:
        out["runs"] = (out["runs"] & 0xFFFF).reshape(nq, stride)
    for f in ("n_best", "n_loci", "n_pairs", "n_best_pairs"):
        if out[f] is not None:
            out[f] &= 0xFFFFFFFF
    return out


def as_dict(rec):
    """A MappedPairs tuple (numpy or torch) as int64 arrays."""
    out = {f: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64) for f, v in zip(FIELDS, rec)}
    out["runs"] &= 0xFFFF
    return out


def same(got, ref, what, reads=None):
    """Every field that was asked for equals the reference; reads: the rows of a selection of
    reads (whole pairs, in order)."""
    pairs = None if reads is None else reads[0::2] // 2
    for f in FIELDS:
        if got[f] is None:
            continue
        rows = reads if f in MAP_FIELDS else pairs
        r = ref[f] if rows is None else ref[f][rows]
        bad = np.flatnonzero((got[f] != r).reshape(len(r), -1).any(1))
        assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:5]], r[bad[:5]])


def forward_loci(c):
    """Per pair, the forward-strand loci of both mates: the join kernel's segment of that pair."""
    per_read = np.array([intervals(np.asarray(a[0])) for a in c.A[0]])
    return per_read[0::2] + per_read[1::2]


def test_cases_hold_every_shape_that_matters(cases):
    """From the brute force and the reference alone."""
    for name, k, mh in RUNS:
        c = cases(name, k, mh)
        w = c.windows[0]
        lens = c.qlen.astype(np.int64)
        assert set(LENGTHS) <= set(lens[0::2].tolist()) and set(LENGTHS) <= set(lens[1::2].tolist()), (name, k)
        fl = c.single["qflags"]
        assert (fl & 2).any() and (fl & 4).any()  # SAS_ED_SHORT, SAS_ED_LONG
        assert bool((fl & 1).any()) == (mh != 0), (name, k, mh)  # SAS_ED_TRUNCATED only in the capped runs
        if name == "zeros":  # the reverse complement of a run of As does not occur in it: no categories
            continue
        cat = categories(c.A, lens, c.ref(w), c.single)
        assert all(v.any() for v in cat.values()), (name, k, mh, {f: int(v.sum()) for f, v in cat.items()})
        # the narrow window cuts both ways: proper pairs and pairs just outside it
        narrow = c.ref((150, 151))["pflags"]
        if name != "tiny":
            assert narrow.any() and (c.ref(w)["pflags"] > narrow).any(), (name, k)
    for k, mh in ((1, 0), (3, 0)):
        c = cases("selfrc", k, mh)
        r = c.ref((100, 700))
        fl = forward_loci(c)
        off = np.concatenate([[0], np.cumsum(fl)])
        assert fl.max() > 2 * JOIN_TILE, (k, fl.max())  # whole tiles lie inside one pair's segment
        assert (off[:-1] // JOIN_TILE < (off[1:] - 1) // JOIN_TILE)[fl > 0].sum() >= 20, k  # segments over an edge
        assert r["n_pairs"].max() > 10 ** 4, (k, r["n_pairs"].max())
        # the partner window of some forward locus holds more than 30 reverse loci
        i = int(np.argmax(r["n_pairs"]))
        _, ey = loci_reps(c.A[1][2 * i + 1][0], c.A[1][2 * i + 1][1])
        _, ex = loci_reps(c.A[0][2 * i][0], c.A[0][2 * i][1])
        lo = ex - int(c.qlen[2 * i]) + 100
        held = np.searchsorted(ey, lo + 600, "right") - np.searchsorted(ey, lo, "left")
        assert held.max() > 30, (k, held.max())
    # one locus spans more than a tile of proposals: a read of As owns every end of the text of As,
    # and the sorted list holds each end once per candidate that proposes it (info["prop"])
    c = cases("zeros", 3)
    spans = [a[3]["prop"] for a in c.A[0] if len(a[0]) and intervals(np.asarray(a[0])) == 1]
    assert max(spans) > LOCI_TILE, max(spans)
    # proposals over many compaction tiles, loci heads in every part of them
    c = cases("selfrc", 3)
    prop = sum(a[3]["prop"] for s in (0, 1) for a in c.A[s])
    assert prop > 100 * LOCI_TILE


@pytest.mark.parametrize("build", WHOLE)
@pytest.mark.parametrize("name,k,mh", RUNS)
def test_pairs_equal_reference(sas, cases, name, k, mh, build):
    import torch
    c = cases(name, k, mh)
    idx = sas.SaNaive.build(c.t, **BUILDS[build])
    for w in c.windows:
        what = (name, k, mh, build, w)
        same(dev_call(torch, idx, c, w), c.ref(w), what + ("device",))
        if w == c.windows[0] or build == "quad_p8":
            host = idx.map_pairs(c.qb, c.qoff, c.qlen, k, w[0], w[1], max_seed_hits=mh)
            assert host.end.dtype == np.uint64 and host.runs.dtype == np.uint16 and host.n_pairs.dtype == np.uint32
            same(as_dict(host), c.ref(w), what + ("host",))


@pytest.mark.parametrize("name,k", [("random", 1), ("tiny", 2), ("selfrc", 1)])
def test_without_a_proper_pair_it_is_map_edit(sas, cases, name, k):
    """A window in which the reference shows no proper pair: every per-read field is map_edit's on the
    same interleaved reads, and the per-pair fields are 0."""
    import torch
    c = cases(name, k)
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    w = next(w for w in ((0, 0), (60000, 60000), (4000000000, 4000000000)) if not c.ref(w)["pflags"].any())
    got = dev_call(torch, idx, c, w)
    single = map_as_dict(idx.map_edit(c.qb, c.qoff, c.qlen, k))
    for f in MAP_FIELDS:
        assert np.array_equal(got[f], single[f]), (name, k, w, f)
    assert not any(got[f].any() for f in PAIR_FIELDS)
    same(got, c.ref(w), (name, k, w))


def test_best_pair_against_the_existing_calls(sas, cases):
    """For every proper pair the summed distance is at most that of any two ends, one of each mate on
    opposite strands, of the GPU's own locate_edit answers whose fragment length is in the window."""
    c = cases("random", 1)
    k, w = c.k, c.windows[0]
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    nq = len(c.qs)
    rcb, rco = sas.revcomp(c.qb, c.qoff, c.qlen)
    A = []
    for qb, qoff in ((c.qb, c.qoff), (rcb, rco[:-1])):
        off, end, dist, _ = idx.locate_edit(qb, qoff, c.qlen, k)
        A.append([(end[int(off[i]):int(off[i + 1])].astype(np.int64), dist[int(off[i]):int(off[i + 1])].astype(np.int64))
                  for i in range(nq)])
    got = as_dict(idx.map_pairs(c.qb, c.qoff, c.qlen, k, w[0], w[1]))
    checked = 0
    for i in np.flatnonzero(got["pflags"]):
        least = None
        for o in (0, 1):
            f, v = 2 * i + o, 2 * i + 1 - o
            (ex, dx), (ey, dy) = A[0][f], A[1][v]
            F = ey[None, :] - ex[:, None] + int(c.qlen[f])
            ok = (w[0] <= F) & (F <= w[1])
            if ok.any():
                s = int((dx[:, None] + dy[None, :])[ok].min())
                least = s if least is None else min(least, s)
        assert least is not None and got["dist"][2 * i] + got["dist"][2 * i + 1] <= least, (i, least)
        checked += 1
    assert checked > 20


def test_call_forms(sas, cases):
    import torch
    from sas_amd import _lib
    c = cases("random", 3)
    k, w = c.k, c.windows[0]
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    full = dev_call(torch, idx, c, w)
    same(full, c.ref(w), "device")
    # u32 against u64; the search without the prefix table; validated bytes
    same(dev_call(torch, idx, c, w, u32=True), full, "u32")
    same(dev_call(torch, idx, c, w, flags=_lib.SAS_NO_PREFIX_TABLE), full, "no table")
    same(dev_call(torch, idx, c, w, flags=_lib.SAS_VALIDATE), full, "validated")
    # the Python mirror: device tensors and host arrays, u64 and u32
    dargs = (cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32), k, w[0], w[1])
    mir = idx.map_pairs(*dargs)
    torch.cuda.synchronize()
    assert mir.end.dtype == torch.int64 and mir.runs.shape == (len(c.qs), 2 * k + 1) and mir.dist.is_cuda
    assert mir.n_pairs.shape == (len(c.qs) // 2,) and type(mir) is sas.MappedPairs
    same(as_dict(mir), full, "mirror")
    host = idx.map_pairs(c.qb, c.qoff, c.qlen, k, w[0], w[1], u32=True)
    assert host.end.dtype == np.uint32 and host.start.dtype == np.uint32
    same(as_dict(host), full, "host u32")
    with pytest.raises(ValueError):
        idx.map_pairs(c.qb, c.qoff[:-1], c.qlen[:-1], k, w[0], w[1])
    with pytest.raises(ValueError):
        idx.map_pairs_fixed(c.qb[:96], 32, k, w[0], w[1])
    # each optional output NULL in turn (its buffer stays untouched), and all of them at once
    optional = ("start", "strand", "n_best", "n_loci", "nruns", "runs", "qflags", "pflags", "n_pairs", "n_best_pairs")
    for skip in [(f,) for f in optional] + [optional]:
        got = dev_call(torch, idx, c, w, skip=skip, u32=len(skip) == 1 and skip[0] in ("start", "runs"))
        assert all((got[f] is None) == (f in skip) for f in FIELDS)
        same(got, full, skip)
    # the required outputs
    L = _lib.lib()
    npairs = len(c.qs) // 2
    end, dist = np.zeros(2 * npairs, np.uint64), np.zeros(2 * npairs, np.uint8)
    p = (c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data)
    nulls = (None,) * 10
    _lib.check(L.sas_map_pairs(idx._h, *p, npairs, k, 0, w[0], w[1], end.ctypes.data, None, dist.ctypes.data,
                               *nulls, 0))
    assert np.array_equal(end.astype(np.int64), full["end"]) and np.array_equal(dist.astype(np.int64), full["dist"])
    for e_, d_ in ((None, dist.ctypes.data), (end.ctypes.data, None)):
        assert L.sas_map_pairs(idx._h, *p, npairs, k, 0, w[0], w[1], e_, None, d_, *nulls, 0) == errno.EINVAL
    # bytes > 3: host pointers always validate, device pointers with SAS_VALIDATE
    badq = c.qb.copy()
    badq[int(c.qoff[2])] = 4
    assert c.qlen[2] > 0
    with pytest.raises(sas.SasError) as e:
        idx.map_pairs(badq, c.qoff, c.qlen, k, w[0], w[1])
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.map_pairs(cu(torch, badq, np.uint8), *dargs[1:], flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL


def test_fixed_length_agrees_with_ragged(sas, cases):
    import torch
    for name, k in (("random", 3), ("selfrc", 1)):
        c = cases(name, k)
        w = c.windows[0]
        idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
        lens = c.qlen.astype(np.int64)
        for m in (8, 20, 32, 33, 64, 65, 128, 256, 257):
            pairs = np.flatnonzero((lens[0::2] == m) & (lens[1::2] == m))
            if name == "selfrc" and m == 20:
                pairs = pairs[:4]
            if len(pairs) == 0:
                assert m in (20, 33), (name, k, m)  # the mate lengths that only one of the two texts has
                continue
            reads = np.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)
            fb = np.concatenate([c.qs[i] for i in reads])
            for u32 in (False, True):
                got = dev_call(torch, idx, c, w, u32=u32, fixed=(fb, m))
                same(got, c.ref(w), (name, k, m, u32, "device"), reads=reads)
            same(as_dict(idx.map_pairs_fixed(fb, m, k, w[0], w[1])), c.ref(w), (name, k, m, "host"), reads=reads)
            dev = idx.map_pairs_fixed(cu(torch, fb, np.uint8), m, k, w[0], w[1], u32=True)
            torch.cuda.synchronize()
            assert dev.end.dtype == torch.int32 and dev.runs.shape == (len(reads), 2 * k + 1)
            same(as_dict(dev), c.ref(w), (name, k, m, "mirror"), reads=reads)


def test_errors(sas, cases):
    from sas_amd import _lib
    c = cases("random", 1)
    t, n = c.t, c.n
    for idx in (sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100, n - 5), **BARE),  # sas_build_shard
                sas.SaNaive.build(t, lcp=False, tagged=True)):
        with pytest.raises(sas.SasError) as e:
            idx.map_pairs(c.qb, c.qoff, c.qlen, 1, 0, 400)
        assert e.value.code == errno.ENOTSUP
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    for k, lo, hi in ((16, 0, 400), (1, 0, 65536), (1, 1000, 66536), (1, 401, 400)):
        with pytest.raises(sas.SasError) as e:
            idx.map_pairs(c.qb, c.qoff, c.qlen, k, lo, hi)
        assert e.value.code == errno.EINVAL, (k, lo, hi)
        with pytest.raises(sas.SasError) as e:
            idx.map_pairs_fixed(c.qb[:128], 32, k, lo, hi)
        assert e.value.code == errno.EINVAL, (k, lo, hi)
    # np = 0 writes nothing and returns 0
    end, dist = np.full(4, 7, np.uint64), np.full(4, 7, np.uint8)
    assert _lib.lib().sas_map_pairs(idx._h, None, None, None, 0, 1, 0, 0, 400, end.ctypes.data, None, dist.ctypes.data,
                                    *((None,) * 10), 0) == 0
    assert (end == 7).all() and (dist == 7).all()
    empty = idx.map_pairs(c.qb, c.qoff[:0], c.qlen[:0], 1, 0, 400)
    assert [len(v) for v in empty] == [0] * 12
