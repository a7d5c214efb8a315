"""Read mapping (sas_map_edit / sas_map_edit_fixed / sas_revcomp* and their Python mirrors) against
the numpy restatement of sas.h's definition (tests/test_map_host.py: map_ref_all over the brute
force's answers for each read and its reverse complement), bit for bit.  Texts and queries are
those of tests/test_gpu_edit.py with every second query reverse-complemented and two reads that
equal their own reverse complement added."""
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from test_align_host import NONE_DIST
from test_gpu_edit import BARE, BUILDS, EBrute, TEXTS, make_queries, make_text
from test_gpu_match import pack
from test_map_host import FIELDS, intervals, map_ref, map_ref_all, revcomp_ref

pytestmark = pytest.mark.gpu

# (text, k, max_seed_hits); the last two skip seeds
RUNS = [("tiny", 0, 0), ("tiny", 1, 0), ("tiny", 2, 0), ("tiny", 3, 0), ("random", 1, 0), ("random", 3, 0),
        ("random", 15, 0), ("zero_tail", 3, 0), ("period7", 1, 0), ("period7", 3, 0), ("zeros", 2, 0),
        ("random", 2, 20), ("period7", 1, 64)]
WHOLE = ("quad_p8", "sa40", "quad_notable")
TILE = 2048  # proposals per workgroup tile of the select kernel
CANARY = 64


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


class Case:
    """One (text, k, max_seed_hits) run: the reads, the brute force's answers on both strands and
    the reference records per strand mask.  Computed once, read-only, shared by every build."""

    def __init__(self, name, k, mh):
        self.name, self.k, self.mh = name, k, mh
        self.t = make_text(name)
        self.n = len(self.t)
        br = EBrute(self.t)
        qs, _ = make_queries(self.t, k, 2000 + 10 * TEXTS.index(name) + k)
        qs = [revcomp_ref(q) if i % 2 else q for i, q in enumerate(qs)]
        for w in (4, 16):  # equal to their own reverse complement
            a = self.t[3:3 + w]
            qs.append(np.concatenate([a, revcomp_ref(a)]))
        self.qs = qs
        self.rcs = [revcomp_ref(q) for q in qs]
        self.qb, self.qoff, self.qlen = pack(qs)
        self.A = (br.answers(self.qs, k, mh), br.answers(self.rcs, k, mh))
        self.ref = {s: map_ref_all(self.t, qs, k, self.A[0], self.A[1], s) for s in (1, 2, 3)}
        for v in (self.qb, self.qoff, self.qlen) + tuple(x for r in self.ref.values() for x in r.values()):
            v.setflags(write=False)


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


def dev_call(torch, idx, c, strands=3, u32=False, skip=(), flags=0, fixed=None):
    """sas_map_edit on device pointers (fixed = (bytes, m): sas_map_edit_fixed) into buffers with 64
    canary elements behind every output; the outputs named in `skip` are passed as NULL.  Returns a
    dict of int64 arrays (None for a skipped output) and checks the canaries."""
    from sas_amd import _lib
    k = c.k
    stride = 2 * k + 1
    nq = len(c.qoff) if fixed is None else len(fixed[0]) // fixed[1]
    pt = torch.int32 if u32 else torch.int64
    shape = dict(end=(nq, pt), start=(nq, pt), dist=(nq, torch.uint8), strand=(nq, torch.uint8),
                 n_best=(nq, torch.int32), n_loci=(nq, torch.int32), nruns=(nq, torch.uint8),
                 runs=(nq * stride, torch.int16), qflags=(nq, torch.uint8))
    buf = {f: torch.full((cnt + CANARY,), 77, dtype=dt, device="cuda") for f, (cnt, dt) in shape.items()}
    ptr = [None if f in skip else buf[f].data_ptr() for f in FIELDS]
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    L = _lib.lib()
    if fixed is None:
        dq, do, dl = cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32)
        _lib.check(L.sas_map_edit(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, k, c.mh, strands, *ptr,
                                  st, fl))
    else:
        dq = cu(torch, fixed[0], np.uint8)
        _lib.check(L.sas_map_edit_fixed(idx._h, dq.data_ptr(), fixed[1], nq, k, c.mh, strands, *ptr, st, fl))
    torch.cuda.synchronize()
    out = {}
    for f, (cnt, _) in shape.items():
        assert (buf[f][0 if f in skip else cnt:] == 77).all(), (f, "canary")
        out[f] = None if f in skip else buf[f][:cnt].cpu().numpy().astype(np.int64)
    if out["runs"] is not None:
        out["runs"] = (out["runs"] & 0xFFFF).reshape(nq, stride)
    return out


def as_dict(rec):
    """A Mapped tuple (numpy or torch) as int64 arrays."""
    out = {f: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64) for f, v in zip(FIELDS, rec)}
    out["runs"] &= 0xFFFF
    return out


def same(got, ref, what, rows=None):
    for f in FIELDS:
        if got[f] is None:
            continue
        r = ref[f] if rows is None else ref[f][rows]
        bad = np.flatnonzero((got[f] != r).reshape(len(r), -1).any(1))
        assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:5]], r[bad[:5]])


def test_cases_hold_every_shape_that_matters(cases):
    """From the brute force and the reference alone: every category is present."""
    c = cases("random", 1)
    r, cnt0, cnt1 = c.ref[3], np.array([len(a[0]) for a in c.A[0]]), np.array([len(a[0]) for a in c.A[1]])
    mapped = r["dist"] != NONE_DIST
    assert (~mapped).any() and (mapped & (r["strand"] == 0)).any() and (r["strand"] == 1).any()
    assert ((cnt0 > 0) & (cnt1 > 0)).any() and (r["n_best"] > 1).any()
    assert ((r["n_best"] == 1) & (r["n_loci"] == 1)).any()
    assert np.array_equal(mapped, (cnt0 + cnt1) > 0) and np.array_equal(mapped, r["n_best"] >= 1)
    for name, k in (("period7", 3), ("tiny", 3)):  # two best intervals in one valley
        r = cases(name, k).ref[3]
        assert (r["n_loci"] < r["n_best"]).any(), (name, k)
    for name, k, mh in RUNS:
        c = cases(name, k, mh)
        lens = c.qlen.astype(np.int64)
        assert {0, 8, 32, 257} <= set(lens.tolist()), (name, k)
        if name != "tiny" and mh == 0:  # the bit-vector words' edges, among the mapped reads
            assert {63, 64, 65, 127, 128, 255, 256} <= set(lens[c.ref[3]["dist"] != NONE_DIST].tolist()), (name, k)
        assert all(np.array_equal(q, rq) for q, rq in zip(c.qs[-2:], c.rcs[-2:]))  # their own reverse complement
        fl = c.ref[3]["qflags"]
        assert (fl & 2).any() and (fl & 4).any()  # SAS_ED_SHORT, SAS_ED_LONG
        assert bool((fl & 1).any()) == (mh != 0), (name, k, mh)  # SAS_ED_TRUNCATED only in the capped runs
    for name, k in (("period7", 1), ("period7", 3), ("zeros", 2)):
        # the sorted list on the device holds every proposal of a (read, strand), duplicates included:
        # the brute force counts them (info["prop"]), so these are the segments the select kernel sees
        c = cases(name, k)
        prop = np.array([a[3]["prop"] for s in (0, 1) for a in c.A[s]])
        cnt = np.array([len(a[0]) for s in (0, 1) for a in c.A[s]])
        off = np.concatenate([[0], np.cumsum(prop)])
        assert off[-1] > 100 * TILE, (name, k, off[-1])
        assert (off[:-1] // TILE < (off[1:] - 1) // TILE)[prop > 0].sum() >= 50, (name, k)  # segments over an edge
        assert cnt.max() >= min(c.n, 1500), (name, k, cnt.max())  # one read owns nearly every end of a strand
        if (name, k) != ("period7", 1):
            # a read with more proposals than two tiles hold: whole tiles lie inside its segment; and the
            # valleys of a read that owns nearly every end merge into one interval
            assert (prop > 2 * TILE).sum() >= 20, (name, k)
            big = np.flatnonzero(cnt[:len(c.qs)] >= min(c.n, 1500))
            assert any(intervals(np.asarray(c.A[0][i][0])) == 1 for i in big), (name, k)


@pytest.mark.parametrize("build", WHOLE)
@pytest.mark.parametrize("name,k,mh", RUNS)
def test_map_equals_reference(sas, cases, name, k, mh, build):
    import torch
    c = cases(name, k, mh)
    idx = sas.SaNaive.build(c.t, **BUILDS[build])
    what = (name, k, mh, build)
    same(dev_call(torch, idx, c), c.ref[3], what + ("device",))
    host = idx.map_edit(c.qb, c.qoff, c.qlen, k, max_seed_hits=mh)
    assert host.end.dtype == np.uint64 and host.runs.dtype == np.uint16 and host.n_best.dtype == np.uint32
    same(as_dict(host), c.ref[3], what + ("host",))


@pytest.mark.parametrize("name,k,mh", [("tiny", 2, 0), ("random", 1, 0), ("period7", 3, 0), ("random", 2, 20)])
def test_one_strand_alone(sas, cases, name, k, mh):
    """strands = 1 / 2: the reduction of the forward / the reverse answers alone."""
    import torch
    c = cases(name, k, mh)
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    for strands in (1, 2):
        ref = c.ref[strands]
        assert (ref["strand"][ref["dist"] != NONE_DIST] == strands - 1).all()
        same(dev_call(torch, idx, c, strands=strands), ref, (name, k, mh, strands, "device"))
        same(as_dict(idx.map_edit(c.qb, c.qoff, c.qlen, k, max_seed_hits=mh, strands=strands)), ref,
             (name, k, mh, strands, "host"))
    assert not all(np.array_equal(c.ref[1][f], c.ref[2][f]) for f in FIELDS)


def test_fixed_length_agrees_with_ragged(sas, cases):
    import torch
    for name, k in (("random", 3), ("period7", 1)):
        c = cases(name, k)
        idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
        for m in (1, 33, 64, 65, 128, 129, 256, 257):
            sel = np.array([i for i, q in enumerate(c.qs) if len(q) == m])
            assert len(sel), (name, k, m)
            fb = np.concatenate([c.qs[i] for i in sel])
            for strands in (3, 2):
                for u32 in (False, True):
                    got = dev_call(torch, idx, c, strands=strands, u32=u32, fixed=(fb, m))
                    same(got, c.ref[strands], (name, k, m, strands, u32, "device"), rows=sel)
            same(as_dict(idx.map_edit_fixed(fb, m, k)), c.ref[3], (name, k, m, "host"), rows=sel)
            dev = idx.map_edit_fixed(cu(torch, fb, np.uint8), m, k, u32=True)
            torch.cuda.synchronize()
            assert dev.end.dtype == torch.int32 and dev.runs.shape == (len(sel), 2 * k + 1)
            same(as_dict(dev), c.ref[3], (name, k, m, "mirror"), rows=sel)


def test_call_forms(sas, cases):
    import torch
    from sas_amd import _lib
    c = cases("random", 3)
    k = c.k
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    full = dev_call(torch, idx, c)
    same(full, c.ref[3], "device")
    # u32 against u64; the search without the prefix table; validated bytes
    same(dev_call(torch, idx, c, u32=True), full, "u32")
    same(dev_call(torch, idx, c, flags=_lib.SAS_NO_PREFIX_TABLE), full, "no table")
    same(dev_call(torch, idx, c, flags=_lib.SAS_VALIDATE), full, "validated")
    # the Python mirror: device tensors and host arrays, u64 and u32
    dargs = (cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32), k)
    mir = idx.map_edit(*dargs)
    torch.cuda.synchronize()
    assert mir.end.dtype == torch.int64 and mir.runs.shape == (len(c.qs), 2 * k + 1) and mir.dist.is_cuda
    same(as_dict(mir), full, "mirror")
    host = idx.map_edit(c.qb, c.qoff, c.qlen, k, u32=True)
    assert host.end.dtype == np.uint32 and host.start.dtype == np.uint32
    same(as_dict(host), full, "host u32")
    # each optional output NULL in turn (its buffer stays untouched), and all of them at once
    optional = ("start", "strand", "n_best", "n_loci", "nruns", "runs", "qflags")
    for skip in [(f,) for f in optional] + [optional]:
        got = dev_call(torch, idx, c, skip=skip, u32=len(skip) == 1 and skip[0] in ("start", "runs"))
        assert all((got[f] is None) == (f in skip) for f in FIELDS)
        same(got, full, skip)
    L = _lib.lib()
    nq = len(c.qs)
    end, dist = np.zeros(nq, np.uint64), np.zeros(nq, np.uint8)
    p = (c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data)
    _lib.check(L.sas_map_edit(idx._h, *p, nq, k, 0, 3, end.ctypes.data, None, dist.ctypes.data, None, None, None,
                              None, None, None, None, 0))
    assert np.array_equal(end.astype(np.int64), full["end"]) and np.array_equal(dist.astype(np.int64), full["dist"])
    # the required outputs
    for e_, d_ in ((None, dist.ctypes.data), (end.ctypes.data, None)):
        assert L.sas_map_edit(idx._h, *p, nq, k, 0, 3, e_, None, d_, None, None, None, None, None, None, None,
                              0) == errno.EINVAL
    # bytes > 3: host pointers always validate, device pointers with SAS_VALIDATE
    badq = c.qb.copy()
    badq[int(c.qoff[-2])] = 4
    with pytest.raises(sas.SasError) as e:
        idx.map_edit(badq, c.qoff, c.qlen, k)
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.map_edit(cu(torch, badq, np.uint8), *dargs[1:], flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL


def test_revcomp(sas, cases):
    import torch
    c = cases("random", 1)
    rng = np.random.default_rng(5)
    # ragged, the inputs overlapping: slices of one buffer, in no order, an empty one among them
    buf = rng.integers(0, 4, 3000).astype(np.uint8)
    qlen = np.concatenate([rng.integers(0, 300, 400), [0, 1, 2999, 0]]).astype(np.uint32)
    qoff = np.array([rng.integers(0, 3000 - int(ln) + 1) for ln in qlen], np.uint64)
    exp = [revcomp_ref(buf[int(o):int(o) + int(ln)]) for o, ln in zip(qoff, qlen)]
    eoff = np.concatenate([[0], np.cumsum(qlen.astype(np.int64))])
    assert eoff[-1] > 20 * 1024 and eoff[-1] > 3 * len(buf)
    out, off = sas.revcomp(buf, qoff, qlen)
    assert out.dtype == np.uint8 and off.dtype == np.uint64
    assert np.array_equal(off.astype(np.int64), eoff) and np.array_equal(out, np.concatenate(exp))
    dout, doff = sas.revcomp(cu(torch, buf, np.uint8), cu(torch, qoff, np.int64), cu(torch, qlen, np.int32))
    torch.cuda.synchronize()
    assert np.array_equal(doff.cpu().numpy(), eoff) and np.array_equal(dout.cpu().numpy(), out)
    # the case's own reads
    out, off = sas.revcomp(c.qb, c.qoff, c.qlen)
    assert np.array_equal(out, np.concatenate(c.rcs))
    # fixed, m = 1 among them; nq = 0
    for m in (1, 2, 33, 100, 257):
        fb = rng.integers(0, 4, 37 * m).astype(np.uint8)
        fexp = np.concatenate([revcomp_ref(fb[i * m:(i + 1) * m]) for i in range(37)])
        assert np.array_equal(sas.revcomp(fb, m=m), fexp), m
        dev = sas.revcomp(cu(torch, fb, np.uint8), m=m)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), fexp), m
    out, off = sas.revcomp(buf, qoff[:0], qlen[:0])
    assert len(out) == 0 and off.tolist() == [0]
    dout, doff = sas.revcomp(cu(torch, buf, np.uint8), cu(torch, qoff[:0], np.int64), cu(torch, qlen[:0], np.int32))
    torch.cuda.synchronize()
    assert dout.numel() == 0 and doff.cpu().tolist() == [0]
    assert len(sas.revcomp(buf[:0], m=5)) == 0
    # bytes > 3
    bad = buf.copy()
    bad[int(qoff[3])] = 7
    assert qlen[3] > 0
    with pytest.raises(sas.SasError) as e:
        sas.revcomp(bad, qoff, qlen)
    assert e.value.code == errno.EINVAL


@pytest.mark.parametrize("name,k", [("random", 3), ("period7", 1)])
def test_composition_of_the_existing_calls(sas, cases, name, k):
    """The GPU's own locate_edit + align_edit on the reads and on sas.revcomp of them, reduced by the
    definition in numpy, give the records of map_edit."""
    c = cases(name, k)
    idx = sas.SaNaive.build(c.t, **BUILDS["quad_p8"])
    nq, n = len(c.qs), c.n
    rcb, rco = sas.revcomp(c.qb, c.qoff, c.qlen)
    A = []
    for qb, qoff in ((c.qb, c.qoff), (rcb, rco[:-1])):
        off, end, dist, qfl = idx.locate_edit(qb, qoff, c.qlen, k)
        A.append([(end[int(off[i]):int(off[i + 1])], dist[int(off[i]):int(off[i + 1])], int(qfl[i]))
                  for i in range(nq)])
    rec = np.array([map_ref(n, a0, a1, 3) for a0, a1 in zip(*A)], np.int64)
    got = as_dict(idx.map_edit(c.qb, c.qoff, c.qlen, k))
    for col, f in enumerate(("end", "dist", "strand", "n_best", "n_loci", "qflags")):
        assert np.array_equal(got[f], rec[:, col]), (name, k, f)
    # the winners through align_edit: one ragged batch of both strands' bytes
    mapped = rec[:, 1] != NONE_DIST
    both = np.concatenate([c.qb, rcb])
    choff = np.where(rec[:, 2] == 1, len(c.qb) + rco[:-1].astype(np.int64), c.qoff.astype(np.int64))
    aoff = np.concatenate([[0], np.cumsum(mapped)])
    start, dist, nruns, runs = idx.align_edit(both, choff, c.qlen, k, aoff, rec[mapped, 0])
    assert np.array_equal(got["start"][mapped], start.astype(np.int64))
    assert np.array_equal(got["dist"][mapped], dist.astype(np.int64))
    assert np.array_equal(got["nruns"][mapped], nruns.astype(np.int64))
    assert np.array_equal(got["runs"][mapped], runs.astype(np.int64))
    assert (got["start"][~mapped] == n).all() and not got["nruns"][~mapped].any() and not got["runs"][~mapped].any()


def test_errors(sas, cases):
    from sas_amd import _lib
    c = cases("random", 1)
    t, n = c.t, c.n
    for idx in (sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100, n - 5), **BARE),  # sas_build_shard
                sas.SaNaive.build(t, lcp=False, tagged=True)):
        with pytest.raises(sas.SasError) as e:
            idx.map_edit(c.qb, c.qoff, c.qlen, 1)
        assert e.value.code == errno.ENOTSUP
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    with pytest.raises(sas.SasError) as e:
        idx.map_edit(c.qb, c.qoff, c.qlen, 16)
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.map_edit_fixed(c.qb[:64], 32, 16)
    assert e.value.code == errno.EINVAL
    for strands in (0, 4):
        with pytest.raises(sas.SasError) as e:
            idx.map_edit(c.qb, c.qoff, c.qlen, 1, strands=strands)
        assert e.value.code == errno.EINVAL
    # nq = 0 writes nothing and returns 0
    end, dist = np.full(4, 7, np.uint64), np.full(4, 7, np.uint8)
    assert _lib.lib().sas_map_edit(idx._h, None, None, None, 0, 1, 0, 3, end.ctypes.data, None, dist.ctypes.data,
                                   None, None, None, None, None, None, None, 0) == 0
    assert (end == 7).all() and (dist == 7).all()
    empty = idx.map_edit(c.qb, c.qoff[:0], c.qlen[:0], 1)
    assert [len(v) for v in empty] == [0] * 9
