"""Alignment start and edit script (sas_align_edit / sas_align_edit_fixed and SaNaive.align_edit*)
against the numpy restatement of sas.h's definition (tests/test_align_host.py: align_ref), bit for
bit, and against structural facts that need no reference.  The alignments fed in are the brute
force's ends (tests/test_gpu_edit.py: EBrute), so nothing here rests on sas_locate_edit except
the one chained run."""
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from test_align_host import DEL, EQ, INS, NONE_DIST, X, align_ref_all, align_ref_sel
from test_gpu_edit import BARE, BUILDS, EBrute, TEXTS, expected, make_queries, make_text
from test_gpu_match import pack

pytestmark = pytest.mark.gpu

RUNS = [("tiny", 0), ("tiny", 1), ("tiny", 2), ("tiny", 3), ("random", 1), ("random", 3), ("random", 15),
        ("zero_tail", 3), ("period7", 1), ("zeros", 2)]
WHOLE = ("quad_p8", "sa40")
COMPARE_ALL = 5000   # a run with at most this many alignments is compared in full
SAMPLE = 3000        # otherwise: at least this many, with each query's first and last alignment
EDGES = (63, 64, 65, 127, 128, 129, 255, 256)


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


def make_index(sas, t, build):
    if build == "shard":  # a rank range of the SA: the text is whole, so it is served
        return sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100 if len(t) > 200 else 3, len(t) - 5), **BARE)
    return sas.SaNaive.build(t, **BUILDS[build])


class Case:
    """One (text, k) run: the queries, the brute force's ends and the reference of the compared
    alignments.  Computed once, read-only, shared by every build."""

    def __init__(self, name, k):
        self.name, self.k = name, k
        self.t = make_text(name)
        self.n = len(self.t)
        self.br = EBrute(self.t)
        self.qs, _ = make_queries(self.t, k, 2000 + 10 * TEXTS.index(name) + k)
        self.qb, self.qoff, self.qlen = pack(self.qs)
        exp = expected(self.br, self.qs, k, 0)
        self.off, self.end, self.dist = exp["off"], exp["end"], exp["dist"]
        self.na = len(self.end)
        self.qi = np.searchsorted(self.off, np.arange(self.na), side="right") - 1
        if self.na <= COMPARE_ALL:
            self.sel = np.arange(self.na)
        else:
            cnt = np.diff(self.off)
            edge = np.concatenate([self.off[:-1][cnt > 0], self.off[1:][cnt > 0] - 1])
            rnd = np.random.default_rng(77).choice(self.na, SAMPLE, replace=False)
            self.sel = np.unique(np.concatenate([edge, rnd]))
        self.ref = align_ref_sel(self.t, self.qs, self.qi, self.end, k, self.sel)
        for v in (self.qb, self.qoff, self.qlen, self.qi, self.sel) + tuple(self.ref):
            v.setflags(write=False)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name, k):
        if (name, k) not in made:
            made[(name, k)] = Case(name, k)
        return made[(name, k)]
    return get


def cu(torch, a, dtype):
    """A device copy (the fixtures' arrays are read-only)."""
    return torch.from_numpy(np.array(a, dtype)).cuda()


def dev_call(torch, idx, qb, qoff, qlen, k, off, end, na=None, u32=False, outs=(True, True, True), flags=0,
             fixed_m=None):
    """sas_align_edit (or _fixed) on device pointers into buffers with 64 canary elements behind
    every output; `na` below len(end): nothing at or past it is written.  Returns numpy (start,
    dist, nruns, runs), None for an output passed as NULL."""
    from sas_amd import _lib
    stride = 2 * k + 1
    full = len(end)
    na = full if na is None else na
    dq, doff = cu(torch, qb, np.uint8), cu(torch, off, np.int64)
    dend = cu(torch, end, np.int32 if u32 else np.int64)
    start = torch.full((full + 64,), -7, dtype=torch.int32 if u32 else torch.int64, device="cuda")
    dist = torch.full((full + 64,), 99, dtype=torch.uint8, device="cuda")
    nruns = torch.full((full + 64,), 99, dtype=torch.uint8, device="cuda")
    runs = torch.full(((full + 64) * stride,), -7, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    tail = (k, doff.data_ptr(), dend.data_ptr(), na, start.data_ptr(), dist.data_ptr() if outs[0] else None,
            nruns.data_ptr() if outs[1] else None, runs.data_ptr() if outs[2] else None, st, fl)
    if fixed_m is None:
        do, dl = cu(torch, qoff, np.int64), cu(torch, qlen, np.int32)
        _lib.check(_lib.lib().sas_align_edit(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), len(qoff), *tail))
    else:
        _lib.check(_lib.lib().sas_align_edit_fixed(idx._h, dq.data_ptr(), fixed_m, len(off) - 1, *tail))
    torch.cuda.synchronize()
    w = min(na, int(off[-1]))
    assert (start[w:] == -7).all() and (runs[w * stride:] == -7).all()
    assert (dist[0 if not outs[0] else w:] == 99).all() and (nruns[0 if not outs[1] else w:] == 99).all()
    assert outs[2] or (runs == -7).all()
    return (start[:w].cpu().numpy().astype(np.int64), dist[:w].cpu().numpy().astype(np.int64) if outs[0] else None,
            nruns[:w].cpu().numpy().astype(np.int64) if outs[1] else None,
            runs[:w * stride].cpu().numpy().astype(np.int64).reshape(w, stride) if outs[2] else None)


def structure(c, got, what):
    """Every alignment of a run, from the GPU output alone (and the brute force's D(e))."""
    start, dist, nruns, runs = got
    k, stride = c.k, 2 * c.k + 1
    m = c.qlen[c.qi].astype(np.int64)
    assert np.array_equal(dist, c.dist), (what, "dist")
    assert (nruns <= stride).all() and (nruns >= 1).all(), (what, "nruns")
    used = np.arange(stride)[None, :] < nruns[:, None]
    ops, lens = runs & 3, runs >> 2
    assert not runs[~used].any() and (lens[used] > 0).all(), (what, "slots")
    assert (np.where(ops != DEL, lens, 0).sum(1) == m).all(), (what, "query chars")
    assert (np.where(ops != INS, lens, 0).sum(1) == c.end - start).all(), (what, "text chars")
    assert (np.where(used & (ops != EQ), lens, 0).sum(1) == dist).all(), (what, "edits")
    assert (ops[:, 1:] != ops[:, :-1])[used[:, 1:]].all(), (what, "adjacent runs")
    assert (start >= np.maximum(c.end - m - k, 0)).all() and (start <= c.end).all(), (what, "window")
    # the replay: every = run copies the text, every X run differs from it char by char
    qlens = np.where(ops != DEL, lens, 0)
    tlens = np.where(ops != INS, lens, 0)
    i0 = np.cumsum(qlens, axis=1) - qlens + c.qoff[c.qi].astype(np.int64)[:, None]
    j0 = np.cumsum(tlens, axis=1) - tlens + start[:, None]
    for a0 in range(0, len(start), 20000):
        sl = slice(a0, a0 + 20000)
        diag = used[sl] & (ops[sl] <= X)
        ln, iq, jt, op = lens[sl][diag], i0[sl][diag], j0[sl][diag], ops[sl][diag]
        within = np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln)
        same = c.qb[np.repeat(iq, ln) + within] == c.t[np.repeat(jt, ln) + within]
        assert np.array_equal(same, np.repeat(op, ln) == EQ), (what, "replay")


def compare(c, got, what):
    """Bit for bit against the reference, on the run's compared alignments."""
    for g, r, nm in zip(got, c.ref, ("start", "dist", "nruns", "runs")):
        bad = np.flatnonzero((g[c.sel] != r).reshape(len(c.sel), -1).any(1))
        assert len(bad) == 0, (what, nm, c.sel[bad[:3]], g[c.sel[bad[:3]]], r[bad[:3]])


def test_cases_hold_the_shapes_that_matter(cases):
    """The caps on what is compared, and what the cases must contain, from the brute force and
    the reference alone."""
    ops_seen, longest = set(), 0
    for name, k in RUNS:
        c = cases(name, k)
        cnt = np.diff(c.off)
        if c.na <= COMPARE_ALL:
            assert len(c.sel) == c.na
        else:
            assert len(c.sel) >= SAMPLE
            assert np.isin(c.off[:-1][cnt > 0], c.sel).all() and np.isin(c.off[1:][cnt > 0] - 1, c.sel).all()
        start, dist, nruns, runs = c.ref
        assert np.array_equal(dist, c.dist[c.sel])  # d is D(e) wherever that is <= k
        assert (nruns >= 1).all() and (nruns <= 2 * k + 1).all()
        assert ((runs[:, 0] & 3) != DEL).all()  # the largest start: the script never opens with D
        ops_seen |= set(np.unique(runs[runs > 0] & 3).tolist())
        longest = max(longest, int(nruns.max()))
        m = c.qlen[c.qi[c.sel]].astype(np.int64)
        if name != "zeros":
            assert (c.end[c.sel] == c.n).any() and (start == 0).any(), (name, k)
        if k:
            assert (c.end[c.sel] < m).any(), (name, k)  # the window is cut at 0
        if name in ("random", "period7", "zero_tail"):
            assert set(EDGES) <= set(m.tolist()), (name, k)
            # more than two tiles; queries without an alignment between queries that have some
            has = np.flatnonzero(cnt > 0)
            assert c.na > 2048 and (cnt[has[0]:has[-1]] == 0).any(), (name, k)
        if k == 0:
            assert (nruns == 1).all() and ((runs[:, 0] & 3) == EQ).all()
    assert cases("tiny", 3).na <= COMPARE_ALL and cases("random", 15).na > COMPARE_ALL
    c = cases("period7", 1)  # one query's alignments span several tiles
    assert (c.off[:-1] // 2048 < (c.off[1:] - 1) // 2048)[np.diff(c.off) > 0].any()
    assert ops_seen == {EQ, X, INS, DEL} and longest > 15, (ops_seen, longest)


@pytest.mark.parametrize("build", WHOLE + ("shard",))
@pytest.mark.parametrize("name,k", RUNS)
def test_align_equals_reference(sas, cases, name, k, build):
    import torch
    c = cases(name, k)
    idx = make_index(sas, c.t, build)
    what = (name, k, build)
    got = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end)
    structure(c, got, what + ("device",))
    compare(c, got, what + ("device",))
    got32 = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end, u32=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, got32)), what + ("u32",)
    # the Python mirror: device tensors and host arrays
    mir = idx.align_edit(cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32), k,
                         cu(torch, c.off, np.int64), cu(torch, c.end, np.int64))
    torch.cuda.synchronize()
    assert mir[0].dtype == torch.int64 and mir[3].shape == (c.na, 2 * k + 1)
    assert all(np.array_equal(a, b.cpu().numpy().astype(np.int64)) for a, b in zip(got, mir)), what + ("mirror",)
    host = idx.align_edit(c.qb, c.qoff, c.qlen, k, c.off, c.end)
    assert host[0].dtype == np.uint64 and host[3].dtype == np.uint16 and host[1].dtype == np.uint8
    assert all(np.array_equal(a, b.astype(np.int64)) for a, b in zip(got, host)), what + ("host",)
    host = idx.align_edit(c.qb, c.qoff, c.qlen, k, c.off, c.end, u32=True)
    assert host[0].dtype == np.uint32
    assert all(np.array_equal(a, b.astype(np.int64)) for a, b in zip(got, host)), what + ("host u32",)


def test_fixed_length_agrees_with_ragged(sas, cases):
    import torch
    for name, k in (("random", 3), ("random", 15), ("period7", 1)):
        c = cases(name, k)
        idx = make_index(sas, c.t, "quad_p8")
        full = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end)
        for m in (33, 64, 65, 128, 129, 256):
            sel = [i for i, q in enumerate(c.qs) if len(q) == m]
            assert sel, (name, k, m)
            fb = np.concatenate([c.qs[i] for i in sel] + [np.zeros(64, np.uint8)])
            cnt = np.array([c.off[i + 1] - c.off[i] for i in sel], np.int64)
            assert cnt.sum() > 0, (name, k, m)
            foff = np.concatenate([[0], np.cumsum(cnt)])
            rows = np.concatenate([np.arange(c.off[i], c.off[i + 1]) for i in sel])
            for u32 in (False, True):
                got = dev_call(torch, idx, fb[:len(sel) * m], None, None, k, foff, c.end[rows], u32=u32, fixed_m=m)
                assert all(np.array_equal(g, f[rows]) for g, f in zip(got, full)), (name, k, m, u32)
            host = idx.align_edit_fixed(fb[:len(sel) * m], m, k, foff, c.end[rows])
            assert all(np.array_equal(h.astype(np.int64), f[rows]) for h, f in zip(host, full)), (name, k, m, "host")
            dev = idx.align_edit_fixed(cu(torch, fb, np.uint8)[:len(sel) * m], m, k, cu(torch, foff, np.int64),
                                       cu(torch, c.end[rows], np.int64))
            torch.cuda.synchronize()
            assert all(np.array_equal(d.cpu().numpy().astype(np.int64), f[rows]) for d, f in zip(dev, full))


def test_inputs_without_an_alignment(sas, cases):
    """Ends shifted off a true end, a fabricated end for the empty query and for m = 257, and
    e = n + 1: start = n, dist = 255, nruns = 0, every run slot 0."""
    import torch
    for name, k in (("random", 3), ("tiny", 2), ("zero_tail", 3)):
        c = cases(name, k)
        n = c.n
        lens = [len(q) for q in c.qs]
        pick = [i for i in range(len(c.qs)) if c.off[i + 1] > c.off[i]][::7][:40]
        pick += [lens.index(257), len(c.qs) - 1]  # too long; the empty query
        assert lens[-1] == 0
        qs = [c.qs[i] for i in pick]
        qb, qoff, qlen = pack(qs)
        ends, off, none = [], [0], []
        for x, i in enumerate(pick):
            mine = []
            if 0 < lens[i] <= 256:
                D = c.br.rows([c.qs[i]])[0]
                true = c.end[c.off[i]:c.off[i + 1]]
                shifted = np.unique(np.clip(np.concatenate([true + d for d in (-k - 1, -1, 1, k + 1)]), 0, n))
                shifted = shifted[D[shifted] > k][:6]  # the brute force: nothing within k ends there
                mine = [(int(e), True) for e in shifted] + [(int(true[0]), False), (n + 1, True)]
            else:
                mine = [(min(5, n), True), (n, True)]
            ends += [e for e, _ in mine]
            none += [v for _, v in mine]
            off.append(len(ends))
        ends, off, none = np.array(ends, np.int64), np.array(off, np.int64), np.array(none)
        assert none.sum() > 40 and (~none).sum() > 10
        idx = make_index(sas, c.t, "quad_p8")
        for u32 in (False, True):
            start, dist, nruns, runs = dev_call(torch, idx, qb, qoff, qlen, k, off, ends, u32=u32)
            assert (start[none] == n).all() and (dist[none] == NONE_DIST).all() and (nruns[none] == 0).all()
            assert not runs[none].any()
            assert (dist[~none] <= k).all() and (nruns[~none] >= 1).all()
            ref = align_ref_all(c.t, qs, off, ends, k)
            assert all(np.array_equal(g, r) for g, r in zip((start, dist, nruns, runs), ref)), (name, k, u32)
        host = idx.align_edit(qb, qoff, qlen, k, off, ends)
        assert all(np.array_equal(h.astype(np.int64), r) for h, r in zip(host, ref)), (name, k, "host")


def test_call_forms(sas, cases):
    import torch
    from sas_amd import _lib
    c = cases("random", 3)
    k = c.k
    idx = make_index(sas, c.t, "quad_p8")
    full = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end)
    # na below the total: nothing at or past it is written (dev_call checks the canaries from na on)
    for na in (0, 1, 2047, 2049, c.na - 1):
        got = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end, na=na)
        assert all(np.array_equal(g, f[:na]) for g, f in zip(got, full)), na
    # na above the total: off[nq] bounds what is written
    got = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, np.concatenate([c.end, c.end[:100]]), na=c.na + 100)
    assert all(np.array_equal(g, f) for g, f in zip(got, full))
    # each optional output NULL, on device and on host pointers
    for outs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end, outs=outs, u32=outs[0])
        assert all(g is None or np.array_equal(g, f) for g, f in zip(got, full)), outs
        assert [g is None for g in got[1:]] == [not o for o in outs]
    L = _lib.lib()
    start = np.zeros(c.na, np.uint64)
    nr = np.zeros(c.na, np.uint8)
    off = c.off.astype(np.uint64)
    end = c.end.astype(np.uint64)
    _lib.check(L.sas_align_edit(idx._h, c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data, len(c.qs), k,
                                off.ctypes.data, end.ctypes.data, c.na, start.ctypes.data, None, nr.ctypes.data,
                                None, None, 0))
    assert np.array_equal(start.astype(np.int64), full[0]) and np.array_equal(nr.astype(np.int64), full[2])
    # host pointers, na below the total: the rest is left alone
    start[:] = 7
    _lib.check(L.sas_align_edit(idx._h, c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data, len(c.qs), k,
                                off.ctypes.data, end.ctypes.data, 1000, start.ctypes.data, None, None, None, None, 0))
    assert np.array_equal(start[:1000].astype(np.int64), full[0][:1000]) and (start[1000:] == 7).all()
    # na = 0 and nq = 0: nothing is read or written
    assert L.sas_align_edit(idx._h, None, None, None, 5, k, None, None, 0, None, None, None, None, None, 0) == 0
    empty = idx.align_edit(c.qb, c.qoff, c.qlen, k, c.off, c.end[:0])
    assert [len(v) for v in empty] == [0, 0, 0, 0]
    # SAS_VALIDATE with a byte of 4; host pointers always validate
    badq = c.qb.copy()
    badq[int(c.qoff[-2])] = 4
    with pytest.raises(sas.SasError) as e:
        idx.align_edit(badq, c.qoff, c.qlen, k, c.off, c.end)
    assert e.value.code == errno.EINVAL
    dargs = (cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32), k, cu(torch, c.off, np.int64),
             cu(torch, c.end, np.int64))
    with pytest.raises(sas.SasError) as e:
        idx.align_edit(cu(torch, badq, np.uint8), *dargs, flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL
    ok = idx.align_edit(cu(torch, c.qb, np.uint8), *dargs, flags=_lib.SAS_VALIDATE)
    assert all(np.array_equal(o.cpu().numpy().astype(np.int64), f) for o, f in zip(ok, full))
    # errors
    p = (c.qb.ctypes.data, c.qoff.ctypes.data, c.qlen.ctypes.data)
    for args in ((off.ctypes.data, end.ctypes.data, c.na, None), (None, end.ctypes.data, c.na, start.ctypes.data),
                 (off.ctypes.data, None, c.na, start.ctypes.data)):
        assert L.sas_align_edit(idx._h, *p, len(c.qs), k, *args, None, None, None, None, 0) == errno.EINVAL
    assert L.sas_align_edit(idx._h, *p, len(c.qs), 16, off.ctypes.data, end.ctypes.data, c.na, start.ctypes.data,
                            None, None, None, None, 0) == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.align_edit_fixed(c.qb[:64], 32, 16, np.array([0, 1, 2]), np.array([40, 50]))
    assert e.value.code == errno.EINVAL
    # tagged and tag-line indexes keep the packed text: served
    h = int(np.flatnonzero(c.off > 500)[0])  # the first queries, with more than 500 alignments
    for kw in (dict(tagged=True), dict(tagged=True, tag_lines=True)):
        tag = sas.SaNaive.build(c.t, lcp=False, **kw)
        got = tag.align_edit(c.qb, c.qoff[:h], c.qlen[:h], k, c.off[:h + 1], c.end[:int(c.off[h])])
        assert all(np.array_equal(g.astype(np.int64), f[:int(c.off[h])]) for g, f in zip(got, full)), kw


def test_chained_behind_locate_edit(sas, cases):
    """sas_locate_edit's device outputs go straight into sas_align_edit on the same stream."""
    import torch
    from sas_amd import _lib
    c = cases("random", 3)
    k = c.k
    idx = make_index(sas, c.t, "quad_p8")
    fed = dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end)
    nq, stride = len(c.qs), 2 * k + 1
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dq, do, dl = cu(torch, c.qb, np.uint8), cu(torch, c.qoff, np.int64), cu(torch, c.qlen, np.int32)
        cap = c.na + 500
        off = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        end = torch.empty(cap, dtype=torch.int32, device="cuda")
        start = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
        dist = torch.full((cap,), 99, dtype=torch.uint8, device="cuda")
        nruns = torch.full((cap,), 99, dtype=torch.uint8, device="cuda")
        runs = torch.full((cap, stride), -7, dtype=torch.int16, device="cuda")
        fl = _lib.SAS_DEVICE_PTRS | _lib.SAS_LOCATE_U32
        L = _lib.lib()
        _lib.check(L.sas_locate_edit(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, k, 0, off.data_ptr(),
                                     end.data_ptr(), None, None, cap, None, stream.cuda_stream, fl))
        _lib.check(L.sas_align_edit(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, k, off.data_ptr(),
                                    end.data_ptr(), cap, start.data_ptr(), dist.data_ptr(), nruns.data_ptr(),
                                    runs.data_ptr(), stream.cuda_stream, fl))
    stream.synchronize()
    assert int(off[nq]) == c.na and (start[c.na:] == -7).all() and (runs[c.na:] == -7).all()
    got = (start[:c.na], dist[:c.na], nruns[:c.na], runs[:c.na])
    assert all(np.array_equal(g.cpu().numpy().astype(np.int64), f) for g, f in zip(got, fed))
    assert sas.cigar(runs[0], nruns[0]) == sas.cigar(fed[3][0], fed[2][0]) != ""
