"""k-mismatch locate (sas_locate_mismatch / sas_locate_mismatch_fixed and SaNaive.locate_mismatch*)
against a brute force that knows none of the new code: the Hamming distance of every alignment
with numpy, the occurrences of each piece with bytes.find, the skipped-seed, first-piece and
order rules from sas.h's text, and the SA ranks from the CPU oracle's suffix array."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_match import pack

pytestmark = pytest.mark.gpu

TRUNCATED, SHORT = 1, 2
MS = (1, 2, 5, 8, 31, 32, 33, 63, 64, 65, 129, 200)
EDGES = (31, 32, 33, 63, 64, 65, 127, 128)  # the 32-char compare steps' boundaries
QUAD = dict(lcp=False, stree=False, sector=False, quad=True, llcp=False)
BARE = dict(lcp=False, stree=False, sector=False, quad=False, llcp=False)
BUILDS = {
    "quad_p2": dict(QUAD, prefix=2),
    "quad_p8": dict(QUAD, prefix=8),
    "inline2": dict(QUAD, prefix=4, prefix_inline=2),
    "sa40": dict(QUAD, sa40=True),
    "quad_notable": dict(QUAD, prefix=False),
}
TEXTS = ("random", "zeros", "period7", "zero_tail")
# (k, max_seed_hits) runs per text; the capped ones skip seeds
RUNS = {
    "random": [(0, 0), (1, 0), (2, 0), (3, 0), (15, 0), (2, 20)],
    "zeros": [(0, 0), (1, 0), (2, 0), (3, 0)],
    "period7": [(0, 0), (1, 0), (2, 0), (3, 0), (1, 64), (2, 64)],
    "zero_tail": [(0, 0), (1, 0), (2, 0), (3, 0), (1, 64)],
}


def make_text(name):
    if name == "random":
        return O.random_string(4099, seed=11)
    if name == "zeros":
        return np.zeros(300, np.uint8)
    if name == "period7":
        return np.tile(np.array([0, 1, 3, 2, 2, 0, 3], np.uint8), 286)[:2000]
    assert name == "zero_tail"
    return np.concatenate([O.random_string(1500, seed=12), np.zeros(20, np.uint8)])


class MBrute:
    """The definition of sas.h, on bytes and numpy."""

    def __init__(self, t: np.ndarray):
        self.t = t
        self.tb = t.tobytes()
        self.n = len(t)
        sa = O.build_sa(t).astype(np.int64)
        self.rank = np.empty(self.n, np.int64)
        self.rank[sa] = np.arange(self.n)
        self._count = {}

    def count(self, p: bytes) -> int:
        c = self._count.get(p)
        if c is None:
            c, i = 0, self.tb.find(p)
            while i >= 0:
                c += 1
                i = self.tb.find(p, i + 1)
            self._count[p] = c
        return c

    def answer(self, q: np.ndarray, k: int, max_hits: int):
        """(positions, distances, flags, candidates) of one query."""
        t, n, m = self.t, self.n, len(q)
        if m <= k:
            return [], [], SHORT, 0
        b = [j * m // (k + 1) for j in range(k + 2)]
        skipped, cand = [], 0
        for j in range(k + 1):
            c = self.count(q[b[j]:b[j + 1]].tobytes())
            skipped.append(bool(max_hits) and c > max_hits)
            if not skipped[-1]:
                cand += c
        flags = TRUNCATED if any(skipped) else 0
        A = n - m + 1  # alignments: the padding behind the text matches nothing
        if A <= 0:
            return [], [], flags, cand
        per = np.zeros((k + 1, A), np.int64)
        for j in range(k + 1):
            for c in range(b[j], b[j + 1]):
                per[j] += t[c:c + A] != q[c]
        d = per.sum(0)
        res = []
        for s in np.flatnonzero(d <= k):
            for j in range(k + 1):  # reported by the first non-skipped piece that matches exactly
                if not skipped[j] and per[j, s] == 0:
                    res.append((j, int(self.rank[s + b[j]]), int(s), int(d[s])))
                    break
        res.sort()
        return [r[2] for r in res], [r[3] for r in res], flags, cand


def make_queries(t: np.ndarray, k: int, seed: int):
    rng = np.random.default_rng(seed)
    n, qs = len(t), []

    def cut(s, m):
        return t[s:s + m].copy()

    def subst(q, places):
        for j in places:
            q[j] = (q[j] + rng.integers(1, 4)) & 3
        return q

    for m in MS:
        if m > n:
            continue
        for nsub in range(0, k + 2):  # 0 .. k + 1 substitutions at random places
            for _ in range(2):
                q = cut(int(rng.integers(0, n - m + 1)), m)
                qs.append(subst(q, rng.choice(m, min(nsub, m), replace=False)))
        edges = [e for e in EDGES if e < m]
        for e in edges:  # at the word edges, alone and with company
            qs.append(subst(cut(int(rng.integers(0, n - m + 1)), m), [e]))
        for c in range(2, min(k + 1, len(edges)) + 1):
            qs.append(subst(cut(int(rng.integers(0, n - m + 1)), m), edges[:c]))
        for s in (0, n - m):  # the first and the last alignment
            q = cut(s, m)
            qs.append(subst(q, rng.choice(m, min(int(rng.integers(0, k + 1)), m), replace=False)))
        for r in (1, m // 2, m - 1):  # run past the text end: candidates fall off the right end
            if 0 < r < m:
                qs.append(np.concatenate([t[n - r:], rng.integers(0, 4, m - r).astype(np.uint8)]))
        for x in (1, m // 2, m - 1):  # later pieces occur at the text start: candidates fall off the left end
            if 0 < x < m:
                qs.append(np.concatenate([rng.integers(0, 4, x).astype(np.uint8), t[:m - x]]))
    for m in (1, 3, 8, 19, 20, 21, 33, 64, 65, 200):  # zeros: the padding behind the text must not match
        qs.append(np.zeros(m, np.uint8))
    for m in (5, 8, 33):
        qs.append(rng.integers(0, 4, m).astype(np.uint8))
    qs.append(np.zeros(0, np.uint8))  # the empty query
    return qs


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def cases():
    """Per text: the text and per (k, max_seed_hits) run the queries, their ragged batch and the
    brute-force answer (computed once, read-only, shared by every build)."""
    out = {}
    for ti, name in enumerate(TEXTS):
        t = make_text(name)
        br = MBrute(t)
        runs = {}
        for k, mh in RUNS[name]:
            qs = make_queries(t, k, 1000 + 10 * ti + k)
            ans = [br.answer(q, k, mh) for q in qs]
            off = np.zeros(len(qs) + 1, np.int64)
            off[1:] = np.cumsum([len(a[0]) for a in ans])
            exp = dict(off=off, pos=np.array([p for a in ans for p in a[0]], np.int64),
                       dist=np.array([d for a in ans for d in a[1]], np.int64),
                       qflags=np.array([a[2] for a in ans], np.int64), cand=int(sum(a[3] for a in ans)))
            for v in exp.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            runs[(k, mh)] = (qs, pack(qs), exp)
        out[name] = (t, runs)
    return out


def same(got, exp, what):
    off, pos, dist, qfl = (np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64) for g in got)
    assert np.array_equal(qfl, exp["qflags"]), (what, "qflags", np.flatnonzero(qfl != exp["qflags"])[:5])
    bad = np.flatnonzero(off != exp["off"])
    assert len(bad) == 0, (what, "off", bad[:5], off[bad[:5]], exp["off"][bad[:5]])
    assert np.array_equal(pos, exp["pos"]), (what, "pos")
    assert np.array_equal(dist, exp["dist"]), (what, "dist")


def dev_call(torch, idx, qb, qoff, qlen, k, mh, capacity, u32=False, flags=0):
    """sas_locate_mismatch on device pointers into buffers with 64 sentinel elements behind
    `capacity`; returns (off, pos, dist, qflags, total) and checks the sentinels."""
    from sas_amd import _lib
    nq = len(qoff)
    dq = torch.from_numpy(qb).cuda()
    do = torch.from_numpy(qoff.astype(np.int64)).cuda()
    dl = torch.from_numpy(qlen.astype(np.int32)).cuda()
    off = torch.full((nq + 1 + 64,), -7, dtype=torch.int64, device="cuda")
    pos = torch.full((capacity + 64,), -7, dtype=torch.int32 if u32 else torch.int64, device="cuda")
    dist = torch.full((capacity + 64,), 99, dtype=torch.uint8, device="cuda")
    qfl = torch.full((nq + 64,), 99, dtype=torch.uint8, device="cuda")
    total = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    _lib.check(_lib.lib().sas_locate_mismatch(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, k, mh,
                                              off.data_ptr(), pos.data_ptr(), dist.data_ptr(), qfl.data_ptr(),
                                              capacity, total.data_ptr(), st, fl))
    torch.cuda.synchronize()
    assert (off[nq + 1:] == -7).all() and (pos[capacity:] == -7).all() and (dist[capacity:] == 99).all()
    assert (qfl[nq:] == 99).all() and int(total[1]) == -7
    return (off[:nq + 1].cpu().numpy(), pos[:capacity].cpu().numpy(), dist[:capacity].cpu().numpy(),
            qfl[:nq].cpu().numpy(), int(total[0]))


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("text", TEXTS)
def test_mismatch_equals_brute_force(sas, cases, text, build, monkeypatch):
    import torch
    from sas_amd import _lib
    t, runs = cases[text]
    idx = sas.SaNaive.build(t, **BUILDS[build])
    for (k, mh), (qs, (qb, qoff, qlen), exp) in runs.items():
        what = (text, build, k, mh)
        total = int(exp["off"][-1])
        # device pointers, u64 positions, exact capacity
        off, pos, dist, qfl, tot = dev_call(torch, idx, qb, qoff, qlen, k, mh, total)
        assert tot == total, what
        same((off, pos, dist, qfl), exp, what + ("device",))
        # u32 positions through the Python mirror (a sizing call, then the real one)
        dq = torch.from_numpy(qb).cuda()
        do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
        got = idx.locate_mismatch(dq, do, dl, k, max_seed_hits=mh, u32=True)
        torch.cuda.synchronize()
        assert got[1].dtype == torch.int32 and got[2].dtype == torch.uint8
        same(got, exp, what + ("device u32",))
        # host pointers
        host = idx.locate_mismatch(qb, qoff, qlen, k, max_seed_hits=mh)
        assert host[0].dtype == np.uint64 and host[1].dtype == np.uint64 and host[2].dtype == np.uint8
        same(host, exp, what + ("host",))
        if k == 1:  # per text and build: u32 on host pointers, the search without the table, the A/B knob
            same(idx.locate_mismatch(qb, qoff, qlen, k, max_seed_hits=mh, u32=True), exp, what + ("host u32",))
            same(idx.locate_mismatch(dq, do, dl, k, max_seed_hits=mh, flags=_lib.SAS_NO_PREFIX_TABLE), exp,
                 what + ("no table",))
            monkeypatch.setenv("SAS_MM_QWORDS", "packed")  # the other way to the query words
            same(idx.locate_mismatch(dq, do, dl, k, max_seed_hits=mh), exp, what + ("query words prepacked",))
            monkeypatch.delenv("SAS_MM_QWORDS")
        # the fixed-length entry points agree with the ragged answer of the same queries
        for m in (2, 33, 64, 200):
            sel = [i for i, q in enumerate(qs) if len(q) == m]
            if not sel:
                continue
            fb = np.concatenate([qs[i] for i in sel] + [np.zeros(64, np.uint8)])
            cnt = np.array([exp["off"][i + 1] - exp["off"][i] for i in sel], np.int64)
            fexp = dict(off=np.concatenate([[0], np.cumsum(cnt)]),
                        pos=np.concatenate([exp["pos"][exp["off"][i]:exp["off"][i + 1]] for i in sel]),
                        dist=np.concatenate([exp["dist"][exp["off"][i]:exp["off"][i + 1]] for i in sel]),
                        qflags=exp["qflags"][sel])
            same(idx.locate_mismatch_fixed(fb[:len(sel) * m], m, k, max_seed_hits=mh), fexp, what + ("fixed host", m))
            got = idx.locate_mismatch_fixed(torch.from_numpy(fb).cuda()[:len(sel) * m], m, k, max_seed_hits=mh)
            torch.cuda.synchronize()
            same(got, fexp, what + ("fixed device", m))


def test_brute_force_shapes(cases):
    """What the cases must contain, asserted from the brute force alone."""
    _, runs = cases["period7"]
    assert runs[(1, 0)][2]["cand"] > 3 * 2048  # tiles cross piece and query boundaries
    for key in ((1, 64), (2, 64)):
        fl = runs[key][2]["qflags"]
        assert (fl & TRUNCATED).any() and (fl == 0).any(), key
    # truncated queries with a non-empty, exactly defined answer
    qs, _, exp = cases["zero_tail"][1][(1, 64)]
    cnt = np.diff(exp["off"])
    assert ((exp["qflags"] & TRUNCATED) != 0)[cnt > 0].any()
    for name in TEXTS:
        for (k, mh), (qs, _, exp) in cases[name][1].items():
            fl = exp["qflags"]
            assert all(bool(f & SHORT) == (len(q) <= k) for f, q in zip(fl, qs))
            assert fl[-1] == SHORT and len(qs[-1]) == 0  # the empty query
            if name == "random" and mh == 0:
                assert (exp["dist"] == k).any() and (exp["dist"] == 0).any()


@pytest.mark.parametrize("build", list(BUILDS))
def test_k0_equals_locate(sas, cases, build):
    import torch
    for text in TEXTS:
        t, runs = cases[text]
        qs = [q for q in runs[(0, 0)][0] if len(q)]  # the empty query is SAS_MM_SHORT at every k
        qb, qoff, qlen = pack(qs)
        idx = sas.SaNaive.build(t, **BUILDS[build])
        loff, lpos = idx.locate(qb, qoff, qlen)
        off, pos, dist, qfl = idx.locate_mismatch(qb, qoff, qlen, 0)
        assert np.array_equal(off, loff) and np.array_equal(pos, lpos) and not dist.any() and not qfl.any()
        dq = torch.from_numpy(qb).cuda()
        do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
        dloff, dlpos = idx.locate(dq, do, dl)
        doff, dpos, _, _ = idx.locate_mismatch(dq, do, dl, 0)
        assert torch.equal(doff, dloff) and torch.equal(dpos, dlpos)


def test_capacity(sas, cases):
    import torch
    t, runs = cases["period7"]
    qs, (qb, qoff, qlen), exp = runs[(1, 0)]
    total = int(exp["off"][-1])
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    for cap in (0, 1, total // 2, total - 1):
        off, pos, dist, qfl, tot = dev_call(torch, idx, qb, qoff, qlen, 1, 0, cap)  # sentinels past cap checked
        assert tot == total and np.array_equal(off, exp["off"]) and np.array_equal(qfl, exp["qflags"])
        assert np.array_equal(pos, exp["pos"][:cap]) and np.array_equal(dist, exp["dist"][:cap])
    # out_total and out_dist / out_qflags may be NULL on device pointers
    from sas_amd import _lib
    got = idx.locate_mismatch(torch.from_numpy(qb).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda(),
                              torch.from_numpy(qlen.astype(np.int32)).cuda(), 1, dist=False, capacity=total)
    torch.cuda.synchronize()
    assert got[2] is None and np.array_equal(got[1].cpu().numpy(), exp["pos"])
    # host pointers: ENOSPC, nothing copied, the total and the offsets still reported
    L = _lib.lib()
    nq = len(qoff)
    off = np.zeros(nq + 1, np.uint64)
    pos = np.full(total, 7, np.uint64)
    dist = np.full(total, 7, np.uint8)
    qfl = np.full(nq, 7, np.uint8)
    tot = C.c_uint64(0)
    rc = L.sas_locate_mismatch(idx._h, qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, nq, 1, 0, off.ctypes.data,
                               pos.ctypes.data, dist.ctypes.data, qfl.ctypes.data, total - 1, C.byref(tot), None, 0)
    assert rc == errno.ENOSPC and tot.value == total and (pos == 7).all() and (dist == 7).all()
    assert np.array_equal(off.astype(np.int64), exp["off"]) and np.array_equal(qfl.astype(np.int64), exp["qflags"])


def test_errors(sas, cases):
    import torch
    from sas_amd import _lib
    t, runs = cases["random"]
    qs, (qb, qoff, qlen), exp = runs[(1, 0)]
    n = len(t)
    L = _lib.lib()
    for idx in (sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100, n - 5), **BARE),
                sas.SaNaive.build_part(t, 1, 3, lcp=False, stree=False, sector=False, quad=True, llcp=False),
                sas.SaNaive.build(t, lcp=False, tagged=True),
                sas.SaNaive.build(t, lcp=False, tagged=True, tag_lines=True)):
        with pytest.raises(sas.SasError) as e:
            idx.locate_mismatch(qb, qoff, qlen, 1)
        assert e.value.code == errno.ENOTSUP
    bare = sas.SaNaive.build(t, **BARE)
    with pytest.raises(sas.SasError) as e:  # the range search's own refusal
        bare.locate_mismatch(qb, qoff, qlen, 1)
    assert e.value.code == errno.EINVAL and "sas_search_range" in str(e.value)
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    with pytest.raises(sas.SasError) as e:
        idx.locate_mismatch(qb, qoff, qlen, 16)
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.locate_mismatch_fixed(qb[:64], 32, 16)
    assert e.value.code == errno.EINVAL
    # null arguments
    off = np.zeros(len(qoff) + 1, np.uint64)
    tot = C.c_uint64(0)
    p = (qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data)
    assert L.sas_locate_mismatch(idx._h, None, p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0,
                                 C.byref(tot), None, 0) == errno.EINVAL
    assert L.sas_locate_mismatch(idx._h, p[0], None, p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0,
                                 C.byref(tot), None, 0) == errno.EINVAL
    assert L.sas_locate_mismatch(idx._h, p[0], p[1], p[2], 2, 1, 0, None, None, None, None, 0, C.byref(tot), None,
                                 0) == errno.EINVAL
    assert L.sas_locate_mismatch(idx._h, p[0], p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 5,
                                 C.byref(tot), None, 0) == errno.EINVAL  # a capacity without out_pos
    assert L.sas_locate_mismatch(idx._h, p[0], p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0, None, None,
                                 0) == errno.EINVAL  # host pointers need out_total
    # bytes > 3: host pointers always validate, device pointers with SAS_VALIDATE
    badq = qb.copy()
    badq[int(qoff[-2])] = 4
    with pytest.raises(sas.SasError) as e:
        idx.locate_mismatch(badq, qoff, qlen, 1)
    assert e.value.code == errno.EINVAL
    do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
    with pytest.raises(sas.SasError) as e:
        idx.locate_mismatch(torch.from_numpy(badq).cuda(), do, dl, 1, flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL
    same(idx.locate_mismatch(torch.from_numpy(qb).cuda(), do, dl, 1, flags=_lib.SAS_VALIDATE), exp, "validated")
    # nq = 0
    off, pos, dist, qfl = idx.locate_mismatch(qb, qoff[:0], qlen[:0], 1)
    assert off.tolist() == [0] and len(pos) == 0 and len(dist) == 0 and len(qfl) == 0
