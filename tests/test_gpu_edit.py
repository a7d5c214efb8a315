"""k-difference locate (sas_locate_edit / sas_locate_edit_fixed and SaNaive.locate_edit*) against a
brute force written from sas.h's text alone: Sellers' rows with numpy over all n + 1 columns,
the occurrences of each piece with bytes.find, the skipped-seed formula, the flags and the
ascending order."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_match import pack

pytestmark = pytest.mark.gpu

TRUNCATED, SHORT, LONG = 1, 2, 4
MAX_M = 256
MS = (1, 2, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257)
EDGES = (63, 64, 65, 127, 128)  # the bit-vector words' edges
ZEROS = (1, 3, 19, 20, 21, 33, 64, 65, 200)
QUAD = dict(lcp=False, stree=False, sector=False, quad=True, llcp=False)
BARE = dict(lcp=False, stree=False, sector=False, quad=False, llcp=False)
BUILDS = {
    "quad_p2": dict(QUAD, prefix=2),
    "quad_p8": dict(QUAD, prefix=8),
    "inline2": dict(QUAD, prefix=4, prefix_inline=2),
    "sa40": dict(QUAD, sa40=True),
    "quad_notable": dict(QUAD, prefix=False),
}
TEXTS = ("random", "zeros", "period7", "zero_tail", "tiny")
# (k, max_seed_hits) runs per text; the capped ones skip seeds
RUNS = {
    "random": [(0, 0), (1, 0), (2, 0), (3, 0), (15, 0), (2, 20)],
    "zeros": [(0, 0), (1, 0), (2, 0), (3, 0)],
    "period7": [(0, 0), (1, 0), (2, 0), (3, 0), (1, 64), (2, 64)],
    "zero_tail": [(0, 0), (1, 0), (2, 0), (3, 0), (1, 64)],
    "tiny": [(0, 0), (1, 0), (2, 0), (3, 0)],
}


def make_text(name):
    if name == "random":
        return O.random_string(4099, seed=11)
    if name == "zeros":
        return np.zeros(300, np.uint8)
    if name == "period7":
        return np.tile(np.array([0, 1, 3, 2, 2, 0, 3], np.uint8), 286)[:2000]
    if name == "zero_tail":
        return np.concatenate([O.random_string(1500, seed=12), np.zeros(20, np.uint8)])
    assert name == "tiny"
    return O.random_string(40, seed=13)


class EBrute:
    """The definition of sas.h, on bytes and numpy."""

    def __init__(self, t: np.ndarray):
        self.t = t
        self.tb = t.tobytes()
        self.n = len(t)
        self._occ = {}

    def occurrences(self, p: bytes) -> list:
        o = self._occ.get(p)
        if o is None:
            o, i = [], self.tb.find(p)
            while i >= 0:
                o.append(i)
                i = self.tb.find(p, i + 1)
            self._occ[p] = o
        return o

    def rows(self, qs) -> np.ndarray:
        """D(e) for e in [0, n] of each of the equally long queries qs: Sellers' rows, one per
        query char.  Row 0 is 0 (an alignment starts anywhere); row i, column e is the least of
        the cell above + 1, the diagonal cell + (q[i-1] != t[e-1]) and the cell to the left + 1;
        the last goes through a running minimum of row - arange."""
        n, B = self.n, len(qs)
        Q = np.array(qs, np.uint8).reshape(B, -1)
        ar = np.arange(n + 1, dtype=np.int16)
        eq = np.stack([self.t == c for c in range(4)]).astype(np.int16)  # eq[c, e - 1] = (t[e - 1] == c)
        P = np.zeros((B, n + 1), np.int16) - ar  # row - arange
        S = np.empty_like(P)
        for i in range(Q.shape[1]):
            # row - arange before the horizontal term: above + 1, diagonal + (chars differ);
            # the diagonal cell of column e is P[e - 1] + (e - 1): minus e that is P[e - 1] - 1 + (differ)
            np.minimum(P[:, 1:] + 1, P[:, :-1] - eq[Q[:, i]], out=S[:, 1:])
            S[:, 0] = i + 1
            np.minimum.accumulate(S, axis=1, out=P)
        return P + ar

    def full(self, q, k, D=None):
        """The k-difference answer: {e: D(e)} for every e with D(e) <= k."""
        D = self.rows([q])[0] if D is None else D
        return {int(e): int(D[e]) for e in np.flatnonzero(D <= k)}

    def answer(self, q: np.ndarray, k: int, max_hits: int, D=None):
        """(ends, distances, flags, info) of one query; info counts the candidates and the
        candidates with a negative s0."""
        n, m = self.n, len(q)
        info = dict(cand=0, neg=0, prop=0)
        if m <= k:
            return [], [], SHORT, info
        if m > MAX_M:
            return [], [], LONG, info
        b = [j * m // (k + 1) for j in range(k + 2)]
        near = np.zeros(n + 2, np.int64)  # per end: the candidates whose pv - b_j + m is within k of it
        flags = 0
        for j in range(k + 1):
            occ = self.occurrences(q[b[j]:b[j + 1]].tobytes())
            if max_hits and len(occ) > max_hits:
                flags |= TRUNCATED
                continue
            info["cand"] += len(occ)
            c = np.array(occ, np.int64) - b[j] + m
            info["neg"] += int((c < m).sum())
            lo, hi = np.maximum(c - k, 0), np.minimum(c + k, n) + 1
            ok = lo < hi
            np.add.at(near, lo[ok], 1)
            np.add.at(near, hi[ok], -1)
        near = np.cumsum(near)[:n + 1]
        D = self.rows([q])[0] if D is None else D
        ends = np.flatnonzero((D <= k) & (near > 0))
        info["prop"] = int(near[ends].sum())  # ends proposed, duplicates counted
        return ends.tolist(), D[ends].tolist(), flags, info

    def answers(self, qs, k, max_hits):
        """answer() of every query, the rows computed per group of equally long queries."""
        out = [None] * len(qs)
        by_len = {}
        for i, q in enumerate(qs):
            by_len.setdefault(len(q), []).append(i)
        for m, sel in by_len.items():
            if m <= k or m > MAX_M:
                for i in sel:
                    out[i] = self.answer(qs[i], k, max_hits)
                continue
            for g in range(0, len(sel), 64):
                grp = sel[g:g + 64]
                D = self.rows([qs[i] for i in grp])
                for r, i in enumerate(grp):
                    out[i] = self.answer(qs[i], k, max_hits, D[r])
        return out


def edited(rng, src, ops):
    """src after the edits ops = [(kind, place)], applied in turn ("sub", "ins", "del"; the place is
    taken modulo the current length)."""
    q = list(src)
    for kind, at in ops:
        if kind == "ins":
            q.insert(at % (len(q) + 1), int(rng.integers(0, 4)))
        elif q:
            at %= len(q)
            if kind == "sub":
                q[at] = (q[at] + int(rng.integers(1, 4))) & 3
            else:
                del q[at]
    return np.array(q, np.uint8)


def make_queries(t: np.ndarray, k: int, seed: int):
    """(queries, planted): planted[i] = query i is a slice of the text with at most k edits."""
    rng = np.random.default_rng(seed)
    n, qs, planted = len(t), [], []
    kinds = ("sub", "ins", "del")

    def plant(m, ops, s=None):
        """a query of m chars: a text slice of the length that the edits turn into m"""
        ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
        if ln < 1 or ln > n:
            return
        s = int(rng.integers(0, n - ln + 1)) if s is None else (s if s >= 0 else n - ln)
        q = edited(rng, t[s:s + ln], ops)
        if len(q) == m:
            qs.append(q)
            planted.append(len(ops) <= k)

    def free(q):
        qs.append(np.asarray(q, np.uint8))
        planted.append(False)

    turn = 0
    for m in MS:
        if m > MAX_M:  # SAS_ED_LONG
            if m <= n:
                plant(m, [])
            free(rng.integers(0, 4, m))
            continue
        for c in range(0, k + 2):  # 0 .. k + 1 edits of each kind and mixed, at random places
            for kind in kinds + ("mixed",):
                if c == 0 and kind != "sub":
                    continue
                plant(m, [(kind if kind != "mixed" else kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20)))
                          for _ in range(c)])
        rows = [e for e in EDGES if e < m]
        for j in range(1, k + 1):  # the piece boundaries
            rows += [j * m // (k + 1) - 1, j * m // (k + 1)]
        for r in rows:  # one edit exactly there, the kinds in turn
            if 0 <= r < m and k >= 1:
                plant(m, [(kinds[turn % 3], r)])
                turn += 1
        for kind in ("ins", "del"):  # as the query's first and as its last char
            if k >= 1:
                plant(m, [(kind, 0)])
                # the slice has m - 1 chars before an insertion (at its end: m - 1), m + 1 before a deletion
                plant(m, [(kind, m - 1 if kind == "ins" else m)])
        for s in (0, -1):  # the text's start and end: the window is cut at 0 and at n
            plant(m, [], s)
            plant(m, [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20)))
                      for _ in range(int(rng.integers(0, k + 1)))], s)
        for r in (1, m // 2, m - 1):  # run past the text end: a text tail, then random chars
            if 0 < r < m and r <= n:
                free(np.concatenate([t[n - r:], rng.integers(0, 4, m - r).astype(np.uint8)]))
        for x in (1, m // 2, m - 1):  # later pieces occur at the text start: s0 < 0
            if 0 < x < m and m - x <= n:
                free(np.concatenate([rng.integers(0, 4, x).astype(np.uint8), t[:m - x]]))
    for m in ZEROS:  # zeros: the padding behind the text must not match
        free(np.zeros(m, np.uint8))
    for m in (5, 8, 33):
        free(rng.integers(0, 4, m))
    if n < 64:  # the tiny text: longer queries than the text
        free(rng.integers(0, 4, 64))                         # n < m - k: no answer
        for extra in range(1, k + 1):                        # m - k <= n < m: only through deletions
            free(np.concatenate([t, rng.integers(0, 4, extra).astype(np.uint8)]))
            free(edited(rng, t, [("ins", n // 2 + i) for i in range(extra)]))
    for m in sorted({1, k} - {0}):  # m <= k: SAS_ED_SHORT
        if m <= k:
            free(rng.integers(0, 4, m))
    free(np.zeros(0, np.uint8))  # the empty query
    return qs, np.array(planted, bool)


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


def expected(br, qs, k, mh):
    ans = br.answers(qs, k, mh)
    off = np.zeros(len(qs) + 1, np.int64)
    off[1:] = np.cumsum([len(a[0]) for a in ans])
    exp = dict(off=off, end=np.array([e for a in ans for e in a[0]], np.int64),
               dist=np.array([d for a in ans for d in a[1]], np.int64),
               qflags=np.array([a[2] for a in ans], np.int64), cand=int(sum(a[3]["cand"] for a in ans)),
               neg=int(sum(a[3]["neg"] for a in ans)), prop=int(sum(a[3]["prop"] for a in ans)))
    for v in exp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return exp


@pytest.fixture(scope="module")
def cases():
    """Per text: the text and per (k, max_seed_hits) run the queries, their ragged batch, which
    of them are planted and the brute-force answer (computed once, read-only, shared by every
    build)."""
    out = {}
    for ti, name in enumerate(TEXTS):
        t = make_text(name)
        br = EBrute(t)
        runs = {}
        for k, mh in RUNS[name]:
            qs, planted = make_queries(t, k, 2000 + 10 * ti + k)
            runs[(k, mh)] = (qs, pack(qs), expected(br, qs, k, mh), planted)
        out[name] = (t, runs)
    return out


def same(got, exp, what):
    off, end, dist, qfl = (None if g is None else np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64)
                           for g in got)
    assert np.array_equal(qfl, exp["qflags"]), (what, "qflags", np.flatnonzero(qfl != exp["qflags"])[:5])
    bad = np.flatnonzero(off != exp["off"])
    assert len(bad) == 0, (what, "off", bad[:5], off[bad[:5]], exp["off"][bad[:5]])
    assert np.array_equal(end, exp["end"]), (what, "end")
    if dist is not None:
        assert np.array_equal(dist, exp["dist"]), (what, "dist")


def dev_call(torch, idx, qb, qoff, qlen, k, mh, capacity, u32=False, flags=0):
    """sas_locate_edit on device pointers into buffers with 64 canary elements behind `capacity`;
    returns (off, end, dist, qflags, total) and checks the canaries."""
    from sas_amd import _lib
    nq = len(qoff)
    dq = torch.from_numpy(qb).cuda()
    do = torch.from_numpy(qoff.astype(np.int64)).cuda()
    dl = torch.from_numpy(qlen.astype(np.int32)).cuda()
    off = torch.full((nq + 1 + 64,), -7, dtype=torch.int64, device="cuda")
    end = torch.full((capacity + 64,), -7, dtype=torch.int32 if u32 else torch.int64, device="cuda")
    dist = torch.full((capacity + 64,), 99, dtype=torch.uint8, device="cuda")
    qfl = torch.full((nq + 64,), 99, dtype=torch.uint8, device="cuda")
    total = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    _lib.check(_lib.lib().sas_locate_edit(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, k, mh,
                                          off.data_ptr(), end.data_ptr(), dist.data_ptr(), qfl.data_ptr(), capacity,
                                          total.data_ptr(), st, fl))
    torch.cuda.synchronize()
    assert (off[nq + 1:] == -7).all() and (end[capacity:] == -7).all() and (dist[capacity:] == 99).all()
    assert (qfl[nq:] == 99).all() and int(total[1]) == -7
    return (off[:nq + 1].cpu().numpy(), end[:capacity].cpu().numpy(), dist[:capacity].cpu().numpy(),
            qfl[:nq].cpu().numpy(), int(total[0]))


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("text", TEXTS)
def test_edit_equals_brute_force(sas, cases, text, build):
    import torch
    from sas_amd import _lib
    t, runs = cases[text]
    idx = sas.SaNaive.build(t, **BUILDS[build])
    for (k, mh), (qs, (qb, qoff, qlen), exp, _) in runs.items():
        what = (text, build, k, mh)
        total = int(exp["off"][-1])
        # device pointers, u64 ends, exact capacity
        off, end, dist, qfl, tot = dev_call(torch, idx, qb, qoff, qlen, k, mh, total)
        assert tot == total, what
        same((off, end, dist, qfl), exp, what + ("device",))
        # u32 ends through the Python mirror (a sizing call, then the real one)
        dq = torch.from_numpy(qb).cuda()
        do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
        got = idx.locate_edit(dq, do, dl, k, max_seed_hits=mh, u32=True)
        torch.cuda.synchronize()
        assert got[1].dtype == torch.int32 and got[2].dtype == torch.uint8
        same(got, exp, what + ("device u32",))
        # host pointers, u64 and u32
        host = idx.locate_edit(qb, qoff, qlen, k, max_seed_hits=mh)
        assert host[0].dtype == np.uint64 and host[1].dtype == np.uint64 and host[2].dtype == np.uint8
        same(host, exp, what + ("host",))
        host = idx.locate_edit(qb, qoff, qlen, k, max_seed_hits=mh, u32=True)
        assert host[1].dtype == np.uint32
        same(host, exp, what + ("host u32",))
        # without distances; the search without the prefix table
        got = idx.locate_edit(dq, do, dl, k, max_seed_hits=mh, dist=False)
        assert got[2] is None
        same(got, exp, what + ("device, no dist",))
        host = idx.locate_edit(qb, qoff, qlen, k, max_seed_hits=mh, dist=False)
        assert host[2] is None
        same(host, exp, what + ("host, no dist",))
        same(idx.locate_edit(dq, do, dl, k, max_seed_hits=mh, flags=_lib.SAS_NO_PREFIX_TABLE), exp,
             what + ("no table",))
        # the fixed-length entry points (1, 2 and 4 words of rows; too long) agree with the ragged answer
        for m in (2, 33, 64, 65, 128, 129, 256, 257):
            sel = [i for i, q in enumerate(qs) if len(q) == m]
            if not sel:
                continue
            fb = np.concatenate([qs[i] for i in sel] + [np.zeros(64, np.uint8)])
            cnt = np.array([exp["off"][i + 1] - exp["off"][i] for i in sel], np.int64)
            fexp = dict(off=np.concatenate([[0], np.cumsum(cnt)]),
                        end=np.concatenate([exp["end"][exp["off"][i]:exp["off"][i + 1]] for i in sel]),
                        dist=np.concatenate([exp["dist"][exp["off"][i]:exp["off"][i + 1]] for i in sel]),
                        qflags=exp["qflags"][sel])
            same(idx.locate_edit_fixed(fb[:len(sel) * m], m, k, max_seed_hits=mh), fexp, what + ("fixed host", m))
            same(idx.locate_edit_fixed(fb[:len(sel) * m], m, k, max_seed_hits=mh, u32=True), fexp,
                 what + ("fixed host u32", m))
            dfb = torch.from_numpy(fb).cuda()[:len(sel) * m]
            got = idx.locate_edit_fixed(dfb, m, k, max_seed_hits=mh)
            torch.cuda.synchronize()
            same(got, fexp, what + ("fixed device", m))
            got = idx.locate_edit_fixed(dfb, m, k, max_seed_hits=mh, u32=True)
            torch.cuda.synchronize()
            same(got, fexp, what + ("fixed device u32", m))


def test_brute_force_shapes(cases):
    """What the cases must contain, asserted from the brute force alone."""
    for name in ("period7", "zeros"):  # a query's candidates span tiles, most proposals are duplicates
        exps = [cases[name][1][(k, 0)][2] for k in (1, 2, 3)]
        assert all(e["cand"] > 2048 for e in exps), name
        assert any(e["prop"] > 2 * len(e["end"]) for e in exps), (name, [(e["prop"], len(e["end"])) for e in exps])
    for key in ((1, 64), (2, 64)):
        fl = cases["period7"][1][key][2]["qflags"]
        assert (fl & TRUNCATED).any() and (fl == 0).any(), key
    fl = cases["random"][1][(2, 20)][2]["qflags"]
    assert (fl & TRUNCATED).any() and (fl == 0).any()
    for name in TEXTS:
        t, runs = cases[name]
        n = len(t)
        for (k, mh), (qs, _, exp, planted) in runs.items():
            fl, cnt = exp["qflags"], np.diff(exp["off"])
            assert all(bool(f & SHORT) == (len(q) <= k) for f, q in zip(fl, qs))
            assert all(bool(f & LONG) == (len(q) > MAX_M) for f, q in zip(fl, qs))
            assert fl[-1] == SHORT and len(qs[-1]) == 0  # the empty query
            assert (cnt[(fl & (SHORT | LONG)) != 0] == 0).all()
            assert any(len(q) == 257 for q in qs)
            # planted with at most k edits inside the text: an answer exists
            assert planted.sum() > 10 and (cnt[planted & (fl == 0)] > 0).all(), (name, k, mh)
            if mh == 0:
                assert exp["end"].max() == n and exp["end"].min() >= 0  # e = n is an answer; none behind it
                assert k == 0 or exp["neg"] > 0  # a later piece occurs at the text start: s0 < 0
            if name == "random" and mh == 0:
                assert (exp["dist"] == k).any() and (exp["dist"] == 0).any()
    # tiny: n < m - k has no answer; m - k <= n < m is answered, through deletions only
    t, runs = cases["tiny"]
    n = len(t)
    for (k, mh), (qs, _, exp, _) in runs.items():
        cnt = np.diff(exp["off"])
        assert all(cnt[i] == 0 for i, q in enumerate(qs) if MAX_M >= len(q) > n + k)
        assert any(len(q) == 64 for q in qs)
        if k:
            assert any(cnt[i] > 0 for i, q in enumerate(qs) if n < len(q) <= n + k)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cross_checks_against_locate_and_mismatch(sas, cases, build):
    """k = 0: the ends are the sorted locate positions + m; every (s, d) of locate_mismatch at the
    same k appears as the end s + m with a distance <= d."""
    for text in TEXTS:
        t, runs = cases[text]
        idx = sas.SaNaive.build(t, **BUILDS[build])
        qs = [q for q in runs[(0, 0)][0] if 0 < len(q) <= MAX_M]
        qb, qoff, qlen = pack(qs)
        loff, lpos = idx.locate(qb, qoff, qlen)
        off, end, dist, qfl = idx.locate_edit(qb, qoff, qlen, 0)
        assert np.array_equal(off, loff) and not dist.any() and not qfl.any()
        for i, q in enumerate(qs):
            a, b = int(off[i]), int(off[i + 1])
            assert np.array_equal(end[a:b], np.sort(lpos[a:b]) + len(q)), (text, i)
        for k in (1, 2, 3):
            qs = [q for q in runs[(k, 0)][0] if len(q) <= MAX_M]
            qb, qoff, qlen = pack(qs)
            moff, mpos, mdist, _ = idx.locate_mismatch(qb, qoff, qlen, k)
            off, end, dist, _ = idx.locate_edit(qb, qoff, qlen, k)
            assert len(mpos) > 0
            for i, q in enumerate(qs):
                got = dict(zip(end[int(off[i]):int(off[i + 1])].tolist(), dist[int(off[i]):int(off[i + 1])].tolist()))
                for s, d in zip(mpos[int(moff[i]):int(moff[i + 1])].tolist(),
                                mdist[int(moff[i]):int(moff[i + 1])].tolist()):
                    assert got.get(s + len(q), 99) <= d, (text, k, i, s, d)


def test_capacity(sas, cases):
    import torch
    from sas_amd import _lib
    t, runs = cases["period7"]
    qs, (qb, qoff, qlen), exp, _ = runs[(1, 0)]
    total = int(exp["off"][-1])
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    for cap in (0, 1, total // 2, total - 1):
        off, end, dist, qfl, tot = dev_call(torch, idx, qb, qoff, qlen, 1, 0, cap)  # canaries past cap checked
        assert tot == total and np.array_equal(off, exp["off"]) and np.array_equal(qfl, exp["qflags"])
        assert np.array_equal(end, exp["end"][:cap]) and np.array_equal(dist, exp["dist"][:cap])
    off, end, dist, qfl, tot = dev_call(torch, idx, qb, qoff, qlen, 1, 0, total // 2, u32=True)
    assert tot == total and np.array_equal(off, exp["off"]) and np.array_equal(end, exp["end"][:total // 2])
    # out_total and out_dist may be NULL on device pointers
    got = idx.locate_edit(torch.from_numpy(qb).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda(),
                          torch.from_numpy(qlen.astype(np.int32)).cuda(), 1, dist=False, capacity=total)
    torch.cuda.synchronize()
    assert got[2] is None and np.array_equal(got[1].cpu().numpy(), exp["end"])
    # host pointers: ENOSPC, nothing copied, the total and the offsets still reported
    L = _lib.lib()
    nq = len(qoff)
    off = np.zeros(nq + 1, np.uint64)
    end = np.full(total, 7, np.uint64)
    dist = np.full(total, 7, np.uint8)
    qfl = np.full(nq, 7, np.uint8)
    tot = C.c_uint64(0)
    rc = L.sas_locate_edit(idx._h, qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, nq, 1, 0, off.ctypes.data,
                           end.ctypes.data, dist.ctypes.data, qfl.ctypes.data, total - 1, C.byref(tot), None, 0)
    assert rc == errno.ENOSPC and tot.value == total and (end == 7).all() and (dist == 7).all()
    assert np.array_equal(off.astype(np.int64), exp["off"]) and np.array_equal(qfl.astype(np.int64), exp["qflags"])


def test_errors(sas, cases):
    import torch
    from sas_amd import _lib
    t, runs = cases["random"]
    qs, (qb, qoff, qlen), exp, _ = runs[(1, 0)]
    n = len(t)
    L = _lib.lib()
    for idx in (sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100, n - 5), **BARE),  # sas_build_shard
                sas.SaNaive.build_part(t, 1, 3, lcp=False, stree=False, sector=False, quad=True, llcp=False),
                sas.SaNaive.build(t, lcp=False, tagged=True),
                sas.SaNaive.build(t, lcp=False, tagged=True, tag_lines=True)):
        with pytest.raises(sas.SasError) as e:
            idx.locate_edit(qb, qoff, qlen, 1)
        assert e.value.code == errno.ENOTSUP
    bare = sas.SaNaive.build(t, **BARE)
    with pytest.raises(sas.SasError) as e:  # the range search's own refusal
        bare.locate_edit(qb, qoff, qlen, 1)
    assert e.value.code == errno.EINVAL and "sas_search_range" in str(e.value)
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    with pytest.raises(sas.SasError) as e:
        idx.locate_edit(qb, qoff, qlen, 16)
    assert e.value.code == errno.EINVAL
    with pytest.raises(sas.SasError) as e:
        idx.locate_edit_fixed(qb[:64], 32, 16)
    assert e.value.code == errno.EINVAL
    same(idx.locate_edit(qb, qoff, qlen, 1, u32=True), exp, "SAS_LOCATE_U32 below 2^32")
    # null arguments
    off = np.zeros(len(qoff) + 1, np.uint64)
    tot = C.c_uint64(0)
    p = (qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data)
    assert L.sas_locate_edit(idx._h, None, p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0, C.byref(tot),
                             None, 0) == errno.EINVAL
    assert L.sas_locate_edit(idx._h, p[0], None, p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0, C.byref(tot),
                             None, 0) == errno.EINVAL
    assert L.sas_locate_edit(idx._h, p[0], p[1], p[2], 2, 1, 0, None, None, None, None, 0, C.byref(tot), None,
                             0) == errno.EINVAL
    assert L.sas_locate_edit(idx._h, p[0], p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 5, C.byref(tot),
                             None, 0) == errno.EINVAL  # a capacity without out_end
    assert L.sas_locate_edit(idx._h, p[0], p[1], p[2], 2, 1, 0, off.ctypes.data, None, None, None, 0, None, None,
                             0) == errno.EINVAL  # host pointers need out_total
    # bytes > 3: host pointers always validate, device pointers with SAS_VALIDATE
    badq = qb.copy()
    badq[int(qoff[-2])] = 4
    with pytest.raises(sas.SasError) as e:
        idx.locate_edit(badq, qoff, qlen, 1)
    assert e.value.code == errno.EINVAL
    do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
    with pytest.raises(sas.SasError) as e:
        idx.locate_edit(torch.from_numpy(badq).cuda(), do, dl, 1, flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL
    same(idx.locate_edit(torch.from_numpy(qb).cuda(), do, dl, 1, flags=_lib.SAS_VALIDATE), exp, "validated")
    # nq = 0
    off, end, dist, qfl = idx.locate_edit(qb, qoff[:0], qlen[:0], 1)
    assert off.tolist() == [0] and len(end) == 0 and len(dist) == 0 and len(qfl) == 0
