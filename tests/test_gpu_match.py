"""Longest-prefix match and matching statistics (sas_match / sas_match_fixed / sas_match_stats
and SaNaive.match*) against a brute force that knows neither the GPU-built suffix array nor
the range kernels: the length by bytes.find with bisection on the prefix length, the ranks by
bisect over the suffix slices of the CPU oracle's suffix array (O.build_sa)."""
import bisect
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

LENS = (0, 1, 2, 5, 7, 8, 31, 32, 33, 64, 65, 129, 200)  # with p - 1 and p of the p = 2 and p = 8 tables
EDGES = (31, 32, 33, 63, 64, 65, 127, 128, 129)          # the query words' boundaries
BARE = dict(lcp=False, stree=False, sector=False, quad=False, llcp=False)
QUAD = dict(lcp=False, stree=False, sector=False, quad=True, llcp=False)
BUILDS = {
    "bare": dict(BARE),                            # no table, no trees: len and pos only
    "quad_p2": dict(QUAD, prefix=2),               # dense buckets
    "quad_p8": dict(QUAD, prefix=8),               # mostly empty buckets at these n
    "inline2": dict(QUAD, prefix=4, prefix_inline=2),
    "sa40": dict(QUAD, sa40=True),                 # packed 40-bit SA, 5-byte table entries, default p
}


def make_text(name):
    if name == "random":
        return O.random_string(4099, seed=11)
    if name == "zeros":
        return np.zeros(300, np.uint8)
    if name == "period7":
        return np.tile(np.array([0, 1, 3, 2, 2, 0, 3], np.uint8), 286)[:2000]
    assert name == "zero_tail"  # suffixes shorter than p at the text end, keyed zero padded
    return np.concatenate([O.random_string(1500, seed=12), np.zeros(20, np.uint8)])


TEXTS = ("random", "zeros", "period7", "zero_tail")


def lcp_of(a: bytes, b: bytes) -> int:
    k, e = 0, min(len(a), len(b))
    while k < e and a[k] == b[k]:
        k += 1
    return k


class Brute:
    """The definition, on bytes: Python's bytes order is Rust's slice order."""

    def __init__(self, t: np.ndarray):
        self.tb = t.tobytes()
        self.n = len(t)
        self.sa = O.build_sa(t).astype(np.int64)
        self.suf = [self.tb[i:] for i in self.sa]

    def match(self, q: bytes):
        """(len, pos, lo, hi) of sas.h's sas_match for one query."""
        n, lo_k, hi_k = self.n, 0, len(q)
        while lo_k < hi_k:  # q[:k] occurs for every k up to the answer and for none past it
            mid = (lo_k + hi_k + 1) // 2
            if self.tb.find(q[:mid]) >= 0:
                lo_k = mid
            else:
                hi_k = mid - 1
        ln = lo_k
        lb = bisect.bisect_left(self.suf, q)
        a = lcp_of(q, self.suf[lb - 1]) if lb > 0 else 0
        b = lcp_of(q, self.suf[lb]) if lb < n else 0
        assert max(a, b) == ln, "the two-neighbour claim itself"
        if ln == 0:
            return 0, n, 0, n
        pos = int(self.sa[lb]) if lb < n and b == ln else int(self.sa[lb - 1])
        pre = q[:ln]
        return ln, pos, bisect.bisect_left(self.suf, pre), bisect.bisect_left(self.suf, pre + b"\xff")


def make_queries(t: np.ndarray, seed: int):
    rng = np.random.default_rng(seed)
    n, qs = len(t), []

    def sl(off, m):
        return t[off:off + m].copy()

    for m in LENS:  # exact text slices and random strings
        for _ in range(30):
            qs.append(sl(int(rng.integers(0, max(n - m, 0) + 1)), m))
            qs.append(rng.integers(0, 4, m).astype(np.uint8))
    for m in LENS:  # one char changed: across the word boundaries, and anywhere
        js = [j for j in EDGES if j < m] + ([int(x) for x in rng.integers(0, m, 12)] if m else [])
        for j in js:
            for _ in range(4):
                q = sl(int(rng.integers(0, max(n - m, 0) + 1)), m)
                if len(q) > j:
                    q[j] = (q[j] + rng.integers(1, 4)) & 3
                qs.append(q)
    for k in range(1, 120):  # slices that run past the text end, extra chars appended
        qs.append(np.concatenate([t[n - min(k, n):], rng.integers(0, 4, int(rng.integers(0, 70))).astype(np.uint8)]))
    for k in range(1, 41):  # runs of code 0 (the zero-padded keys of the last suffixes)
        qs.append(np.zeros(k, np.uint8))
        qs.append(np.concatenate([np.zeros(k, np.uint8), rng.integers(1, 4, 3).astype(np.uint8)]))
    return qs


def pack(qs):
    """Ragged batch: bytes (64 spare bytes behind), offsets, lengths."""
    qlen = np.array([len(q) for q in qs], np.uint32)
    qoff = np.zeros(len(qs), np.uint64)
    qoff[1:] = np.cumsum(qlen[:-1], dtype=np.uint64)
    return np.concatenate(list(qs) + [np.zeros(64, np.uint8)]), qoff, qlen


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def cases():
    """Per text: the text, its queries as a ragged batch, and the brute-force answers (computed
    once, read-only, shared by every build)."""
    out = {}
    for k, name in enumerate(TEXTS):
        t = make_text(name)
        qs = make_queries(t, 100 + k)
        br = Brute(t)
        exp = np.array([br.match(q.tobytes()) for q in qs], np.int64)
        exp.setflags(write=False)
        out[name] = (t, qs, pack(qs), exp)
    return out


def dev_match(torch, idx, qb, qoff, qlen, ranges, flags=0, pos=True):
    """sas_match on device pointers into buffers over-allocated by 64 sentinel elements;
    returns the results and checks the sentinels."""
    from sas_amd import _lib
    nq = len(qoff)
    dq = torch.from_numpy(qb).cuda()
    do = torch.from_numpy(qoff.astype(np.int64)).cuda()
    dl = torch.from_numpy(qlen.astype(np.int32)).cuda()
    ln = torch.full((nq + 64,), -7, dtype=torch.int32, device="cuda")
    outs = [torch.full((nq + 64,), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    use = [pos, ranges, ranges]
    ptr = [o.data_ptr() if u else None for o, u in zip(outs, use)]
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().sas_match(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, ln.data_ptr(), *ptr, st,
                                    flags | _lib.SAS_DEVICE_PTRS))
    torch.cuda.synchronize()
    assert (ln[nq:] == -7).all()
    for o, u in zip(outs, use):
        assert (o[nq if u else 0:] == -7).all()
    return [ln[:nq].cpu().numpy().astype(np.int64)] + [o[:nq].cpu().numpy() for o in outs]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("text", TEXTS)
def test_match_equals_brute_force(sas, cases, text, build):
    import torch
    from sas_amd import _lib
    t, qs, (qb, qoff, qlen), exp = cases[text]
    assert len(qs) > 1500
    idx = sas.SaNaive.build(t, **BUILDS[build])
    ranges = build != "bare"
    ncol = 4 if ranges else 2
    got = dev_match(torch, idx, qb, qoff, qlen, ranges)
    for c, name in enumerate(("len", "pos", "lo", "hi")[:ncol]):
        bad = np.flatnonzero(got[c] != exp[:, c])
        assert len(bad) == 0, (name, bad[:5], [qs[i].tolist() for i in bad[:2]], got[c][bad[:5]], exp[bad[:5], c])
    for k, q in enumerate(qs):  # the position holds the prefix
        ln, p = int(got[0][k]), int(got[1][k])
        assert np.array_equal(t[p:p + ln], q[:ln]) and (ln > 0 or p == len(t))
    if ranges:  # every query from [0, n): the same answers
        alt = dev_match(torch, idx, qb, qoff, qlen, True, flags=_lib.SAS_NO_PREFIX_TABLE)
        for c in range(4):
            assert np.array_equal(alt[c], got[c]), c
    # NULL optional outputs
    only_len = dev_match(torch, idx, qb, qoff, qlen, False, pos=False)
    assert np.array_equal(only_len[0], got[0])
    # host pointers agree with device pointers
    host = idx.match(qb, qoff, qlen, ranges=ranges)
    assert host[0].dtype == np.uint32 and host[1].dtype == np.uint64
    for c in range(ncol):
        assert np.array_equal(host[c].astype(np.int64), got[c]), c
    # the fixed-length entry point agrees with the ragged one
    for m in (1, 5, 32, 33, 65, 129):
        sel = [q for q in qs if len(q) == m]
        fb = np.concatenate(sel + [np.zeros(64, np.uint8)])
        fo = np.arange(len(sel), dtype=np.uint64) * m
        ref = dev_match(torch, idx, fb, fo, np.full(len(sel), m, np.uint32), ranges)
        fixed = idx.match_fixed(torch.from_numpy(fb[:len(sel) * m]).cuda(), m, ranges=ranges)
        torch.cuda.synchronize()
        for c in range(ncol):
            assert np.array_equal(fixed[c].cpu().numpy().astype(np.int64), ref[c]), (m, c)
        hfixed = idx.match_fixed(fb[:len(sel) * m], m, ranges=ranges)
        for c in range(ncol):
            assert np.array_equal(hfixed[c].astype(np.int64), ref[c]), (m, c)


@pytest.mark.parametrize("build", ["bare", "quad_p8", "sa40"])
def test_matching_statistics(sas, cases, build):
    import torch
    t = cases["random"][0]
    n, plen = len(t), 3000
    rng = np.random.default_rng(3)
    parts = []
    while sum(map(len, parts)) < plen:
        m = int(rng.integers(5, 150))
        s = t[int(rng.integers(0, n - m)):][:m].copy()
        s[int(rng.integers(0, m))] ^= 1
        parts.append(s)
    pat = np.concatenate(parts)[:plen]
    idx = sas.SaNaive.build(t, **BUILDS[build])
    ranges = build != "bare"
    dpat = torch.from_numpy(np.concatenate([pat, np.zeros(64, np.uint8)])).cuda()
    for max_len in (1, 64, 200):
        st = idx.match_stats(dpat[:plen], max_len, ranges=ranges)
        qoff = np.arange(plen, dtype=np.uint64)
        qlen = np.minimum(max_len, plen - np.arange(plen)).astype(np.uint32)
        ref = idx.match(dpat, torch.from_numpy(qoff.astype(np.int64)).cuda(),
                        torch.from_numpy(qlen.astype(np.int32)).cuda(), ranges=ranges)
        torch.cuda.synchronize()
        host = idx.match_stats(pat, max_len, ranges=ranges)
        for c in range(len(ref)):
            assert np.array_equal(st[c].cpu().numpy(), ref[c].cpu().numpy()), (max_len, c)
            assert np.array_equal(host[c].astype(np.int64), ref[c].cpu().numpy().astype(np.int64)), (max_len, c)
        ln = st[0].cpu().numpy().astype(np.int64)
        assert (ln[1:] >= ln[:-1] - 1).all() and (ln <= qlen).all()
        pos = st[1].cpu().numpy()
        for i in range(0, plen, 37):
            assert np.array_equal(t[pos[i]:pos[i] + ln[i]], pat[i:i + ln[i]])


def test_mid_size_one_substitution(sas):
    """n = 2^20, the default table, 10^5 len-48 slices with one substituted char."""
    import torch
    n, m, nq = 1 << 20, 48, 100_000
    t = O.random_string(n, seed=21)
    rng = np.random.default_rng(22)
    off = rng.integers(0, n - m, nq)
    q = t[off[:, None] + np.arange(m)[None, :]].copy()
    j = rng.integers(0, m, nq)
    q[np.arange(nq), j] = (q[np.arange(nq), j] + rng.integers(1, 4, nq)) & 3
    idx = sas.SaNaive.build(torch.from_numpy(t).cuda(), lcp=False, stree=False, sector=False, llcp=False)
    assert idx.stats()["prefix_chars"] > 0
    dq = torch.from_numpy(np.concatenate([q.reshape(-1), np.zeros(64, np.uint8)])).cuda()
    ln, pos, lo, hi = idx.match_fixed(dq[:nq * m], m)
    qoff = torch.arange(nq, dtype=torch.int64, device="cuda") * m
    rlo, rhi = idx.search_range(dq, qoff, ln)
    nxt = torch.clamp(ln + 1, max=m)
    elo, ehi = idx.search_range(dq, qoff, nxt)
    torch.cuda.synchronize()
    ln, pos = ln.cpu().numpy().astype(np.int64), pos.cpu().numpy()
    assert (ln >= j).all() and (ln <= m).all()  # everything before the substitution occurs
    # t[pos : pos + len] == q[: len]
    tp = np.concatenate([t, np.full(m, 9, np.uint8)])
    win = tp[pos[:, None] + np.arange(m)[None, :]]
    assert ((win == q) | (np.arange(m)[None, :] >= ln[:, None])).all()
    assert torch.equal(lo, rlo) and torch.equal(hi, rhi) and bool((hi > lo).all())
    short = torch.from_numpy(ln < m).cuda()
    assert bool((ehi[short] == elo[short]).all())  # one more char occurs nowhere
    # a sample against the oracle's lower bound and the two neighbours' lcps
    sa = O.build_sa(t)
    tpad = O.padded(t)
    for k in range(0, nq, nq // 2000):
        lb = O.lower_bound_rank(tpad, n, sa, q[k])
        a = lcp_of(q[k].tobytes(), t[sa[lb - 1]:sa[lb - 1] + m].tobytes()) if lb > 0 else 0
        b = lcp_of(q[k].tobytes(), t[sa[lb]:sa[lb] + m].tobytes()) if lb < n else 0
        assert ln[k] == max(a, b), k
        assert pos[k] == (sa[lb] if lb < n and b == ln[k] else sa[lb - 1]), k


def test_errors(sas, cases):
    import torch
    from sas_amd import _lib
    t, qs, (qb, qoff, qlen), exp = cases["random"]
    n = len(t)
    sa = O.build_sa(t)
    for idx in (sas.SaNaive.build(t, sa=sa, rank_range=(100, n - 5), **BARE),
                sas.SaNaive.build_part(t, 1, 3, lcp=False, stree=False, sector=False, quad=True, llcp=False),
                sas.SaNaive.build(t, lcp=False, tagged=True),
                sas.SaNaive.build(t, lcp=False, tagged=True, tag_lines=True)):
        with pytest.raises(sas.SasError) as e:
            idx.match(qb, qoff, qlen, ranges=False)
        assert e.value.code == errno.ENOTSUP
    bare = sas.SaNaive.build(t, **BARE)
    with pytest.raises(sas.SasError) as e:  # the range search's own refusal
        bare.match(qb, qoff, qlen, ranges=True)
    assert e.value.code == errno.EINVAL and "sas_search_range" in str(e.value)
    badq = qb.copy()
    badq[int(qoff[-1])] = 4
    with pytest.raises(sas.SasError) as e:  # host pointers always validate
        bare.match(badq, qoff, qlen, ranges=False)
    assert e.value.code == errno.EINVAL
    dq = torch.from_numpy(badq).cuda()
    do, dl = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
    with pytest.raises(sas.SasError) as e:
        bare.match(dq, do, dl, ranges=False, flags=_lib.SAS_VALIDATE)
    assert e.value.code == errno.EINVAL
    bare.match(torch.from_numpy(qb).cuda(), do, dl, ranges=False, flags=_lib.SAS_VALIDATE)
    # nq = 0: nothing is read or written
    assert _lib.lib().sas_match(bare._h, None, None, None, 0, None, None, None, None, None, 0) == 0
    assert _lib.lib().sas_match_stats(bare._h, None, 0, 64, None, None, None, None, None, _lib.SAS_DEVICE_PTRS) == 0
    ln, pos = bare.match(qb, qoff[:0], qlen[:0], ranges=False)
    assert len(ln) == 0 and len(pos) == 0
