"""Maximal exact matches on the GPU (sas_mems / sas_mems_fixed and SaNaive.mems*) against
test_mems_host.ref_mems, the diagonal-run reference that knows none of the GPU's code."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_match import pack
from test_gpu_mismatch import BARE, BUILDS, TEXTS, make_text
from test_mems_host import SHORT, TRUNCATED, Text, ref_mems

pytestmark = pytest.mark.gpu

LS = (1, 8, 20, 33)
HITS = (0, 4)
SLICES = (1, 31, 32, 33, 63, 64, 65, 129, 300, 5000)
# substitutions at these query offsets leave matches of 31, 32, 33, 63, 64 and 65 chars between them
PLANTS = (31, 64, 98, 162, 227, 293)


def wrap(t, s, m):
    """m chars of t from s on, the text joined to itself at its end."""
    return t[(s + np.arange(m)) % len(t)].copy()


def subst(q, places, rng):
    for j in places:
        if j < len(q):
            q[j] = (q[j] + rng.integers(1, 4)) & 3
    return q


def make_queries(t, seed):
    rng = np.random.default_rng(seed)
    n, qs = len(t), []
    for m in SLICES:
        s = 2 * int(rng.integers(0, n // 2)) + 1  # an odd j: no match starts on a word of the text
        qs.append(wrap(t, s, m))
        qs.append(subst(wrap(t, s + 2, m), PLANTS, rng))
    qs.append(t[n - min(n, 50):].copy())  # ends at n
    qs.append(t[:min(n, 50)].copy())      # starts at 0
    qs.append(subst(t[n - min(n, 70):].copy(), [33], rng))
    for m in (5, 40, 200):
        qs.append(rng.integers(0, 4, m).astype(np.uint8))
    qs.append(np.zeros(40, np.uint8))  # all A: the padding behind the text must not extend a match
    qs.append(t[3:10].copy())          # SAS_MEM_SHORT from L = 8 on
    qs.append(np.zeros(0, np.uint8))   # the empty query
    return qs


def frozen(r):
    for a in r:
        a.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def cases():
    """Per text: the Text, the queries, their ragged batch and the reference answer of every
    (L, max_hits) run (computed once, read-only, shared by every build)."""
    out = {}
    for ti, name in enumerate(TEXTS):
        T = Text(make_text(name))
        qs = make_queries(T.t, 300 + ti)
        exp = {(L, mh): frozen(ref_mems(T, qs, L, max_hits=mh)) for L in LS for mh in HITS}
        out[name] = (T, qs, pack(qs), exp)
    return out


def same(got, exp, what):
    got = [np.asarray(g.cpu() if hasattr(g, "cpu") else g).astype(np.int64) for g in got]
    for name, g, e in zip(("off", "qpos", "tpos", "len", "qflags"), got, exp):
        bad = np.flatnonzero(g != e) if g.shape == e.shape else None
        assert bad is not None and len(bad) == 0, (what, name, g.shape, e.shape,
                                                   None if bad is None else (bad[:5], g[bad[:5]], e[bad[:5]]))


def dev_call(torch, idx, batch, L, mh, capacity, u32=False, flags=0, fixed_m=None):
    """sas_mems / sas_mems_fixed on device pointers into buffers with 64 sentinel elements behind
    every output; returns ((off, qpos, tpos, len, qflags), total) and checks the sentinels."""
    from sas_amd import _lib
    qb, qoff, qlen = batch
    nq = len(qoff) if fixed_m is None else len(qb) // fixed_m
    dq = torch.from_numpy(qb).cuda()
    off = torch.full((nq + 1 + 64,), -7, dtype=torch.int64, device="cuda")
    qpos = torch.full((capacity + 64,), -7, dtype=torch.int32, device="cuda")
    tpos = torch.full((capacity + 64,), -7, dtype=torch.int32 if u32 else torch.int64, device="cuda")
    ln = torch.full((capacity + 64,), -7, dtype=torch.int32, device="cuda")
    qfl = torch.full((nq + 64,), 99, dtype=torch.uint8, device="cuda")
    total = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fl = flags | _lib.SAS_DEVICE_PTRS | (_lib.SAS_LOCATE_U32 if u32 else 0)
    tail = (L, mh, off.data_ptr(), qpos.data_ptr(), tpos.data_ptr(), ln.data_ptr(), qfl.data_ptr(), capacity,
            total.data_ptr(), st, fl)
    if fixed_m is None:
        do = torch.from_numpy(qoff.astype(np.int64)).cuda()
        dl = torch.from_numpy(qlen.astype(np.int32)).cuda()
        _lib.check(_lib.lib().sas_mems(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, *tail))
    else:
        _lib.check(_lib.lib().sas_mems_fixed(idx._h, dq.data_ptr(), fixed_m, nq, *tail))
    torch.cuda.synchronize()
    assert (off[nq + 1:] == -7).all() and (qpos[capacity:] == -7).all() and (tpos[capacity:] == -7).all()
    assert (ln[capacity:] == -7).all() and (qfl[nq:] == 99).all() and int(total[1]) == -7
    return (off[:nq + 1].cpu().numpy(), qpos[:capacity].cpu().numpy(), tpos[:capacity].cpu().numpy(),
            ln[:capacity].cpu().numpy(), qfl[:nq].cpu().numpy()), int(total[0])


def on_device(torch, batch):
    qb, qoff, qlen = batch
    return (torch.from_numpy(qb).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda(),
            torch.from_numpy(qlen.astype(np.int32)).cuda())


def test_reference_shapes(cases):
    """What the cases must contain, asserted from the reference alone."""
    for name in TEXTS:
        T, qs, _, exp = cases[name]
        for (L, mh), r in exp.items():
            off, qpos, tpos, ln, qfl = r
            assert all(bool(f & SHORT) == (len(q) < L) for f, q in zip(qfl, qs))
            assert qfl[-1] == SHORT and len(qs[-1]) == 0
            assert L == 1 or qfl[-2] == SHORT
            assert (ln >= L).all() and (tpos + ln <= T.n).all()
        assert set((31, 32, 33, 63, 64, 65)) <= set(exp[(8, 0)][3].tolist()), name
        assert (exp[(1, 4)][4] & TRUNCATED).any(), name
    # truncated queries with a non-empty, exactly defined answer beside unflagged ones
    off, _, _, _, fl = cases["zero_tail"][3][(8, 4)]
    assert ((fl & TRUNCATED) != 0)[np.diff(off) > 0].any() and (fl == 0).any()
    # a match of the all-A query that ends at the text end, where the padding goes on
    T, qs, _, exp = cases["zero_tail"]
    off, qpos, tpos, ln, _ = exp[(8, 0)]
    a = len(qs) - 3
    assert np.array_equal(qs[a], np.zeros(40, np.uint8))
    assert (tpos[off[a]:off[a + 1]] + ln[off[a]:off[a + 1]] == T.n).any()


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("text", TEXTS)
def test_mems_equal_reference(sas, cases, text, build):
    import torch
    from sas_amd import _lib
    T, qs, batch, exp = cases[text]
    idx = sas.SaNaive.build(T.t, **BUILDS[build])
    dbatch = on_device(torch, batch)
    for (L, mh), r in exp.items():
        what = (text, build, L, mh)
        total = int(r[0][-1])
        got, tot = dev_call(torch, idx, batch, L, mh, total)  # device pointers, u64, exact capacity
        assert tot == total, what
        same(got, r, what + ("device",))
        got, tot = dev_call(torch, idx, batch, L, mh, total, u32=True)
        assert tot == total and got[2].dtype == np.int32, what
        same(got, r, what + ("device u32",))
        if mh == 4:  # host pointers; the Python mirror on device pointers (a sizing call first)
            host = idx.mems(*batch, L, max_hits=mh)
            assert [a.dtype for a in host] == [np.uint64, np.uint32, np.uint64, np.uint32, np.uint8]
            same(host, r, what + ("host",))
            got = idx.mems(*dbatch, L, max_hits=mh, u32=True)
            torch.cuda.synchronize()
            assert got[2].dtype == torch.int32 and got[1].dtype == torch.int32 and got[4].dtype == torch.uint8
            same(got, r, what + ("mirror u32",))
        if L == 8:  # the range search without the prefix table: the same bytes
            got, _ = dev_call(torch, idx, batch, L, mh, total, flags=_lib.SAS_NO_PREFIX_TABLE)
            same(got, r, what + ("no table",))


@pytest.mark.parametrize("build", ["quad_p8", "sa40"])
@pytest.mark.parametrize("text", ["period7", "random"])
def test_unique(sas, cases, text, build):
    import torch
    from sas_amd import _lib
    T, qs, _, exp = cases[text]
    # the whole text as a query: on period7 its full-length match is the only string that occurs once
    qs = [q for q in qs if len(q) <= 300] + [T.t.copy()]
    batch = pack(qs)
    idx = sas.SaNaive.build(T.t, **BUILDS[build])
    for L, mh in ((8, 0), (20, 0), (8, 4)):
        r = ref_mems(T, qs, L, max_hits=mh, unique=True)
        plain = ref_mems(T, qs, L, max_hits=mh)
        # the flag keeps some matches and, where short ones are many, drops some
        assert r[0][-1] <= plain[0][-1] and (r[0][-1] < plain[0][-1] or (L, mh) != (8, 0)), (text, L, mh)
        assert r[0][-1] > 0 or (text, mh) == ("period7", 4)  # there every window occurs more than 4 times
        got, tot = dev_call(torch, idx, batch, L, mh, int(r[0][-1]), flags=_lib.SAS_MEM_UNIQUE)
        assert tot == r[0][-1]
        same(got, r, (text, build, L, mh, "unique"))
        same(idx.mems(*batch, L, max_hits=mh, unique=True), r, (text, build, L, mh, "unique host"))


# a gap (1800..1900), two touching segments (at 1000, a record start, and at 2500) on the random text
SEQ_START = [0, 1000, 2500, 4099]
SEG_LO = [0, 1000, 1900, 2500]
SEG_HI = [1000, 1800, 2500, 4099]


@pytest.mark.parametrize("build", ["quad_p8", "sa40", "quad_notable"])
def test_layout(sas, cases, build):
    import torch
    from sas_amd import _lib
    T, qs, _, _ = cases["random"]
    t, n = T.t, T.n
    assert n == SEQ_START[-1]
    rng = np.random.default_rng(77)
    qs = [q for q in qs if len(q) <= 300]
    qs += [t[900:1100].copy(),   # a record start inside a match
           t[1700:2000].copy(),  # a match across the gap
           t[2400:2600].copy(),  # two touching segments
           subst(t[990:1030].copy(), [5], rng),
           t[1790:1810].copy(), t[1880:1925].copy(), t[999:1001].copy()]
    batch = pack(qs)
    lay = (SEG_LO, SEG_HI)
    idx = sas.SaNaive.build(t, **BUILDS[build])
    for L, mh, uniq in ((1, 0, False), (8, 0, False), (20, 0, False), (8, 4, False), (8, 0, True)):
        fl = _lib.SAS_MEM_UNIQUE if uniq else 0
        none = ref_mems(T, qs, L, max_hits=mh, unique=uniq)
        r = ref_mems(T, qs, L, max_hits=mh, unique=uniq, layout=lay)
        assert not np.array_equal(r[3], none[3])  # the layout cuts matches
        idx.set_layout(None)
        plain, tot0 = dev_call(torch, idx, batch, L, mh, int(none[0][-1]), flags=fl)
        same(plain, none, (build, L, mh, uniq, "no layout"))
        idx.set_layout([0, n], [0], [n])  # one segment [0, n): byte-identical to none
        one, tot1 = dev_call(torch, idx, batch, L, mh, int(none[0][-1]), flags=fl)
        assert tot0 == tot1 and all(np.array_equal(a, b) for a, b in zip(plain, one))
        idx.set_layout(SEQ_START, SEG_LO, SEG_HI)
        got, tot = dev_call(torch, idx, batch, L, mh, int(r[0][-1]), flags=fl)
        assert tot == r[0][-1]
        same(got, r, (build, L, mh, uniq, "layout"))
        same(idx.mems(*batch, L, max_hits=mh, unique=uniq), r, (build, L, mh, uniq, "layout host"))
    idx.set_layout(None)


def tile_cases():
    """(name, text, queries, L): a tile inside one window, and a tile's slice of the candidate
    offsets longer than the kernel's LDS stage (4,096 windows)."""
    rng = np.random.default_rng(9)
    zeros = np.zeros(2500, np.uint8)  # longer than make_text's: a window owns more than 2,048 candidates
    t = make_text("random")
    a, b = t[101:131].copy(), t[2001:2041].copy()
    long = np.concatenate([a, rng.integers(0, 4, 3 * 4096 + 500).astype(np.uint8), b])
    return [("inside one window", zeros, [np.zeros(40, np.uint8)], 8),
            ("sparse windows", t, [long, t[5:60].copy()], 20)]


@pytest.mark.parametrize("case", [0, 1])
def test_tile_paths(sas, case, monkeypatch):
    import torch
    name, t, qs, L = tile_cases()[case]
    T = Text(t)
    r = ref_mems(T, qs, L)
    off, qpos = r[0], r[1]
    if case == 0:
        assert T.n - L + 1 > 2048  # every window's candidates
    else:  # matches at both ends of the long query and at least 3 x 4,096 windows without a candidate between
        first = qpos[off[0]:off[1]]
        assert first.min() == 0 and np.diff(np.sort(first)).max() >= 3 * 4096 + L
    batch = pack(qs)
    total = int(off[-1])
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    monkeypatch.delenv("SAS_TILE_GRID", raising=False)
    free, _ = dev_call(torch, idx, batch, L, 0, total)
    monkeypatch.setenv("SAS_TILE_GRID", "1")  # read per call: one workgroup loops over every tile
    assert sas._lib.lib().sas_tile_grid_cap() == 1
    capped, _ = dev_call(torch, idx, batch, L, 0, total)
    monkeypatch.delenv("SAS_TILE_GRID")
    assert all(np.array_equal(x, y) for x, y in zip(free, capped)), name
    same(free, r, (name, "uncapped"))
    same(capped, r, (name, "capped"))


def test_contract(sas, cases):
    import torch
    from sas_amd import _lib
    T, qs, batch, exp = cases["period7"]
    qb, qoff, qlen = batch
    Lm, mh = 20, 0
    r = exp[(Lm, mh)]
    total = int(r[0][-1])
    assert total > 8
    idx = sas.SaNaive.build(T.t, **BUILDS["quad_p8"])
    # device pointers: a capacity below the total leaves everything at and past it alone
    for cap in (0, 1, total // 2, total - 1):
        got, tot = dev_call(torch, idx, batch, Lm, mh, cap)  # sentinels past cap checked
        assert tot == total and np.array_equal(got[0], r[0]) and np.array_equal(got[4], r[4])
        assert all(np.array_equal(g, e[:cap]) for g, e in zip(got[1:4], r[1:4]))
    # out_total and out_qflags may be NULL on device pointers
    L = _lib.lib()
    nq = len(qoff)
    dq, do, dl = on_device(torch, batch)
    off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    _lib.check(L.sas_mems(idx._h, dq.data_ptr(), do.data_ptr(), dl.data_ptr(), nq, Lm, mh, off.data_ptr(), None, None,
                          None, None, 0, None, torch.cuda.current_stream().cuda_stream, _lib.SAS_DEVICE_PTRS))
    torch.cuda.synchronize()
    assert np.array_equal(off.cpu().numpy(), r[0])
    # host pointers: the sizing call, the exact capacity, ENOSPC with the total and the offsets
    off = np.zeros(nq + 1, np.uint64)
    qpos, tpos, ln = np.full(total, 7, np.uint32), np.full(total, 7, np.uint64), np.full(total, 7, np.uint32)
    qfl = np.full(nq, 7, np.uint8)
    tot = C.c_uint64(0)
    lead = (idx._h, qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, nq, Lm, mh, off.ctypes.data)
    rc = L.sas_mems(*lead, None, None, None, qfl.ctypes.data, 0, C.byref(tot), None, 0)
    assert rc == errno.ENOSPC and tot.value == total
    assert np.array_equal(off.astype(np.int64), r[0]) and np.array_equal(qfl.astype(np.int64), r[4])
    off[:] = 0
    tot.value = 0
    rc = L.sas_mems(*lead, qpos.ctypes.data, tpos.ctypes.data, ln.ctypes.data, qfl.ctypes.data, total - 1,
                    C.byref(tot), None, 0)
    assert rc == errno.ENOSPC and tot.value == total and (qpos == 7).all() and (tpos == 7).all() and (ln == 7).all()
    assert np.array_equal(off.astype(np.int64), r[0])
    _lib.check(L.sas_mems(*lead, qpos.ctypes.data, tpos.ctypes.data, ln.ctypes.data, qfl.ctypes.data, total,
                          C.byref(tot), None, 0))
    same((off, qpos, tpos, ln, qfl), r, "host exact capacity")
    # nq == 0
    got = idx.mems(qb, qoff[:0], qlen[:0], Lm)
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])
    got = idx.mems(dq, do[:0], dl[:0], Lm)
    torch.cuda.synchronize()
    assert got[0].cpu().tolist() == [0] and got[2].numel() == 0


def test_errors(sas, cases):
    import torch
    from sas_amd import _lib
    T, qs, batch, exp = cases["random"]
    qb, qoff, qlen = batch
    t, n = T.t, T.n
    L = _lib.lib()
    # min_len == 0 is checked before the index
    off = np.zeros(len(qoff) + 1, np.uint64)
    tot = C.c_uint64(0)
    assert L.sas_mems(None, qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, 2, 0, 0, off.ctypes.data, None, None,
                      None, None, 0, C.byref(tot), None, 0) == errno.EINVAL
    assert b"min_len" in L.sas_last_error()
    assert L.sas_mems_fixed(None, qb.ctypes.data, 8, 2, 0, 0, off.ctypes.data, None, None, None, None, 0,
                            C.byref(tot), None, 0) == errno.EINVAL
    for idx in (sas.SaNaive.build(t, sa=O.build_sa(t), rank_range=(100, n - 5), **BARE),
                sas.SaNaive.build_part(t, 1, 3, lcp=False, stree=False, sector=False, quad=True, llcp=False),
                sas.SaNaive.build(t, lcp=False, tagged=True),
                sas.SaNaive.build(t, lcp=False, tagged=True, tag_lines=True)):
        with pytest.raises(sas.SasError) as e:
            idx.mems(qb, qoff, qlen, 8)
        assert e.value.code == errno.ENOTSUP
    bare = sas.SaNaive.build(t, **BARE)
    with pytest.raises(sas.SasError) as e:  # the range search's own refusal
        bare.mems(qb, qoff, qlen, 8)
    assert e.value.code == errno.EINVAL and "sas_search_range" in str(e.value)
    idx = sas.SaNaive.build(t, **BUILDS["quad_p8"])
    with pytest.raises(sas.SasError) as e:
        idx.mems(qb, qoff, qlen, 0)
    assert e.value.code == errno.EINVAL
    # null arguments; a capacity without its outputs; host pointers need out_total
    p = (qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data)
    tail = (None, None, None, None, 0, C.byref(tot), None, 0)
    assert L.sas_mems(idx._h, None, p[1], p[2], 2, 8, 0, off.ctypes.data, *tail) == errno.EINVAL
    assert L.sas_mems(idx._h, p[0], None, p[2], 2, 8, 0, off.ctypes.data, *tail) == errno.EINVAL
    assert L.sas_mems(idx._h, p[0], p[1], p[2], 2, 8, 0, None, *tail) == errno.EINVAL
    assert L.sas_mems(idx._h, p[0], p[1], p[2], 2, 8, 0, off.ctypes.data, None, None, None, None, 5, C.byref(tot),
                      None, 0) == errno.EINVAL
    assert L.sas_mems(idx._h, p[0], p[1], p[2], 2, 8, 0, off.ctypes.data, None, None, None, None, 0, None, None,
                      0) == errno.EINVAL
    # bytes > 3: host pointers always validate (a short query's bytes too), device pointers with SAS_VALIDATE
    for at in (int(qoff[-4]) + 3, int(qoff[-2]) + 1):  # in the all-A query, in the 7-char query
        badq = qb.copy()
        badq[at] = 4
        with pytest.raises(sas.SasError) as e:
            idx.mems(badq, qoff, qlen, 8)
        assert e.value.code == errno.EINVAL
        dq, do, dl = on_device(torch, (badq, qoff, qlen))
        with pytest.raises(sas.SasError) as e:
            idx.mems(dq, do, dl, 8, flags=_lib.SAS_VALIDATE)
        assert e.value.code == errno.EINVAL
    same(idx.mems(*on_device(torch, batch), 8, flags=_lib.SAS_VALIDATE), exp[(8, 0)], "validated")
    # SAS_LOCATE_U32 misuse: 32-bit positions into a 64-bit buffer, and the other way round (the refusal
    # for a text of 2^32 chars and more is seed_index_checks', which every call of the family goes through)
    dq, do, dl = on_device(torch, batch)
    with pytest.raises(ValueError):
        idx.mems(dq, do, dl, 8, u32=True, out=torch.empty(16, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        idx.mems(dq, do, dl, 8, out=torch.empty(16, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        idx.mems_fixed(qb[:64], 0, 8)


@pytest.mark.parametrize("build", ["quad_p8", "sa40"])
def test_fixed_equals_ragged(sas, cases, build):
    import torch
    for text in TEXTS:
        T, _, _, _ = cases[text]
        rng = np.random.default_rng(3)
        for m, L in ((24, 8), (33, 33), (64, 20), (7, 8), (150, 20)):
            qs = [subst(wrap(T.t, int(rng.integers(0, T.n)), m), rng.choice(m, 2, replace=False), rng)
                  for _ in range(9)]
            qs.append(rng.integers(0, 4, m).astype(np.uint8))
            batch = pack(qs)
            r = ref_mems(T, qs, L, max_hits=6)
            idx = sas.SaNaive.build(T.t, **BUILDS[build])
            rag, tot = dev_call(torch, idx, batch, L, 6, int(r[0][-1]))
            same(rag, r, (text, build, m, L, "ragged"))
            fb = (batch[0][:len(qs) * m], None, None)
            fix, tot2 = dev_call(torch, idx, fb, L, 6, int(r[0][-1]), fixed_m=m)
            assert tot == tot2 and all(np.array_equal(a, b) for a, b in zip(rag, fix)), (text, build, m, L)
            same(idx.mems_fixed(fb[0], m, L, max_hits=6), r, (text, build, m, L, "fixed host"))
            got = idx.mems_fixed(torch.from_numpy(fb[0]).cuda(), m, L, max_hits=6, capacity=int(r[0][-1]) + 3)
            torch.cuda.synchronize()
            same([got[0]] + [g[:int(r[0][-1])] for g in got[1:4]] + [got[4]], r, (text, build, m, L, "fixed capacity"))


@pytest.mark.parametrize("build", list(BUILDS))
def test_whole_queries_equal_locate(sas, cases, build):
    """Queries that occur whole, L = m: one match (0, j, m) per occurrence, in locate's order."""
    for text in TEXTS:
        T, _, _, _ = cases[text]
        rng = np.random.default_rng(4)
        m = 24
        qb = np.concatenate([T.t[s:s + m] for s in rng.integers(0, T.n - m, 20)] + [np.zeros(64, np.uint8)])
        idx = sas.SaNaive.build(T.t, **BUILDS[build])
        loff, lpos = idx.locate_fixed(qb[:20 * m], m)
        off, qpos, tpos, ln, qfl = idx.mems_fixed(qb[:20 * m], m, m)
        assert np.array_equal(off, loff) and np.array_equal(tpos, lpos) and len(lpos) >= 20
        assert not qpos.any() and (ln == m).all() and not qfl.any()
