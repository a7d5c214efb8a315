"""The seed-and-verify calls (locate_mismatch, locate_edit, align_edit, map_edit, map_pairs,
map_pairs_rescue) at text positions of 2^15 and more, bit for bit against the shifted reference of
tests/test_far_host.py: the 4099-char `random` text behind a filler over {A, C}, so that every
answer is the brute force's on the filler's last 1024 chars + the text, moved by delta - 1024.

  straddle16   delta = 2^16 - 2048   positions on both sides of 2^16, all >= 2^15; ebits = 17
  pow17        delta = 2^17 - 4099   n = 2^17 exactly: an end equal to n needs ebits = 18
  n24          delta = 2^24          ebits = 25: the proposals' sort keys (query << ebits | end) pass 32 bits

Device pointers with canaries (the dev_call helpers of the calls' own test files), u64 and u32
outputs, and one host-pointer call per call and shape."""
import numpy as np
import pytest

import test_far_host as F
import test_gpu_align as TA
import test_gpu_edit as TE
import test_gpu_map as TM
import test_gpu_mismatch as TMM
import test_gpu_pairs as TP
import test_gpu_rescue as TR
from test_align_host import NONE_DIST

pytestmark = pytest.mark.gpu

DELTA = {"straddle16": (1 << 16) - 2048, "pow17": (1 << 17) - 4099, "n24": 1 << 24}
CASES = [("straddle16", "quad_p8"), ("straddle16", "sa40"), ("pow17", "quad_p8"), ("pow17", "sa40"), ("n24", "quad_p8")]
WINDOWS = TR.WINDOWS


def ed_bits(v):
    """edit_path.hpp: the bits that hold every value in [0, v]."""
    return max(1, int(v).bit_length())


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def indexes(sas):
    """The index of a (shape, build), built once for the module's tests."""
    made = {}

    def get(shape, build):
        if (shape, build) not in made:
            made[(shape, build)] = sas.SaNaive.build(F.big_text(DELTA[shape]), **TE.BUILDS[build])
        return made[(shape, build)]
    yield get
    for idx in made.values():
        idx.free()


def geometry(shape):
    delta = DELTA[shape]
    return delta - F.M, F.M + F.SMALL_N, delta + F.SMALL_N


def check_positions(shape, ends, n, what):
    """What the shape is for, from the expected ends alone."""
    ends = np.asarray(ends)
    assert ends.min() >= 1 << 15, what
    if shape == "straddle16":
        assert (ends < (1 << 16)).any() and (ends >= (1 << 16)).any() and ed_bits(n) == 17, what
    elif shape == "pow17":
        assert n == 1 << 17 and (ends == n).any() and ed_bits(n) == 18 and ed_bits(n - 1) == 17, what
    else:
        assert ends.min() >= 1 << 24 and ed_bits(n) == 25, what


@pytest.mark.parametrize("shape,build", CASES)
def test_locate_and_align_far(sas, indexes, shape, build):
    import torch
    by, n_ref, n = geometry(shape)
    mm = {k: F.reference("mismatch", k) for k in F.MISMATCH_KS}
    ed = {run: F.reference("edit", *run) for run in F.EDIT_RUNS}   # the references stand before the GPU is asked
    idx = indexes(shape, build)
    assert idx.stats()["n"] == n
    for k, (c, exp) in mm.items():
        what = (shape, build, "mismatch", k)
        want = F.shift(exp, by, n_ref, n)
        total = int(want["off"][-1])
        check_positions(shape, want["pos"] + np.repeat(c.qlen.astype(np.int64), np.diff(want["off"])), n, what)
        for u32 in (False, True):
            off, pos, dist, qfl, tot = TMM.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, 0, total, u32=u32)
            assert tot == total, what
            TMM.same((off, pos, dist, qfl), want, what + (u32,))
        if build == "quad_p8" and k == 3:
            TMM.same(idx.locate_mismatch(c.qb, c.qoff, c.qlen, k), want, what + ("host",))
    for (k, mh), (c, exp, al) in ed.items():
        what = (shape, build, "edit", k, mh)
        want = F.shift(exp, by, n_ref, n)
        total = int(want["off"][-1])
        check_positions(shape, want["end"], n, what)
        if shape == "n24":   # sas_edit.hip: the radix sort's key bits
            assert ed_bits(n) + ed_bits(len(c.qs) - 1) > 32, what
        for u32 in (False, True):
            off, end, dist, qfl, tot = TE.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, mh, total, u32=u32)
            assert tot == total, what
            TE.same((off, end, dist, qfl), want, what + (u32,))
        if build == "quad_p8" and k == 3:
            TE.same(idx.locate_edit(c.qb, c.qoff, c.qlen, k, max_seed_hits=mh), want, what + ("host",))
        if al is None:
            continue
        sel = F.align_sel(exp)
        want_al = F.shift(al, by, n_ref, n)
        for u32 in (False, True):
            got = TA.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, want["off"], want["end"], u32=u32)
            for g, r, nm in zip(got, want_al, ("start", "dist", "nruns", "runs")):
                bad = np.flatnonzero((g[sel] != r).reshape(len(sel), -1).any(1))
                assert len(bad) == 0, (what, "align", u32, nm, sel[bad[:3]], g[sel[bad[:3]]], r[bad[:3]])
            assert np.array_equal(got[1], want["dist"]), (what, "align", u32, "every distance")
        if build == "quad_p8" and k == 3:
            host = idx.align_edit(c.qb, c.qoff, c.qlen, k, want["off"], want["end"])
            assert host[0].dtype == np.uint64
            for g, r, nm in zip(host, want_al, ("start", "dist", "nruns", "runs")):
                assert np.array_equal(g.astype(np.int64)[sel], r), (what, "align host", nm)


@pytest.mark.parametrize("shape,build", CASES)
def test_map_and_pairs_far(sas, indexes, shape, build):
    import torch
    by, n_ref, n = geometry(shape)
    mp = {k: F.reference("map", k) for k in F.MAP_KS}
    pr = {run: F.reference("pairs", *run) for run in F.PAIR_RUNS}   # the references stand before the GPU is asked
    idx = indexes(shape, build)
    for k, (c, ref) in mp.items():
        what = (shape, build, "map", k)
        want = F.shift(ref, by, n_ref, n)
        check_positions(shape, want["end"][want["dist"] != NONE_DIST], n, what)
        if shape == "n24":   # sas_map.hip: both strands' proposals in one sort, 2 nq batch queries
            assert ed_bits(n) + ed_bits(2 * len(c.qs) - 1) > 32, what
        for u32 in (False, True):
            TM.same(TM.dev_call(torch, idx, c, strands=3, u32=u32), want, what + (u32,))
        if build == "quad_p8" and k == 3:
            TM.same(TM.as_dict(idx.map_edit(c.qb, c.qoff, c.qlen, k)), want, what + ("host",))
    for (k, kr, anchors), (c, refs) in pr.items():
        if shape == "n24":
            assert ed_bits(n) + ed_bits(2 * len(c.qs) - 1) > 32
        for w in WINDOWS:
            what = (shape, build, "pairs", k, kr, anchors, w)
            want_p, want_r = (F.shift(r, by, n_ref, n) for r in refs[w])
            check_positions(shape, want_r["end"][want_r["dist"] != NONE_DIST], n, what)
            for u32 in (False, True):
                TP.same(TP.dev_call(torch, idx, c, w, u32=u32), want_p, what + ("map_pairs", u32))
                TR.same(TR.dev_call(torch, idx, c, w, anchors=anchors, u32=u32), want_r, what + ("rescue", u32))
            if build == "quad_p8" and w == WINDOWS[0] and k == 1:
                host = idx.map_pairs(c.qb, c.qoff, c.qlen, k, w[0], w[1])
                TP.same(TP.as_dict(host), want_p, what + ("map_pairs host",))
                host = idx.map_pairs_rescue(c.qb, c.qoff, c.qlen, k, kr, w[0], w[1], anchors)
                TR.same(TR.as_dict(host), want_r, what + ("rescue host",))


def check_slice(torch, idx, ht, s, boundary, u32):
    """T_small stands at ht[s ..) inside a large random text (the caller wrote it there before the
    build): locate_edit, align_edit, map_edit and map_pairs_rescue on the reads of
    test_far_host.slice_reads equal the brute force on ht[s - 1024 .. s + 4099 + 1024), moved by
    s - 1024.  The rest of the text is random ACGT, so that nothing matches elsewhere is checked,
    not proven: an end reported outside the slice is verified by a Sellers pass over ht around it.
    u32: the text is below 2^32 chars, the u32 forms are run too (read back modulo 2^32); else every
    one of the six calls must refuse SAS_LOCATE_U32."""
    import errno
    import sas_amd
    n, base = len(ht), s - F.M
    sc = F.SliceCase(ht[base:s + F.SMALL_N + F.M])   # the reference stands before the GPU is asked
    lo, hi, kk = base, base + sc.n, max(F.SLICE_KS)
    mask = (1 << 32) - 1

    def dev(c):
        return TM.cu(torch, c.qb, np.uint8), TM.cu(torch, c.qoff, np.int64), TM.cu(torch, c.qlen, np.int32)

    wants = {}
    for name, c, k, exp in (("reads", sc.c, kk, sc.edit[kk]), ("reverse complements", sc.rc, kk, sc.edit_rc),
                            ("reads, k = 1", sc.c, 1, sc.edit[1])):
        got = idx.locate_edit(*dev(c), k)
        torch.cuda.synchronize()
        off, end, dist, qfl = (np.asarray(g.cpu()).astype(np.int64) for g in got)
        for a in np.flatnonzero((end < lo) | (end > hi))[:1]:
            q = c.qs[int(np.searchsorted(off, a, side="right")) - 1]
            d = F.sellers_at(ht, q, end[a])
            true_match = d <= k and d == dist[a]
            assert False, ("input collision: a read matches outside the slice, choose other reads or another place"
                           if true_match else "kernel error: an end was reported where the read does not match",
                           name, int(end[a]), int(dist[a]), d)
        want = wants[name] = F.shift(exp, base, sc.n, n)
        assert (want["end"] < boundary).any() and (want["end"] >= boundary).any(), (name, boundary)
        TE.same((off, end, dist, qfl), want, ("slice", s, name, "mirror"))
    # with nothing matching elsewhere on either strand, the slice's references are the text's
    want = wants["reads"]
    total = int(want["off"][-1])
    al = F.shift(sc.align, base, sc.n, n)
    sel = F.align_sel(sc.edit[kk])
    ck = F.Reads(sc.c.qs, k=kk, mh=0)
    want_map = F.shift(sc.map, base, sc.n, n)
    want_rescue = F.shift(sc.rescue, base, sc.n, n)
    w = F.SLICE_WINDOW
    for both in (want_map, want_rescue):
        e = both["end"][both["dist"] != NONE_DIST]
        assert (e < boundary).any() and (e >= boundary).any() and (both["dist"] == NONE_DIST).any()
    for form in ((False, True) if u32 else (False,)):
        what = ("slice", s, "u32" if form else "u64")
        off, end, dist, qfl, tot = TE.dev_call(torch, idx, sc.c.qb, sc.c.qoff, sc.c.qlen, kk, 0, total, u32=form)
        assert tot == total, what
        TE.same((off, end.astype(np.int64) & mask if form else end, dist, qfl), want, what + ("locate_edit",))
        got = TA.dev_call(torch, idx, sc.c.qb, sc.c.qoff, sc.c.qlen, kk, want["off"], want["end"], u32=form)
        got = (got[0] & mask if form else got[0],) + got[1:]
        for g, r, nm in zip(got, al, ("start", "dist", "nruns", "runs")):
            assert np.array_equal(g[sel], r), what + ("align_edit", nm)
        got = TM.dev_call(torch, idx, ck, strands=3, u32=form)
        if form:
            got["end"], got["start"] = got["end"] & mask, got["start"] & mask
        TM.same(got, want_map, what + ("map_edit",))
        got = TR.dev_call(torch, idx, sc.c, w, anchors=sc.anchors, u32=form)
        if form:
            got["end"], got["start"] = got["end"] & mask, got["start"] & mask
        TR.same(got, want_rescue, what + ("map_pairs_rescue",))
    if not u32:
        c = sc.c
        refused = {
            "locate_mismatch": lambda: TMM.dev_call(torch, idx, c.qb, c.qoff, c.qlen, 1, 0, 16, u32=True),
            "locate_edit": lambda: TE.dev_call(torch, idx, c.qb, c.qoff, c.qlen, 1, 0, 16, u32=True),
            "align_edit": lambda: TA.dev_call(torch, idx, c.qb, c.qoff, c.qlen, kk, want["off"], want["end"] & mask,
                                              u32=True),
            "map_edit": lambda: TM.dev_call(torch, idx, ck, u32=True),
            "map_pairs": lambda: TP.dev_call(torch, idx, c, w, u32=True),
            "map_pairs_rescue": lambda: TR.dev_call(torch, idx, c, w, anchors=sc.anchors, u32=True),
        }
        for name, call in refused.items():
            with pytest.raises(sas_amd.SasError) as e:
                call()
            assert e.value.code == errno.EINVAL and "SAS_LOCATE_U32" in str(e.value), (name, str(e.value))
    return dict(reads=len(sc.c.qs), ends=len(want["end"]), below=int((want["end"] < boundary).sum()),
                above=int((want["end"] >= boundary).sum()))
