"""The sequence layout on the GPU (sas_set_layout and the approximate calls that honour it:
sas_locate_mismatch*, sas_locate_edit*, sas_align_edit*, sas_map_edit*, sas_map_pairs*,
sas_map_pairs_rescue*; sas_translate), bit for bit against the numpy reference of
tests/test_layout_host.py.

The text has 5,300 chars over 4 sequences: (1) two segments around a 1-char gap, (2) one segment,
adjacent to (1) with no gap, (3) an empty sequence, (4) segments of 40 and 700 chars around a
500-char gap, then a trailing gap.  Every run plants the query classes a .. f below and asserts
from the references alone that the concatenated-text answer of each class differs from the layout
answer, so no comparison passes vacuously; the planted pairs do the same for the join and the rescue."""
import errno
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_edit import TRUNCATED, EBrute, edited
from test_gpu_match import pack
from test_gpu_mismatch import MBrute
from test_layout_host import SEQ_NONE, Layout, LBrute
from test_map_host import revcomp_ref

pytestmark = pytest.mark.gpu

SEQ_START = [0, 2000, 4000, 4000, 5300]
SEG_LO = [0, 1001, 2000, 4000, 4540]
SEG_HI = [1000, 2000, 4000, 4040, 5240]
N = 5300
MS, KS = (20, 100, 200), (0, 1, 3)  # one, two and four Myers words
CAP = 50  # max_seed_hits that skips the poly-A seeds (the 500-char gap holds hundreds of each)
QUAD = dict(lcp=False, stree=False, sector=False, quad=True, llcp=False, prefix=8)


@functools.lru_cache(maxsize=None)
def world():
    t = O.random_string(N, seed=77).copy()
    lay = Layout(SEQ_START, SEG_LO, SEG_HI)
    gap = np.ones(N, bool)
    for lo, hi in zip(SEG_LO, SEG_HI):
        gap[lo:hi] = False
    t[gap] = 0  # what the reader stores for N
    t.setflags(write=False)
    return t, lay, LBrute(t, lay), MBrute(t)


def plant(rng, t, s, m, nedits):
    """a read of exactly m chars: the text from s on with nedits random edits"""
    kinds = ("sub", "ins", "del")
    for _ in range(100):
        ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(nedits)]
        ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
        q = edited(rng, t[s:s + ln], ops)
        if len(q) == m:
            return q
    raise AssertionError("no read of m chars")


@functools.lru_cache(maxsize=None)
def case(m, k):
    """The reads of one (m, k) run, all of m chars, by class, and both references' answers."""
    t, lay, lb, mb = world()
    rng = np.random.default_rng(1000 * m + k)
    cls = {}
    cls["a"] = [t[2000 - m + x:2000 + x] for x in (1, m // 2, m - 1)]             # across the seq 1 / 2 boundary
    cls["b"] = [t[1000 - x:1000 - x + m] for x in (1, m // 2, m - 1)]             # across the single-N gap
    cls["c"] = [np.zeros(m, np.uint8)]                                           # poly-A: the 500-char gap
    cls["d"] = [t[4040 - m:4040]] if m > 40 else []                              # longer than the 40-char segment
    cls["e"] = [t[lo - 1:lo - 1 + m] for lo in (2000, 4540)]                     # the start is clipped at lo
    cls["f"] = []
    for c in range(k + 1):                                                       # 0 .. k edits, both strands
        for s in (17, 1001, 2000 + 3 * m, 4000 + (0 if m <= 40 else 540), 5240 - m - 4):
            q = plant(rng, t, s, m, c)
            cls["f"].append(revcomp_ref(q) if (s + c) & 1 else q)
    qs, of = [], []
    for name in "abcdef":
        for q in cls[name]:
            assert len(q) == m
            qs.append(np.ascontiguousarray(q, np.uint8))
            of.append(name)
    of = np.array(of)
    out = dict(qs=qs, of=of, packed=pack(qs), fixed=np.concatenate(qs + [np.zeros(64, np.uint8)]))
    for mh in (0, CAP):
        ed = [lb.edit(q, k, mh) for q in qs]
        whole = [lb.whole.answer(q, k, mh)[:3] for q in qs]
        mm = [lb.mismatch(mb, q, k, mh) for q in qs]
        mm_whole = [mb.answer(q, k, mh)[:3] for q in qs]
        out[mh] = dict(ed=ed, mm=mm, ed_whole=whole, mm_whole=mm_whole)
    # the layout changes every class's answer (classes a .. e; f holds the ordinary reads, which
    # must be found: on the reverse strand through map_edit)
    for name in "abcde":
        sel = np.flatnonzero(of == name)
        if len(sel) == 0:
            continue
        assert any(out[0]["ed"][i][:2] != out[0]["ed_whole"][i][:2] for i in sel), (m, k, name)
        assert any(out[0]["mm"][i][:2] != out[0]["mm_whole"][i][:2] for i in sel), (m, k, name)
    ci = int(np.flatnonzero(of == "c")[0])
    assert out[CAP]["ed"][ci][2] & TRUNCATED and out[CAP]["mm"][ci][2] & TRUNCATED  # the cap truncates class c
    assert sum(len(out[0]["ed"][i][0]) for i in np.flatnonzero(of == "f")) > 0
    if k >= 1:  # e: found with the layout, at a worse distance than in the concatenated text
        for i in np.flatnonzero(of == "e"):
            assert out[0]["ed"][i][0] and min(out[0]["ed"][i][1]) == 1 and min(out[0]["ed_whole"][i][1]) == 0
    return out


def csr(ans):
    off = np.zeros(len(ans) + 1, np.int64)
    off[1:] = np.cumsum([len(a[0]) for a in ans])
    return (off, np.array([e for a in ans for e in a[0]], np.int64), np.array([d for a in ans for d in a[1]], np.int64),
            np.array([a[2] for a in ans], np.int64))


def same(got, exp, what):
    for g, e, name in zip(got, exp, ("off", "pos", "dist", "qflags")):
        assert np.array_equal(np.asarray(g).astype(np.int64), e), (what, name)


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def idx(sas):
    t, lay, _, _ = world()
    x = sas.SaNaive.build(t, **QUAD)
    x.set_layout(SEQ_START, SEG_LO, SEG_HI)
    got = x.layout()
    assert got[0].tolist() == SEQ_START and got[1].tolist() == SEG_LO and got[2].tolist() == SEG_HI
    return x


def run_locates(x, m, k, u32=False):
    """locate_mismatch, locate_edit and align_edit over the reported ends, ragged and fixed, with and
    without the seed cap, against the reference."""
    t, lay, lb, mb = world()
    c = case(m, k)
    qs, (qb, qoff, qlen) = c["qs"], c["packed"]
    for mh in (0, CAP):
        exp_mm, exp_ed = csr(c[mh]["mm"]), csr(c[mh]["ed"])
        same(x.locate_mismatch(qb, qoff, qlen, k, max_seed_hits=mh, u32=u32), exp_mm, ("mismatch", m, k, mh))
        same(x.locate_mismatch_fixed(c["fixed"][:len(qs) * m], m, k, max_seed_hits=mh, u32=u32), exp_mm,
             ("mismatch_fixed", m, k, mh))
        got = x.locate_edit(qb, qoff, qlen, k, max_seed_hits=mh, u32=u32)
        same(got, exp_ed, ("edit", m, k, mh))
        same(x.locate_edit_fixed(c["fixed"][:len(qs) * m], m, k, max_seed_hits=mh, u32=u32), exp_ed,
             ("edit_fixed", m, k, mh))
        if mh:
            continue
        # the alignments of the reported ends, and of ends in no segment (a gap, a segment's lo, 0)
        off, end = exp_ed[0], exp_ed[1]
        extra = np.array([0, 1000, 1001, 4040, 4041, 4300, 4540, 5241, N], np.int64)
        off2 = off.copy()
        off2[-1] += len(extra)  # they go to the last query
        end2 = np.concatenate([end, extra])
        qi = np.searchsorted(off2, np.arange(len(end2)), side="right") - 1
        exp_al = lb.align(qs, qi, end2, k, list(range(len(end2))))
        assert (exp_al[1][len(end):][[0, 1, 2, 4, 5, 6, 7]] == 255).all()  # no segment: no alignment
        ends_in = end2.astype(np.uint32 if u32 else np.uint64)
        for got_al in (x.align_edit(qb, qoff, qlen, k, off2.astype(np.uint64), ends_in, u32=u32),
                       x.align_edit_fixed(c["fixed"][:len(qs) * m], m, k, off2.astype(np.uint64), ends_in, u32=u32)):
            for g, e, name in zip(got_al, exp_al, ("start", "dist", "nruns", "runs")):
                assert np.array_equal(np.asarray(g).astype(np.int64), e), ("align", m, k, name)


def run_map(x, m, k, u32=False):
    t, lay, lb, mb = world()
    c = case(m, k)
    qs, (qb, qoff, qlen) = c["qs"], c["packed"]
    for mh, strands in ((0, 3), (CAP, 3), (0, 1), (0, 2)):
        exp = lb.map(qs, k, mh, strands)
        if mh == 0 and strands == 3:  # the layout changes the winners, and reads map on both strands
            whole_best = [min(a[1]) if a[1] else 255 for a in c[0]["ed_whole"]]
            assert (np.array(whole_best) != exp["dist"]).any() or k == 0
            assert {0, 1} <= set(exp["strand"][exp["dist"] != 255].tolist())
        for got in (x.map_edit(qb, qoff, qlen, k, max_seed_hits=mh, strands=strands, u32=u32),
                    x.map_edit_fixed(c["fixed"][:len(qs) * m], m, k, max_seed_hits=mh, strands=strands, u32=u32)):
            for name in exp:
                assert np.array_equal(np.asarray(getattr(got, name)).astype(np.int64), exp[name]), \
                    ("map", m, k, mh, strands, name)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
def test_locates_and_alignments(idx, m, k):
    run_locates(idx, m, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
def test_map_edit(idx, m, k):
    run_map(idx, m, k)


def test_u32_outputs(idx):
    run_locates(idx, 100, 1, u32=True)
    run_map(idx, 100, 1, u32=True)


def test_sa40(sas):
    t = world()[0]
    x = sas.SaNaive.build(t, **dict(QUAD, prefix=False, sa40=True))
    assert x.stats()["sa_width"] == 5
    x.set_layout(SEQ_START, SEG_LO, SEG_HI)
    run_locates(x, 100, 3)
    run_map(x, 20, 1)


def test_tile_grid_of_one(idx, monkeypatch):
    monkeypatch.setenv("SAS_TILE_GRID", "1")
    run_locates(idx, 100, 3)
    run_map(idx, 200, 1)


# ---------------------------------------------------------------- pairs and rescue
PM, PK, PKR, FRAG, ANCHORS = 30, 1, 3, (100, 900), 4


def mutate(rng, q, ne):
    q = q.copy()
    for p in rng.choice(len(q), ne, replace=False):
        q[p] ^= 1 + int(rng.integers(0, 3))
    return q


@functools.lru_cache(maxsize=None)
def pair_case():
    """Pairs of PM-char reads (mate 1 forward at s1, mate 2 the reverse complement of the PM chars that
    end at e2, each with some substitutions) and both references' records."""
    t, lay, lb, mb = world()
    rng = np.random.default_rng(4)
    plan = dict(
        cross=(1800, 2100, 0, 0),        # 300 apart in concatenated coordinates, but in sequences 1 and 2
        across_gap=(4005, 4630, 0, 0),   # the mates span the 500-char gap inside sequence 4
        plain=(2500, 2900, 1, 0),
        lost_at_edge=(4005, 4570, 0, 3),  # the lost mate starts at the segment's lo, 4540, behind the gap
        lost_rev_anchor=(4001, 4700, 3, 0),  # the forward mate is lost: the window runs back over the gap
        past_seq_end=(3900, 4590, 0, 0),  # the window of the forward anchor runs past the end of sequence 2
        lost_across=(1700, 2130, 0, 3),  # the lost mate lies in the next sequence
        lost_plain=(2600, 3000, 0, 2),
    )
    qs = []
    for s1, e2, n1, n2 in plan.values():
        qs += [mutate(rng, t[s1:s1 + PM], n1), mutate(rng, revcomp_ref(t[e2 - PM:e2]), n2)]
    names = list(plan)
    whole = lb.whole
    A_f, A_r = whole.answers(qs, PK, 0), whole.answers([revcomp_ref(q) for q in qs], PK, 0)
    from test_pairs_host import pairs_ref_all
    from test_rescue_host import rescue_ref_all
    cp = pairs_ref_all(t, qs, PK, A_f, A_r, *FRAG)
    cr = rescue_ref_all(t, qs, PK, PKR, A_f, A_r, *FRAG, ANCHORS)
    lp = lb.pairs(qs, PK, 0, *FRAG)
    lr = lb.rescue(qs, PK, PKR, 0, *FRAG, ANCHORS)
    ix = {n: i for i, n in enumerate(names)}
    # from the references alone: what the layout changes, and what it must keep
    assert cp["n_pairs"][ix["cross"]] == 1 and lp["n_pairs"][ix["cross"]] == 0
    assert cp["n_pairs"][ix["past_seq_end"]] == 1 and lp["n_pairs"][ix["past_seq_end"]] == 0
    assert lr["pflags"][ix["past_seq_end"]] == 0 and lr["pflags"][ix["cross"]] == 0
    assert lp["n_pairs"][ix["across_gap"]] == 1 and lp["n_pairs"][ix["plain"]] == 1
    for n in ("lost_at_edge", "lost_rev_anchor", "lost_plain"):
        assert lp["n_pairs"][ix[n]] == 0 and lr["pflags"][ix[n]] == 2 and lr["n_rescue"][ix[n]] >= 1, n
    assert cr["pflags"][ix["lost_across"]] == 2 and lr["pflags"][ix["lost_across"]] == 0
    edge = 2 * ix["lost_at_edge"] + 1  # placed beside the segment's lo, never before it
    assert abs(int(lr["end"][edge]) - 4570) <= PKR and 4540 <= lr["start"][edge] <= 4540 + PKR
    return qs, lp, lr, cp, cr


LONG_FRAG = (100, 1300)
LONG = {100: (1, 3), 200: (3, 5)}  # m: (k, k_rescue): two and four Myers words in the rescue scan


@functools.lru_cache(maxsize=None)
def long_pair_case(m):
    """pair_case for reads of m = 100 and 200 chars, longer than the 40-char segment: a lost mate has
    k_rescue substitutions, more than k."""
    t, lay, lb, mb = world()
    k, kr = LONG[m]
    rng = np.random.default_rng(40 + m)
    plan = dict(
        plain=(2300, 2900, 0, 0),
        cross=(1750, 2250 + m - 100, 0, 0),        # mate 1 ends before 2000, mate 2 starts behind it
        lost_fwd_at_lo=(4540, 5200, kr, 0),        # the lost forward mate starts at the segment's lo behind the
                                                   # 500-char gap: the reverse anchor's window runs back over it
        lost_rev_behind_gap=(500, 1001 + m, 0, kr),  # the lost mate starts at lo = 1001, behind the single-N gap
        lost_at_seq_end=(1300, 2000, 0, kr),       # the window runs over the 1 / 2 boundary; the mate ends on it
        lost_across=(1500, 2050 + m, 0, kr),       # the lost mate lies behind the boundary, in sequence 2
        past_seq_end=(3700, 4540 + m, 0, 0),       # the forward anchor's window runs past the end of sequence 2
    )
    qs = []
    for s1, e2, n1, n2 in plan.values():
        assert lay.inside(s1, s1 + m) and lay.inside(e2 - m, e2), (s1, e2)
        qs += [mutate(rng, t[s1:s1 + m], n1), mutate(rng, revcomp_ref(t[e2 - m:e2]), n2)]
    whole = lb.whole
    A_f, A_r = whole.answers(qs, k, 0), whole.answers([revcomp_ref(q) for q in qs], k, 0)
    from test_pairs_host import pairs_ref_all
    from test_rescue_host import rescue_ref_all
    cp = pairs_ref_all(t, qs, k, A_f, A_r, *LONG_FRAG)
    cr = rescue_ref_all(t, qs, k, kr, A_f, A_r, *LONG_FRAG, ANCHORS)
    lp = lb.pairs(qs, k, 0, *LONG_FRAG)
    lr = lb.rescue(qs, k, kr, 0, *LONG_FRAG, ANCHORS)
    ix = {n: i for i, n in enumerate(plan)}
    assert lp["n_pairs"][ix["plain"]] == 1
    for n in ("cross", "past_seq_end"):  # proper in the concatenated text only, and no rescue across either
        assert cp["n_pairs"][ix[n]] == 1 and lp["n_pairs"][ix[n]] == 0 and lr["pflags"][ix[n]] == 0, n
    for n in ("lost_fwd_at_lo", "lost_rev_behind_gap", "lost_at_seq_end"):
        assert lp["n_pairs"][ix[n]] == 0 and lr["pflags"][ix[n]] == 2 and lr["n_rescue"][ix[n]] >= 1, n
    assert cr["pflags"][ix["lost_across"]] == 2 and lr["pflags"][ix["lost_across"]] == 0
    f = 2 * ix["lost_fwd_at_lo"]  # placed at the segment's lo, never before it
    assert lr["strand"][f] == 0 and 4540 <= lr["start"][f] <= 4540 + kr and lr["qflags"][f] & 8
    v = 2 * ix["lost_rev_behind_gap"] + 1
    assert lr["strand"][v] == 1 and 1001 <= lr["start"][v] <= 1001 + kr
    v = 2 * ix["lost_at_seq_end"] + 1
    assert abs(int(lr["end"][v]) - 2000) <= kr and lr["end"][v] <= 2000
    return qs, lp, lr


@pytest.mark.parametrize("m", sorted(LONG))
def test_map_pairs_and_rescue_long_reads(idx, m):
    from test_pairs_host import FIELDS as PF
    from test_rescue_host import FIELDS as RF
    k, kr = LONG[m]
    qs, lp, lr = long_pair_case(m)
    qb, qoff, qlen = pack(qs)
    fixed = qb[:len(qs) * m]
    same_records(idx.map_pairs(qb, qoff, qlen, k, *LONG_FRAG), lp, PF, ("pairs", m))
    same_records(idx.map_pairs_fixed(fixed, m, k, *LONG_FRAG), lp, PF, ("pairs_fixed", m))
    same_records(idx.map_pairs_rescue(qb, qoff, qlen, k, kr, *LONG_FRAG, ANCHORS), lr, RF, ("rescue", m))
    same_records(idx.map_pairs_rescue_fixed(fixed, m, k, kr, *LONG_FRAG, ANCHORS), lr, RF, ("rescue_fixed", m))


def same_records(got, exp, fields, what):
    for name in fields:
        assert np.array_equal(np.asarray(getattr(got, name)).astype(np.int64), exp[name]), (what, name)


@pytest.mark.parametrize("u32", (False, True))
def test_map_pairs_and_rescue(idx, u32):
    from test_pairs_host import FIELDS as PF
    from test_rescue_host import FIELDS as RF
    qs, lp, lr, _, _ = pair_case()
    qb, qoff, qlen = pack(qs)
    fixed = qb[:len(qs) * PM]
    same_records(idx.map_pairs(qb, qoff, qlen, PK, *FRAG, u32=u32), lp, PF, "pairs")
    same_records(idx.map_pairs_fixed(fixed, PM, PK, *FRAG, u32=u32), lp, PF, "pairs_fixed")
    same_records(idx.map_pairs_rescue(qb, qoff, qlen, PK, PKR, *FRAG, ANCHORS, u32=u32), lr, RF, "rescue")
    same_records(idx.map_pairs_rescue_fixed(fixed, PM, PK, PKR, *FRAG, ANCHORS, u32=u32), lr, RF, "rescue_fixed")


def test_pairs_tile_grid_of_one_and_sa40(sas, idx, monkeypatch):
    from test_rescue_host import FIELDS as RF
    qs, lp, lr, _, _ = pair_case()
    qb, qoff, qlen = pack(qs)
    x = sas.SaNaive.build(world()[0], **dict(QUAD, prefix=False, sa40=True))
    x.set_layout(SEQ_START, SEG_LO, SEG_HI)
    same_records(x.map_pairs_rescue(qb, qoff, qlen, PK, PKR, *FRAG, ANCHORS), lr, RF, "rescue sa40")
    monkeypatch.setenv("SAS_TILE_GRID", "1")
    same_records(idx.map_pairs_rescue(qb, qoff, qlen, PK, PKR, *FRAG, ANCHORS), lr, RF, "rescue grid 1")


# ---------------------------------------------------------------- translate
def translate_ref(lb, pos, span):
    r = [lb.translate(int(p), 1 if span is None else int(s)) for p, s in zip(pos, span if span is not None else pos)]
    return np.array([a for a, _ in r], np.int64), np.array([b for _, b in r], np.int64)


def test_translate_every_position_and_edge(idx):
    import torch
    t, lay, lb, mb = world()
    pos = np.arange(N + 3, dtype=np.uint64)  # past the text too
    es, eo = translate_ref(lb, pos, None)
    assert set(es.tolist()) == {0, 1, 3, SEQ_NONE}  # the empty sequence 2 owns no position
    seq, off = idx.translate(pos)
    assert np.array_equal(seq.astype(np.int64), es) and np.array_equal(off.astype(np.int64), eo)
    # spans across each kind of edge: the 1-char gap, the sequence boundary without a gap, the empty
    # sequence, the 500-char gap, the trailing gap, the text end; span 0 counts as 1
    p2 = np.array([990, 995, 999, 999, 1001, 1990, 1999, 1999, 2000, 3990, 3999, 4000, 4030, 4039, 4040, 4539, 4540,
                   5230, 5239, 5240, 5299, 0, 0], np.uint64)
    s2 = np.array([10, 10, 1, 2, 999, 10, 1, 2, 2000, 10, 2, 40, 11, 0, 1, 2, 700, 10, 2, 1, 1, 1000, 1001], np.uint32)
    es2, eo2 = translate_ref(lb, p2, s2)
    assert (es2 == SEQ_NONE).sum() >= 8 and (es2 != SEQ_NONE).sum() >= 8
    seq, off = idx.translate(p2, s2)
    assert np.array_equal(seq.astype(np.int64), es2) and np.array_equal(off.astype(np.int64), eo2)
    # u32, and device pointers (asynchronous) in both widths
    seq, off = idx.translate(p2.astype(np.uint32), s2, u32=True)
    assert off.dtype == np.uint32 and np.array_equal(seq.astype(np.int64), es2) and np.array_equal(off.astype(np.int64), eo2)
    for u32 in (False, True):
        dp = torch.from_numpy(p2.astype(np.int32 if u32 else np.int64)).cuda()
        ds = torch.from_numpy(s2.astype(np.int32)).cuda()
        seq, off = idx.translate(dp, ds, u32=u32)
        torch.cuda.synchronize()
        assert np.array_equal(seq.cpu().numpy().astype(np.uint32).astype(np.int64), es2)
        assert np.array_equal(off.cpu().numpy().astype(np.int64), eo2)


def test_translate_bisects_global_memory(sas):
    """5,000 one-char segments do not fit the LDS stage."""
    t = world()[0]
    x = sas.SaNaive.build(t, **QUAD)
    starts = [0, 1000, 1000, N]  # one-char segments never cross a start
    seg_lo = np.array([p for p in range(N) if p % 18 != 5][:5000], np.int64)  # mostly adjacent, a hole every 18
    seg_hi = seg_lo + 1
    assert len(seg_lo) == 5000 and len(starts) + 2 * len(seg_lo) > 6144  # the kernel's LDS stage, in u64 words
    x.set_layout(starts, seg_lo, seg_hi)
    lb = Layout(starts, seg_lo, seg_hi)
    pos = np.arange(N + 1, dtype=np.uint64)
    span = (1 + (pos % 3 == 0)).astype(np.uint32)
    es, eo = translate_ref(lb, pos, span)
    assert (es == SEQ_NONE).sum() > 100 and (es == 0).sum() > 100 and (es == 2).sum() > 100
    for u32 in (False, True):
        seq, off = x.translate(pos.astype(np.uint32) if u32 else pos, span, u32=u32)
        assert np.array_equal(seq.astype(np.int64), es) and np.array_equal(off.astype(np.int64), eo)


def test_translate_needs_a_layout(sas):
    x = sas.SaNaive.build(world()[0][:500], **QUAD)
    with pytest.raises(sas.SasError) as ei:
        x.translate(np.zeros(1, np.uint64))
    assert ei.value.code == errno.EINVAL and "no layout" in str(ei.value)


# ---------------------------------------------------------------- identity, clearing, exact calls, pairs
def all_calls(x, m, k):
    c = case(m, k)
    qs, (qb, qoff, qlen) = c["qs"], c["packed"]
    out = []
    out += list(x.locate_mismatch(qb, qoff, qlen, k))
    ed = x.locate_edit(qb, qoff, qlen, k)
    out += list(ed)
    out += list(x.align_edit(qb, qoff, qlen, k, ed[0], ed[1]))
    out += list(x.map_edit(qb, qoff, qlen, k))
    out += list(x.locate(qb, qoff, qlen))  # an exact call: it ignores the layout
    return [np.asarray(a).tobytes() for a in out if a is not None]


def test_identity_layout_and_clearing(sas):
    t = world()[0]
    x = sas.SaNaive.build(t, **QUAD)
    assert x.layout() is None
    m, k = 100, 1
    before = all_calls(x, m, k)
    c = case(m, k)
    assert csr(c[0]["ed_whole"])[1].tolist() == np.frombuffer(before[5], np.uint64).tolist()  # the no-layout ends
    qb, qoff, qlen = c["packed"]
    pairs = (len(c["qs"]) // 2) * 2
    pr0 = x.map_pairs(qb, qoff[:pairs], qlen[:pairs], k, 0, 500)
    rs0 = x.map_pairs_rescue(qb, qoff[:pairs], qlen[:pairs], k, 3, 0, 500, max_anchors=4)
    x.set_layout([0, N], [0], [N])
    assert all_calls(x, m, k) == before
    pr_id = x.map_pairs(qb, qoff[:pairs], qlen[:pairs], k, 0, 500)
    rs_id = x.map_pairs_rescue(qb, qoff[:pairs], qlen[:pairs], k, 3, 0, 500, max_anchors=4)
    pq = pair_case()[0]
    pqb, pqoff, pqlen = pack(pq)
    pr_id2 = x.map_pairs_fixed(pqb[:len(pq) * PM], PM, PK, *FRAG)
    rs_id2 = x.map_pairs_rescue(pqb, pqoff, pqlen, PK, PKR, *FRAG, ANCHORS)
    x.set_layout(SEQ_START, SEG_LO, SEG_HI)
    with_layout = all_calls(x, m, k)
    assert with_layout[:-2] != before[:-2] and with_layout[-2:] == before[-2:]  # the exact locate is untouched
    x.set_layout(None)
    assert x.layout() is None and all_calls(x, m, k) == before
    pr1 = x.map_pairs(qb, qoff[:pairs], qlen[:pairs], k, 0, 500)
    rs1 = x.map_pairs_rescue(qb, qoff[:pairs], qlen[:pairs], k, 3, 0, 500, max_anchors=4)
    for a, b, c in zip(list(pr0) + list(rs0), list(pr1) + list(rs1), list(pr_id) + list(rs_id)):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a), np.asarray(c))
    # the planted pairs: the identity layout gives the concatenated text's records, rescue included
    from test_pairs_host import FIELDS as PF
    from test_rescue_host import FIELDS as RF
    same_records(pr_id2, pair_case()[3], PF, "identity pairs")
    same_records(rs_id2, pair_case()[4], RF, "identity rescue")
    assert (pair_case()[4]["pflags"] & 2).sum() >= 4 and (pair_case()[3]["n_pairs"] > 0).sum() >= 4
    with pytest.raises(sas.SasError) as ei:
        x.set_layout([0, N - 1], [0], [N - 1])
    assert ei.value.code == errno.EINVAL and x.layout() is None
