"""An exact reference for approximate matching at any text position: the shifted text (CPU only).

T_small is the 4099-char `random` text of tests/test_gpu_edit.py, F a random filler over the codes
{0, 1} (A, C) of length delta, M = 1024.  T_big = F ++ T_small and T_ref = F[delta - M:] ++ T_small
(5123 chars: the brute forces hold).  For a read with more than K chars in {G, T} and more than K
chars in {A, C}, K the largest of k and k_rescue:

* neither the read nor its reverse complement is within K edits or mismatches of a string over
  {A, C} (each of those chars costs one edit), so nothing is found inside the filler;
* a decision D(e) <= K depends only on the m + K text chars before e, and M >= 256 + 15.

Hence every answer of every call on T_big is the answer on T_ref with ends and starts moved by
delta - M and n for n, everything else bit for bit (with a cap on the seed hits: for reads without
a seed piece over {A, C} alone or {G, T} alone, whose hit counts differ between the texts).  This
file holds the builders, the read filter, shift() and the references on T_ref (computed once and
shared with tests/test_gpu_far.py), and tests the lemma itself: the brute forces and numpy
references of the suite run on T_big at delta = 9000 and must equal the shifted reference."""
import functools

import numpy as np

from test_align_host import NONE_DIST, align_ref_sel
from test_gpu_edit import EBrute, expected, make_queries, make_text
from test_gpu_match import pack
from test_gpu_mismatch import MBrute, make_queries as mm_make_queries
from test_gpu_rescue import RUNS as RESCUE_RUNS, WINDOWS, make_pairs
from test_map_host import map_ref_all, revcomp_ref
from test_pairs_host import pairs_ref_all
from test_rescue_host import PROPER, RESCUED, SKIPPED, Rows, rescue_ref_all

M = 1024
SMALL_N = 4099
HOST_DELTA = 9000
# (k, max_seed_hits) of the locate_edit runs (align_edit: the uncapped ones), k of the others
EDIT_RUNS = ((1, 0), (3, 0), (15, 0), (2, 20))
MISMATCH_KS = (1, 3)
MAP_KS = (1, 3)
# (k, k_rescue, max_anchors): the filter drops the short reads that have many loci (with k_rescue = 15
# every kept read has 32 chars or more), so a pair is over the bound on the anchors only where the
# bound is small
PAIR_RUNS = ((1, 3, 2), (0, 15, 1))
EDIT_FIELDS = ("off", "end", "dist", "qflags")


def small_text():
    t = make_text("random")
    assert len(t) == SMALL_N
    return t


def filler(delta):
    """delta chars over {A, C}; the last M are the same for every delta, so T_ref is one text."""
    assert delta >= M
    head = np.random.default_rng(delta).integers(0, 2, delta - M, dtype=np.uint8)
    return np.concatenate([head, np.random.default_rng(99).integers(0, 2, M, dtype=np.uint8)])


def big_text(delta):
    return np.concatenate([filler(delta), small_text()])


def ref_text():
    return big_text(M)


def pieces(q, k):
    b = [j * len(q) // (k + 1) for j in range(k + 2)]
    return [q[b[j]:b[j + 1]] for j in range(k + 1)]


def far_read(q, K, capped_k=None):
    """The lemma's condition on one read; capped_k: the k of a run with a cap on the seed hits."""
    q = np.asarray(q, np.uint8)
    gt = int((q >= 2).sum())
    if not (gt > K and len(q) - gt > K):
        return False
    if capped_k is not None:
        for r in (q, revcomp_ref(q)):
            for p in pieces(r, capped_k):
                if len(p) == 0 or (p >= 2).all() or (p < 2).all():
                    return False
    return True


def far_reads(qs, K, capped_k=None, pairs=False):
    """The reads that the lemma covers, in order; pairs: whole pairs only."""
    ok = [far_read(q, K, capped_k) for q in qs]
    if pairs:
        ok = [ok[i - i % 2] and ok[i - i % 2 + 1] for i in range(len(qs))]
    return [q for q, o in zip(qs, ok) if o]


def shift(ref, by, n_ref, n_big):
    """A call's reference on T_ref as it must come out on T_big.  The locate calls' dicts (`pos` or
    `end` per occurrence), align_ref_sel's tuple (start first), and the mapping calls' records
    (`end` and `start` per read, n for an unmapped one)."""
    if isinstance(ref, tuple):
        return (ref[0] + by,) + tuple(ref[1:])
    out = dict(ref)
    if "strand" in ref:
        mapped = ref["dist"] != NONE_DIST
        assert (ref["end"][~mapped] == n_ref).all() and (ref["start"][~mapped] == n_ref).all()
        assert (ref["end"][mapped] <= n_ref).all() and (ref["start"] <= ref["end"]).all()
        out["end"] = np.where(mapped, ref["end"] + by, n_big)
        out["start"] = np.where(mapped, ref["start"] + by, n_big)
    else:
        f = "pos" if "pos" in ref else "end"
        out[f] = ref[f] + by
    return out


def frozen(x):
    for v in (x.values() if isinstance(x, dict) else x):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


class Reads:
    """A run's reads as the calls take them."""

    def __init__(self, qs, **kw):
        self.qs = qs
        self.qb, self.qoff, self.qlen = pack(qs)
        self.__dict__.update(kw)


def edit_reads(k, mh):
    qs, _ = make_queries(small_text(), k, 2000 + k)
    return Reads(far_reads(qs, k, k if mh else None), k=k, mh=mh)


def mismatch_reads(k):
    qs = [q for seed in (1000 + k, 1100 + k) for q in mm_make_queries(small_text(), k, seed)]   # 200 answered reads
    return Reads(far_reads(qs, k), k=k, mh=0)


def map_reads(k):
    qs, _ = make_queries(small_text(), k, 2000 + k)
    return Reads(far_reads([revcomp_ref(q) if i % 2 else q for i, q in enumerate(qs)], k), k=k, mh=0)


def pair_reads(k, kr):
    qs = make_pairs(small_text(), "random", k, kr, 0, 7000 + RESCUE_RUNS.index(("random", k, kr, 0)))
    return Reads(far_reads(qs, max(k, kr), pairs=True), k=k, kr=kr, mh=0)


def edit_ref(t, c):
    return frozen(expected(EBrute(t), c.qs, c.k, c.mh))


def align_sel(exp):
    """The compared alignments: each read's first and last, and a fixed random 2000 of the rest."""
    na = len(exp["end"])
    cnt = np.diff(exp["off"])
    edge = np.concatenate([exp["off"][:-1][cnt > 0], exp["off"][1:][cnt > 0] - 1])
    rnd = np.random.default_rng(77).choice(na, min(na, 2000), replace=False)
    return np.unique(np.concatenate([edge, rnd]))


def align_ref(t, c, exp):
    qi = np.searchsorted(exp["off"], np.arange(len(exp["end"])), side="right") - 1
    return frozen(align_ref_sel(t, c.qs, qi, exp["end"], c.k, align_sel(exp)))


def mismatch_ref(t, c):
    br = MBrute(t)
    ans = [br.answer(q, c.k, 0) for q in c.qs]
    off = np.zeros(len(c.qs) + 1, np.int64)
    off[1:] = np.cumsum([len(a[0]) for a in ans])
    return frozen(dict(off=off, pos=np.array([p for a in ans for p in a[0]], np.int64),
                       dist=np.array([d for a in ans for d in a[1]], np.int64),
                       qflags=np.array([a[2] for a in ans], np.int64)))


def strand_answers(t, c, k):
    br = EBrute(t)
    return br, (br.answers(c.qs, k, c.mh), br.answers([revcomp_ref(q) for q in c.qs], k, c.mh))


def map_ref(t, c):
    _, A = strand_answers(t, c, c.k)
    return frozen(map_ref_all(t, c.qs, c.k, A[0], A[1], 3))


def pair_refs(t, c, anchors, windows=WINDOWS):
    """Per window (sas_map_pairs' records at k, sas_map_pairs_rescue's at (k, k_rescue))."""
    br, A = strand_answers(t, c, c.k)
    rows = Rows(br)
    single_k = map_ref_all(t, c.qs, c.k, A[0], A[1], 3)
    single_kr = map_ref_all(t, c.qs, c.kr, A[0], A[1], 3)
    return {w: (frozen(pairs_ref_all(t, c.qs, c.k, A[0], A[1], w[0], w[1], base=single_k)),
                frozen(rescue_ref_all(t, c.qs, c.k, c.kr, A[0], A[1], w[0], w[1], anchors, rows=rows, base=single_kr)))
            for w in windows}


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """(reads, reference on T_ref) of a run, computed once: ("edit", k, mh) -> (reads, locate_edit's,
    align_edit's or None), ("mismatch", k), ("map", k), ("pairs", k, k_rescue, max_anchors) ->
    (reads, {window: (map_pairs', map_pairs_rescue's)})."""
    t = ref_text()
    if kind == "edit":
        c = edit_reads(*key)
        exp = edit_ref(t, c)
        return c, exp, (align_ref(t, c, exp) if key[1] == 0 else None)
    if kind == "mismatch":
        c = mismatch_reads(*key)
        return c, mismatch_ref(t, c)
    if kind == "map":
        c = map_reads(*key)
        return c, map_ref(t, c)
    assert kind == "pairs"
    c = pair_reads(key[0], key[1])
    return c, pair_refs(t, c, key[2])


SLICE_MIN_M = 48
SLICE_KS = (1, 3)
SLICE_PAIR = (1, 3, 1)   # k, k_rescue, max_anchors
SLICE_WINDOW = WINDOWS[0]


def slice_reads():
    """The reads for a copy of T_small inside a random ACGT text: every second of the filtered pairs
    and single reads of 48 chars and more (the singles two by two as pairs) and some random reads."""
    pairs = pair_reads(SLICE_PAIR[0], SLICE_PAIR[1]).qs
    keep = [i % 4 < 2 and min(len(pairs[i - i % 2]), len(pairs[i - i % 2 + 1])) >= SLICE_MIN_M for i in range(len(pairs))]
    qs = [q for q, o in zip(pairs, keep) if o]
    singles = [q for q in edit_reads(3, 0).qs if len(q) >= SLICE_MIN_M][::2]
    qs += singles[:len(singles) - len(singles) % 2]
    rng = np.random.default_rng(48)
    qs += [rng.integers(0, 4, int(rng.integers(SLICE_MIN_M, 130)), dtype=np.uint8) for _ in range(40)]
    return qs


def answers_multi(br, qs, ks):
    """EBrute.answers(qs, k, 0) for every k of ks from one computation of the Sellers rows (which
    do not depend on k)."""
    out = {k: [None] * len(qs) for k in ks}
    by_len = {}
    for i, q in enumerate(qs):
        by_len.setdefault(len(q), []).append(i)
    for m, sel in by_len.items():
        for g in range(0, len(sel), 64):
            grp = sel[g:g + 64]
            D = br.rows([qs[i] for i in grp]) if 0 < m <= 256 else None
            for r, i in enumerate(grp):
                for k in ks:
                    out[k][i] = br.answer(qs[i], k, 0, None if D is None else D[r])
    return out


def as_expected(ans):
    """test_gpu_edit.expected's compared fields from the answers."""
    off = np.zeros(len(ans) + 1, np.int64)
    off[1:] = np.cumsum([len(a[0]) for a in ans])
    return frozen(dict(off=off, end=np.array([e for a in ans for e in a[0]], np.int64),
                       dist=np.array([d for a in ans for d in a[1]], np.int64),
                       qflags=np.array([a[2] for a in ans], np.int64)))


def rows_of(ref, reads, nq):
    """The records of a selection of reads (whole pairs) out of a mapping call's dict."""
    return {f: v[reads] if len(v) == nq else v[reads[0::2] // 2] for f, v in ref.items()}


def take(exp, reads):
    """The answers of a selection of reads out of a locate call's dict."""
    cnt = np.diff(exp["off"])[reads]
    sel = np.concatenate([np.arange(exp["off"][i], exp["off"][i + 1]) for i in reads] + [np.zeros(0, np.int64)])
    return dict(off=np.concatenate([[0], np.cumsum(cnt)]), end=exp["end"][sel], dist=exp["dist"][sel],
                qflags=exp["qflags"][reads])


class SliceCase:
    """The references of slice_reads() on `sl`, a slice of a large text that holds T_small M chars
    behind its start and M chars before its end.  They are the large text's answers moved by the
    slice's offset as long as nothing matches elsewhere (which the caller checks from the ends it
    gets) and nothing matches in the slice's margins, where an alignment could reach past the slice
    (asserted here: a failure is a collision of the inputs, not an error of the code under test)."""

    def __init__(self, sl):
        assert len(sl) == SMALL_N + 2 * M and np.array_equal(sl[M:M + SMALL_N], small_text())
        k, kr, self.anchors = SLICE_PAIR
        kk = max(SLICE_KS)
        assert k in SLICE_KS
        self.n = len(sl)
        self.c = Reads(slice_reads(), k=k, kr=kr, mh=0)
        self.rc = Reads([revcomp_ref(q) for q in self.c.qs], k=kk, mh=0)
        br = EBrute(sl)
        fwd, rev = answers_multi(br, self.c.qs, SLICE_KS), answers_multi(br, self.rc.qs, SLICE_KS)
        self.edit = {q: as_expected(fwd[q]) for q in SLICE_KS}
        self.edit_rc = as_expected(rev[kk])
        for exp in list(self.edit.values()) + [self.edit_rc]:
            assert len(exp["end"]) and exp["end"].min() >= M // 2 and exp["end"].max() <= self.n - M // 2, \
                "input collision: a read matches in the slice's margin"
        self.align = align_ref(sl, Reads(self.c.qs, k=kk, mh=0), self.edit[kk])
        self.map = frozen(map_ref_all(sl, self.c.qs, kk, fwd[kk], rev[kk], 3))
        w = SLICE_WINDOW
        self.rescue = frozen(rescue_ref_all(sl, self.c.qs, k, kr, fwd[k], rev[k], w[0], w[1], self.anchors, rows=Rows(br)))


def sellers_at(text, q, e):
    """D(e) of q on `text` by a Sellers pass over the m + 15 chars before e (any D <= 15 is exact)."""
    lo = max(0, int(e) - len(q) - 15)
    return int(EBrute(np.asarray(text[lo:int(e)], np.uint8)).rows([np.asarray(q, np.uint8)])[0][-1])


def test_slice_case_inside_a_random_text():
    """SliceCase on a slice of a 7000-char random ACGT text equals the suite's references on the
    whole text, moved by the slice's offset."""
    rng = np.random.default_rng(31)
    s = 1500
    t = rng.integers(0, 4, 7000, dtype=np.uint8)
    t[s:s + SMALL_N] = small_text()
    base = s - M
    sc = SliceCase(t[base:s + SMALL_N + M])
    br = EBrute(t)
    fwd, rev = answers_multi(br, sc.c.qs, SLICE_KS), answers_multi(br, sc.rc.qs, SLICE_KS)
    for kk in SLICE_KS:
        got = as_expected(fwd[kk])
        want = shift(sc.edit[kk], base, sc.n, len(t))
        same_dict({f: got[f] for f in EDIT_FIELDS}, {f: want[f] for f in EDIT_FIELDS}, ("slice edit", kk))
        for e, q in ((got["end"][0], sc.c.qs[int(np.flatnonzero(np.diff(got["off"]))[0])]),):
            assert sellers_at(t, q, e) == got["dist"][0]
    kk = max(SLICE_KS)
    same_dict(map_ref_all(t, sc.c.qs, kk, fwd[kk], rev[kk], 3), shift(sc.map, base, sc.n, len(t)), "slice map")
    k, kr, anchors = SLICE_PAIR
    w = SLICE_WINDOW
    same_dict(rescue_ref_all(t, sc.c.qs, k, kr, fwd[k], rev[k], w[0], w[1], anchors, rows=Rows(br)),
              shift(sc.rescue, base, sc.n, len(t)), "slice rescue")
    ref = sc.rescue
    assert (ref["pflags"] & PROPER).any() and (ref["pflags"] & RESCUED).any() and (ref["pflags"] & SKIPPED).any()
    assert (ref["dist"] == NONE_DIST).any() and (sc.edit[1]["end"] < M + 2048).any() and (sc.edit[1]["end"] >= M + 2048).any()


def same_dict(got, want, what):
    assert set(got) == set(want), what
    for f in want:
        if isinstance(want[f], np.ndarray):
            assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), (what, f)
        else:
            assert got[f] == want[f], (what, f)


def test_reads_hold_every_shape_that_matters():
    """From the references on T_ref alone: what each filtered run still contains."""
    n = M + SMALL_N
    for k, mh in EDIT_RUNS:
        c, exp, _ = reference("edit", k, mh)
        cnt = np.diff(exp["off"])
        assert (cnt > 0).sum() >= 200 and (cnt == 0).any() and (exp["end"] == n).any(), (k, mh, (cnt > 0).sum())
        assert exp["end"].min() > M    # nothing ends inside the filler
        if mh:
            assert (exp["qflags"] & 1).any() and (exp["qflags"] == 0).any()
    for k in MISMATCH_KS:
        c, exp = reference("mismatch", k)
        cnt = np.diff(exp["off"])
        ends = exp["pos"] + np.repeat(c.qlen.astype(np.int64), cnt)
        assert (cnt > 0).sum() >= 200 and (cnt == 0).any() and (ends == n).any(), (k, (cnt > 0).sum())
    for k in MAP_KS:
        c, ref = reference("map", k)
        mapped = ref["dist"] != NONE_DIST
        assert mapped.sum() >= 200 and (~mapped).any() and (ref["end"][mapped] == n).any(), (k, mapped.sum())
        assert (ref["strand"][mapped] == 0).any() and (ref["strand"][mapped] == 1).any()
    for k, kr, anchors in PAIR_RUNS:
        c, refs = reference("pairs", k, kr, anchors)
        for w, (pr, rr) in refs.items():
            for ref in (pr, rr):
                mapped = ref["dist"] != NONE_DIST
                assert mapped.sum() >= 200 and (~mapped).any(), (k, kr, w, mapped.sum())
            assert (rr["pflags"] & SKIPPED).any(), (k, kr, w)
            assert np.array_equal(pr["pflags"] & PROPER, rr["pflags"] & PROPER)
        assert any((rr["end"][rr["dist"] != NONE_DIST] == n).any() for _, rr in refs.values()), (k, kr)
        for w in (WINDOWS[0], WINDOWS[2]):   # the narrow window (150, 151) holds no proper pair
            assert (refs[w][1]["pflags"] & PROPER).any() and (refs[w][1]["pflags"] & RESCUED).any(), (k, kr, w)
        assert any(((rr["dist"] > k) & (rr["dist"] != NONE_DIST)).any() for _, rr in refs.values())  # beyond k


def test_the_lemma_at_9000():
    """The brute forces and references themselves on T_big, delta = 9000 (13099 chars: the int16
    rows hold): every record equals the shifted reference of T_ref.  The lemma holds read by read
    (pair by pair), so the costly runs are checked on every second or third of their reads."""
    big = big_text(HOST_DELTA)
    by, n_ref, n_big = HOST_DELTA - M, M + SMALL_N, HOST_DELTA + SMALL_N
    assert np.array_equal(big[by:], ref_text()) and len(big) == n_big and (big[:HOST_DELTA] < 2).all()
    br = EBrute(big)
    for k, mh in EDIT_RUNS:
        c, exp, al = reference("edit", k, mh)
        # (the candidate counts differ: a seed piece occurs in the filler too; k = 15: every third read)
        reads = np.arange(0, len(c.qs), 3 if k == 15 else 1)
        got = as_expected(br.answers([c.qs[i] for i in reads], k, mh))
        want = shift(take(exp, reads), by, n_ref, n_big)
        same_dict(got, want, ("edit", k, mh))
        if al is not None and k != 15:
            got_al = align_ref(big, c, got)
            for g, w_, nm in zip(got_al, shift(al, by, n_ref, n_big), ("start", "dist", "nruns", "runs")):
                assert np.array_equal(g, w_), ("align", k, nm)
    for k in MISMATCH_KS:
        c, exp = reference("mismatch", k)
        same_dict(mismatch_ref(big, c), shift(exp, by, n_ref, n_big), ("mismatch", k))
    # the mapping calls: every second read, every second pair (the lemma holds read by read)
    for k in MAP_KS:
        c, ref = reference("map", k)
        reads = np.arange(0, len(c.qs), 2)
        got = map_ref(big, Reads([c.qs[i] for i in reads], k=k, mh=0))
        same_dict(got, shift(rows_of(ref, reads, len(c.qs)), by, n_ref, n_big), ("map", k))
    k, kr, anchors = PAIR_RUNS[0]
    c, refs = reference("pairs", k, kr, anchors)
    reads = np.flatnonzero(np.arange(len(c.qs)) % 4 < 2)
    got = pair_refs(big, Reads([c.qs[i] for i in reads], k=k, kr=kr, mh=0), anchors)
    for w in WINDOWS:
        for g, r, nm in zip(got[w], refs[w], ("pairs", "rescue")):
            same_dict(g, shift(rows_of(r, reads, len(c.qs)), by, n_ref, n_big), (nm, k, kr, w))
