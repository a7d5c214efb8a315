"""CPU checks of the mate-rescue boundary (sas_map_pairs_rescue / sas_map_pairs_rescue_fixed; no
kernel is launched): the calls are declared, exported and bound with the declared signatures and
constants; a null index, a k_rescue outside k .. 15 and a bad fragment window are refused before
any device call; the C++ mirror (sas::SaNaive::map_pairs_rescue) compiles warning-free; and the
numpy restatement of sas.h's definition (rescue_ref, rescue_ref_all, which
tests/test_gpu_rescue.py compares the GPU against bit for bit) agrees on the golden definition
texts with a plain triple loop over anchors and window ends, and with the chunking argument of
the scan kernel: D from the columns of one chunk and its lead-in alone is D wherever either is
within k_rescue."""
import ctypes as C
import errno
import itertools
import json
import os
import subprocess

import numpy as np

from sas_amd import _lib
from test_align_host import MAX_M, NONE_DIST, align_ref_sel, check_script
from test_gpu_edit import EBrute, edited
from test_map_host import FIELDS as MAP_FIELDS, intervals, map_ref_all, revcomp_ref
from test_pairs_host import FIELDS as PAIR_ALL_FIELDS, loci_reps, pairs_ref_all

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, k_rescue, max_seed_hits, min_frag, max_frag, max_anchors, out_end, out_start, out_dist, out_strand, out_nbest,
# out_nloci, out_nruns, out_runs, out_qflags, out_pflags, out_npairs, out_nbestpairs, out_nrescue, stream, flags
TAIL = [U32, U32, U64, U32, U32, U64] + [VP] * 14 + [U32]
SIGNATURES = {
    "sas_map_pairs_rescue": [VP, VP, VP, VP, U64] + TAIL,
    "sas_map_pairs_rescue_fixed": [VP, VP, U32, U64] + TAIL,
}
FIELDS = PAIR_ALL_FIELDS + ("n_rescue",)
PROPER, RESCUED, SKIPPED, MAP_RESCUED = 1, 2, 4, 8
CLAMP = 0xFFFFFFFF


class Rows:
    """EBrute.rows of single queries, kept: D(e) for e in [0, n] of a query, no seeds involved."""

    def __init__(self, br):
        self.br, self.kept = br, {}

    def __call__(self, q):
        key = np.asarray(q, np.uint8).tobytes()
        if key not in self.kept:
            self.kept[key] = self.br.rows([np.asarray(q, np.uint8)])[0].astype(np.int64)
        return self.kept[key]


def anchors_of(A, i):
    """The anchors of pair i: (a, s, D_a, e_a) for every locus of reads 2i and 2i + 1 on both strands."""
    out = []
    for a in (2 * i, 2 * i + 1):
        for s in (0, 1):
            d, e = loci_reps(A[s][a][0], A[s][a][1])
            out += [(a, s, int(dd), int(ee)) for dd, ee in zip(d, e)]
    return out


def window_of(n, s, e_a, m_a, m_b, min_frag, max_frag):
    """The ends [lo, hi] of the partner that the anchor's fragment window allows, cut to [0, n]
    (lo > hi: empty)."""
    lo, hi = (e_a - m_a + min_frag, e_a - m_a + max_frag) if s == 0 else (e_a + m_b - max_frag, e_a + m_b - min_frag)
    return max(lo, 0), min(hi, n)


def rescue_ref(n, A, qs, rows, k_rescue, min_frag, max_frag, max_anchors, n_pairs):
    """sas.h's definition of the rescue.  A = (A_0, A_1) as for pairs_ref, rows(q) = the full D of a
    query, n_pairs: sas_map_pairs' per-pair count.  Per pair (skipped, n_rescue, best): best =
    (D_x + D_y, o, e_x, e_y, D_x, D_y, s) of the least (sum, o, e_x, e_y) over the candidates of all
    anchors, s the anchor's strand; None without one."""
    out = []
    for i in range(len(qs) // 2):
        anchors = anchors_of(A, i) if n_pairs[i] == 0 and max_anchors > 0 else []
        if len(anchors) > max_anchors:
            out.append((True, 0, None))
            continue
        runs, best = 0, None
        for a, s, d_a, e_a in anchors:
            b = a ^ 1
            m_a, m_b = len(qs[a]), len(qs[b])
            if m_b <= k_rescue or m_b > MAX_M:
                continue
            lo, hi = window_of(n, s, e_a, m_a, m_b, min_frag, max_frag)
            if lo > hi:
                continue
            D = rows(qs[b] if s == 1 else revcomp_ref(qs[b]))[lo:hi + 1]
            cand = D <= k_rescue
            runs += int((cand & ~np.concatenate([[False], cand[:-1]])).sum())
            ends = lo + np.flatnonzero(cand)
            if len(ends) == 0:
                continue
            dd = D[cand]
            if s == 0:   # the anchor is the forward mate: the least (D_y, e_y)
                j = np.lexsort((ends, dd))[0]
                c = (d_a + int(dd[j]), a - 2 * i, e_a, int(ends[j]), d_a, int(dd[j]), 0)
            else:        # the anchor is the reverse mate: the least (D_x, e_x)
                j = np.lexsort((ends, dd))[0]
                c = (d_a + int(dd[j]), b - 2 * i, int(ends[j]), e_a, int(dd[j]), d_a, 1)
            F = c[3] - c[2] + len(qs[2 * i + c[1]])
            assert min_frag <= F <= max_frag, (i, c, F)
            best = c if best is None or c[:4] < best[:4] else best
        out.append((False, runs, best))
    return out


def rescue_ref_all(t, qs, k, k_rescue, A_fwd, A_rev, min_frag, max_frag, max_anchors, rows=None, base=None):
    """The thirteen fields as int64 arrays: pairs_ref_all's records with the alignments of k_rescue
    (`base`: map_ref_all(t, qs, k_rescue, ...) of the same answers, when the caller has it), the
    rescued pairs' reads replaced by the anchor's locus and the best candidate and re-aligned on
    their strands, the flags, and n_rescue."""
    assert k <= k_rescue <= 15
    n, nq = len(t), len(qs)
    rows = Rows(EBrute(t)) if rows is None else rows
    base = map_ref_all(t, qs, k_rescue, A_fwd, A_rev, 3) if base is None else base
    ref = pairs_ref_all(t, qs, k_rescue, A_fwd, A_rev, min_frag, max_frag, base=base)
    out = {f: ref[f].copy() for f in PAIR_ALL_FIELDS}
    rr = rescue_ref(n, (A_fwd, A_rev), qs, rows, k_rescue, min_frag, max_frag, max_anchors, out["n_pairs"])
    out["n_rescue"] = np.array([min(r[1], CLAMP) for r in rr], np.int64)
    chosen, sel = [None] * nq, []
    for i, (skipped, _, best) in enumerate(rr):
        if skipped:
            out["pflags"][i] |= SKIPPED
        if best is None:
            continue
        _, o, ex, ey, dx, dy, s = best
        f, v = 2 * i + o, 2 * i + 1 - o
        out["pflags"][i] |= RESCUED
        out["end"][f], out["dist"][f], out["strand"][f] = ex, dx, 0
        out["end"][v], out["dist"][v], out["strand"][v] = ey, dy, 1
        out["qflags"][v if s == 0 else f] |= MAP_RESCUED
        chosen[f], chosen[v] = qs[f], revcomp_ref(qs[v])
        sel += [f, v]
    if sel:
        sel = np.array(sorted(sel))
        start, dist, nruns, runs = align_ref_sel(t, chosen, np.arange(nq), out["end"], k_rescue, sel)
        assert np.array_equal(dist, out["dist"][sel])  # the alignment's distance is D(e)
        out["start"][sel], out["nruns"][sel], out["runs"][sel] = start, nruns, runs
    return out


def categories(ref, k):
    """What the pairs of a case are, from the reference records alone: boolean arrays, one per pair."""
    resc = (ref["pflags"] & RESCUED) != 0
    got = (ref["qflags"] & MAP_RESCUED) != 0
    placed = got[0::2] | got[1::2]
    assert np.array_equal(placed, resc) and not (got[0::2] & got[1::2]).any()
    got_read = np.where(got[0::2], 0, 1) + 2 * np.arange(len(resc))   # the read that the scan placed
    anchor_strand = ref["strand"][got_read ^ 1]
    eligible = ((ref["pflags"] & (PROPER | SKIPPED)) == 0) & ((ref["n_loci"][0::2] + ref["n_loci"][1::2]) > 0)
    return dict(fwd_anchor=resc & (anchor_strand == 0), rev_anchor=resc & (anchor_strand == 1),
                beyond_k=resc & (ref["dist"][got_read] > k),
                truncated=resc & ((ref["qflags"][got_read] & 1) != 0),
                skipped=(ref["pflags"] & SKIPPED) != 0, nothing=eligible & ~resc, runs2=ref["n_rescue"] >= 2)


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert (_lib.SAS_PAIR_RESCUED, _lib.SAS_PAIR_RESCUE_SKIPPED, _lib.SAS_MAP_RESCUED) == (RESCUED, SKIPPED, MAP_RESCUED)
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    for name, val in (("SAS_PAIR_RESCUED", 2), ("SAS_PAIR_RESCUE_SKIPPED", 4), ("SAS_MAP_RESCUED", 8),
                      ("SAS_RESCUE_CHUNK", _lib.SAS_RESCUE_CHUNK)):
        assert any(ln.split()[:3] == ["#define", name, f"{val}u"] for ln in src.splitlines()), name
    ctype = {"const sas_index*": VP, "const uint8_t*": VP, "const uint64_t*": VP, "const uint32_t*": VP,
             "uint8_t*": VP, "uint16_t*": VP, "uint32_t*": VP, "uint64_t*": VP, "void*": VP, "uint64_t": U64,
             "uint32_t": U32}
    for name, sig in SIGNATURES.items():
        params = src.split("int " + name + "(")[1].split(")")[0]
        types = [" ".join(p.split()[:-1]) for p in params.replace("\n", " ").split(",")]
        assert [ctype[t] for t in types] == sig, (name, types)
        # sas_map_pairs' parameters with k_rescue behind k, max_anchors behind max_frag, out_nrescue
        # behind out_nbestpairs
        names = [p.split()[-1] for p in params.replace("\n", " ").split(",")]
        plain = src.split("int " + name.replace("_rescue", "") + "(")[1].split(")")[0]
        pnames = [p.split()[-1] for p in plain.replace("\n", " ").split(",")]
        for new, behind in (("k_rescue", "k"), ("max_anchors", "max_frag"), ("out_nrescue", "out_nbestpairs")):
            pnames.insert(pnames.index(behind) + 1, new)
        assert names == pnames, name
    import sas_amd
    assert sas_amd.MappedPairsRescue._fields == FIELDS
    assert callable(sas_amd.SaNaive.map_pairs_rescue) and callable(sas_amd.SaNaive.map_pairs_rescue_fixed)


def test_bad_arguments_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    outs = (p,) * 13

    def both(index, k, kr, lo, hi, anchors=4):
        return (L.sas_map_pairs_rescue(index, p, p, p, 1, k, kr, 0, lo, hi, anchors, *outs, None, 0),
                L.sas_map_pairs_rescue_fixed(index, p, 4, 1, k, kr, 0, lo, hi, anchors, *outs, None, 0))
    for k, kr in ((1, 1), (1, 3), (0, 15), (15, 15)):
        for rc in both(None, k, kr, 100, 500):
            assert rc == errno.EINVAL and b"null index" in L.sas_last_error()
    for rc in both(None, 1, 3, 0, _lib.SAS_PAIR_MAX_SPREAD, 0):  # the widest window that is served
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()
    for k, kr in ((1, 0), (3, 2), (15, 14), (1, 16), (0, 16), (16, 16), (2, 0xFFFFFFFF)):
        for rc in both(None, k, kr, 100, 500):
            assert rc == errno.EINVAL and b"k_rescue" in L.sas_last_error(), (k, kr)
    for rc in both(None, 1, 3, 501, 500):
        assert rc == errno.EINVAL and b"min_frag" in L.sas_last_error()
    for lo, hi in ((0, _lib.SAS_PAIR_MAX_SPREAD + 1), (7, 7 + _lib.SAS_PAIR_MAX_SPREAD + 1), (0, 0xFFFFFFFF)):
        for rc in both(None, 1, 3, lo, hi):
            assert rc == errno.EINVAL and b"SAS_PAIR_MAX_SPREAD" in L.sas_last_error()


def loop_ref(n, A, qs, rows, i, k_rescue, min_frag, max_frag, max_anchors):
    """The rescue of pair i (known to have no proper candidate) by plain loops: the loci from a
    groupby on e - index, every end of every window in turn."""
    anchors = []
    for a in (2 * i, 2 * i + 1):
        for s in (0, 1):
            ends, dists = A[s][a][0], A[s][a][1]
            groups = itertools.groupby(enumerate(zip(ends, dists)), key=lambda x: x[1][0] - x[0])
            anchors += [(a, s) + min((int(d), int(e)) for _, (e, d) in g) for _, g in groups]
    if max_anchors == 0 or len(anchors) > max_anchors:
        return max_anchors > 0, 0, None
    runs, cands = 0, []
    for a, s, d_a, e_a in anchors:
        b = a ^ 1
        m_a, m_b = len(qs[a]), len(qs[b])
        if m_b <= k_rescue or m_b > MAX_M:
            continue
        D = rows(qs[b] if s == 1 else revcomp_ref(qs[b]))
        before = False
        for F in (range(min_frag, max_frag + 1) if s == 0 else range(max_frag, min_frag - 1, -1)):
            e = e_a - m_a + F if s == 0 else e_a + m_b - F   # ascending in both cases
            if not 0 <= e <= n:
                before = False
                continue
            now = int(D[e]) <= k_rescue
            runs += now and not before
            before = now
            if now:
                cands.append((d_a + int(D[e]), a - 2 * i, e_a, e, d_a, int(D[e]), 0) if s == 0 else
                             (d_a + int(D[e]), b - 2 * i, e, e_a, int(D[e]), d_a, 1))
    return False, runs, (min(cands) if cands else None)


def golden_cases(golden_dir):
    for c in json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]:
        t = np.array(c["text"], np.uint8)
        if 64 <= len(t) <= 1000:
            yield c["name"], t


def test_reference_agrees_with_a_plain_loop(golden_dir):
    rng = np.random.default_rng(5)
    kinds = ("sub", "ins", "del")
    lo, hi = 20, 60
    seen = {}
    for name, t in golden_cases(golden_dir):
        n = len(t)
        br = EBrute(t)
        rows = Rows(br)
        for k, kr, anchors in ((0, 0, 3), (0, 2, 2), (1, 1, 4), (1, 3, 3), (2, 3, 1), (1, 2, 0)):
            def cut(s, m, edits):
                ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(edits)]
                return edited(rng, t[s:s + m], ops)
            qs = []
            for j in range(16):
                m1, m2 = (int(x) for x in rng.integers(6, 14, 2))
                L = int(rng.integers(lo, hi + 1)) if j % 8 != 5 else int(rng.choice([lo - 3, hi + 3]))
                L = min(max(L, m1, m2), n)
                s = int(rng.integers(0, n - L + 1))
                heavy = int(rng.integers(k + 1, kr + 1)) if kr > k else k   # more edits than the seeds bear
                e1, e2 = ((heavy, 0), (0, heavy), (0, 0), (k, k))[j % 4]
                a, b = cut(s, m1, e1), revcomp_ref(cut(s + L - m2, m2, e2))
                if j % 8 == 6:
                    b = rng.integers(0, 4, 12).astype(np.uint8)       # one random mate
                if j % 8 == 7:
                    b = b[:kr]                                        # a partner too short to look for
                qs += [b, a] if j % 2 else [a, b]
            A = (br.answers(qs, k, 0), br.answers([revcomp_ref(q) for q in qs], k, 0))
            ref = rescue_ref_all(t, qs, k, kr, A[0], A[1], lo, hi, anchors, rows=rows)
            plain = pairs_ref_all(t, qs, k, A[0], A[1], lo, hi)
            rr = rescue_ref(n, A, qs, rows, kr, lo, hi, anchors, plain["n_pairs"])
            for f_ in ("n_pairs", "n_best_pairs", "n_best", "n_loci"):   # always sas_map_pairs' values
                assert np.array_equal(ref[f_], plain[f_]), (name, k, kr, f_)
            assert np.array_equal(ref["pflags"] & PROPER, plain["pflags"])
            assert np.array_equal(ref["qflags"] & 7, plain["qflags"])
            for i in range(len(qs) // 2):
                r0 = 2 * i
                if plain["n_pairs"][i]:
                    assert rr[i] == (False, 0, None) and ref["pflags"][i] == PROPER and ref["n_rescue"][i] == 0
                    for f_ in ("end", "start", "dist", "strand", "nruns"):   # a proper pair is unchanged
                        assert np.array_equal(ref[f_][r0:r0 + 2], plain[f_][r0:r0 + 2]), (name, k, kr, i, f_)
                    assert np.array_equal(ref["runs"][r0:r0 + 2, :2 * k + 1], plain["runs"][r0:r0 + 2])
                    assert not ref["runs"][r0:r0 + 2, 2 * k + 1:].any()
                    continue
                assert rr[i] == loop_ref(n, A, qs, rows, i, kr, lo, hi, anchors), (name, k, kr, i)
                skipped, runs, best = rr[i]
                assert ref["n_rescue"][i] == runs and bool(ref["pflags"][i] & SKIPPED) == skipped
                if anchors == 0:
                    assert (skipped, runs, best, ref["pflags"][i]) == (False, 0, None, 0)
                if best is None:
                    assert not ref["pflags"][i] & RESCUED
                    for f_ in ("end", "start", "dist", "strand", "nruns", "qflags"):
                        assert np.array_equal(ref[f_][r0:r0 + 2], plain[f_][r0:r0 + 2]), (name, k, kr, i, f_)
                    continue
                assert ref["pflags"][i] == RESCUED and runs >= 1
                f, v = 2 * i + best[1], 2 * i + 1 - best[1]
                got, anchor = (v, f) if best[6] == 0 else (f, v)
                assert (ref["strand"][f], ref["strand"][v]) == (0, 1)
                assert ref["qflags"][got] & MAP_RESCUED and not ref["qflags"][anchor] & MAP_RESCUED
                assert ref["dist"][anchor] <= k and ref["dist"][got] <= kr
                # the anchor's end is a locus representative of its read on its strand; the other end is not
                s = best[6]
                reps = loci_reps(A[s][anchor][0], A[s][anchor][1])[1]
                assert int(ref["end"][anchor]) in reps.tolist()
                other = loci_reps(A[1 - s][got][0], A[1 - s][got][1])[1]
                assert int(ref["end"][got]) not in other.tolist()
                F = int(ref["end"][v] - ref["end"][f]) + len(qs[f])
                assert lo <= F <= hi
                for r, q in ((f, qs[f]), (v, revcomp_ref(qs[v]))):
                    check_script(t, q, int(ref["start"][r]), int(ref["end"][r]), int(ref["dist"][r]), ref["runs"][r],
                                 int(ref["nruns"][r]))
            if kr > k and anchors:
                for cname, flag in categories(ref, k).items():
                    seen[cname] = seen.get(cname, 0) + int(flag.sum())
            unm = ref["dist"] == NONE_DIST
            assert (ref["end"][unm] == n).all() and not ref["nruns"][unm].any()
    seen.pop("truncated")  # no seed is skipped here
    assert len(seen) == 6 and all(v > 3 for v in seen.values()), seen


def test_a_chunk_and_its_lead_in_give_the_full_distance(golden_dir):
    """The scan kernel's exactness: for the ends [c0, c1] of a chunk, D computed from the text
    columns [max(0, c0 - m - k_r), c1) alone equals the full D wherever either is <= k_r; one column
    more in front does the same for the end c0 - 1, which the run heads need."""
    rng = np.random.default_rng(6)
    checked = within = 0
    for name, t in golden_cases(golden_dir):
        n = len(t)
        br = EBrute(t)
        for m, kr in ((5, 0), (9, 2), (12, 3), (20, 15), (33, 4)):
            s = int(rng.integers(0, n - m + 1))
            q = edited(rng, t[s:s + m], [("sub", int(rng.integers(0, 1 << 20))), ("del", int(rng.integers(0, 1 << 20)))])
            q = q if int(rng.integers(0, 2)) else t[s:s + m].copy()
            m = len(q)
            if m <= kr:
                continue
            D = br.rows([q])[0].astype(np.int64)
            for chunk in (1, 7, 64):
                for c0 in list(range(0, n + 1, chunk))[:: max(1, (n // chunk) // 40)]:
                    c1 = min(c0 + chunk - 1, n)
                    for lead in (0, 1):   # the issue's statement, and the kernel's column for the heads
                        w0 = max(0, c0 - lead - m - kr)
                        part = EBrute(t[w0:c1]).rows([q])[0].astype(np.int64)   # ends w0 .. c1
                        first = max(c0 - lead, 0)
                        a, b = D[first:c1 + 1], part[first - w0:]
                        assert (a <= b).all(), (name, m, kr, chunk, c0)
                        near = (a <= kr) | (b <= kr)
                        assert np.array_equal(a[near], b[near]), (name, m, kr, chunk, c0, lead)
                        checked += len(a)
                        within += int(near.sum())
    assert checked > 10 ** 4 and within > 100, (checked, within)


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const std::vector<sas::Seq> qs = {s.slice(0, 30), s.slice(300, 50)};
    const sas::SaNaive::MappedPairsRescue a = idx.map_pairs_rescue(qs, 1, 3, 100, 500, 16);
    const sas::SaNaive::MappedPairsRescue b =
        idx.map_pairs_rescue(qs, 2, 2, 0, SAS_PAIR_MAX_SPREAD, 0, 100, SAS_NO_PREFIX_TABLE);
    return (int)(a.end[0] + a.start[0] + a.dist[0] + a.strand[0] + a.n_best[0] + a.n_loci[0] + a.nruns[0] +
                 a.runs[0] + a.qflags[0] + a.stride + a.pflags[0] + a.n_pairs[0] + a.n_best_pairs[0] +
                 a.n_rescue[0] + b.end.size() + SAS_PAIR_RESCUED + SAS_PAIR_RESCUE_SKIPPED + SAS_MAP_RESCUED +
                 SAS_RESCUE_CHUNK);
}
"""


def test_cpp_map_pairs_rescue_compiles(tmp_path):
    src = tmp_path / "rescue.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
