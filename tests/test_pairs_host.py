"""CPU checks of the paired-end boundary (sas_map_pairs / sas_map_pairs_fixed; no kernel is
launched): the calls are declared, exported and bound with the declared signatures and constants;
a null index and a bad fragment window are refused before any device call; the C++ mirror
(sas::SaNaive::map_pairs) compiles warning-free; and the numpy restatement of sas.h's definition
(pairs_ref, pairs_ref_all, which tests/test_gpu_pairs.py compares the GPU against bit for bit)
agrees with a plain double loop over the ends of both lists on the golden definition texts."""
import ctypes as C
import errno
import itertools
import json
import os
import subprocess

import numpy as np

from sas_amd import _lib
from test_align_host import NONE_DIST, align_ref_sel, check_script
from test_gpu_edit import EBrute, edited
from test_map_host import FIELDS as MAP_FIELDS, map_ref_all, revcomp_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, max_seed_hits, min_frag, max_frag, out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns,
# out_runs, out_qflags, out_pflags, out_npairs, out_nbestpairs, stream, flags
TAIL = [U32, U64, U32, U32] + [VP] * 13 + [U32]
SIGNATURES = {
    "sas_map_pairs": [VP, VP, VP, VP, U64] + TAIL,
    "sas_map_pairs_fixed": [VP, VP, U32, U64] + TAIL,
}
PAIR_FIELDS = ("pflags", "n_pairs", "n_best_pairs")
FIELDS = MAP_FIELDS + PAIR_FIELDS
EMASK = (1 << 42) - 1


def loci_reps(ends, dists):
    """(D, e) of the representative of every locus, ascending in e: a locus is a maximal run
    e, e + 1, e + 2, ... of the ascending ends, its representative the least (D, e) in it."""
    e, d = np.asarray(ends, np.int64), np.asarray(dists, np.int64)
    if len(e) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.concatenate([[0], np.flatnonzero(np.diff(e) != 1) + 1])
    rep = np.minimum.reduceat((d << 42) | e, first)
    return rep >> 42, rep & EMASK


def pairs_ref(n, A, lens, k, min_frag, max_frag):
    """sas.h's definition of the join.  A = (A_0, A_1): per read the answer of the read and of its
    reverse complement as EBrute.answer gives them; lens: the reads' lengths.  Per pair
    (n_pairs, n_best_pairs, best): best = (D_x + D_y, o, e_x, e_y, D_x, D_y) of the least
    (sum, o, e_x, e_y) over the proper candidates, None without one."""
    assert len(A[0]) == len(A[1]) == len(lens) and len(lens) % 2 == 0 and min_frag <= max_frag and k >= 0
    out = []
    for i in range(len(lens) // 2):
        cols = []
        for o in (0, 1):
            f, v = 2 * i + o, 2 * i + 1 - o
            dx, ex = loci_reps(A[0][f][0], A[0][f][1])
            dy, ey = loci_reps(A[1][v][0], A[1][v][1])
            if len(ex) == 0 or len(ey) == 0:
                continue
            # F = e_y - e_x + m_f in [min_frag, max_frag]: the partners of x are a slice of the ascending e_y
            w0 = np.searchsorted(ey, ex - int(lens[f]) + min_frag, "left")
            w1 = np.searchsorted(ey, ex - int(lens[f]) + max_frag, "right")
            cnt = w1 - w0
            xi = np.repeat(np.arange(len(ex)), cnt)
            yj = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(w0, cnt)
            F = ey[yj] - ex[xi] + int(lens[f])
            assert ((min_frag <= F) & (F <= max_frag)).all() and (ex <= n).all() and (ey <= n).all()
            cols.append(np.stack([dx[xi] + dy[yj], np.full(len(xi), o), ex[xi], ey[yj], dx[xi], dy[yj]], 1))
        c = np.concatenate(cols) if cols else np.zeros((0, 6), np.int64)
        if len(c) == 0:
            out.append((0, 0, None))
            continue
        best = c[np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))[0]]
        out.append((len(c), int((c[:, 0] == best[0]).sum()), tuple(int(x) for x in best)))
    return out


def pairs_ref_all(t, qs, k, A_fwd, A_rev, min_frag, max_frag, base=None):
    """The twelve fields as int64 arrays: map_ref_all's single-read records (`base`, when the
    caller has them already), the proper pairs' reads replaced by the best candidate's ends and
    re-aligned (align_ref_sel) on their strands, and the three per-pair fields."""
    n, nq = len(t), len(qs)
    base = map_ref_all(t, qs, k, A_fwd, A_rev, 3) if base is None else base
    out = {f: base[f].copy() for f in MAP_FIELDS}
    pr = pairs_ref(n, (A_fwd, A_rev), [len(q) for q in qs], k, min_frag, max_frag)
    out["n_pairs"] = np.array([min(p[0], 0xFFFFFFFF) for p in pr], np.int64)
    out["n_best_pairs"] = np.array([min(p[1], 0xFFFFFFFF) for p in pr], np.int64)
    out["pflags"] = (out["n_pairs"] > 0).astype(np.int64)
    chosen, sel = list(qs), []
    for i, (_, _, best) in enumerate(pr):
        if best is None:
            continue
        _, o, ex, ey, dx, dy = best
        f, v = 2 * i + o, 2 * i + 1 - o
        out["end"][f], out["dist"][f], out["strand"][f] = ex, dx, 0
        out["end"][v], out["dist"][v], out["strand"][v] = ey, dy, 1
        chosen[v] = revcomp_ref(qs[v])
        sel += [f, v]
    if sel:
        sel = np.array(sorted(sel))
        start, dist, nruns, runs = align_ref_sel(t, chosen, np.arange(nq), out["end"], k, sel)
        assert np.array_equal(dist, out["dist"][sel])  # the alignment's distance is D(e)
        out["start"][sel], out["nruns"][sel], out["runs"][sel] = start, nruns, runs
    return out


def categories(A, lens, ref, single):
    """What the pairs of a case are, from the answers and the reference records alone: a dict of
    boolean arrays, one entry per pair.  `single`: map_ref_all's records of the same reads."""
    npairs = len(lens) // 2
    has = [np.array([len(a[0]) > 0 for a in A[s]]) for s in (0, 1)]
    mapped = has[0] | has[1]
    m1, m2 = mapped[0::2], mapped[1::2]
    # some forward locus of one mate and some reverse locus of the other: only the distance can be wrong
    opposite = (has[0][0::2] & has[1][1::2]) | (has[0][1::2] & has[1][0::2])
    proper = ref["pflags"] == 1
    best_o = np.where(ref["strand"][0::2] == 0, 0, 1)
    moved = np.array([proper[i] and any(ref[f][r] != single[f][r] for r in (2 * i, 2 * i + 1)
                                        for f in ("end", "strand")) for i in range(npairs)])
    return dict(proper_o0=proper & (best_o == 0), proper_o1=proper & (best_o == 1),
                wrong_distance=~proper & m1 & m2 & opposite, same_strand=~proper & m1 & m2 & ~opposite,
                one_unmapped=m1 ^ m2, many_best=ref["n_best_pairs"] > 1, moved=moved)


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert (_lib.SAS_PAIR_PROPER, _lib.SAS_PAIR_MAX_SPREAD) == (1, 65535)
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    for line in ("#define SAS_PAIR_PROPER 1u", "#define SAS_PAIR_MAX_SPREAD 65535u"):
        assert line in src, line
    # the header's parameter lists, type by type
    ctype = {"const sas_index*": VP, "const uint8_t*": VP, "const uint64_t*": VP, "const uint32_t*": VP,
             "uint8_t*": VP, "uint16_t*": VP, "uint32_t*": VP, "uint64_t*": VP, "void*": VP, "uint64_t": U64,
             "uint32_t": U32}
    for name, sig in SIGNATURES.items():
        params = src.split("int " + name + "(")[1].split(")")[0]
        types = [" ".join(p.split()[:-1]) for p in params.replace("\n", " ").split(",")]
        assert [ctype[t] for t in types] == sig, (name, types)
    import sas_amd
    assert sas_amd.MappedPairs._fields == FIELDS


def test_bad_arguments_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    outs = (p,) * 12

    def both(index, lo, hi):
        return (L.sas_map_pairs(index, p, p, p, 1, 1, 0, lo, hi, *outs, None, 0),
                L.sas_map_pairs_fixed(index, p, 4, 1, 1, 0, lo, hi, *outs, None, 0))
    for rc in both(None, 100, 500):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()
    for rc in both(None, 0, _lib.SAS_PAIR_MAX_SPREAD):  # the widest window that is served
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()
    # the window is checked first: no index is needed to refuse it
    for rc in both(None, 501, 500):
        assert rc == errno.EINVAL and b"min_frag" in L.sas_last_error()
    for lo, hi in ((0, _lib.SAS_PAIR_MAX_SPREAD + 1), (7, 7 + _lib.SAS_PAIR_MAX_SPREAD + 1), (0, 0xFFFFFFFF)):
        for rc in both(None, lo, hi):
            assert rc == errno.EINVAL and b"SAS_PAIR_MAX_SPREAD" in L.sas_last_error()


def loop_ref(A, lens, i, min_frag, max_frag):
    """The join of pair i by a plain double loop over all ends of both lists; the loci from a
    groupby on e - index."""
    cands = []
    for o in (0, 1):
        f, v = 2 * i + o, 2 * i + 1 - o
        lists = []
        for ends, dists in ((A[0][f][0], A[0][f][1]), (A[1][v][0], A[1][v][1])):
            groups = itertools.groupby(enumerate(zip(ends, dists)), key=lambda x: x[1][0] - x[0])
            lists.append([min((int(d), int(e)) for _, (e, d) in g) for _, g in groups])
        for dx, ex in lists[0]:
            for dy, ey in lists[1]:
                if min_frag <= ey - ex + int(lens[f]) <= max_frag:
                    cands.append((dx + dy, o, ex, ey, dx, dy))
    if not cands:
        return 0, 0, None
    best = min(cands)
    return len(cands), sum(c[0] == best[0] for c in cands), best


def test_reference_agrees_with_independent_facts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(3)
    kinds = ("sub", "ins", "del")
    lo, hi = 20, 60
    seen = {}
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        if n < 64 or n > 1000:
            continue
        br = EBrute(t)
        for k in (0, 1, 2):
            def cut(s, m):
                ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20)))
                       for _ in range(int(rng.integers(0, k + 1)))]
                return edited(rng, t[s:s + m], ops)
            qs = []
            for j in range(14):
                m1, m2 = (int(x) for x in rng.integers(4, 13, 2))
                L = int(rng.integers(lo, hi + 1)) if j % 7 != 5 else int(rng.choice([lo - 3, hi + 3, hi + 9]))
                L = min(max(L, m1, m2), n)
                s = int(rng.integers(0, n - L + 1))
                a, b = cut(s, m1), revcomp_ref(cut(s + L - m2, m2))
                if j % 7 == 3:
                    b = revcomp_ref(b)                                # both mates from one strand
                if j % 7 == 4:
                    b = rng.integers(0, 4, 12).astype(np.uint8)       # one random mate
                if j % 7 == 6:
                    a, b = revcomp_ref(a), revcomp_ref(b)             # facing outwards: F <= 0
                qs += [b, a] if j % 2 else [a, b]
            lens = [len(q) for q in qs]
            A = (br.answers(qs, k, 0), br.answers([revcomp_ref(q) for q in qs], k, 0))
            pr = pairs_ref(n, A, lens, k, lo, hi)
            for i in range(len(qs) // 2):
                assert pr[i] == loop_ref(A, lens, i, lo, hi), (c["name"], k, i)
            ref = pairs_ref_all(t, qs, k, A[0], A[1], lo, hi)
            single = map_ref_all(t, qs, k, A[0], A[1], 3)
            for i, (cnt, nbest, best) in enumerate(pr):
                r0, r1 = 2 * i, 2 * i + 1
                for f_ in ("n_best", "n_loci", "qflags"):  # always the single-read values
                    assert np.array_equal(ref[f_][r0:r1 + 1], single[f_][r0:r1 + 1])
                if best is None:
                    assert (cnt, nbest, ref["pflags"][i]) == (0, 0, 0)
                    assert all(np.array_equal(ref[f_][r0:r1 + 1], single[f_][r0:r1 + 1]) for f_ in MAP_FIELDS)
                    continue
                assert 1 <= nbest <= cnt == ref["n_pairs"][i] and ref["pflags"][i] == 1
                f, v = 2 * i + best[1], 2 * i + 1 - best[1]
                assert (ref["strand"][f], ref["strand"][v]) == (0, 1)
                assert ref["dist"][f] + ref["dist"][v] == best[0]
                # each mate alone is at least as close as in the pair
                assert single["dist"][f] <= ref["dist"][f] and single["dist"][v] <= ref["dist"][v]
                # the true template length differs from F by at most k, and the scripts replay
                F = int(ref["end"][v] - ref["end"][f]) + lens[f]
                assert lo <= F <= hi and abs(int(ref["end"][v] - ref["start"][f]) - F) <= k
                for r, q in ((f, qs[f]), (v, revcomp_ref(qs[v]))):
                    check_script(t, q, int(ref["start"][r]), int(ref["end"][r]), int(ref["dist"][r]), ref["runs"][r],
                                 int(ref["nruns"][r]))
            for name, flag in categories(A, lens, ref, single).items():
                seen[name] = seen.get(name, 0) + int(flag.sum())
            unm = ref["dist"] == NONE_DIST
            assert (ref["end"][unm] == n).all() and not ref["nruns"][unm].any()
    assert len(seen) == 7 and all(v > 3 for v in seen.values()), seen


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const std::vector<sas::Seq> qs = {s.slice(0, 30), s.slice(300, 50)};
    const sas::SaNaive::MappedPairs a = idx.map_pairs(qs, 2, 100, 500);
    const sas::SaNaive::MappedPairs b = idx.map_pairs(qs, 2, 0, SAS_PAIR_MAX_SPREAD, 100, SAS_NO_PREFIX_TABLE);
    return (int)(a.end[0] + a.start[0] + a.dist[0] + a.strand[0] + a.n_best[0] + a.n_loci[0] + a.nruns[0] +
                 a.runs[0] + a.qflags[0] + a.stride + a.pflags[0] + a.n_pairs[0] + a.n_best_pairs[0] + b.end.size() +
                 SAS_PAIR_PROPER);
}
"""


def test_cpp_map_pairs_compiles(tmp_path):
    src = tmp_path / "pairs.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
