"""CPU checks of the read-mapping boundary (sas_map_edit / sas_map_edit_fixed / sas_revcomp /
sas_revcomp_fixed; no kernel is launched): the calls are declared, exported and bound with the
declared signatures and constants; a null index and a bad strand mask are refused before any
device call; the C++ mirror (sas::SaNaive::map_edit) compiles warning-free; and the numpy
restatement of sas.h's definition (revcomp_ref, map_ref, map_ref_all, which tests/test_gpu_map.py
compares the GPU against bit for bit) agrees with facts computed another way on the golden
definition texts."""
import ctypes as C
import errno
import json
import os
import subprocess

import numpy as np

from sas_amd import _lib
from test_align_host import NONE_DIST, align_ref_sel, check_script
from test_gpu_edit import EBrute, edited

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, max_seed_hits, strands, out_end, out_start, out_dist, out_strand, out_nbest, out_nloci, out_nruns, out_runs,
# out_qflags, stream, flags
TAIL = [U32, U64, U32, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, U32]
SIGNATURES = {
    "sas_revcomp": [VP, VP, VP, U64, VP, VP, VP, U32],
    "sas_revcomp_fixed": [VP, U32, U64, VP, VP, U32],
    "sas_map_edit": [VP, VP, VP, VP, U64] + TAIL,
    "sas_map_edit_fixed": [VP, VP, U32, U64] + TAIL,
}
FWD, REV = _lib.SAS_MAP_FWD, _lib.SAS_MAP_REV
FIELDS = ("end", "start", "dist", "strand", "n_best", "n_loci", "nruns", "runs", "qflags")


def revcomp_ref(q):
    """rc(q)[j] = q[m - 1 - j] ^ 3."""
    return (np.asarray(q, np.uint8)[::-1] ^ 3).astype(np.uint8)


def intervals(ends):
    """The number of maximal runs e, e + 1, e + 2, ... in an ascending list of ends."""
    return 0 if len(ends) == 0 else 1 + int((np.diff(ends) != 1).sum())


def map_ref(n, A_0, A_1, strands):
    """sas.h's definition for one read: A_s = (ends ascending, their distances, SAS_ED_* flags, ...) as
    EBrute.answer gives them for q (s = 0) and rc(q) (s = 1); only the strands of the mask take
    part.  Returns (end, dist, strand, n_best, n_loci, qflags)."""
    part = [(s, np.asarray(A[0], np.int64), np.asarray(A[1], np.int64), int(A[2]))
            for s, A in ((0, A_0), (1, A_1)) if (strands >> s) & 1]
    qflags = 0
    for _, _, _, fl in part:
        qflags |= fl
    triples = [(int(d.min()), s, int(e[d == d.min()][0])) for s, e, d, _ in part if len(e)]
    if not triples:
        return n, NONE_DIST, 0, 0, 0, qflags
    dist, strand, end = min(triples)
    n_best = sum(intervals(e[d == dist]) for _, e, d, _ in part)
    n_loci = sum(intervals(e) for _, e, _, _ in part)
    return end, dist, strand, n_best, n_loci, qflags


def map_ref_all(t, qs, k, A_fwd, A_rev, strands):
    """The records of every read: map_ref per read, then sas_align_edit's definition (align_ref_sel)
    for the winner against the chosen strand's chars.  A dict of int64 arrays named as FIELDS."""
    n, nq, stride = len(t), len(qs), 2 * k + 1
    rec = np.array([map_ref(n, a0, a1, strands) for a0, a1 in zip(A_fwd, A_rev)], np.int64).reshape(nq, 6)
    out = dict(end=rec[:, 0], dist=rec[:, 1], strand=rec[:, 2], n_best=rec[:, 3], n_loci=rec[:, 4], qflags=rec[:, 5],
               start=np.full(nq, n, np.int64), nruns=np.zeros(nq, np.int64), runs=np.zeros((nq, stride), np.int64))
    chosen = [revcomp_ref(q) if s else q for q, s in zip(qs, out["strand"])]
    sel = np.flatnonzero(out["dist"] != NONE_DIST)
    if len(sel):
        start, dist, nruns, runs = align_ref_sel(t, chosen, np.arange(nq), out["end"], k, sel)
        assert np.array_equal(dist, out["dist"][sel])  # the alignment's distance is D(e)
        out["start"][sel], out["nruns"][sel], out["runs"][sel] = start, nruns, runs
    return out


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert (_lib.SAS_MAP_FWD, _lib.SAS_MAP_REV) == (1, 2)
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    for line in ("#define SAS_MAP_FWD 1u", "#define SAS_MAP_REV 2u"):
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
    assert sas_amd.Mapped._fields == FIELDS


def test_bad_arguments_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    outs = (p, p, p, p, p, p, p, p, p)
    for rc in (L.sas_map_edit(None, p, p, p, 1, 1, 0, FWD | REV, *outs, None, 0),
               L.sas_map_edit_fixed(None, p, 4, 1, 1, 0, FWD, *outs, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()
    for strands in (0, 4):  # checked first: no index is needed to refuse them
        for rc in (L.sas_map_edit(None, p, p, p, 1, 1, 0, strands, *outs, None, 0),
                   L.sas_map_edit_fixed(None, p, 4, 1, 1, 0, strands, *outs, None, 0)):
            assert rc == errno.EINVAL and b"strands" in L.sas_last_error()
    # sas_revcomp: the ragged form needs its offsets' output; nq = 0 writes out_off[0] alone
    assert L.sas_revcomp(p, p, p, 1, p, None, None, 0) == errno.EINVAL
    off = np.full(2, 7, np.uint64)
    assert L.sas_revcomp(None, None, None, 0, None, off.ctypes.data, None, 0) == 0 and off.tolist() == [0, 7]
    assert L.sas_revcomp_fixed(None, 5, 0, None, None, 0) == 0


def test_reference_agrees_with_independent_facts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(1)
    kinds = ("sub", "ins", "del")
    seen = dict(unmapped=0, fwd=0, rev=0, both=0, multi=0, unique=0, valley=0, self_rc=0)
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        br = EBrute(t)
        qs = [np.array(qd["q"], np.uint8) for qd in c["queries"][:10]]
        qs += [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(1, 9, 4)]
        for i in range(0, n, max(n // 12, 1)):  # text slices with 0..2 edits, every second one reversed
            ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(i % 3)]
            q = edited(rng, t[i:i + 9 + i % 7], ops)
            qs.append(revcomp_ref(q) if (i // max(n // 12, 1)) % 2 else q)
        a = t[:4] if n >= 4 else rng.integers(0, 4, 4).astype(np.uint8)
        qs.append(np.concatenate([a, revcomp_ref(a)]))  # equal to its own reverse complement
        qs = [q for q in qs if len(q)]
        rcs = [revcomp_ref(q) for q in qs]
        assert all(np.array_equal(revcomp_ref(r), q) for q, r in zip(qs, rcs))  # rc(rc(q)) == q
        assert np.array_equal(qs[-1], rcs[-1])
        for k in (0, 1, 2, 3):
            A0, A1 = br.answers(qs, k, 0), br.answers(rcs, k, 0)
            both = map_ref_all(t, qs, k, A0, A1, FWD | REV)
            fwd = map_ref_all(t, qs, k, A0, A1, FWD)
            rev = map_ref_all(t, qs, k, A0, A1, REV)
            assert not fwd["strand"].any() and (rev["strand"] == (rev["dist"] != NONE_DIST)).all()
            for i, q in enumerate(qs):
                m = len(q)
                D = [br.rows([q])[0], br.rows([rcs[i]])[0]] if k < m else [None, None]
                end, dist, strand = int(both["end"][i]), int(both["dist"][i]), int(both["strand"][i])
                every = [(d, s, e) for s, A in ((0, A0[i]), (1, A1[i])) for e, d in zip(A[0], A[1])]
                if not every:
                    assert (end, dist, strand, both["n_best"][i], both["n_loci"][i], both["start"][i],
                            both["nruns"][i]) == (n, NONE_DIST, 0, 0, 0, n, 0) and not both["runs"][i].any()
                    assert k >= m or (D[0].min() > k and D[1].min() > k)
                    seen["unmapped"] += 1
                    continue
                # the winner is an end of the brute answer, and none is smaller
                assert (dist, strand, end) in every and not any(x < (dist, strand, end) for x in every)
                # the counts again, by a plain loop over every end position of the full rows
                nb = nl = 0
                for s in (0, 1):
                    for e in range(n + 1):
                        here, left = int(D[s][e]), int(D[s][e - 1]) if e else 99
                        nl += here <= k and left > k
                        nb += here == dist and left != dist
                assert (nb, nl) == (both["n_best"][i], both["n_loci"][i]), (c["name"], k, i)
                assert 1 <= nb and 1 <= nl
                # the script replays on the chosen strand's chars
                chosen = rcs[i] if strand else q
                check_script(t, chosen, int(both["start"][i]), end, dist, both["runs"][i], int(both["nruns"][i]))
                # both strands = the merge of the two one-strand records
                f, r = ((int(x["dist"][i]), int(x["strand"][i]), int(x["end"][i])) for x in (fwd, rev))
                assert (dist, strand, end) == min(f, r)
                assert both["n_loci"][i] == fwd["n_loci"][i] + rev["n_loci"][i]
                assert nb == sum(int(x["n_best"][i]) for x in (fwd, rev) if x["dist"][i] == dist)
                win = rev if strand else fwd
                assert all(np.array_equal(both[f_][i], win[f_][i]) for f_ in ("start", "nruns", "runs"))
                assert both["qflags"][i] == fwd["qflags"][i] | rev["qflags"][i] == 0
                seen["fwd"] += strand == 0
                seen["rev"] += strand == 1
                seen["both"] += len(A0[i][0]) > 0 and len(A1[i][0]) > 0
                seen["multi"] += nb > 1
                seen["unique"] += nb == 1 and nl == 1
                seen["valley"] += nl < nb
                if i == len(qs) - 1 and len(A0[i][0]):  # its own reverse complement: each place once per strand
                    assert nb == 2 * fwd["n_best"][i] and nl == 2 * fwd["n_loci"][i] and strand == 0
                    seen["self_rc"] += 1
    assert all(v > 10 for v in seen.values()), seen


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const std::vector<sas::Seq> qs = {s.slice(0, 30), s.slice(5, 50)};
    const sas::SaNaive::Mapped a = idx.map_edit(qs, 2);
    const sas::SaNaive::Mapped b = idx.map_edit(qs, 2, 100, SAS_MAP_REV, SAS_NO_PREFIX_TABLE);
    return (int)(a.end[0] + a.start[0] + a.dist[0] + a.strand[0] + a.n_best[0] + a.n_loci[0] + a.nruns[0] +
                 a.runs[0] + a.qflags[0] + a.stride + b.end.size() + SAS_MAP_FWD);
}
"""


def test_cpp_map_edit_compiles(tmp_path):
    src = tmp_path / "map.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
