"""CPU checks of the alignment boundary (sas_align_edit / sas_align_edit_fixed; no kernel is
launched): the calls are declared, exported and bound with the declared signatures and constants;
a null index is refused before any device call; the C++ mirror (sas::SaNaive::align_edit)
compiles warning-free; and the numpy restatement of sas.h's definition (align_ref, which
tests/test_gpu_align.py compares the GPU against bit for bit) agrees with independent facts on
the golden definition texts."""
import ctypes as C
import errno
import json
import os
import subprocess

import numpy as np

from sas_amd import _lib
from test_gpu_edit import EBrute, edited

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, off, end, na, out_start, out_dist, out_nruns, out_runs, stream, flags
TAIL = [U32, VP, VP, U64, VP, VP, VP, VP, VP, U32]
SIGNATURES = {
    "sas_align_edit": [VP, VP, VP, VP, U64] + TAIL,
    "sas_align_edit_fixed": [VP, VP, U32, U64] + TAIL,
}
# the library's own values (without the calls the module fails here); the header's are checked below
EQ, X, INS, DEL = _lib.SAS_AL_EQ, _lib.SAS_AL_X, _lib.SAS_AL_INS, _lib.SAS_AL_DEL
NONE_DIST, MAX_M = _lib.SAS_AL_NONE_DIST, _lib.SAS_ED_MAX_M
BATCH = 64


def align_ref(t, qs, ends, k):
    """sas.h's definition for up to 64 alignments of equally long queries qs[b] that end at
    ends[b]: (start, dist, nruns, runs[B, 2k + 1]).  R[b, i, c] = ed(q[i:], t[j:e]) over the columns
    j = e - m - k + c, c in [0, m + k] (a superset of [w0, e]: the columns with j < 0 are masked
    where row 0 is read, and no cell of a larger j depends on them).  A row is the running
    minimum, from the right, of min(diagonal + (chars differ), below + 1)."""
    n, B, stride = len(t), len(qs), 2 * k + 1
    assert B <= BATCH
    m = len(qs[0])
    start = np.full(B, n, np.int64)
    dist = np.full(B, NONE_DIST, np.int64)
    nruns = np.zeros(B, np.int64)
    runs = np.zeros((B, stride), np.int64)
    e = np.asarray(ends, np.int64)
    if m == 0 or m > MAX_M:
        return start, dist, nruns, runs
    inside = e <= n
    e = np.where(inside, e, 0)
    W = m + k + 1
    ar = np.arange(W, dtype=np.int16)
    j = (e - m - k)[:, None] + ar[None, :].astype(np.int64)
    T = np.where((j >= 0) & (j < e[:, None]), t[np.clip(j, 0, max(n - 1, 0))] if n else 0, 255)
    Q = np.array(qs, np.int64).reshape(B, m)
    R = np.empty((B, m + 1, W), np.int16)
    R[:, m, :] = (W - 1) - ar  # R[m][j] = e - j
    for i in range(m - 1, -1, -1):
        A = np.empty((B, W), np.int16)
        A[:, :-1] = np.minimum(R[:, i + 1, 1:] + (T[:, :-1] != Q[:, i, None]), R[:, i + 1, :-1] + 1)
        A[:, -1] = m - i  # R[i][e] = m - i
        R[:, i, :] = np.minimum.accumulate((A + ar)[:, ::-1], axis=1)[:, ::-1] - ar
    R0 = np.where(j >= 0, R[:, 0, :], np.int16(30000))
    d = R0.min(axis=1)
    cs = W - 1 - np.argmin(R0[:, ::-1], axis=1)  # the largest column that reaches d
    has = inside & (d <= k)
    start[has] = (e - m - k + cs)[has]
    dist[has] = d[has]
    # the walk, all alignments in step
    b = np.arange(B)
    i, c = np.zeros(B, np.int64), cs.copy()
    ops = []
    while True:
        act = has & ((i < m) | (c < W - 1))
        if not act.any():
            break
        cur = R[b, i, c].astype(np.int64)
        i1, c1 = np.minimum(i + 1, m), np.minimum(c + 1, W - 1)
        ne = Q[b, np.minimum(i, m - 1)] != T[b, np.minimum(c, W - 2)]
        r1 = (i < m) & (c < W - 1) & (R[b, i1, c1] + ne == cur)
        r2 = ~r1 & (c < W - 1) & (R[b, i, c1] + 1 == cur)
        op = np.where(r1, np.where(ne, X, EQ), np.where(r2, DEL, INS))
        ops.append(np.where(act, op, 9))
        i = np.where(act & (r1 | ~r2), i + 1, i)
        c = np.where(act & (r1 | r2), c + 1, c)
    if ops:
        ops = np.stack(ops, axis=1)
        for x in np.flatnonzero(has):
            row = ops[x][ops[x] != 9]
            cut = np.flatnonzero(np.diff(row)) + 1
            first = np.concatenate([[0], cut])
            lens = np.diff(np.concatenate([first, [len(row)]]))
            assert len(first) <= stride, (qs[x], ends[x], k)
            nruns[x] = len(first)
            runs[x, :len(first)] = (lens << 2) | row[first]
    return start, dist, nruns, runs


def align_ref_all(t, qs, off, end, k):
    """align_ref of every alignment a (query i with off[i] <= a < off[i + 1]), in batches of at most
    64 of equal query length."""
    na = len(end)
    qi = np.searchsorted(np.asarray(off, np.int64), np.arange(na), side="right") - 1
    return align_ref_sel(t, qs, qi, end, k, np.arange(na))


def align_ref_sel(t, qs, qi, end, k, sel):
    """(start, dist, nruns, runs) of the alignments sel (indices into end; qi[a] = its query)."""
    stride = 2 * k + 1
    out = (np.zeros(len(sel), np.int64), np.zeros(len(sel), np.int64), np.zeros(len(sel), np.int64),
           np.zeros((len(sel), stride), np.int64))
    by_len = {}
    for x, a in enumerate(sel):
        by_len.setdefault(len(qs[qi[a]]), []).append(x)
    for m, xs in by_len.items():
        for g in range(0, len(xs), BATCH):
            grp = xs[g:g + BATCH]
            got = align_ref(t, [qs[qi[sel[x]]] for x in grp], [int(end[sel[x]]) for x in grp], k)
            for o, v in zip(out, got):
                o[grp] = v
    return out


def ed_loops(a, b):
    """The unit-cost edit distance of two sequences, cell by cell."""
    prev = list(range(len(b) + 1))
    for x in range(1, len(a) + 1):
        cur = [x] + [0] * len(b)
        for y in range(1, len(b) + 1):
            cur[y] = min(prev[y - 1] + (a[x - 1] != b[y - 1]), prev[y] + 1, cur[y - 1] + 1)
        prev = cur
    return prev[len(b)]


def check_script(t, q, s, e, d, runs_row, nr):
    """Replaying the script on t[s:e) yields q: the = runs copy the text, the X runs differ from it
    char by char, the ops use up exactly q and t[s:e), the chars that are not = number d, and
    adjacent runs differ in op."""
    i, j, edits, prev = 0, s, 0, -1
    for r in runs_row[:nr]:
        ln, op = int(r) >> 2, int(r) & 3
        assert ln > 0 and op != prev, (q, s, e, runs_row)
        prev = op
        if op in (EQ, X):
            assert i + ln <= len(q) and j + ln <= e, (q, s, e, runs_row)
            same = q[i:i + ln] == t[j:j + ln]
            assert same.all() if op == EQ else not same.any(), (q, s, e, runs_row)
        i += ln if op != DEL else 0
        j += ln if op != INS else 0
        edits += ln if op != EQ else 0
    assert (i, j, edits) == (len(q), e, d), (q, s, e, d, runs_row)


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert (_lib.SAS_AL_EQ, _lib.SAS_AL_X, _lib.SAS_AL_INS, _lib.SAS_AL_DEL, _lib.SAS_AL_NONE_DIST) == \
        (0, 1, 2, 3, 255)
    # the header's parameter lists, type by type, and its constants
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    for line in ("#define SAS_AL_EQ  0u", "#define SAS_AL_X   1u", "#define SAS_AL_INS 2u", "#define SAS_AL_DEL 3u",
                 "#define SAS_AL_NONE_DIST 255u", "#define SAS_ED_MAX_M     256u"):
        assert line in src, line
    assert _lib.SAS_ED_MAX_M == 256
    ctype = {"const sas_index*": VP, "const uint8_t*": VP, "const uint64_t*": VP, "const uint32_t*": VP,
             "const void*": VP, "uint8_t*": VP, "uint16_t*": VP, "void*": VP, "uint64_t": U64, "uint32_t": U32}
    for name, sig in SIGNATURES.items():
        params = src.split("int " + name + "(")[1].split(")")[0]
        types = [" ".join(p.split()[:-1]) for p in params.replace("\n", " ").split(",")]
        assert [ctype[t] for t in types] == sig, (name, types)


def test_null_index_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    for rc in (L.sas_align_edit(None, p, p, p, 1, 1, p, p, 1, p, None, None, None, None, 0),
               L.sas_align_edit_fixed(None, p, 4, 1, 1, p, p, 1, p, None, None, None, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()


def test_cigar_helper():
    import sas_amd
    row = np.array([(17 << 2) | EQ, (1 << 2) | X, (14 << 2) | EQ, (2 << 2) | INS, (1 << 2) | DEL, 0, 0], np.uint16)
    assert sas_amd.cigar(row, 3) == "17=1X14=" and sas_amd.cigar(row, 5) == "17=1X14=2I1D"
    assert sas_amd.cigar(row.astype(np.int16), 0) == ""


def test_reference_agrees_with_independent_facts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(0)
    kinds = ("sub", "ins", "del")
    checked = none = looped = 0
    seen_ops, start0, max_runs = set(), 0, 0
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        br = EBrute(t)
        qs = [np.array(qd["q"], np.uint8) for qd in c["queries"][:12]]
        qs += [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(1, 9, 6)]
        for i in range(0, n, max(n // 10, 1)):  # text slices with 1..3 edits
            ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(1 + i % 3)]
            qs.append(edited(rng, t[i:i + 9 + i % 7], ops))
        qs = [q for q in qs if len(q)]
        for k in (0, 1, 2, 3):
            D = {}
            by_len = {}
            for x, q in enumerate(qs):
                by_len.setdefault(len(q), []).append(x)
            for m, xs in by_len.items():
                for r, x in zip(br.rows([qs[x] for x in xs]), xs):
                    D[x] = r
            # per query: up to 6 ends within k (the first, the last, a sample), and 2 without
            qi, end = [], []
            for x in range(len(qs)):
                hit, miss = np.flatnonzero(D[x] <= k), np.flatnonzero(D[x] > k)
                pick = set(hit[:2].tolist() + hit[-2:].tolist())
                if len(hit):
                    pick |= set(rng.choice(hit, min(2, len(hit)), replace=False).tolist())
                if len(miss):
                    pick |= set(rng.choice(miss, min(2, len(miss)), replace=False).tolist())
                for e in sorted(pick):
                    qi.append(x)
                    end.append(e)
            qi, end = np.array(qi), np.array(end, np.int64)
            start, dist, nruns, runs = align_ref_sel(t, qs, qi, end, k, np.arange(len(end)))
            for a in range(len(end)):
                q, e, De = qs[qi[a]], int(end[a]), int(D[qi[a]][end[a]])
                m = len(q)
                if De > k:  # no alignment within k ends here
                    assert (start[a], dist[a], nruns[a]) == (n, NONE_DIST, 0) and not runs[a].any()
                    none += 1
                    continue
                s, d, nr = int(start[a]), int(dist[a]), int(nruns[a])
                assert d == De and max(0, e - m - k) <= s <= e, (c["name"], q, e, k)
                assert nr <= 2 * k + 1 and not runs[a, nr:].any()
                check_script(t, q, s, e, d, runs[a], nr)
                if m * (m + k) <= 1500:  # the plain loops, where they take no time
                    assert ed_loops(q.tolist(), t[s:e].tolist()) == d
                    # no later start reaches d: the last row of ed(reversed q, reversed t[.. e))
                    # over every prefix length is ed(q, t[s' .. e)) for every s'
                    rq, rt = q[::-1].tolist(), t[max(0, e - m - k):e][::-1].tolist()
                    prev = list(range(len(rt) + 1))
                    for x in range(1, m + 1):
                        cur = [x] + [0] * len(rt)
                        for y in range(1, len(rt) + 1):
                            cur[y] = min(prev[y - 1] + (rq[x - 1] != rt[y - 1]), prev[y] + 1, cur[y - 1] + 1)
                        prev = cur
                    assert prev[e - s] == d and min(prev) == d and all(v > d for v in prev[:e - s])
                    looped += 1
                seen_ops |= {int(r) & 3 for r in runs[a, :nr]}
                start0 += s == 0
                max_runs = max(max_runs, nr)
                checked += 1
    assert checked > 2000 and none > 500 and looped > 1000, (checked, none, looped)
    assert seen_ops == {EQ, X, INS, DEL} and start0 > 0 and max_runs >= 5, (seen_ops, start0, max_runs)


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const std::vector<sas::Seq> qs = {s.slice(0, 30), s.slice(5, 50)};
    const sas::SaNaive::Edited r = idx.locate_edit(qs, 2);
    const sas::SaNaive::Aligned a = idx.align_edit(qs, 2, r);
    const std::string c = sas::cigar(a, 0);
    return (int)(a.start[0] + a.dist[0] + a.nruns[0] + a.runs[0] + a.stride + c.size() +
                 (a.runs[0] & 3u) + SAS_AL_EQ + SAS_AL_X + SAS_AL_INS + SAS_AL_DEL + SAS_AL_NONE_DIST);
}
"""


def test_cpp_align_edit_compiles(tmp_path):
    src = tmp_path / "align.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
