"""The reference of the maximal-exact-match call (sas.h: sas_mems) on the CPU, and the checks that
need no GPU.

ref_mems is built on the diagonal-run statement of the definition, which knows nothing of how the
GPU finds the matches: the MEMs of a query p and a text t are the maximal runs of `true`, of at
least L cells, on the diagonals of the matrix [p[i] == t[j]].  The order key is the SA rank of the
CPU oracle's suffix array; occurrence counts (max_hits, unique) come from bytes.find."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUNCATED, SHORT = 1, 2
CELLS = 1 << 22  # matrix cells per block of diagonals


def diagonal_runs(p: np.ndarray, t: np.ndarray):
    """(i, j, len) of every maximal run of p[i + x] == t[j + x] (len >= 1), as int64 arrays."""
    m, n = len(p), len(t)
    if m == 0 or n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    ii = np.arange(m, dtype=np.int64)[None, :]
    out = []
    rows = max(1, CELLS // m)
    for d0 in range(-(m - 1), n, rows):
        d = np.arange(d0, min(d0 + rows, n), dtype=np.int64)[:, None]  # j - i of each diagonal
        jj = ii + d
        inside = (jj >= 0) & (jj < n)
        eq = inside & (p[ii] == t[np.clip(jj, 0, n - 1)])
        z = np.zeros((len(d), m + 2), np.int8)
        z[:, 1:-1] = eq
        df = np.diff(z, axis=1)
        s, e = np.argwhere(df == 1), np.argwhere(df == -1)  # row-major both: run k starts s[k], ends e[k]
        assert len(s) == len(e) and np.array_equal(s[:, 0], e[:, 0])
        out.append((s[:, 1], s[:, 1] + d[s[:, 0], 0], e[:, 1] - s[:, 1]))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


class Text:
    """A text with what the reference needs of it, computed once."""

    def __init__(self, t):
        self.t = np.ascontiguousarray(t, np.uint8)
        self.n = len(self.t)
        self.tb = self.t.tobytes()
        sa = O.build_sa(self.t).astype(np.int64) if self.n else np.zeros(0, np.int64)
        self.rank = np.empty(self.n, np.int64)
        self.rank[sa] = np.arange(self.n)
        self._more = {}
        self._runs = {}

    def runs(self, p: np.ndarray, lo: int, hi: int):
        """diagonal_runs of p against the segment [lo, hi) as a text of its own, j shifted by lo;
        kept (as int32), since they depend on neither L nor max_hits."""
        key = (p.tobytes(), lo, hi)
        r = self._runs.get(key)
        if r is None:
            i, j, l = diagonal_runs(p, self.t[lo:hi])
            r = self._runs[key] = (i.astype(np.int32), (j + lo).astype(np.int32), l.astype(np.int32))
        return tuple(x.astype(np.int64) for x in r)

    def more_than(self, s: bytes, k: int) -> bool:
        """s occurs more than k times in the text (overlapping occurrences count)."""
        key = (s, k)
        r = self._more.get(key)
        if r is None:
            c, at = 0, self.tb.find(s)
            while at >= 0 and c <= k:
                c += 1
                at = self.tb.find(s, at + 1)
            r = self._more[key] = c > k
        return r


def ref_mems(t, queries, L, max_hits=0, unique=False, layout=None):
    """(off, qpos, tpos, len, qflags), int64 arrays, of sas_mems on the text t (an array or a
    Text) for a list of queries.  layout: (seg_lo, seg_hi), each segment a text of its own."""
    T = t if isinstance(t, Text) else Text(t)
    assert L >= 1
    segs = [(0, T.n)] if layout is None else list(zip(*layout))
    off, qpos, tpos, ln, qfl = [0], [], [], [], []
    for p in queries:
        p = np.ascontiguousarray(p, np.uint8)
        m, fl = len(p), 0
        if m < L:
            qfl.append(SHORT)
            off.append(off[-1])
            continue
        ri, rj, rl = [], [], []
        for lo, hi in segs:
            i, j, l = T.runs(p, int(lo), int(hi))
            keep = l >= L
            ri.append(i[keep]), rj.append(j[keep]), rl.append(l[keep])
        i, j, l = np.concatenate(ri), np.concatenate(rj), np.concatenate(rl)
        pb = p.tobytes()
        if max_hits:
            skipped = np.array([T.more_than(pb[x:x + L], max_hits) for x in range(m - L + 1)], bool)
            if skipped.any():
                fl |= TRUNCATED
            keep = ~skipped[i]
            i, j, l = i[keep], j[keep], l[keep]
        if unique:
            keep = np.array([not T.more_than(T.tb[b:b + c], 1) for b, c in zip(j.tolist(), l.tolist())], bool)
            i, j, l = i[keep], j[keep], l[keep]
        order = np.lexsort((T.rank[j], i))
        qpos.append(i[order]), tpos.append(j[order]), ln.append(l[order])
        qfl.append(fl)
        off.append(off[-1] + len(order))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)  # noqa: E731
    return np.array(off, np.int64), cat(qpos), cat(tpos), cat(ln), np.array(qfl, np.int64)


def brute_mems(t, p, L, lo=0, hi=None):
    """The definition cell by cell, for the reference's own check: a set of (i, j, len)."""
    t, p = list(t), list(p)
    hi = len(t) if hi is None else hi
    out = set()
    for i in range(len(p)):
        for j in range(lo, hi):
            if p[i] != t[j] or (i > 0 and j > lo and p[i - 1] == t[j - 1]):
                continue
            x = 0
            while i + x < len(p) and j + x < hi and p[i + x] == t[j + x]:
                x += 1
            if x >= L:
                out.add((i, j, x))
    return out


def triples(r, q=0):
    off, qpos, tpos, ln, _ = r
    return [(int(qpos[k]), int(tpos[k]), int(ln[k])) for k in range(off[q], off[q + 1])]


CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def codes(s):
    return np.array([CODE[c] for c in s], np.uint8)


ACGT2, CGTA = codes("ACGTACGT"), codes("CGTA")
ROWS = [  # text, query, L, keywords, expected (i, j, len) in order, flags
    (ACGT2, CGTA, 2, {}, [(0, 5, 3), (0, 1, 4)], 0),
    (ACGT2, CGTA, 2, dict(unique=True), [(0, 1, 4)], 0),
    (ACGT2, CGTA, 2, dict(max_hits=1), [], TRUNCATED),
    (ACGT2, CGTA, 1, {}, [(0, 5, 3), (0, 1, 4), (3, 0, 1)], 0),
    # the zero padding behind the text is 'A' and must not extend a match
    (codes("CGAAA"), codes("GAAAAA"), 2, {}, [(0, 1, 4), (1, 3, 2), (2, 2, 3), (3, 2, 3), (4, 2, 2)], 0),
    # two touching segments cut the match (0, 1, 4) in two; its second half is shorter than L
    (ACGT2, CGTA, 2, dict(layout=([0, 4], [4, 8])), [(0, 5, 3), (0, 1, 3)], 0),
    (ACGT2, CGTA, 1, dict(layout=([0, 4], [4, 8])), [(0, 5, 3), (0, 1, 3), (3, 4, 1), (3, 0, 1)], 0),
]


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_reference_rows(row):
    t, q, L, kw, exp, fl = ROWS[row]
    r = ref_mems(t, [q], L, **kw)
    assert triples(r) == exp and r[4].tolist() == [fl] and r[0].tolist() == [0, len(exp)]


def test_reference_equals_cell_by_cell_definition():
    rng = np.random.default_rng(5)
    for n, m, L, sigma in ((40, 17, 1, 2), (64, 64, 2, 2), (97, 33, 3, 4), (1, 1, 1, 1), (30, 50, 2, 2)):
        t, p = rng.integers(0, sigma, n).astype(np.uint8), rng.integers(0, sigma, m).astype(np.uint8)
        got = triples(ref_mems(t, [p], L))
        assert len(set(got)) == len(got) and set(got) == brute_mems(t, p, L), (n, m, L)
        lay = ([0, n // 3, n // 3 + 5], [n // 3, n // 3 + 2, n]) if n > 20 else None
        if lay:
            exp = set().union(*(brute_mems(t, p, L, lo, hi) for lo, hi in zip(*lay)))
            assert set(triples(ref_mems(t, [p], L, layout=lay))) == exp
    # one segment [0, n) is no layout; short and empty queries; several queries
    t = rng.integers(0, 2, 50).astype(np.uint8)
    qs = [t[3:20], np.zeros(0, np.uint8), t[:2], rng.integers(0, 2, 9).astype(np.uint8)]
    a, b = ref_mems(t, qs, 3), ref_mems(t, qs, 3, layout=([0], [50]))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[4].tolist() == [0, SHORT, SHORT, 0] and a[0][1] == a[0][2] == a[0][3]


def test_symbols_exported_and_bound():
    from sas_amd import _lib
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, nargs in (("sas_mems", 16), ("sas_mems_fixed", 15), ("sas_mems_verify_ms", 1)):
        assert name in declared and hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    assert L.sas_mems_verify_ms.restype == C.c_double
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    assert _lib.SAS_MEM_TRUNCATED == 1 and "#define SAS_MEM_TRUNCATED 1u" in src
    assert _lib.SAS_MEM_SHORT == 2 and "#define SAS_MEM_SHORT     2u" in src
    assert _lib.SAS_MEM_UNIQUE == 2 and "#define SAS_MEM_UNIQUE    (1u << 1)" in src
    # the call flag shares no bit with a flag the call accepts
    accepted = _lib.SAS_DEVICE_PTRS | _lib.SAS_LOCATE_U32 | _lib.SAS_VALIDATE | _lib.SAS_NO_PREFIX_TABLE
    assert _lib.SAS_MEM_UNIQUE & accepted == 0
