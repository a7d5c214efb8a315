#!/usr/bin/env python3
"""Writes tests/golden/cpp_api_cases.txt: the recorded answers that tests/cpp/test_calls.cpp compares
the C++ API's batched calls (include/sas.hpp) with on the GPU.

Every expected value comes from the numpy / Python references of the suite (the brute forces of
tests/test_gpu_*.py and the restatements of tests/test_*_host.py) and from the CPU oracle's suffix
array; no call of the library computes any of them.  Deterministic, no GPU.  Unlike make_golden.py
this script imports the repository's test modules: it records what the suite already trusts in a
form that a C++ program reads without a JSON library.

The format: `#` starts a comment; a record is a header line `name count` followed by `count`
unsigned decimal integers separated by whitespace.  Strings (cigars) are stored as their bytes,
one string per line (byte 10 ends each).  See RECORDS below for the names.

    python tests/golden/make_cpp_cases.py          # rewrite the fixture
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "suffix-array-searching_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from oracle import pyoracle as O  # noqa: E402
from test_align_host import DEL, EQ, INS, NONE_DIST, X, align_ref_all  # noqa: E402
from test_gpu_edit import LONG, SHORT, TRUNCATED, EBrute, edited, expected  # noqa: E402
from test_gpu_match import Brute  # noqa: E402
from test_gpu_mismatch import MBrute  # noqa: E402
from test_layout_host import SEQ_NONE, Layout, LBrute  # noqa: E402
from test_map_host import FIELDS as MAP_FIELDS, map_ref_all, revcomp_ref  # noqa: E402
from test_pairs_host import FIELDS as PAIR_FIELDS, pairs_ref_all  # noqa: E402
from test_rescue_host import FIELDS as RESCUE_FIELDS, MAP_RESCUED, PROPER, RESCUED, SKIPPED, rescue_ref_all  # noqa: E402

FIXTURE = os.path.join(HERE, "cpp_api_cases.txt")
MAX_BYTES = 256 * 1024

# the texts
N, BLOCK, COPIES, MUTATED = 1600, (200, 300), (700, 1200), (30, 70)
LN, SEQ_START, SEG_LO, SEG_HI = 900, (0, 300, 650, 900), (0, 300, 470, 650), (300, 450, 650, 900)
# the runs: name -> (k, max_seed_hits)
MM_RUNS = {"k0": (0, 0), "k2": (2, 0), "k2cap": (2, 2)}
ED_RUNS = {"k1": (1, 0), "k3": (3, 0), "k3cap": (3, 2)}
MAP_K, MAP_RUNS = 3, {"both": 3, "fwd": 1}          # name -> strands
FRAG = (50, 300)
PAIRS_K = 2
RESCUE_K, RESCUE_KR, RESCUE_ANCHORS = 1, 3, 4
LAY_K = 1


def make_text():
    """Random chars with t[200:300] planted again at 700 and, with two chars changed, at 1200: exact
    repeats, equally good places and a worse third place all exist."""
    t = O.random_string(N, seed=21).copy()
    blk = t[BLOCK[0]:BLOCK[1]].copy()
    t[COPIES[0]:COPIES[0] + 100] = blk
    blk[list(MUTATED)] = (blk[list(MUTATED)] + 1) & 3
    t[COPIES[1]:COPIES[1] + 100] = blk
    return t


def make_layout_text():
    """Three records; the second has a gap of N (code 0, in no segment) at [450, 470)."""
    t = O.random_string(LN, seed=22).copy()
    t[SEG_HI[1]:SEG_LO[2]] = 0
    return t


class Out:
    """The records in order; every value is checked to be an unsigned integer."""

    def __init__(self):
        self.rec = []

    def comment(self, text):
        self.rec.append(("#", text))

    def put(self, name, values):
        v = np.asarray(values).reshape(-1)
        v = v.astype(np.int64) if v.size else np.zeros(0, np.int64)
        assert (v >= 0).all(), name
        assert all(name != r[0] for r in self.rec), name
        self.rec.append((name, v))

    def batch(self, name, qs):
        self.put(name + ".qlen", [len(q) for q in qs])
        self.put(name + ".qbytes", np.concatenate([np.asarray(q, np.uint8) for q in qs] + [np.zeros(0, np.uint8)]))

    def strings(self, name, strs):
        self.put(name, np.frombuffer("".join(s + "\n" for s in strs).encode(), np.uint8))

    def text(self):
        lines = []
        for name, v in self.rec:
            if name == "#":
                lines.append("# " + v)
                continue
            lines.append(f"{name} {len(v)}")
            lines += [" ".join(str(int(x)) for x in v[i:i + 32]) for i in range(0, len(v), 32)]
        return "\n".join(lines) + "\n"


def cigar(row, nr):
    return "".join(f"{int(r) >> 2}{'=XID'[int(r) & 3]}" for r in row[:nr])


def u(a):
    return np.asarray(a, np.uint8)


def rnd(rng, m):
    return rng.integers(0, 4, m).astype(np.uint8)


def absent(rng, tb, m):
    """m random chars that occur nowhere in the text"""
    while True:
        q = rnd(rng, m)
        if tb.find(q.tobytes()) < 0:
            return q


# ---------------------------------------------------------------- the groups
def group_locate(out, t, br, rank, rng):
    n, tb = len(t), t.tobytes()
    qs = [t[50:70], t[210:225], t[240:252], t[235:275], absent(rng, tb, 20), t[n - 15:n], t[900:960], absent(rng, tb, 12)]
    occ = [sorted(br.occurrences(q.tobytes()), key=lambda p: rank[p]) for q in qs]
    cap = 2
    assert any(len(o) == 0 for o in occ) and any(len(o) >= 2 for o in occ) and any(len(o) > cap for o in occ)
    out.comment("locate: every occurrence (bytes.find) in SA rank order; locate.cap: max_per_query, then the capped answer")
    out.batch("locate", qs)
    for name, lists in (("locate", occ), ("locate.capped", [o[:cap] for o in occ])):
        out.put(name + ".off", np.concatenate([[0], np.cumsum([len(o) for o in lists])]))
        out.put(name + ".pos", [p for o in lists for p in o])
    out.put("locate.cap", [cap])
    none = [absent(rng, tb, m) for m in (12, 16, 31)]
    assert all(not br.occurrences(q.tobytes()) for q in none)
    out.comment("locate.none: a batch in which nothing occurs (the sizing call returns 0)")
    out.batch("locate.none", none)


def group_match(out, t, rng):
    n = len(t)
    b = Brute(t)
    part = np.concatenate([t[400:415], [(t[415] + 1) & 3], rnd(rng, 10)])
    qs = [t[100:130], part, np.zeros(0, np.uint8), rnd(rng, 25), t[220:250], t[n - 12:n],
          np.concatenate([t[n - 12:n], rnd(rng, 5)])]
    ans = [b.match(q.tobytes()) for q in qs]
    lens = [len(q) for q in qs]
    assert any(a[0] == m > 0 for a, m in zip(ans, lens)) and any(0 < a[0] < m for a, m in zip(ans, lens))
    assert any(m == 0 and a[0] == 0 and a[1] == n for a, m in zip(ans, lens))
    assert any(a[3] - a[2] >= 2 for a in ans)
    out.comment("match: test_gpu_match.Brute.match (len, pos, lo, hi)")
    out.batch("match", qs)
    for j, f in enumerate(("len", "pos", "lo", "hi")):
        out.put("match." + f, [a[j] for a in ans])


def subst(rng, q, places):
    q = q.copy()
    for j in places:
        q[j] = (q[j] + rng.integers(1, 4)) & 3
    return q


def group_mismatch(out, t, rng):
    n = len(t)
    mb = MBrute(t)
    qs = [t[60:80], subst(rng, t[330:350], [3]), subst(rng, t[420:453], [2, 20]), subst(rng, t[500:540], [1, 15, 30]),
          t[205:235], subst(rng, t[241:265], [4, 17]), t[n - 20:n], rnd(rng, 24), t[10:12], np.zeros(0, np.uint8),
          subst(rng, t[1000:1012], [11]), t[262:274]]
    out.comment("mismatch: test_gpu_mismatch.MBrute.answer; <run>.params = k, max_seed_hits")
    out.batch("mismatch", qs)
    seen = {}
    for run, (k, mh) in MM_RUNS.items():
        ans = [mb.answer(q, k, mh) for q in qs]
        out.put(f"mismatch.{run}.params", [k, mh])
        out.put(f"mismatch.{run}.off", np.concatenate([[0], np.cumsum([len(a[0]) for a in ans])]))
        out.put(f"mismatch.{run}.pos", [p for a in ans for p in a[0]])
        out.put(f"mismatch.{run}.dist", [d for a in ans for d in a[1]])
        out.put(f"mismatch.{run}.qflags", [a[2] for a in ans])
        seen[run] = ({d for a in ans for d in a[1]}, {a[2] for a in ans})
    assert {0, 2} <= seen["k2"][0] and 0 in seen["k0"][0] and any(f & TRUNCATED for f in seen["k2cap"][1])
    assert all(any(f & SHORT for f in s[1]) for s in seen.values())


def edit_queries(t, rng):
    n = len(t)

    def cut(s, m, ops=()):
        """m query chars: the text slice at s that the edits turn into m chars"""
        ln = m - sum(o[0] == "ins" for o in ops) + sum(o[0] == "del" for o in ops)
        q = edited(rng, t[s:s + ln], list(ops))
        assert len(q) == m
        return q

    return [cut(40, 20), cut(330, 20, [("sub", 7)]), cut(360, 20, [("ins", 11)]), cut(390, 20, [("del", 9)]),
            cut(420, 64, [("sub", 5), ("ins", 40)]), cut(500, 65, [("del", 20), ("sub", 50), ("ins", 60)]),
            cut(580, 100, [("ins", 30), ("del", 70)]), cut(820, 100), cut(900, 257), cut(n - 20, 20),
            cut(n - 30, 20, [("del", 10)]), cut(215, 20), cut(245, 64, [("sub", 31)]), rnd(rng, 20), rnd(rng, 1),
            rnd(rng, 3), cut(1010, 20, [("sub", 2), ("sub", 9), ("sub", 16)]), cut(1100, 24, [("sub", 3), ("del", 12), ("ins", 20), ("sub", 22)])]


def group_edit(out, t, br, rng):
    n = len(t)
    qs = edit_queries(t, rng)
    assert {20, 64, 65, 100, 257} <= {len(q) for q in qs}
    out.comment("edit: test_gpu_edit.expected over EBrute; <run>.params = k, max_seed_hits")
    out.batch("edit", qs)
    exp = {}
    for run, (k, mh) in ED_RUNS.items():
        e = exp[run] = expected(br, qs, k, mh)
        out.put(f"edit.{run}.params", [k, mh])
        for f in ("off", "end", "dist", "qflags"):
            out.put(f"edit.{run}.{f}", e[f])
        fl = e["qflags"].tolist()
        assert any(f & LONG for f in fl) and any(f & SHORT for f in fl) and (mh or n in e["end"].tolist()), run
    assert any(f & TRUNCATED for f in exp["k3cap"]["qflags"]) and {0, 3} <= set(exp["k3"]["dist"].tolist())
    return qs, exp


def put_aligned(out, name, got):
    start, dist, nruns, runs = got
    out.put(name + ".start", start)
    out.put(name + ".dist", dist)
    out.put(name + ".nruns", nruns)
    out.put(name + ".runs", runs)
    out.strings(name + ".cigar", [cigar(r, nr) for r, nr in zip(runs, nruns)])
    return {int(x) & 3 for r, nr in zip(runs, nruns) for x in r[:nr]}


def group_align(out, t, qs, exp):
    n = len(t)
    out.comment("align: test_align_host.align_ref_all of every end of the edit runs (runs: stride 2k + 1 per end)")
    ops = set()
    for run, (k, _) in ED_RUNS.items():
        e = exp[run]
        ops |= put_aligned(out, f"align.{run}", align_ref_all(t, qs, e["off"], e["end"], k))
    assert ops == {EQ, X, INS, DEL}
    out.comment("align.bad: a hand-made Edited (k = 1) whose second end has no alignment within k")
    q, off, end, k = [t[400:430]], [0, 2], [430, 900], 1
    got = align_ref_all(t, q, off, end, k)
    assert (got[0][1], got[1][1], got[2][1]) == (n, NONE_DIST, 0) and got[1][0] == 0
    out.batch("align.bad", q)
    out.put("align.bad.params", [k])
    out.put("align.bad.off", off)
    out.put("align.bad.end", end)
    put_aligned(out, "align.bad", got)


def put_mapped(out, name, ref, fields):
    for f in fields:
        out.put(f"{name}.{f}", ref[f])
    out.strings(name + ".cigar", [cigar(r, nr) for r, nr in zip(ref["runs"], ref["nruns"])])


def group_map(out, t, br, rng):
    n = len(t)
    rc = revcomp_ref
    qs = [t[60:100], rc(t[330:370]), edited(rng, t[420:460], [("sub", 5), ("del", 20)]),
          rc(edited(rng, t[500:545], [("ins", 9), ("sub", 30)])), rnd(rng, 40), t[205:228], rc(t[232:262]),
          t[215:255], t[n - 30:n], rc(t[0:30]), rnd(rng, 2)]
    rcs = [rc(q) for q in qs]
    k = MAP_K
    A = (br.answers(qs, k, 0), br.answers(rcs, k, 0))
    out.comment("map: test_map_host.map_ref_all; <run>.params = k, max_seed_hits, strands")
    out.batch("map", qs)
    refs = {}
    for run, strands in MAP_RUNS.items():
        r = refs[run] = map_ref_all(t, qs, k, A[0], A[1], strands)
        out.put(f"map.{run}.params", [k, 0, strands])
        put_mapped(out, f"map.{run}", r, MAP_FIELDS)
    b = refs["both"]
    assert (b["strand"] == 1).any() and (b["dist"] == NONE_DIST).any() and (b["n_best"] > 1).any()
    assert (b["n_loci"] > b["n_best"]).any() and not refs["fwd"]["strand"].any()
    assert ((b["dist"] != NONE_DIST) & (refs["fwd"]["dist"] == NONE_DIST)).any()


def mates(t, s, L, m1, m2):
    """a pair from the fragment t[s : s + L): mate 1 forward at its start, mate 2 reversed at its end"""
    return [t[s:s + m1].copy(), revcomp_ref(t[s + L - m2:s + L])]


def group_pairs(out, t, br, rng):
    k = PAIRS_K
    qs = []
    qs += mates(t, 330, 200, 35, 35)                                        # proper
    qs += mates(t, 40, 120, 30, 40)[::-1]                                   # proper, mate 2 forward
    qs += mates(t, 820, 600, 35, 35)                                        # too far apart
    qs += [t[560:595].copy(), revcomp_ref(t[720:755])]                      # mate 2 moves to the second copy
    qs += [t[200:230].copy(), revcomp_ref(t[262:290])]                      # inside the block: equally good pairs
    qs += [t[1400:1435].copy(), rnd(rng, 35)]                               # one mate unmapped
    qs += [t[1450:1480].copy(), t[1500:1530].copy()]                        # both forward
    m = mates(t, 1010, 150, 32, 32)
    qs += [edited(rng, m[0], [("sub", 10)]), edited(rng, m[1], [("del", 15)])]  # proper, with edits
    rcs = [revcomp_ref(q) for q in qs]
    A = (br.answers(qs, k, 0), br.answers(rcs, k, 0))
    single = map_ref_all(t, qs, k, A[0], A[1], 3)
    ref = pairs_ref_all(t, qs, k, A[0], A[1], FRAG[0], FRAG[1], base=single)
    out.comment("pairs: test_pairs_host.pairs_ref_all; params = k, max_seed_hits, min_frag, max_frag; "
                "pairs.single.* = map_edit's record of each read")
    out.batch("pairs", qs)
    out.put("pairs.params", [k, 0, FRAG[0], FRAG[1]])
    put_mapped(out, "pairs", ref, PAIR_FIELDS)
    put_mapped(out, "pairs.single", single, MAP_FIELDS)
    proper = ref["pflags"] == PROPER
    moved = [proper[i] and any(ref[f][r] != single[f][r] for r in (2 * i, 2 * i + 1) for f in ("end", "strand"))
             for i in range(len(proper))]
    assert proper.any() and (~proper).any() and any(moved) and (ref["n_best_pairs"] > 1).any()
    return qs, ref


def group_rescue(out, t, br, rng):
    k, kr = RESCUE_K, RESCUE_KR
    qs = []
    m = mates(t, 330, 200, 36, 36)
    qs += [m[0], edited(rng, m[1], [("sub", 6), ("sub", 20), ("sub", 31)])]      # mate 2 beyond k: rescued
    m = mates(t, 40, 150, 36, 36)
    qs += [edited(rng, m[0], [("sub", 8), ("del", 22)]), m[1]]                   # mate 1 beyond k: rescued
    qs += mates(t, 820, 180, 35, 35)                                             # proper: no rescue
    qs += [t[205:228].copy(), t[245:268].copy()]                                 # 6 loci on one strand: skipped
    qs += [t[1400:1435].copy(), rnd(rng, 35)]                                    # nothing in the window
    rcs = [revcomp_ref(q) for q in qs]
    A = (br.answers(qs, k, 0), br.answers(rcs, k, 0))
    ref = rescue_ref_all(t, qs, k, kr, A[0], A[1], FRAG[0], FRAG[1], RESCUE_ANCHORS)
    out.comment("rescue: test_rescue_host.rescue_ref_all; params = k, k_rescue, max_seed_hits, min_frag, max_frag, "
                "max_anchors (runs: stride 2 k_rescue + 1 per read)")
    out.batch("rescue", qs)
    out.put("rescue.params", [k, kr, 0, FRAG[0], FRAG[1], RESCUE_ANCHORS])
    put_mapped(out, "rescue", ref, RESCUE_FIELDS)
    assert kr > k and (ref["pflags"] & RESCUED).any() and (ref["pflags"] & SKIPPED).any() and (ref["n_rescue"] > 0).any()
    assert (((ref["qflags"] & MAP_RESCUED) != 0) & (ref["dist"] > k) & (ref["dist"] != NONE_DIST)).any()
    assert (ref["pflags"] == PROPER).any()


def group_layout(out, rng):
    t = make_layout_text()
    n = len(t)
    lay = Layout(SEQ_START, SEG_LO, SEG_HI)
    assert lay.n == n and len(SEQ_START) - 1 >= 3 and not t[SEG_HI[1]:SEG_LO[2]].any()
    lb, br = LBrute(t, lay), EBrute(t)
    k = LAY_K
    qs = [t[100:130], t[285:315], t[300:330], t[425:455], t[465:495], t[600:640], revcomp_ref(t[700:740]),
          edited(rng, t[500:530], [("sub", 12)]), revcomp_ref(t[280:310]), t[n - 25:n], t[636:664],
          np.zeros(24, np.uint8)]
    rcs = [revcomp_ref(q) for q in qs]
    out.comment("layout: a second text of three records with a gap of N; on = test_layout_host.LBrute, off = the "
                "plain references; edit.params = k, max_seed_hits; map.params = k, max_seed_hits, strands")
    out.put("layout.text", t)
    out.put("layout.seq_start", SEQ_START)
    out.put("layout.seg_lo", SEG_LO)
    out.put("layout.seg_hi", SEG_HI)
    out.batch("layout", qs)
    out.put("layout.edit.params", [k, 0])
    ans = [lb.edit(q, k, 0) for q in qs]
    on = dict(off=np.concatenate([[0], np.cumsum([len(a[0]) for a in ans])]), end=[e for a in ans for e in a[0]],
              dist=[d for a in ans for d in a[1]], qflags=[a[2] for a in ans])
    off = expected(br, qs, k, 0)
    for f in ("off", "end", "dist", "qflags"):
        out.put(f"layout.edit.on.{f}", on[f])
        out.put(f"layout.edit.off.{f}", off[f])
    gone = set(off["end"].tolist()) - set(on["end"])
    assert any(lay.seg_of_end(e) < 0 for e in gone), "an end in the gap"
    assert any(lay.seg_of_end(e) >= 0 for e in gone), "an end whose alignment crosses a record start"
    out.put("layout.map.params", [k, 0, 3])
    m_on = lb.map(qs, k, 0, 3)
    m_off = map_ref_all(t, qs, k, br.answers(qs, k, 0), br.answers(rcs, k, 0), 3)
    put_mapped(out, "layout.map.on", m_on, MAP_FIELDS)
    put_mapped(out, "layout.map.off", m_off, MAP_FIELDS)
    assert any(not np.array_equal(m_on[f], m_off[f]) for f in ("end", "dist"))
    pos = [0, 295, 299, 300, 455, 469, 470, 640, 649, 650, 899, 440]
    span = [10, 10, 1, 150, 5, 2, 180, 11, 0, 250, 1, 10]
    one = [lay.translate(p, 1) for p in pos]
    sp = [lay.translate(p, s) for p, s in zip(pos, span)]
    assert any(lay.seg_of_pos(p) < 0 and r[0] == SEQ_NONE for p, r in zip(pos, one))
    assert any(a[0] != SEQ_NONE and b[0] == SEQ_NONE for a, b in zip(one, sp))
    assert {r[0] for r in one} >= {0, 1, 2}
    out.put("layout.translate.pos", pos)
    out.put("layout.translate.span", span)
    for name, res in (("layout.translate.one", one), ("layout.translate.spans", sp)):
        out.put(name + ".seq", [r[0] for r in res])
        out.put(name + ".off", [r[1] for r in res])


def group_between(out, t, sa):
    tb = t.tobytes()
    suf = [(tb[i:], int(i)) for i in sa]
    assert all(suf[i][0] < suf[i + 1][0] for i in range(len(suf) - 1))
    pairs = [(u([1, 0, 2, 3]), u([1, 0, 3, 1])), (t[500:520], np.concatenate([t[500:512], u([3])])),
             (u([2, 2]), u([1, 3]))]
    res = [[p for s, p in suf if a.tobytes() <= s < b.tobytes()] for a, b in pairs]
    assert len(res[0]) >= 2 and len(res[1]) >= 1 and res[2] == [] and pairs[2][0].tobytes() > pairs[2][1].tobytes()
    out.comment("between: search_between(a, b) of the query pairs (0, 1), (2, 3), (4, 5): the suffixes sorted in "
                "bytes order with a <= s < b, as CSR")
    out.batch("between", [x for ab in pairs for x in ab])
    out.put("between.off", np.concatenate([[0], np.cumsum([len(r) for r in res])]))
    out.put("between.pos", [p for r in res for p in r])


def generate() -> str:
    rng = np.random.default_rng(20240)
    t = make_text()
    assert 1000 <= len(t) <= 2000
    sa = O.build_sa(t).astype(np.int64)
    rank = np.empty(len(t), np.int64)
    rank[sa] = np.arange(len(t))
    br = EBrute(t)
    out = Out()
    out.comment("Recorded answers for tests/cpp/test_calls.cpp, written by tests/golden/make_cpp_cases.py from the")
    out.comment("suite's CPU references.  A record: `name count`, then count unsigned integers.  Do not edit.")
    out.put("text", t)
    group_locate(out, t, br, rank, rng)
    group_match(out, t, rng)
    group_mismatch(out, t, rng)
    qs, exp = group_edit(out, t, br, rng)
    group_align(out, t, qs, exp)
    group_map(out, t, br, rng)
    group_pairs(out, t, br, rng)
    group_rescue(out, t, br, rng)
    group_layout(out, rng)
    group_between(out, t, sa)
    text = out.text()
    assert len(text.encode()) <= MAX_BYTES, len(text)
    return text


if __name__ == "__main__":
    data = generate()
    with open(FIXTURE, "w", newline="\n") as f:
        f.write(data)
    print(f"{FIXTURE}: {len(data)} bytes")
