"""The recorded answers of the C++ API's batched calls (tests/golden/cpp_api_cases.txt; no kernel is
launched): the committed file is what tests/golden/make_cpp_cases.py writes, byte for byte; parsed
on its own, it holds the cases in which a wrapper of include/sas.hpp can go wrong (an absent and a
repeated query, a truncating cap, every flag, both strands, a moved mate, a rescued one, a gap, ...);
and tests/cpp/test_calls builds and reads every record of it (`--parse`).  tests/test_cpp_calls.py
runs the calls against it on the GPU."""
import importlib.util
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
FIXTURE = os.path.join(REPO, "tests", "golden", "cpp_api_cases.txt")
MAX_BYTES = 256 * 1024
NONE_DIST, SEQ_NONE = 255, 0xFFFFFFFF
TRUNCATED, SHORT, LONG = 1, 2, 4                       # SAS_MM_* / SAS_ED_*
PROPER, RESCUED, SKIPPED, MAP_RESCUED = 1, 2, 4, 8     # SAS_PAIR_* and SAS_MAP_RESCUED


def parse(data: str) -> dict:
    """`#` starts a comment; a record is `name count` and count unsigned decimal integers."""
    tok = " ".join(line.split("#", 1)[0] for line in data.splitlines()).split()
    rec, i = {}, 0
    while i < len(tok):
        name, count = tok[i], int(tok[i + 1])
        assert not name.isdigit() and name not in rec, name
        vals = tok[i + 2:i + 2 + count]
        assert len(vals) == count and all(v.isdigit() for v in vals), name
        rec[name] = [int(v) for v in vals]
        i += 2 + count
    return rec


@pytest.fixture(scope="module")
def rec():
    with open(FIXTURE, newline="") as f:
        return parse(f.read())


def queries(rec, name):
    out, at = [], 0
    for m in rec[name + ".qlen"]:
        out.append(bytes(rec[name + ".qbytes"][at:at + m]))
        at += m
    assert at == len(rec[name + ".qbytes"])
    return out


def rows(rec, name, field):
    """the CSR record name.field, per query"""
    off = rec[name + ".off"]
    assert off[0] == 0 and off[-1] == len(rec[f"{name}.{field}"])
    return [rec[f"{name}.{field}"][a:b] for a, b in zip(off, off[1:])]


def ops(rec, name, stride):
    nruns, runs = rec[name + ".nruns"], rec[name + ".runs"]
    assert len(runs) == len(nruns) * stride
    return {runs[a * stride + i] & 3 for a in range(len(nruns)) for i in range(nruns[a])}


def test_fixture_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_cpp_cases", os.path.join(REPO, "tests", "golden",
                                                                                 "make_cpp_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(FIXTURE, "rb") as f:
        committed = f.read()
    assert gen.generate().encode() == committed, "run python tests/golden/make_cpp_cases.py"
    assert gen.MAX_BYTES == MAX_BYTES


def test_size_and_texts(rec):
    assert os.path.getsize(FIXTURE) <= MAX_BYTES
    assert 1000 <= len(rec["text"]) <= 2000 and max(rec["text"]) <= 3
    t = bytes(rec["text"])
    blk = t[200:300]
    assert t.count(blk) >= 2 and len(blk) == 100, "the planted block"


def test_locate_cases(rec):
    t = bytes(rec["text"])
    full, capped = rows(rec, "locate", "pos"), rows(rec, "locate.capped", "pos")
    cap = rec["locate.cap"][0]
    assert len(full) == len(capped) == len(rec["locate.qlen"])
    assert any(len(o) == 0 for o in full) and any(len(o) >= 2 for o in full)
    assert cap > 0 and any(len(c) < len(o) for c, o in zip(capped, full))
    assert all(c == o[:cap] for c, o in zip(capped, full))
    for q, o in zip(queries(rec, "locate"), full):
        assert all(t[p:p + len(q)] == q for p in o) and len(o) == sum(t.startswith(q, i) for i in range(len(t)))
    none = queries(rec, "locate.none")
    assert none and all(q and t.find(q) < 0 for q in none)


def test_match_cases(rec):
    n, m = len(rec["text"]), rec["match.qlen"]
    ln, pos = rec["match.len"], rec["match.pos"]
    assert len(ln) == len(pos) == len(rec["match.lo"]) == len(rec["match.hi"]) == len(m)
    assert any(a == b > 0 for a, b in zip(ln, m)) and any(0 < a < b for a, b in zip(ln, m))
    assert any(b == 0 and a == 0 and p == n for a, b, p in zip(ln, m, pos))


def test_mismatch_cases(rec):
    ks, flags, capped_flags = set(), [], []
    for run in ("k0", "k2", "k2cap"):
        k, mh = rec[f"mismatch.{run}.params"]
        ks.add(k)
        fl = rec[f"mismatch.{run}.qflags"]
        assert len(fl) == len(rec["mismatch.qlen"]) and len(rows(rec, f"mismatch.{run}", "pos")) == len(fl)
        dist = rec[f"mismatch.{run}.dist"]
        assert len(dist) == len(rec[f"mismatch.{run}.pos"]) and {0, k} <= set(dist) and max(dist) <= k
        flags += fl
        capped_flags += fl if mh else []
    assert ks == {0, 2}
    assert any(f & SHORT for f in flags) and any(f & TRUNCATED for f in capped_flags)


def test_edit_and_align_cases(rec):
    n = len(rec["text"])
    assert {20, 64, 65, 100, 257} <= set(rec["edit.qlen"])
    ks, seen_ops = set(), set()
    for run in ("k1", "k3", "k3cap"):
        k, mh = rec[f"edit.{run}.params"]
        ks.add(k)
        fl, end = rec[f"edit.{run}.qflags"], rec[f"edit.{run}.end"]
        assert len(fl) == len(rec["edit.qlen"]) and len(rows(rec, f"edit.{run}", "end")) == len(fl)
        assert len(rec[f"edit.{run}.dist"]) == len(end)
        assert any(f & LONG for f in fl) and any(f & SHORT for f in fl)
        assert (n in end) if not mh else any(f & TRUNCATED for f in fl)
        # every end of the run has its alignment
        for f in ("start", "dist", "nruns"):
            assert len(rec[f"align.{run}.{f}"]) == len(end)
        assert rec[f"align.{run}.dist"] == rec[f"edit.{run}.dist"]
        seen_ops |= ops(rec, f"align.{run}", 2 * k + 1)
        assert rec[f"align.{run}.cigar"].count(10) == len(end)
    assert ks == {1, 3} and seen_ops == {0, 1, 2, 3}
    # the hand-made Edited: an end without an alignment within k
    assert rec["align.bad.off"] == [0, 2] and rec["align.bad.start"][1] == n
    assert rec["align.bad.dist"][1] == NONE_DIST and rec["align.bad.nruns"][1] == 0
    k = rec["align.bad.params"][0]
    assert not any(rec["align.bad.runs"][2 * k + 1:]) and rec["align.bad.dist"][0] <= k


def test_map_cases(rec):
    n = len(rec["text"])
    assert rec["map.both.params"][2] == 3 and rec["map.fwd.params"][2] == 1
    b, f = ({x: rec[f"map.{run}.{x}"] for x in ("end", "start", "dist", "strand", "n_best", "n_loci", "nruns")}
            for run in ("both", "fwd"))
    nq = len(rec["map.qlen"])
    assert all(len(v) == nq for v in list(b.values()) + list(f.values()))
    assert any(s == 1 and d != NONE_DIST for s, d in zip(b["strand"], b["dist"])) and not any(f["strand"])
    unmapped = [i for i in range(nq) if b["dist"][i] == NONE_DIST]
    assert unmapped and all(b["end"][i] == b["start"][i] == n and b["n_best"][i] == 0 and b["nruns"][i] == 0
                            for i in unmapped)
    assert any(x > 1 for x in b["n_best"]) and any(x > y for x, y in zip(b["n_loci"], b["n_best"]))


def test_pairs_cases(rec):
    k, _, lo, hi = rec["pairs.params"]
    assert lo <= hi
    np_ = len(rec["pairs.qlen"]) // 2
    pf = rec["pairs.pflags"]
    assert len(pf) == len(rec["pairs.n_pairs"]) == len(rec["pairs.n_best_pairs"]) == np_
    assert PROPER in pf and 0 in pf and any(x > 1 for x in rec["pairs.n_best_pairs"])
    moved = [i for i in range(np_) if pf[i] == PROPER and any(
        rec[f"pairs.{f}"][r] != rec[f"pairs.single.{f}"][r] for r in (2 * i, 2 * i + 1) for f in ("end", "strand"))]
    assert moved, "a mate that pairing moves away from its single-read winner"
    for i in range(np_):  # a proper pair: one mate on each strand, the fragment inside the window
        if pf[i] == PROPER:
            f, v = (2 * i, 2 * i + 1) if rec["pairs.strand"][2 * i] == 0 else (2 * i + 1, 2 * i)
            assert (rec["pairs.strand"][f], rec["pairs.strand"][v]) == (0, 1)
            assert lo <= rec["pairs.end"][v] - rec["pairs.end"][f] + rec["pairs.qlen"][f] <= hi


def test_rescue_cases(rec):
    k, kr, _, lo, hi, anchors = rec["rescue.params"]
    assert kr > k and anchors > 0
    pf, qf, dist = rec["rescue.pflags"], rec["rescue.qflags"], rec["rescue.dist"]
    assert len(rec["rescue.runs"]) == len(qf) * (2 * kr + 1)
    assert any(p & RESCUED for p in pf) and any(p & SKIPPED for p in pf) and PROPER in pf
    assert any(q & MAP_RESCUED and k < d != NONE_DIST for q, d in zip(qf, dist))
    assert any(x > 0 for x in rec["rescue.n_rescue"]) and len(rec["rescue.n_rescue"]) == len(pf)


def test_layout_cases(rec):
    t, ss = rec["layout.text"], rec["layout.seq_start"]
    lo, hi = rec["layout.seg_lo"], rec["layout.seg_hi"]
    n = len(t)
    assert len(ss) - 1 >= 3 and ss[0] == 0 and ss[-1] == n and len(lo) == len(hi)
    covered = set().union(*(range(a, b) for a, b in zip(lo, hi)))
    gap = [p for p in range(n) if p not in covered]
    assert gap and all(t[p] == 0 for p in gap) and all(ss[0] < p < ss[-1] and p not in ss for p in gap)

    def seg_of_end(e):
        return any(a < e <= b for a, b in zip(lo, hi))
    on, off = set(rec["layout.edit.on.end"]), set(rec["layout.edit.off.end"])
    gone = off - on
    assert any(not seg_of_end(e) for e in gone), "an end in the gap"
    assert any(seg_of_end(e) for e in gone), "an end whose alignment crosses a record start or the gap"
    assert any(rec[f"layout.map.on.{f}"] != rec[f"layout.map.off.{f}"] for f in ("end", "dist"))
    pos, span = rec["layout.translate.pos"], rec["layout.translate.span"]
    one, sp = rec["layout.translate.one.seq"], rec["layout.translate.spans.seq"]
    assert any(p in gap and s == SEQ_NONE for p, s in zip(pos, one))
    assert any(a != SEQ_NONE and b == SEQ_NONE and w > 1 for a, b, w in zip(one, sp, span))
    assert set(range(len(ss) - 1)) <= set(one)
    for p, s, o in zip(pos, one, rec["layout.translate.one.off"]):
        assert o == (p if s == SEQ_NONE else p - ss[s])


def test_between_cases(rec):
    t = bytes(rec["text"])
    qs = queries(rec, "between")
    got = rows(rec, "between", "pos")
    assert len(qs) == 6 and len(got) == 3
    suf = sorted(range(len(t)), key=lambda i: t[i:])
    for (a, b), g in zip(zip(qs[0::2], qs[1::2]), got):
        assert g == [i for i in suf if a <= t[i:] < b]
    assert qs[4] > qs[5] and got[2] == [] and len(got[0]) >= 2


def test_test_calls_builds_and_reads_the_fixture(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP])
    exe = os.path.join(CPP, "test_calls")
    assert os.access(exe, os.X_OK)
    r = subprocess.run([exe, "--parse", FIXTURE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "parse ok" in r.stdout, r.stderr[-3000:]
    # the reader notices a fixture that does not fit together: a record cut short, a missing one
    with open(FIXTURE) as f:
        lines = f.read().splitlines()
    at = lines.index(next(ln for ln in lines if ln.startswith("map.both.n_loci ")))
    for name, broken in (("short", lines[:at + 1] + lines[at + 2:]), ("missing", lines[:at] + lines[at + 2:])):
        p = tmp_path / (name + ".txt")
        p.write_text("\n".join(broken) + "\n")
        r = subprocess.run([exe, "--parse", str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (name, r.stdout, r.stderr[-1000:])
