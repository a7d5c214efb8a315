"""CPU checks of the k-difference locate boundary (no kernel is launched): the calls are declared,
exported and bound with the declared signatures; a null index is refused before any device
call; the brute-force reference of tests/test_gpu_edit.py agrees with a plain nested-loop dynamic
program, with the oracle at k = 0 and with sas.h's seed-and-window argument on the golden
definition texts; and the C++ mirror (sas::SaNaive::locate_edit) compiles warning-free."""
import ctypes as C
import errno
import json
import os
import subprocess

import numpy as np

from oracle import pyoracle as O
from sas_amd import _lib
from test_gpu_edit import EBrute, LONG, SHORT, TRUNCATED, edited

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, max_seed_hits, out_off, out_end, out_dist, out_qflags, capacity, out_total, stream, flags
TAIL = [U32, U64, VP, VP, VP, VP, U64, VP, VP, U32]
SIGNATURES = {
    "sas_locate_edit": [VP, VP, VP, VP, U64] + TAIL,
    "sas_locate_edit_fixed": [VP, VP, U32, U64] + TAIL,
}


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert "sas_locate_edit_verify_ms" in declared and hasattr(raw, "sas_locate_edit_verify_ms")
    assert L.sas_locate_edit_verify_ms.restype == C.c_double
    assert "sas_tile_grid_cap" in declared and hasattr(raw, "sas_tile_grid_cap")
    assert L.sas_tile_grid_cap.restype == U32 and list(L.sas_tile_grid_cap.argtypes) == []
    assert (_lib.SAS_ED_TRUNCATED, _lib.SAS_ED_SHORT, _lib.SAS_ED_LONG) == (1, 2, 4) == (TRUNCATED, SHORT, LONG)
    # the header's parameter lists, type by type, and its flag values
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    for line in ("#define SAS_ED_TRUNCATED 1u", "#define SAS_ED_SHORT     2u", "#define SAS_ED_LONG      4u",
                 "#define SAS_ED_MAX_M     256u"):
        assert line in src, line
    ctype = {"const sas_index*": VP, "const uint8_t*": VP, "const uint64_t*": VP, "const uint32_t*": VP,
             "uint8_t*": VP, "uint64_t*": VP, "void*": VP, "uint64_t": U64, "uint32_t": U32}
    for name, sig in SIGNATURES.items():
        params = src.split("int " + name + "(")[1].split(")")[0]
        types = [" ".join(p.split()[:-1]) for p in params.replace("\n", " ").split(",")]
        assert [ctype[t] for t in types] == sig, (name, types)


def test_null_index_refused_before_any_device_call():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    for rc in (L.sas_locate_edit(None, p, p, p, 1, 1, 0, p, None, None, None, 0, p, None, 0),
               L.sas_locate_edit_fixed(None, p, 4, 1, 1, 0, p, None, None, None, 0, p, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()


def sellers_loops(t, q):
    """D(e) for every e in [0, n], cell by cell: rows = query chars, columns = ends; row 0 is 0."""
    n, m = len(t), len(q)
    prev = [0] * (n + 1)
    for i in range(1, m + 1):
        cur = [i] * (n + 1)
        for e in range(1, n + 1):
            best = prev[e - 1] + (1 if q[i - 1] != t[e - 1] else 0)
            for other in (prev[e] + 1, cur[e - 1] + 1):
                if other < best:
                    best = other
            cur[e] = best
        prev = cur
    return prev


def windows_union(br, q, k):
    """sas.h's seed-and-window argument: every occurrence pv of every piece j proposes the ends
    in [s0 + m - k, s0 + m + k], clamped to [0, n], whose free-start distance over the window
    t[max(0, s0 - 2k) .. min(n, s0 + m + k)) is <= k (s0 = pv - b_j).  Returns {end: distance} and
    asserts that equal ends never get different distances."""
    t, n, m = br.t, br.n, len(q)
    b = [j * m // (k + 1) for j in range(k + 2)]
    out = {}
    for j in range(k + 1):
        for pv in br.occurrences(q[b[j]:b[j + 1]].tobytes()):
            s0 = pv - b[j]
            w0, w1 = max(0, s0 - 2 * k), min(n, s0 + m + k)
            D = EBrute(t[w0:w1]).rows([q])[0] if w1 > w0 else np.array([m])
            for e in range(max(s0 + m - k, w0, 0), min(s0 + m + k, w1) + 1):
                d = int(D[e - w0])
                if d <= k:
                    assert out.setdefault(e, d) == d, (q, k, e)
    return out


def test_brute_force_agrees_with_the_definition_texts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(0)
    checked = looped = unions = 0
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        br = EBrute(t)
        sa = np.array(c["sa"], np.uint32)
        tp = O.padded(t)
        qs = [np.array(qd["q"], np.uint8) for qd in c["queries"]]
        qs += [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(0, 9, 10)]
        kinds = ("sub", "ins", "del")
        for i in range(0, n, max(n // 12, 1)):  # text slices with 1..3 edits
            ops = [(kinds[int(rng.integers(0, 3))], int(rng.integers(0, 1 << 20))) for _ in range(1 + i % 3)]
            qs.append(edited(rng, t[i:i + 9 + i % 7], ops))
        qs.append(np.tile(t, 2)[:257] if n >= 129 else np.zeros(257, np.uint8))
        for q in qs:
            m = len(q)
            D = br.rows([q])[0] if m else np.zeros(n + 1, np.int64)
            if m * (n + 1) <= 20000:  # the plain loops, where they take no time
                assert D.tolist() == sellers_loops(t.tolist(), q.tolist()), (c["name"], q)
                looped += 1
            # k = 0: the prefix range of the oracle, through the golden SA, as ascending ends
            ends, dist, fl, info = br.answer(q, 0, 0, D)
            if m == 0:
                assert (ends, fl) == ([], SHORT)
            elif m > 256:
                assert (ends, fl) == ([], LONG) and br.answer(q, 3, 0)[2] == LONG
                continue
            else:
                lo, hi = O.prefix_range(tp, n, sa, q)
                assert ends == sorted((sa[lo:hi].astype(np.int64) + m).tolist()) and not any(dist) and fl == 0
                assert info["cand"] == hi - lo
            for k in (1, 2, 3):
                ends, dist, fl, info = br.answer(q, k, 0, D)
                if m <= k:
                    assert (ends, fl) == ([], SHORT)
                    continue
                # unflagged: the seeded definition is the full k-difference answer
                full = br.full(q, k, D)
                assert fl == 0 and dict(zip(ends, dist)) == full and ends == sorted(full), (c["name"], q, k)
                # a capped run keeps exactly the ends near an occurrence of a piece that stays
                cends, cdist, cfl, cinfo = br.answer(q, k, 3, D)
                assert set(cends) <= set(ends) and (cfl == TRUNCATED) == (cinfo["cand"] < info["cand"])
                if cfl == 0:
                    assert cends == ends
                if info["cand"] <= 40:  # the candidates' windows propose exactly the answer
                    assert windows_union(br, q, k) == full, (c["name"], q, k)
                    unions += 1
            checked += 1
    assert checked > 200 and looped > 200 and unions > 200, (checked, looped, unions)


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const sas::SaNaive::Edited r = idx.locate_edit({s.slice(0, 30), s.slice(5, 50)}, 2);
    const sas::SaNaive::Edited c = idx.locate_edit({s}, 1, 1024, SAS_NO_PREFIX_TABLE);
    return (int)(r.off.size() + r.end[0] + r.dist[0] + (r.qflags[1] & (SAS_ED_TRUNCATED | SAS_ED_SHORT | SAS_ED_LONG)) +
                 c.end.size());
}
"""


def test_cpp_locate_edit_compiles(tmp_path):
    src = tmp_path / "edit.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
