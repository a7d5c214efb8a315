"""CPU checks of the k-mismatch locate boundary (no kernel is launched): the calls are declared,
exported and bound with the declared signatures; a null index is refused before any device
call; the brute-force reference of tests/test_gpu_mismatch.py agrees with the oracle and with a
plain double loop on the golden definition texts; and the C++ mirror
(sas::SaNaive::locate_mismatch) compiles warning-free."""
import ctypes as C
import errno
import json
import os
import subprocess

import numpy as np

from oracle import pyoracle as O
from sas_amd import _lib
from test_gpu_mismatch import MBrute, SHORT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
# k, max_seed_hits, out_off, out_pos, out_dist, out_qflags, capacity, out_total, stream, flags
TAIL = [U32, U64, VP, VP, VP, VP, U64, VP, VP, U32]
SIGNATURES = {
    "sas_locate_mismatch": [VP, VP, VP, VP, U64] + TAIL,
    "sas_locate_mismatch_fixed": [VP, VP, U32, U64] + TAIL,
}


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    assert (_lib.SAS_MM_TRUNCATED, _lib.SAS_MM_SHORT) == (1, 2)
    # the header's parameter lists, type by type, and its flag values
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    assert "#define SAS_MM_TRUNCATED 1u" in src and "#define SAS_MM_SHORT     2u" in src
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
    for rc in (L.sas_locate_mismatch(None, p, p, p, 1, 1, 0, p, None, None, None, 0, p, None, 0),
               L.sas_locate_mismatch_fixed(None, p, 4, 1, 1, 0, p, None, None, None, 0, p, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()


def hamming_double_loop(t, q, k):
    """Every alignment of distance <= k, char by char."""
    n, m = len(t), len(q)
    out = {}
    for s in range(0, n - m + 1):
        d = 0
        for j in range(m):
            d += int(t[s + j] != q[j])
        if d <= k:
            out[s] = d
    return out


def test_brute_force_agrees_with_the_definition_texts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(0)
    checked = 0
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        br = MBrute(t)
        sa = np.array(c["sa"], np.uint32)
        assert np.array_equal(np.argsort(br.rank), sa), c["name"]
        tp = O.padded(t)
        qs = [np.array(qd["q"], np.uint8) for qd in c["queries"]]
        qs += [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(0, 9, 30)]
        for i in range(0, n, max(n // 15, 1)):
            q = t[i:i + 7].copy()
            if len(q):
                q[int(rng.integers(0, len(q)))] ^= 1
            qs.append(q)
        for q in qs:
            # k = 0: the prefix range of the oracle, expanded through the golden SA, in SA order
            pos, dist, fl, cand = br.answer(q, 0, 0)
            if len(q) == 0:
                assert (pos, fl) == ([], SHORT)
            else:
                lo, hi = O.prefix_range(tp, n, sa, q)
                assert pos == sa[lo:hi].tolist() and not any(dist) and fl == 0 and cand == hi - lo, (c["name"], q)
            # k = 1: exactly the alignments of the double loop, each once, with its distance
            pos, dist, fl, _ = br.answer(q, 1, 0)
            if len(q) <= 1:
                assert (pos, fl) == ([], SHORT)
            else:
                ref = hamming_double_loop(t, q, 1)
                assert len(pos) == len(set(pos)) and dict(zip(pos, dist)) == ref and fl == 0, (c["name"], q)
            checked += 1
    assert checked > 200


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const sas::SaNaive::Mismatched r = idx.locate_mismatch({s.slice(0, 30), s.slice(5, 50)}, 2);
    const sas::SaNaive::Mismatched c = idx.locate_mismatch({s}, 1, 1024, SAS_NO_PREFIX_TABLE);
    return (int)(r.off.size() + r.pos[0] + r.dist[0] + (r.qflags[1] & SAS_MM_TRUNCATED) + c.pos.size());
}
"""


def test_cpp_locate_mismatch_compiles(tmp_path):
    src = tmp_path / "mismatch.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
