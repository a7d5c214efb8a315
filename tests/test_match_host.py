"""CPU checks of the longest-prefix match boundary (no kernel is launched): the three calls are
declared, exported and bound with the declared signatures; the brute-force reference of
tests/test_gpu_match.py agrees with the oracle on the golden definition texts; and the C++
mirror (sas::SaNaive::match) compiles warning-free."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from oracle import pyoracle as O
from sas_amd import _lib
from test_gpu_match import Brute, lcp_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
OUTS = [VP, VP, VP, VP, VP, U32]  # out_len, out_pos, out_lo, out_hi, stream, flags
SIGNATURES = {
    "sas_match": [VP, VP, VP, VP, U64] + OUTS,
    "sas_match_fixed": [VP, VP, U32, U64] + OUTS,
    "sas_match_stats": [VP, VP, U64, U32] + OUTS,
}


def test_symbols_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, sig in SIGNATURES.items():
        assert name in declared and hasattr(raw, name), name
        assert list(getattr(L, name).argtypes) == sig, name
    # the header's parameter lists, type by type
    src = open(os.path.join(REPO, "include", "sas.h")).read()
    ctype = {"const sas_index*": VP, "const uint8_t*": VP, "const uint64_t*": VP, "const uint32_t*": VP,
             "uint32_t*": VP, "uint64_t*": VP, "void*": VP, "uint64_t": U64, "uint32_t": U32}
    for name, sig in SIGNATURES.items():
        params = src.split("int " + name + "(")[1].split(")")[0]
        types = [" ".join(p.split()[:-1]) for p in params.replace("\n", " ").split(",")]
        assert [ctype[t] for t in types] == sig, (name, types)


def test_null_arguments_refused_before_any_device_call():
    import errno
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    for rc in (L.sas_match(None, p, p, p, 1, p, p, None, None, None, 0),
               L.sas_match_fixed(None, p, 4, 1, p, p, None, None, None, 0),
               L.sas_match_stats(None, p, 4, 4, p, p, None, None, None, 0)):
        assert rc == errno.EINVAL and b"null index" in L.sas_last_error()


def test_brute_force_agrees_with_the_oracle_on_the_definition_texts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sa_definition.json")))["cases"]
    rng = np.random.default_rng(0)
    checked = 0
    for c in cases:
        t = np.array(c["text"], np.uint8)
        n = len(t)
        br = Brute(t)
        assert br.sa.tolist() == c["sa"], c["name"]
        tp = O.padded(t)
        sa = np.array(c["sa"], np.uint32)
        qs = [np.array(qd["q"], np.uint8) for qd in c["queries"]]
        qs += [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(0, 12, 40)]
        qs += [np.concatenate([t[i:i + 6], rng.integers(0, 4, 2).astype(np.uint8)]) for i in range(0, n, max(n // 20, 1))]
        for q in qs:
            ln, pos, lo, hi = br.match(q.tobytes())
            lb = O.lower_bound_rank(tp, n, sa, q)
            a = lcp_of(q.tobytes(), br.suf[lb - 1]) if lb > 0 else 0
            b = lcp_of(q.tobytes(), br.suf[lb]) if lb < n else 0
            assert ln == max(a, b), (c["name"], q.tolist())
            assert (lo, hi) == ((0, n) if ln == 0 else O.prefix_range(tp, n, sa, q[:ln])), (c["name"], q.tolist())
            assert ln == 0 or t[pos:pos + ln].tolist() == q[:ln].tolist()
            checked += 1
    assert checked > 300


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // compiled, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const sas::SaNaive::Matched r = idx.match({s.slice(0, 3), s.slice(5, 5), s.slice(10, 40)});
    return (int)(r.len.size() + r.pos[0] + r.lo[1] + r.hi[2] + idx.match({s}, false).lo.size());
}
"""


def test_cpp_match_compiles(tmp_path):
    src = tmp_path / "match.cpp"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(REPO, "include"), str(src)])
