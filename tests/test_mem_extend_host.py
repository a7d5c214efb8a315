"""The scalar steps of the maximal-exact-match extension on the CPU (no GPU):
tests/cpp/mem_extend_check.cpp drives the functions k_mem_verify calls (csrc/mem_extend.hpp: the
first differing char of two packed words within a bound, one extension step, one char of the packed
text) beside char-by-char loops: every bound 0..32, differences behind the bound, runs around the
32-char word edges at unaligned text positions, and zero padding behind the bound."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "mem_extend_check.cpp")


def test_mem_extend_cpu(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "mem_extend_check"
    subprocess.run([hipcc, "-O2", "-std=c++17", SRC, "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "mem extend ok" in r.stdout
