"""The bisect step of k_sa_quad_llcp's walk on the CPU (no GPU): tests/cpp/qllcp_bisect_check.cpp
drives the function the kernel calls (csrc/qllcp_bisect.hpp) with 32-bit ranks beside a plain
64-bit restatement of binary_search (sas/sa_search.rs:98-112) at sa_n = 2^31 - 1, 2^31,
2^31 + 12345, 2^32 - 5 and 2^32 - 1, with [L0, U) at the bottom, in the middle, across 2^31 and in
the SA's top 1, 2, 100 and 12345 ranks: the same mids, the same final rank, at most 34 steps.  A
32-bit l + r fails it (the program caps the loop that the kernel would never leave)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "qllcp_bisect_check.cpp")


def test_quad_llcp_bisect_cpu(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "qllcp_bisect_check"
    subprocess.run([hipcc, "-O2", "-std=c++17", SRC, "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "qllcp bisect ok" in r.stdout
