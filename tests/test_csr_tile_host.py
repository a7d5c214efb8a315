"""The tile-owner scalars of the output-centric tiled kernels on the CPU (no GPU):
tests/cpp/csr_tile_check.cpp drives the functions the kernels call (csrc/csr_tile.hpp: the owner of
an element in the whole offset array, the slice of a tile, the clamp of an offset to a tile-relative
u32, the staged and the unstaged bisect) at T = 8, SLICE = 4 beside a linear scan: empty owners at
the front, the middle and the end, a tile inside one owner, slices of exactly SLICE and SLICE + 1
owners, a last partial tile, offsets at and beyond 2^32, v at and past the total."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "csr_tile_check.cpp")


def test_csr_tile_owner_cpu(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "csr_tile_check"
    subprocess.run([hipcc, "-O2", "-std=c++17", SRC, "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "csr tile ok" in r.stdout
