"""sas::SaNaive::mems (include/sas.hpp) run on the GPU by tests/cpp/mems/test_mems.cpp in a fresh
process: every field of its result struct, element for element, against the answers that
tests/golden/make_cpp_mems_cases.py recorded on the CPU from the diagonal-run reference
(tests/test_cpp_mems_host.py keeps the file and the generator together), the empty batch and the
refusal of min_len == 0."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "tests", "cpp", "mems", "test_mems")
FIXTURE = os.path.join(REPO, "tests", "golden", "cpp_mems_cases.txt")


@pytest.mark.gpu
def test_cpp_mems_on_gpu():
    assert os.path.exists(EXE), "build() compiles tests/cpp/mems/test_mems"
    r = subprocess.run([EXE, FIXTURE], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "mems ok" in r.stdout
