"""The batched calls of the C++ host API (include/sas.hpp: set_layout / translate, locate, match,
locate_mismatch, locate_edit, align_edit, map_edit, map_pairs, map_pairs_rescue, search_between,
cigar, read_fasta_file) run on the GPU by tests/cpp/test_calls.cpp, one group per test, each in a
fresh process.  The program compares every field of every result struct, element for element, with
the answers that tests/golden/make_cpp_cases.py recorded on the CPU from the suite's numpy
references (tests/test_cpp_cases_host.py keeps the file and the generator together), and checks the
empty batch and the argument errors of each call."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "tests", "cpp", "test_calls")
FIXTURE = os.path.join(REPO, "tests", "golden", "cpp_api_cases.txt")
GROUPS = ("locate", "match", "mismatch", "edit", "align", "map", "pairs", "rescue", "layout", "misc")


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_cpp_calls_on_gpu(group, tmp_path):
    assert os.path.exists(EXE), "build() compiles tests/cpp/test_calls"
    r = subprocess.run([EXE, group, FIXTURE, str(tmp_path)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"{group} ok" in r.stdout
