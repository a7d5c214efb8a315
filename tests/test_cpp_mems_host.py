"""The recorded answers of the C++ mems test, checked without a GPU: the committed file is what
tests/golden/make_cpp_mems_cases.py writes, byte for byte; it holds the cases in which the wrapper
can go wrong (a match that occurs twice, a unique run that drops it, a capped run with a truncated
query, a layout that cuts a match, a short and an empty query); and tests/cpp/mems/test_mems
builds and reads every record of it (`--parse`).  tests/test_cpp_mems.py runs it on the GPU."""
import importlib.util
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp", "mems")
FIXTURE = os.path.join(REPO, "tests", "golden", "cpp_mems_cases.txt")
TRUNCATED, SHORT = 1, 2


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_cpp_mems_cases",
                                                  os.path.join(REPO, "tests", "golden", "make_cpp_mems_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    out, tok = {}, []
    for line in open(FIXTURE):
        tok += line.split("#")[0].split()
    i = 0
    while i < len(tok):
        name, count = tok[i], int(tok[i + 1])
        out[name] = [int(x) for x in tok[i + 2:i + 2 + count]]
        i += 2 + count
    return out


def test_fixture_is_what_the_generator_writes(gen):
    with open(FIXTURE, "rb") as f:
        committed = f.read()
    assert gen.generate().encode() == committed, "run python tests/golden/make_cpp_mems_cases.py"
    assert len(committed) <= gen.MAX_BYTES


def test_cases(rec, gen):
    runs = [k[:-7] for k in rec if k.endswith(".params")]
    assert rec["runs"] == [len(runs)] and set(runs) == set(gen.RUNS)
    nq = len(rec["qlen"])
    t = bytes(rec["text"])
    for run in runs:
        L, mh, fl, lay = rec[f"{run}.params"]
        off = rec[f"{run}.off"]
        assert len(off) == nq + 1 and len(rec[f"{run}.qflags"]) == nq
        assert all(len(rec[f"{run}.{f}"]) == off[-1] for f in ("qpos", "tpos", "len")) and off[-1] > 0
        assert all(bool(f & SHORT) == (m < L) for f, m in zip(rec[f"{run}.qflags"], rec["qlen"]))
        q0 = bytes(rec["qbytes"][:rec["qlen"][0]])
        for i, j, ln in zip(rec[f"{run}.qpos"][:off[1]], rec[f"{run}.tpos"][:off[1]], rec[f"{run}.len"][:off[1]]):
            assert ln >= L and q0[i:i + ln] == t[j:j + ln]
    plain, uniq = rec["l12.len"], rec["l12unique.len"]
    assert 0 < len(uniq) < len(plain)                      # the planted block occurs twice
    assert rec["l12layout.len"] != plain                   # the layout cuts a match
    assert any(f & TRUNCATED for f in rec["l5cap.qflags"]) and any(f == 0 for f in rec["l5cap.qflags"])
    assert any(f & SHORT for f in rec["l12.qflags"]) and 0 in rec["qlen"]
    assert {33, 64} <= set(plain)


def test_program_reads_the_fixture():
    subprocess.run(["make", "-s", "-C", CPP], check=True, capture_output=True, timeout=300)
    r = subprocess.run([os.path.join(CPP, "test_mems"), "--parse", FIXTURE], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "mems fixture ok" in r.stdout
