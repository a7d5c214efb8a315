#!/usr/bin/env python3
"""Writes tests/golden/cpp_mems_cases.txt: the recorded answers that tests/cpp/mems/test_mems.cpp
compares sas::SaNaive::mems (include/sas.hpp) with on the GPU.

Every expected value comes from tests/test_mems_host.ref_mems, the diagonal-run reference, and the
CPU oracle's suffix array; no call of the library computes any of them.  Deterministic, no GPU.

The format is that of cpp_api_cases.txt: `#` starts a comment; a record is a header line
`name count` followed by `count` unsigned decimal integers separated by whitespace.

    python tests/golden/make_cpp_mems_cases.py          # rewrite the fixture
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "suffix-array-searching_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from oracle import pyoracle as O  # noqa: E402
from test_mems_host import Text, ref_mems  # noqa: E402

FIXTURE = os.path.join(HERE, "cpp_mems_cases.txt")
MAX_BYTES = 64 * 1024
N, BLOCK, COPY = 1200, (100, 180), 700
SEG_LO, SEG_HI, SEQ_START = (0, 400, 720), (400, 700, 1200), (0, 400, 1200)
UNIQUE = 1 << 1  # SAS_MEM_UNIQUE
# name -> (min_len, max_hits, flags, layout)
RUNS = {"l12": (12, 0, 0, False), "l5cap": (5, 4, 0, False), "l12unique": (12, 0, UNIQUE, False),
        "l12layout": (12, 0, 0, True), "l40": (40, 0, 0, False)}


def make_text():
    """Random chars with t[100:180] planted again at 700: a match that occurs twice."""
    t = O.random_string(N, seed=23).copy()
    t[COPY:COPY + BLOCK[1] - BLOCK[0]] = t[BLOCK[0]:BLOCK[1]]
    return t


def make_queries(t):
    rng = np.random.default_rng(8)
    q = t[90:200].copy()  # the planted block with its own flanks: the longer match is unique
    r = t[300:520].copy()  # across the touching segments at 400
    r[[33, 98, 163]] = (r[[33, 98, 163]] + 1) & 3  # matches of 33, 64, 64 and 56 chars
    return [q, r, t[690:790].copy(), t[N - 45:].copy(), t[:30].copy(), rng.integers(0, 4, 60).astype(np.uint8),
            t[5:16].copy(), np.zeros(0, np.uint8), t[110:170].copy()]


def generate() -> str:
    t = make_text()
    T = Text(t)
    qs = make_queries(t)
    lines = ["# written by tests/golden/make_cpp_mems_cases.py from tests/test_mems_host.ref_mems; do not edit"]

    def put(name, values):
        v = np.asarray(values).reshape(-1).astype(np.int64) if len(values) else np.zeros(0, np.int64)
        assert (v >= 0).all(), name
        lines.append(f"{name} {len(v)}")
        for a in range(0, len(v), 32):
            lines.append(" ".join(str(int(x)) for x in v[a:a + 32]))

    put("text", t)
    put("qlen", [len(q) for q in qs])
    put("qbytes", np.concatenate(qs))
    put("layout.seq_start", SEQ_START)
    put("layout.seg_lo", SEG_LO)
    put("layout.seg_hi", SEG_HI)
    put("runs", [len(RUNS)])
    for name, (L, mh, fl, lay) in RUNS.items():
        r = ref_mems(T, qs, L, max_hits=mh, unique=bool(fl & UNIQUE), layout=(SEG_LO, SEG_HI) if lay else None)
        put(f"{name}.params", [L, mh, fl, int(lay)])
        for field, v in zip(("off", "qpos", "tpos", "len", "qflags"), r):
            put(f"{name}.{field}", v)
    text = "\n".join(lines) + "\n"
    assert len(text) <= MAX_BYTES
    return text


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(generate())
    print(f"wrote {FIXTURE}")
