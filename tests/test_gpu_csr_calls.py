"""The calls that return per-query lists (sas_locate, sas_locate_mismatch, sas_locate_edit, sas_mems
and their _fixed forms) go through one two-pass call path on host pointers.  What the tests of the
single calls do not state is pinned here, on one table: the return code and the full text of
sas_last_error() of the sizing call, of a capacity one below the total, of a batch that finds
nothing and of a null out_off / out_total.  A call that succeeds leaves the last error as it was.

The case is small and this file's own (make_case), since it needs fixed-length queries that serve the
ragged and the _fixed forms alike and one query no window of which occurs: a 4096-char text with a
planted repeat, as test_gpu_host_outputs.py builds it, 8 queries of 24 chars of which one occurs
nowhere, k = 1, L = 8.  The index builds are test_gpu_mismatch.py's.  The texts, totals and offsets
in FAMILY rest on the library alone: they were recorded from it before the calls were given their
common path (the totals agree with the host references of test_gpu_mismatch.py, test_gpu_edit.py
and test_mems_host.py, which is not asserted here)."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O
from sas_amd import _lib
from test_gpu_mismatch import BUILDS

pytestmark = pytest.mark.gpu

N, M, NQ, K, MIN_LEN, CANARY = 4096, 24, 8, 1, 8, 77

# family: (total of the batch, noun and sizing hint of the ENOSPC text, payload dtypes, offsets)
FAMILY = {
    "locate": (8, "positions", "out_pos", (np.uint64,), [0, 1, 3, 5, 5, 5, 5, 6, 8]),
    "mismatch": (10, "positions", "out_pos", (np.uint64, np.uint8), [0, 1, 3, 5, 6, 7, 7, 8, 10]),
    "edit": (26, "ends", "out_end", (np.uint64, np.uint8), [0, 3, 9, 15, 16, 17, 17, 20, 26]),
    "mems": (13, "matches", "the outputs", (np.uint32, np.uint64, np.uint32), [0, 1, 3, 6, 9, 10, 10, 11, 13]),
}
CALLS = [(fam, fixed) for fam in FAMILY for fixed in (False, True)]
ROWS = ("sizing", "total_minus_1", "nothing", "null_off", "null_total")


def fn_name(fam, fixed):
    base = {"locate": "sas_locate", "mismatch": "sas_locate_mismatch", "edit": "sas_locate_edit", "mems": "sas_mems"}
    return base[fam] + ("_fixed" if fixed else "")


def occurs(tb: bytes, q: np.ndarray, L: int) -> bool:
    return any(tb.find(q[i:i + L].tobytes()) >= 0 for i in range(len(q) - L + 1))


def make_case():
    """The text, the 8 queries as one byte buffer of 24-char rows, and a query none of whose 8-char
    windows occurs in the text (so no call finds anything for it: every seed is longer)."""
    t = O.random_string(N, seed=41).copy()
    t[3000:3200] = t[500:700]  # the planted repeat: a query from it occurs twice
    tb = t.tobytes()
    rng = np.random.default_rng(5)
    nowhere = rng.integers(0, 4, M).astype(np.uint8)
    while occurs(tb, nowhere, MIN_LEN):
        nowhere = rng.integers(0, 4, M).astype(np.uint8)
    qs = [t[s:s + M].copy() for s in (100, 520, 640, 1500, 2000, 2400, 3100)]
    qs[3][7] = (qs[3][7] + 1) & 3   # one substitution: k = 1 finds it, the exact calls its halves
    qs[4][20] = (qs[4][20] + 2) & 3
    qs.insert(5, nowhere)
    assert len(qs) == NQ
    return t, np.concatenate(qs), nowhere


@pytest.fixture(scope="module")
def setup():
    import sas_amd
    t, qb, nowhere = make_case()
    return sas_amd.SaNaive.build(t, **BUILDS["quad_p8"]), qb, np.concatenate([nowhere, nowhere])


def run(idx, fam, fixed, qb, capacity, off=True, total=True, payload=True):
    """One host-pointer call; payload arrays of `capacity` + 8 canaries (NULL without `payload`).
    Returns (rc, the last error's text, out_off, *out_total, the payload arrays)."""
    L = _lib.lib()
    nq = len(qb) // M
    qoff = np.arange(nq, dtype=np.uint64) * M
    qlen = np.full(nq, M, np.uint32)
    queries = (qb.ctypes.data, M, nq) if fixed else (qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, nq)
    out_off = np.full(nq + 1, CANARY, np.uint64)
    tot = C.c_uint64(CANARY)
    pay = [np.full(capacity + 8, CANARY, dt) for dt in FAMILY[fam][3]]
    pp = [a.ctypes.data if payload else None for a in pay]
    po = out_off.ctypes.data if off else None
    pt = C.byref(tot) if total else None
    f = getattr(L, fn_name(fam, fixed))
    if fam == "locate":
        rc = f(idx._h, *queries, 0, po, pp[0], capacity, pt, None, 0)
    elif fam == "mems":
        rc = f(idx._h, *queries, MIN_LEN, 0, po, pp[0], pp[1], pp[2], None, capacity, pt, None, 0)
    else:
        rc = f(idx._h, *queries, K, 0, po, pp[0], pp[1], None, capacity, pt, None, 0)
    return rc, L.sas_last_error().decode(), out_off, tot.value, pay


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("fam,fixed", CALLS)
def test_csr_call_row(setup, fam, fixed, row):
    idx, qb, nothing = setup
    fn = fn_name(fam, fixed)
    want, noun, hint, _, offsets = FAMILY[fam]
    enospc = "[%d] %s: %d %s, capacity %%d (size %s from *out_total and call again)" % (errno.ENOSPC, fn, want, noun,
                                                                                        hint)
    # a known last error, so that a call which succeeds can be seen to leave it alone
    rc, before, _, _, _ = run(idx, fam, fixed, qb, 0, off=False)
    print(fam, fixed, row, "null out_off:", rc, repr(before))
    assert rc == errno.EINVAL and before == "[%d] %s: null argument" % (errno.EINVAL, fn)
    if row == "null_off":
        return
    if row == "null_total":
        if fam == "locate":  # its out_total is optional: the call answers as with it
            rc, msg, off, _, _ = run(idx, fam, fixed, qb, 0, total=False, payload=False)
            print(fam, fixed, row, rc, repr(msg), off.tolist())
            assert rc == errno.ENOSPC and msg == enospc % 0 and off.tolist() == offsets
            return
        rc, msg, off, _, _ = run(idx, fam, fixed, qb, 0, total=False, payload=False)
        print(fam, fixed, row, rc, repr(msg))
        assert rc == errno.EINVAL and msg == before and (off == CANARY).all()
        return
    if row == "nothing":
        rc, msg, off, tot, pay = run(idx, fam, fixed, nothing, 4)
        print(fam, fixed, row, rc, repr(msg), off.tolist(), tot)
        assert rc == 0 and msg == before and tot == 0 and not off.any()
        assert all((a == CANARY).all() for a in pay)
        return
    assert want > 1  # a capacity of want - 1 is a capacity
    cap = 0 if row == "sizing" else want - 1
    rc, msg, off, tot, pay = run(idx, fam, fixed, qb, cap, payload=row != "sizing")
    print(fam, fixed, row, rc, repr(msg), off.tolist(), tot)
    assert rc == errno.ENOSPC and msg == enospc % cap
    assert tot == want and off.tolist() == offsets and offsets[-1] == want
    assert offsets[5] == offsets[6]  # the query that occurs nowhere
    assert all((a == CANARY).all() for a in pay)  # nothing copied
