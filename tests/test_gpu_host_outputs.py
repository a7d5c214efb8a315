"""The host-pointer path of the mapping calls (sas_map_edit, sas_map_pairs, sas_map_pairs_rescue): one
stager copies the queries in and one list of device twins carries the outputs back, so what is
asserted here holds for every call that goes through them.  On host pointers, with u64 and with u32
positions, for ragged queries that overlap in the caller's bytes with an empty read among them:
every optional output passed as NULL in turn leaves the others equal to those of the call with all
outputs (and writes nothing behind any of them), and those equal the device-pointer call's.

The case is small: a 4096-char text with a planted repeat, 8 pairs of 24-char mates, k = 1,
k_rescue = 2, max_frag - min_frag = 64."""
import numpy as np
import pytest

from oracle import pyoracle as O
from sas_amd import _lib
from test_gpu_edit import BUILDS
from test_map_host import revcomp_ref

pytestmark = pytest.mark.gpu

N, M, K, K_RESCUE, FRAG, MAX_ANCHORS, CANARY = 4096, 24, 1, 2, (96, 160), 4, 64
MAP_OUT = ("end", "start", "dist", "strand", "n_best", "n_loci", "nruns", "runs", "qflags")
PAIR_OUT = MAP_OUT + ("pflags", "n_pairs", "n_best_pairs")
RESCUE_OUT = PAIR_OUT + ("n_rescue",)
REQUIRED = ("end", "dist")


def make_case():
    """The text, and 16 reads as (offset, length) slices of one byte buffer in no order."""
    t = O.random_string(N, seed=41).copy()
    t[3000:3200] = t[500:700]  # the planted repeat: a read from it has two loci

    def sub(q, *at):
        q = q.copy()
        for i in at:
            q[i] = (q[i] + 1) & 3
        return q

    def pair(s, L, e1=(), e2=()):
        return sub(t[s:s + M], *e1), sub(revcomp_ref(t[s + L - M:s + L]), *e2)

    pairs = [pair(100, 120), pair(112, 110),        # their first mates t[100 .. 124) and t[112 .. 136) overlap
             pair(1500, 160, e2=(20,)),
             pair(520, 130),                        # both mates in the repeat: two proper candidates
             pair(2000, 128, e2=(3, 17)),           # two substitutions: no seed of k = 1 holds, rescued
             pair(2400, 140, e1=(2, 12)),
             pair(3500, 400),                       # too far apart: no proper pair
             (t[700:700 + M].copy(), np.zeros(0, np.uint8))]  # an empty read
    reads = [r for p in pairs for r in p]
    # reads 0 and 2 are bytes 0 .. 24 and 12 .. 36 of one slice of the caller's buffer
    head = t[100:136]
    chunks, qoff = [head], {0: 0, 2: 12}
    at = len(head)
    for i in reversed(range(len(reads))):  # the other reads back to front: offsets in no order
        if i in qoff:
            continue
        qoff[i] = at if len(reads[i]) else 7  # the empty read points into the middle
        chunks.append(reads[i])
        at += len(reads[i])
    qb = np.concatenate(chunks).astype(np.uint8)
    off = np.array([qoff[i] for i in range(len(reads))], np.uint64)
    ln = np.array([len(r) for r in reads], np.uint32)
    for i, r in enumerate(reads):
        assert np.array_equal(qb[int(off[i]):int(off[i]) + int(ln[i])], r)
    assert off[2] < off[0] + ln[0] and int(ln.sum()) > len(qb) and (ln == 0).sum() == 1
    return t, qb, off, ln


def shapes(fields, nq, kr, u32):
    pos = np.uint32 if u32 else np.uint64
    per_read = dict(end=pos, start=pos, dist=np.uint8, strand=np.uint8, n_best=np.uint32, n_loci=np.uint32,
                    nruns=np.uint8, qflags=np.uint8)
    per_pair = dict(pflags=np.uint8, n_pairs=np.uint32, n_best_pairs=np.uint32, n_rescue=np.uint32)
    out = {}
    for f in fields:
        if f == "runs":
            out[f] = (nq * (2 * kr + 1), np.uint16)
        elif f in per_read:
            out[f] = (nq, per_read[f])
        else:
            out[f] = (nq // 2, per_pair[f])
    return out


def call(torch, idx, what, q, device, u32, skip=()):
    """One call on host or device pointers into buffers with CANARY elements behind every output; the
    outputs named in `skip` are passed as NULL.  Returns a dict of int64 arrays (None: skipped)."""
    qb, qoff, qlen = q
    nq = len(qoff)
    fields = dict(map=MAP_OUT, pairs=PAIR_OUT, rescue=RESCUE_OUT)[what]
    shape = shapes(fields, nq, K_RESCUE if what == "rescue" else K, u32)
    if device:
        tdt = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint16: torch.int16, np.uint8: torch.uint8}
        buf = {f: torch.full((cnt + CANARY,), 77, dtype=tdt[dt], device="cuda") for f, (cnt, dt) in shape.items()}
        keep = [torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda(),
                torch.from_numpy(qlen.astype(np.int32)).cuda()]
        qp = [a.data_ptr() for a in keep]
        ptr = [None if f in skip else buf[f].data_ptr() for f in fields]
        st = torch.cuda.current_stream().cuda_stream
    else:
        buf = {f: np.full(cnt + CANARY, 77, dt) for f, (cnt, dt) in shape.items()}
        qp = [qb.ctypes.data, qoff.ctypes.data, qlen.ctypes.data]
        ptr = [None if f in skip else buf[f].ctypes.data for f in fields]
        st = None
    fl = (_lib.SAS_DEVICE_PTRS if device else 0) | (_lib.SAS_LOCATE_U32 if u32 else 0)
    L = _lib.lib()
    if what == "map":
        _lib.check(L.sas_map_edit(idx._h, *qp, nq, K, 0, _lib.SAS_MAP_FWD | _lib.SAS_MAP_REV, *ptr, st, fl))
    elif what == "pairs":
        _lib.check(L.sas_map_pairs(idx._h, *qp, nq // 2, K, 0, FRAG[0], FRAG[1], *ptr, st, fl))
    else:
        _lib.check(L.sas_map_pairs_rescue(idx._h, *qp, nq // 2, K, K_RESCUE, 0, FRAG[0], FRAG[1], MAX_ANCHORS, *ptr, st,
                                          fl))
    torch.cuda.synchronize()
    out = {}
    for f, (cnt, _) in shape.items():
        b = buf[f].cpu().numpy() if device else buf[f]
        assert (b[0 if f in skip else cnt:] == 77).all(), (what, f, "written past the output, or a NULL output")
        out[f] = None if f in skip else b[:cnt].astype(np.int64) & (0xFFFF if f == "runs" else -1)
    return out


def same(got, ref, what):
    for f, v in got.items():
        if v is not None:
            assert np.array_equal(v, ref[f]), (what, f, v, ref[f])


@pytest.fixture(scope="module")
def setup():
    import sas_amd
    t, qb, qoff, qlen = make_case()
    return sas_amd.SaNaive.build(t, **BUILDS["quad_p8"]), (qb, qoff, qlen), len(t)


@pytest.mark.parametrize("what", ["map", "pairs", "rescue"])
def test_host_outputs_null_in_turn(setup, what):
    import torch
    idx, q, n = setup
    for u32 in (False, True):
        dev = call(torch, idx, what, q, True, u32)
        full = call(torch, idx, what, q, False, u32)
        same(full, dev, (what, u32, "host against device pointers"))
        optional = [f for f in full if f not in REQUIRED]
        for skip in [(f,) for f in optional] + [tuple(optional)]:
            got = call(torch, idx, what, q, False, u32, skip)
            assert all((got[f] is None) == (f in skip) for f in got)
            same(got, full, (what, u32, skip))
        # the case is none of the trivial ones: the empty read is unmapped (end = n), the others are
        # mapped, on both strands, and there are pairs of every kind
        lens = q[2].astype(np.int64)
        assert (full["end"][lens == 0] == n).all() and (full["end"][lens > 0] < n).sum() >= 12
        assert set(full["strand"][lens > 0].tolist()) == {0, 1} and (full["nruns"] > 1).any()
        if what != "map":
            proper = full["pflags"] & _lib.SAS_PAIR_PROPER
            assert proper.any() and not proper.all() and (full["n_pairs"] > 1).any()
        if what == "rescue":
            assert (full["pflags"] & _lib.SAS_PAIR_RESCUED).any() and full["n_rescue"].any()
            assert (full["qflags"] & _lib.SAS_MAP_RESCUED).any()
