"""Batched locate (sas_locate_offsets / sas_locate_fill / sas_locate / sas_locate_fixed and
SaNaive.locate*): every occurrence position of every query in CSR form, against the CPU
oracle's suffix array (O.build_sa, not the GPU-built one).  Synthetic rank ranges drive the
fill kernel with shapes a search rarely produces (long runs of empty queries, ranges around
every tile size, a total past 2^32 into a small buffer); shards emit only their share; the
end-to-end calls agree on host and device pointers and with the oracle's prefix ranges."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

N = 200_003
BUILDS = {
    "u32": dict(),
    "sa40": dict(sa40=True),
    "tagged": dict(tagged=True),
    "tag_lines": dict(tagged=True, tag_lines=True),
}
PLAIN = dict(lcp=False, stree=False, sector=False, quad=False, llcp=False)


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@pytest.fixture(scope="module")
def text():
    t = O.random_string(N, seed=9)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def sa(text):
    s = O.build_sa(text).astype(np.int64)
    s.setflags(write=False)
    return s


def expected(sa, lo, hi, max_per_query=0, rank_lo=0, rank_hi=None):
    """(off, pos) of the ranges [lo, hi) clipped to [rank_lo, rank_hi), by definition."""
    rank_hi = len(sa) if rank_hi is None else rank_hi
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    l, h = np.maximum(lo, rank_lo), np.minimum(hi, rank_hi)
    c = np.where((hi >= lo) & (h > l), h - l, 0)
    if max_per_query:
        c = np.minimum(c, max_per_query)
    off = np.zeros(len(lo) + 1, np.int64)
    np.cumsum(c, out=off[1:])
    ranks = np.repeat(l - off[:-1], c) + np.arange(off[-1])
    return off, sa[ranks]


def synthetic_cases():
    rng = np.random.default_rng(5)
    cases = {}
    lo = rng.integers(0, N - 70, 5000)
    cases["cycle_0_70"] = (lo, lo + np.arange(5000) % 71)
    lo = rng.integers(0, N, 1000)
    cases["all_empty"] = (lo, lo.copy())
    e1, e2, e3 = rng.integers(0, N, 50_000), rng.integers(0, N, 50_000), rng.integers(0, N, 1000)
    lo = np.concatenate([e1, [777], e2, [50_001], [N - 1], e3])
    hi = np.concatenate([e1, [780], e2, [150_001], [N], e3])
    cases["empties_3_empties_100000_1_empties"] = (lo, hi)
    lens = np.array([T + d for T in (256, 1024, 2048, 4096, 8192) for d in (-1, 0, 1, T + 1)])
    lo = rng.integers(0, N - 2 * 8192 - 1, len(lens))
    cases["tile_edges"] = (lo, lo + lens)
    cases["whole_sa"] = (np.array([0]), np.array([N]))
    cases["reversed_and_clipped"] = (np.array([100, N - 10, N + 5, 5, 0, 60_000]),
                                     np.array([50, N + 1000, N + 10, 5, 3, 59_999]))
    return cases


def run_ranges(torch, idx, lo, hi, mpq, u32, total):
    """locate_ranges into a buffer over-allocated by 64 all-ones elements."""
    dlo, dhi = torch.from_numpy(lo.astype(np.int64)).cuda(), torch.from_numpy(hi.astype(np.int64)).cuda()
    out = torch.full((total + 64,), -1, dtype=torch.int32 if u32 else torch.int64, device="cuda")
    off, pos = idx.locate_ranges(dlo, dhi, max_per_query=mpq, out=out, u32=u32)
    torch.cuda.synchronize()
    assert pos.data_ptr() == out.data_ptr()
    got = out.cpu().numpy()
    got = got.view(np.uint32).astype(np.int64) if u32 else got
    return off.cpu().numpy(), got[:total], out[total:].cpu().numpy()


@pytest.mark.parametrize("u32", [False, True], ids=["u64", "u32"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_synthetic_ranges(sas, text, sa, build, u32):
    import torch
    idx = sas.SaNaive.build(text, **{**PLAIN, **BUILDS[build]})
    for name, (lo, hi) in synthetic_cases().items():
        for mpq in (0, 1, 7):
            eoff, epos = expected(sa, lo, hi, mpq)
            off, pos, canary = run_ranges(torch, idx, lo, hi, mpq, u32, int(eoff[-1]))
            assert np.array_equal(off, eoff), (name, mpq)
            assert np.array_equal(pos, epos), (name, mpq)
            assert (canary == -1).all(), (name, mpq)
    # without out= the total is read back and pos is exactly that long
    lo, hi = synthetic_cases()["cycle_0_70"]
    eoff, epos = expected(sa, lo, hi)
    off, pos = idx.locate_ranges(torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), u32=u32)
    got = pos.cpu().numpy()
    assert np.array_equal(got.view(np.uint32).astype(np.int64) if u32 else got, epos)
    assert np.array_equal(off.cpu().numpy(), eoff)


def test_partition_prepass_and_in_block_search_agree(sas, text, sa):
    """SAS_LOCATE_NO_PARTITION (each workgroup bisects for its tiles' first queries) gives the
    same bytes as the partition pre-pass."""
    import torch
    from sas_amd import _lib
    idx = sas.SaNaive.build(text, **PLAIN)
    for name, (lo, hi) in synthetic_cases().items():
        eoff, epos = expected(sa, lo, hi)
        out = torch.full((len(epos) + 64,), -1, dtype=torch.int64, device="cuda")
        off, _ = idx.locate_ranges(torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), out=out,
                                   flags=_lib.SAS_LOCATE_NO_PARTITION)
        got = out.cpu().numpy()
        assert np.array_equal(off.cpu().numpy(), eoff), name
        assert np.array_equal(got[:len(epos)], epos) and (got[len(epos):] == -1).all(), name


def test_capacity_and_64_bit_total(sas, text, sa):
    import torch
    idx = sas.SaNaive.build(text, **PLAIN)
    nq, cap = 25_000, 1 << 20
    lo = torch.zeros(nq, dtype=torch.int64, device="cuda")
    hi = torch.full((nq,), N, dtype=torch.int64, device="cuda")
    for u32 in (False, True):
        out = torch.full((cap + 64,), -1, dtype=torch.int32 if u32 else torch.int64, device="cuda")
        off, pos = idx.locate_ranges(lo, hi, out=out, capacity=cap, u32=u32)
        torch.cuda.synchronize()
        off = off.cpu().numpy()
        assert off[nq] == nq * N > 1 << 32
        assert np.array_equal(off, np.arange(nq + 1, dtype=np.int64) * N)
        got = out.cpu().numpy()
        head = got[:cap].view(np.uint32).astype(np.int64) if u32 else got[:cap]
        assert np.array_equal(head, np.tile(sa, cap // N + 1)[:cap])
        assert (got[cap:] == -1).all()


def test_shards_emit_their_share(sas, text, sa):
    import torch
    rng = np.random.default_rng(6)
    lo = rng.integers(0, N - 70, 5000)
    hi = lo + np.arange(5000) % 71
    lo[100], hi[100] = 40_000, 160_000  # a large range that two cuts fall into
    cuts = [0, 31_111, 90_001, N]
    whole = sas.SaNaive.build(text, **PLAIN)
    dlo, dhi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    woff, wpos = (x.cpu().numpy() for x in whole.locate_ranges(dlo, dhi))
    eoff, epos = expected(sa, lo, hi)
    assert np.array_equal(woff, eoff) and np.array_equal(wpos, epos)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        sh = sas.SaNaive.build(text, sa=sa.astype(np.uint32), rank_range=(a, b), **PLAIN)
        off, pos = (x.cpu().numpy() for x in sh.locate_ranges(dlo, dhi))
        soff, spos = expected(sa, lo, hi, rank_lo=a, rank_hi=b)
        assert np.array_equal(off, soff) and np.array_equal(pos, spos), (a, b)
        parts.append((off, pos))
    for k in range(len(lo)):
        cat = np.concatenate([pos[off[k]:off[k + 1]] for off, pos in parts])
        assert np.array_equal(cat, wpos[woff[k]:woff[k + 1]]), k


def pack(qs):
    lens = np.array([len(q) for q in qs], np.uint32)
    off = np.zeros(len(qs), np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.concatenate([np.asarray(q, np.uint8) for q in qs] + [np.zeros(64, np.uint8)]), off, lens


def as_i64(x, u32=False):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return x.view(np.uint32).astype(np.int64) if (u32 and x.dtype == np.int32) else x.astype(np.int64)


E2E_BUILDS = {
    "quad_prefix8_inline2": dict(lcp=False, stree=False, sector=False, llcp=False, prefix=8, prefix_inline=2),
    "sector_only": dict(lcp=False, stree=False, sector=True, quad=False, llcp=False, prefix=False),
}


@pytest.mark.parametrize("build", list(E2E_BUILDS))
@pytest.mark.parametrize("which", ["random", "period_7"])
def test_end_to_end(sas, text, sa, which, build):
    import torch
    rng = np.random.default_rng(7)
    if which == "random":
        t, tsa = text, sa
    else:
        t = np.tile(rng.integers(0, 4, 7, dtype=np.uint8), 20_000)
        tsa = O.build_sa(t).astype(np.int64)
    n = len(t)
    idx = sas.SaNaive.build(t, **E2E_BUILDS[build])
    qs = [t[o:o + l] for o, l in zip(rng.integers(0, n - 300, 800), rng.integers(0, 301, 800))]
    qs += [rng.integers(0, 4, rng.integers(0, 41), dtype=np.uint8) for _ in range(300)]
    qs += [np.zeros(0, np.uint8), np.full(200, 3, np.uint8)]
    buf, qoff, qlen = pack(qs)
    lo, hi = idx.search_range(buf, qoff, qlen)
    eoff, epos = expected(tsa, lo, hi)
    tp = O.padded(t)
    for k in range(0, len(qs), 7):
        assert (int(lo[k]), int(hi[k])) == O.prefix_range(tp, n, tsa, qs[k]), k
    # host pointers: the sizing call, then the real one
    hoff, hpos = idx.locate(buf, qoff, qlen)
    assert np.array_equal(as_i64(hoff), eoff) and np.array_equal(as_i64(hpos), epos)
    # device pointers: ranges + offsets + one read of the total + fill
    dbuf = torch.from_numpy(buf).cuda()
    dqoff, dqlen = torch.from_numpy(qoff.astype(np.int64)).cuda(), torch.from_numpy(qlen.astype(np.int32)).cuda()
    doff, dpos = idx.locate(dbuf, dqoff, dqlen)
    assert np.array_equal(as_i64(doff), eoff) and np.array_equal(as_i64(dpos), epos)
    # device pointers, caller's buffer: one asynchronous sas_locate call, u64 and u32
    for u32 in (False, True):
        out = torch.full((len(epos) + 64,), -1, dtype=torch.int32 if u32 else torch.int64, device="cuda")
        doff, dpos = idx.locate(dbuf, dqoff, dqlen, out=out, u32=u32)
        torch.cuda.synchronize()
        assert np.array_equal(as_i64(doff), eoff)
        assert np.array_equal(as_i64(dpos[:len(epos)], u32), epos) and (dpos[len(epos):] == -1).all()
    # a per-query cap
    hoff, hpos = idx.locate(buf, qoff, qlen, max_per_query=5, u32=True)
    coff, cpos = expected(tsa, lo, hi, 5)
    assert np.array_equal(as_i64(hoff), coff) and np.array_equal(as_i64(hpos), cpos)
    # fixed-length batches
    for m in (3, 8, 32, 40):
        o = rng.integers(0, n - m, 500)
        fq = np.concatenate([t[i:i + m] for i in o] + [rng.integers(0, 4, 100 * m, dtype=np.uint8)])
        flo, fhi = idx.search_range_fixed(fq, m)
        foff, fpos = expected(tsa, flo, fhi, 1000)
        hoff, hpos = idx.locate_fixed(fq, m, max_per_query=1000)
        assert np.array_equal(as_i64(hoff), foff) and np.array_equal(as_i64(hpos), fpos), m
        doff, dpos = idx.locate_fixed(torch.from_numpy(fq).cuda(), m, max_per_query=1000)
        assert np.array_equal(as_i64(doff), foff) and np.array_equal(as_i64(dpos), fpos), m


def test_enospc_sizing_protocol_and_validation(sas, text, sa):
    from sas_amd import _lib
    L = _lib.lib()
    idx = sas.SaNaive.build(text, **E2E_BUILDS["quad_prefix8_inline2"])
    qs = [text[10:14], text[500:530], np.full(6, 3, np.uint8), text[77:79]]
    buf, qoff, qlen = pack(qs)
    lo, hi = idx.search_range(buf, qoff, qlen)
    eoff, epos = expected(sa, lo, hi)
    off = np.full(len(qs) + 1, 99, np.uint64)
    total = C.c_uint64(0)
    args = (idx._h, buf.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, len(qs), 0, off.ctypes.data)
    # the sizing call: ENOSPC, the total set, the offsets filled
    assert L.sas_locate(*args, None, 0, C.byref(total), None, 0) == errno.ENOSPC
    assert total.value == eoff[-1] and np.array_equal(off.astype(np.int64), eoff)
    assert b"capacity" in L.sas_last_error()
    # one element short: still ENOSPC and nothing copied
    pos = np.full(total.value + 8, 0xABABABABABABABAB, np.uint64)
    assert L.sas_locate(*args, pos.ctypes.data, total.value - 1, C.byref(total), None, 0) == errno.ENOSPC
    assert (pos == 0xABABABABABABABAB).all()
    assert L.sas_locate(*args, pos.ctypes.data, total.value, C.byref(total), None, 0) == 0
    assert np.array_equal(pos[:total.value].astype(np.int64), epos) and (pos[total.value:] == 0xABABABABABABABAB).all()
    # nothing occurs: the sizing call itself succeeds
    none, zoff, zlen = pack([np.full(40, 3, np.uint8)])
    assert L.sas_locate(idx._h, none.ctypes.data, zoff.ctypes.data, zlen.ctypes.data, 1, 0, off.ctypes.data, None, 0,
                        C.byref(total), None, 0) == 0 and total.value == 0
    # a query byte > 3 is rejected on the host path
    bad = buf.copy()
    bad[2] = 4
    with pytest.raises(sas.SasError) as e:
        idx.locate(bad, qoff, qlen)
    assert e.value.code == errno.EINVAL
    # an index without a range-search structure: the requirement of sas_search_range
    bare = sas.SaNaive.build(text[:5000], **PLAIN)
    with pytest.raises(sas.SasError):
        bare.locate(buf, qoff, qlen)


def test_locate_between_matches_brute_force(sas):
    rng = np.random.default_rng(11)
    t = rng.integers(0, 4, 2000, dtype=np.uint8)
    idx = sas.SaNaive.build(t, lcp=False, stree=False, sector=False, llcp=False)
    tb = bytes(t)  # bytes compare like Rust slices: lexicographic, a proper prefix is smaller
    order = sorted(range(len(t)), key=lambda i: tb[i:])
    for a, b in ((b"\x00\x01", b"\x00\x03\x02"), (b"", b"\x02"), (b"\x01\x01\x01", b"\x01\x01\x01"),
                 (b"\x03", b"\x00"), (b"\x02\x00\x03\x01", b"\x03\x03\x03\x03\x03"), (tb[100:140], tb[7:60])):
        want = [i for i in order if a <= tb[i:] < b]
        assert idx.locate_between(a, b).tolist() == want, (a, b)
