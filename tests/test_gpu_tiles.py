"""The tile loops and the unstaged bisect of the output-centric tiled kernels (k_locate_fill,
k_mm_verify, k_ed_verify, k_al_align, k_map_fill, k_map_select, k_pair_heads, k_pair_loci,
k_pair_join), against the brute-force references of the calls' own test modules.

Tile loop: SAS_TILE_GRID=g caps every grid at g workgroups, so the suite's small cases take
`tile += gridDim.x` many times: g = 1 hands every tile to one workgroup in turn, g = 3 gives
adjacent tiles to different workgroups while each still takes several.  What runs only then: the
barrier that ends a tile, the reset of the segment slots, the reuse of k_al_align's scratch and
k_locate_fill's carried prefetch.

Sparse offsets: a batch in which few reads occur, so that one tile's slice of the CSR offsets
(candidates per piece, ends per query, bytes per read) is larger than the kernels' LDS stage and
they bisect global memory instead.

The cases, their references and the premises (tile counts, spans) come from
tests/test_tiles_host.py, which asserts the premises from the brute force alone; no reference is
derived from the library."""
import contextlib

import numpy as np
import pytest

import test_gpu_align as A
import test_gpu_edit as E
import test_gpu_locate as LOC
import test_gpu_map as M
import test_gpu_mismatch as MM
import test_gpu_pairs as P
from oracle import pyoracle as O
from test_map_host import intervals
from test_tiles_host import (AL_SLICE, AL_T, GRIDS, LOC_T, MAP_T, MIN_TILES, MM_SLICE, MM_T, PAIR_RUNS, TILE_RUNS, csr,
                             edit_case, map_case, pair_case, proposals, span, sparse_case, tiles)

pytestmark = pytest.mark.gpu

BUILDS = ("quad_p8", "sa40")


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


@contextlib.contextmanager
def tile_grid(monkeypatch, g):
    """SAS_TILE_GRID=g inside (None: unset), and the library saw it: sas_tile_grid_cap() is g inside
    and 0 outside."""
    from sas_amd import _lib
    L = _lib.lib()
    assert L.sas_tile_grid_cap() == 0
    if g is None:
        yield
        return
    monkeypatch.setenv("SAS_TILE_GRID", g)
    try:
        assert L.sas_tile_grid_cap() == int(g)
        yield
        assert L.sas_tile_grid_cap() == int(g)
    finally:
        monkeypatch.delenv("SAS_TILE_GRID")
    assert L.sas_tile_grid_cap() == 0


@pytest.fixture(scope="module")
def locate_text():
    t = O.random_string(LOC.N, seed=9)
    sa = O.build_sa(t).astype(np.int64)
    t.setflags(write=False)
    sa.setflags(write=False)
    return t, sa


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("build", ("u32", "sa40"))
def test_locate_ranges_tile_loop(sas, locate_text, build, g, monkeypatch):
    """k_locate_fill with the partition pre-pass (the carried prefetch of the next tile's record) and
    without it (each tile bisects for its first query), u64 and u32 positions."""
    import torch
    from sas_amd import _lib
    t, sa = locate_text
    idx = sas.SaNaive.build(t, **{**LOC.PLAIN, **LOC.BUILDS[build]})
    looped = 0
    for name, (lo, hi) in LOC.synthetic_cases().items():
        eoff, epos = LOC.expected(sa, lo, hi)
        total = int(eoff[-1])
        looped += tiles(total, LOC_T) >= MIN_TILES
        dlo, dhi = torch.from_numpy(lo.astype(np.int64)).cuda(), torch.from_numpy(hi.astype(np.int64)).cuda()
        for flags in (0, _lib.SAS_LOCATE_NO_PARTITION):
            for u32 in (False, True):
                out = torch.full((total + 64,), -1, dtype=torch.int32 if u32 else torch.int64, device="cuda")
                with tile_grid(monkeypatch, g):
                    off, _ = idx.locate_ranges(dlo, dhi, out=out, u32=u32, flags=flags)
                    torch.cuda.synchronize()
                got = out.cpu().numpy()
                pos = got[:total].view(np.uint32).astype(np.int64) if u32 else got[:total]
                what = (name, build, g, flags, u32)
                assert np.array_equal(off.cpu().numpy(), eoff), what
                assert np.array_equal(pos, epos) and (got[total:] == -1).all(), what
    assert looped >= 4  # cycle_0_70, the empties, tile_edges, whole_sa


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("name,k", TILE_RUNS)
def test_locate_mismatch_tile_loop(sas, name, k, g, monkeypatch):
    import torch
    c = edit_case(name, k)
    exp, pieces = c.mm
    assert tiles(pieces.sum(), MM_T) >= MIN_TILES
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    total = int(exp["off"][-1])
    with tile_grid(monkeypatch, g):
        off, pos, dist, qfl, tot = MM.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, 0, total)
    assert tot == total
    MM.same((off, pos, dist, qfl), exp, (name, k, g))


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name,k", TILE_RUNS)
def test_locate_edit_tile_loop(sas, name, k, build, g, monkeypatch):
    import torch
    c = edit_case(name, k)
    assert tiles(c.pieces.sum(), MM_T) >= MIN_TILES
    idx = sas.SaNaive.build(c.t, **E.BUILDS[build])
    exp = c.exp
    total = int(exp["off"][-1])
    what = (name, k, build, g)
    with tile_grid(monkeypatch, g):
        off, end, dist, qfl, tot = E.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, 0, total)
    assert tot == total, what
    E.same((off, end, dist, qfl), exp, what + ("ragged",))
    # the kernels of 1 and of 4 words of rows, which only a fixed-length batch selects
    for m in (64, 129):
        sel = [i for i, q in enumerate(c.qs) if len(q) == m]
        assert sel, what + (m,)
        fb = np.concatenate([c.qs[i] for i in sel] + [np.zeros(64, np.uint8)])
        rows = np.concatenate([np.arange(exp["off"][i], exp["off"][i + 1]) for i in sel])
        fexp = dict(off=csr([exp["off"][i + 1] - exp["off"][i] for i in sel]), end=exp["end"][rows],
                    dist=exp["dist"][rows], qflags=exp["qflags"][sel])
        with tile_grid(monkeypatch, g):
            got = idx.locate_edit_fixed(torch.from_numpy(fb).cuda()[:len(sel) * m], m, k)
            torch.cuda.synchronize()
        E.same(got, fexp, what + ("fixed", m))


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("name,k", TILE_RUNS)
def test_align_edit_tile_loop(sas, name, k, g, monkeypatch):
    """k_al_align's threads write their direction words over those of the tile before."""
    import torch
    c = edit_case(name, k)
    assert tiles(c.na, AL_T) >= MIN_TILES
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    with tile_grid(monkeypatch, g):
        got = A.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end)
        got32 = A.dev_call(torch, idx, c.qb, c.qoff, c.qlen, k, c.off, c.end, u32=True)
    A.structure(c, got, (name, k, g))  # every alignment, from the output and the brute force's D(e)
    A.compare(c, got, (name, k, g))    # bit for bit on the compared ones
    assert all(np.array_equal(a, b) for a, b in zip(got, got32)), (name, k, g, "u32")


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("name,k", TILE_RUNS)
def test_map_edit_tile_loop(sas, name, k, g, monkeypatch):
    """k_map_fill, k_map_select (both passes) and the verify and align kernels behind them."""
    import torch
    c = map_case(name, k)
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    for strands in (3, 2):
        assert tiles(proposals(c, strands), MAP_T) >= MIN_TILES
        with tile_grid(monkeypatch, g):
            got = M.dev_call(torch, idx, c, strands=strands)
        M.same(got, c.ref[strands], (name, k, g, strands))


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("name,k,w", PAIR_RUNS)
def test_map_pairs_tile_loop(sas, name, k, w, g, monkeypatch):
    """k_pair_heads, k_pair_loci and k_pair_join (both passes)."""
    import torch
    c = pair_case(name, k)
    assert tiles(proposals(c, 3), MAP_T) >= MIN_TILES  # the loci kernels' elements
    assert tiles(sum(intervals(np.asarray(a[0])) for a in c.A[0]), MAP_T) >= MIN_TILES  # the join's: forward loci
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    with tile_grid(monkeypatch, g):
        got = P.dev_call(torch, idx, c, w)
    P.same(got, c.ref(w), (name, k, w, g))


@pytest.mark.parametrize("g", (None, "1"))
@pytest.mark.parametrize("build", BUILDS)
def test_sparse_locate_mismatch_and_edit(sas, build, g, monkeypatch):
    """mm_tile_candidates without the LDS stage: k_mm_verify and k_ed_verify."""
    import torch
    c = sparse_case()
    exp, pieces = c.mm
    assert span(csr(pieces), MM_T) > MM_SLICE and span(csr(c.pieces), MM_T) > MM_SLICE
    idx = sas.SaNaive.build(c.t, **E.BUILDS[build])
    with tile_grid(monkeypatch, g):
        total = int(exp["off"][-1])
        off, pos, dist, qfl, tot = MM.dev_call(torch, idx, c.qb, c.qoff, c.qlen, c.k, 0, total)
        assert tot == total
        MM.same((off, pos, dist, qfl), exp, ("sparse mismatch", build, g))
        total = int(c.exp["off"][-1])
        off, end, dist, qfl, tot = E.dev_call(torch, idx, c.qb, c.qoff, c.qlen, c.k, 0, total)
        assert tot == total
        E.same((off, end, dist, qfl), c.exp, ("sparse edit", build, g))
        got = idx.locate_edit_fixed(torch.from_numpy(c.qb).cuda()[:len(c.qs) * 24], 24, c.k)
        torch.cuda.synchronize()
        E.same(got, c.exp, ("sparse edit fixed", build, g))


@pytest.mark.parametrize("g", (None, "1"))
def test_sparse_align_edit(sas, g, monkeypatch):
    """al_tile_queries without the LDS stage: k_al_align."""
    import torch
    c = sparse_case()
    assert span(c.off, AL_T) > AL_SLICE and len(c.sel) == c.na
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    with tile_grid(monkeypatch, g):
        got = A.dev_call(torch, idx, c.qb, c.qoff, c.qlen, c.k, c.off, c.end)
    A.structure(c, got, ("sparse align", g))
    A.compare(c, got, ("sparse align", g))


@pytest.mark.parametrize("g", (None, "1"))
def test_sparse_map_edit_and_revcomp(sas, g, monkeypatch):
    """al_tile_queries without the LDS stage in k_map_fill (4096 empty reads in a row: a tile of bytes
    spans them all), through sas_map_edit and through sas_revcomp."""
    import torch
    c = sparse_case()
    e = c.e
    lens = e.qlen.astype(np.int64)
    assert span(csr(np.concatenate([lens, lens])), AL_T) > AL_SLICE and span(csr(lens), AL_T) > AL_SLICE
    idx = sas.SaNaive.build(c.t, **E.BUILDS["quad_p8"])
    with tile_grid(monkeypatch, g):
        got = M.dev_call(torch, idx, e, strands=3)
        M.same(got, e.ref[3], ("sparse map", g))
        out, off = sas.revcomp(M.cu(torch, e.qb, np.uint8), M.cu(torch, e.qoff, np.int64),
                               M.cu(torch, e.qlen, np.int32))
        torch.cuda.synchronize()
    assert np.array_equal(off.cpu().numpy(), csr(lens)) and np.array_equal(out.cpu().numpy(), e.rc)
