"""The Python wrapper over the C ABI, pinned call by call: every public query method of SaNaive
(ragged and fixed), revcomp and pack_queries, called once with numpy arrays and once with torch
CUDA tensors, returns the same tuple shape and field names, the documented dtypes on each side
(numpy unsigned, torch the signed type of the same width), equal lengths and bit-identical
contents; and every one of them takes an empty batch.  No kernel is under test here: the
kernels have their own tests against the oracle.  search_slices (device only, tagged indexes
only) is left to test_gpu_tagged.

The case: one index over random_string(4096) with the default structures and 16 queries, 12
slices of the text of length 24 with one substituted char each, 2 exact slices, one all-3 query
and one empty one; the fixed twins take the 14 of length 24.  The paired calls take 8 pairs 150
apart; one pair's second mate carries two substitutions (no seed of k = 1 holds: rescued at
k_rescue = 2) and one pair's second mate maps nowhere."""
import numpy as np
import pytest

from sas_amd import _lib

pytestmark = pytest.mark.gpu

N, M, K, K_RESCUE, MAX_ANCHORS, FRAG, PAIR_SPAN = 4096, 24, 1, 2, 4, (100, 300), 150
U64, U32, U16, U8 = np.uint64, np.uint32, np.uint16, np.uint8
MAPPED = ("end", "start", "dist", "strand", "n_best", "n_loci", "nruns", "runs", "qflags")
PAIRS = MAPPED + ("pflags", "n_pairs", "n_best_pairs")
RESCUE = PAIRS + ("n_rescue",)


def pack(qs):
    ln = np.array([len(q) for q in qs], U32)
    off = np.zeros(len(qs), U64)
    if len(qs):
        off[1:] = np.cumsum(ln[:-1], dtype=U64)
    return np.concatenate(list(qs) + [np.zeros(0, U8)]).astype(U8), off, ln


def sub(q, *at):
    q = q.copy()
    for i in at:
        q[i] = (q[i] + 1) & 3
    return q


class Case:
    """The index and the same inputs on both sides: .h numpy, .d torch CUDA."""

    def __init__(self, torch, sas):
        self.torch = torch
        t = sas.random_string(N)
        self.idx = sas.SaNaive.build(t)
        qs = [sub(t[s:s + M], (5 * i + 3) % M) for i, s in enumerate(range(200, 200 + 12 * 300, 300))]
        qs += [t[1000:1000 + M].copy(), t[N - M:].copy()]
        fixed = list(qs)
        qs += [np.full(30, 3, U8), np.zeros(0, U8)]
        rc = lambda q: (3 - q[::-1]).astype(U8)  # noqa: E731
        mates = []
        for i, s in enumerate(range(300, 300 + 8 * 400, 400)):
            m2 = rc(t[s + PAIR_SPAN - M:s + PAIR_SPAN])
            if i == 5:
                m2 = sub(m2, 3, 17)
            if i == 6:
                m2 = sub(m2, 1, 6, 11, 16, 21)
            mates += [t[s:s + M].copy(), m2]
        self.h = {"ragged": pack(qs), "fixed": np.concatenate(fixed), "pairs": pack(mates),
                  "pairs_fixed": np.concatenate(mates)}
        self.h["empty"] = (np.zeros(0, U8), np.zeros(0, U64), np.zeros(0, U32))
        self.d = {k: self.dev(v) for k, v in self.h.items()}

    def dev(self, x):
        """numpy -> CUDA: bytes stay uint8, offsets become int64, lengths int32."""
        if isinstance(x, tuple):
            return tuple(self.dev(v) for v in x)
        signed = {U8: U8, U16: np.int16, U32: np.int32, U64: np.int64}[x.dtype.type]
        return self.torch.from_numpy(np.ascontiguousarray(x).view(signed).copy()).cuda()


@pytest.fixture(scope="module")
def case():
    import torch
    import sas_amd
    return Case(torch, sas_amd)


def unsigned(x):
    a = x.cpu().numpy()
    return a.view({np.int64: U64, np.int32: U32, np.int16: U16, np.uint8: U8}[a.dtype.type])


class Checker:
    """Runs the host and the device form of one call and compares the two results; collects what
    differs so one run names every call that is off."""

    def __init__(self, torch):
        self.torch = torch
        self.bad = []
        self.seen = []

    def __call__(self, name, host, device, kinds, fields=None, cut=(), total=None, empty=False):
        """kinds: the numpy dtype of each output (None: the output is None).  cut: indexes of device
        outputs that are whole capacity buffers, compared up to off[nq].  empty: every output has
        length 0, except an `off` of one entry holding 0 (named in `fields`)."""
        tdt = {U64: self.torch.int64, U32: self.torch.int32, U16: self.torch.int16, U8: self.torch.uint8}
        self.seen.append(name)
        try:
            h, d = host(), device()
            self.torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            self.bad.append(f"{name}: {type(e).__name__}: {e}")
            return None, None
        err = []
        if hasattr(h, "_fields") or hasattr(d, "_fields"):
            if type(h) is not type(d) or h._fields != tuple(fields):
                err.append(f"record {type(h).__name__} / {type(d).__name__}")
        hs, ds = (h, d) if isinstance(h, tuple) else ((h,), (d,))
        if not (isinstance(d, tuple) == isinstance(h, tuple) and len(hs) == len(ds) == len(kinds)):
            self.bad.append(f"{name}: {len(hs)} host and {len(ds)} device outputs, {len(kinds)} documented")
            return h, d
        names = fields if fields is not None else range(len(kinds))
        for i, (f, hv, dv, kind) in enumerate(zip(names, hs, ds, kinds)):
            if kind is None:
                if hv is not None or dv is not None:
                    err.append(f"{f}: not None")
                continue
            if not isinstance(hv, np.ndarray) or hv.dtype != kind:
                err.append(f"{f}: host {type(hv).__name__} {getattr(hv, 'dtype', None)}, not numpy {kind.__name__}")
                continue
            if not (self.torch.is_tensor(dv) and dv.is_cuda and dv.dtype == tdt[kind]):
                err.append(f"{f}: device {type(dv).__name__} {getattr(dv, 'dtype', None)}, not CUDA {tdt[kind]}")
                continue
            if i in cut:
                if tuple(dv.shape) != (max(total, 1),):
                    err.append(f"{f}: capacity buffer of {tuple(dv.shape)}, not {max(total, 1)}")
                dv = dv[:len(hv)]
            if hv.shape != tuple(dv.shape):
                err.append(f"{f}: host shape {hv.shape}, device {tuple(dv.shape)}")
            elif not np.array_equal(hv, unsigned(dv)):
                err.append(f"{f}: contents differ")
            if empty:
                want = (1,) if f == "off" else (0,) + hv.shape[1:]
                if hv.shape != want or (f == "off" and int(hv[0]) != 0):
                    err.append(f"{f}: empty batch gives shape {hv.shape}, not {want} (off[0] = 0)")
        if err:
            self.bad.append(f"{name}: " + "; ".join(err))
        return h, d


def run_all(c, chk, ragged, fixed, pairs, pairs_fixed, empty):
    """Every call on the given inputs (names of Case.h / Case.d entries)."""
    import sas_amd
    idx, H, D = c.idx, c.h, c.d
    hr, dr, hf, df = H[ragged], D[ragged], H[fixed], D[fixed]
    hp, dp, hpf, dpf = H[pairs], D[pairs], H[pairs_fixed], D[pairs_fixed]
    nq, nf = len(hr[1]), len(hf) // M
    kw = dict(empty=empty)

    # -- exact lookups
    for probes in (False, True):
        kinds = (U64, U32) if probes else (U64,)
        chk(f"search_batch probes={probes}", lambda: idx.search_batch(*hr, probes=probes),
            lambda: idx.search_batch(*dr, probes=probes), kinds, **kw)
        chk(f"search_fixed probes={probes}", lambda: idx.search_fixed(hf, M, algo="prefix", probes=probes),
            lambda: idx.search_fixed(df, M, algo="prefix", probes=probes), kinds, **kw)
    hout, dout = np.full(nf + 3, 7, U64), c.torch.full((nf + 3,), 7, dtype=c.torch.int64, device="cuda")
    h, d = chk("search_fixed out=", lambda: idx.search_fixed(hf, M, out=hout)[:nf],
               lambda: idx.search_fixed(df, M, out=dout)[:nf], (U64,), **kw)
    if h is not None and not empty:  # the host call returns out[:nq], the device call `out` itself
        assert np.shares_memory(idx.search_fixed(hf, M, out=hout), hout) and len(idx.search_fixed(hf, M, out=hout)) == nf
        assert idx.search_fixed(df, M, out=dout) is dout and (hout[nf:] == 7).all() and (unsigned(dout)[nf:] == 7).all()
    chk("search_range", lambda: idx.search_range(*hr), lambda: idx.search_range(*dr), (U64, U64), **kw)
    chk("search_range_fixed", lambda: idx.search_range_fixed(hf, M), lambda: idx.search_range_fixed(df, M),
        (U64, U64), **kw)
    hw, dw = chk("pack_queries", lambda: idx.pack_queries(hf, M), lambda: idx.pack_queries(df, M), (U64,), **kw)
    if hw is not None:
        for probes in (False, True):
            chk(f"search_packed probes={probes}", lambda: idx.search_packed(hw, M, probes=probes),
                lambda: idx.search_packed(dw, M, probes=probes), (U64, U32) if probes else (U64,), **kw)
    for ranges in (True, False):
        kinds = (U32, U64, U64, U64) if ranges else (U32, U64)
        chk(f"match ranges={ranges}", lambda: idx.match(*hr, ranges=ranges), lambda: idx.match(*dr, ranges=ranges),
            kinds, **kw)
        chk(f"match_fixed ranges={ranges}", lambda: idx.match_fixed(hf, M, ranges=ranges),
            lambda: idx.match_fixed(df, M, ranges=ranges), kinds, **kw)
        chk(f"match_stats ranges={ranges}", lambda: idx.match_stats(hf, 20, ranges=ranges),
            lambda: idx.match_stats(df, 20, ranges=ranges), kinds, **kw)

    # -- revcomp
    chk("revcomp", lambda: sas_amd.revcomp(*hr), lambda: sas_amd.revcomp(*dr), (U8, U64),
        fields=("bytes", "off"), **kw)
    chk("revcomp m=", lambda: sas_amd.revcomp(hf, m=M), lambda: sas_amd.revcomp(df, m=M), (U8,), **kw)

    # -- the sized calls: exact, k-mismatch and k-difference locate, then the alignment of the ends
    for u32 in (False, True):
        P = U32 if u32 else U64
        csr = ("off", "pos")
        h, d = chk(f"locate u32={u32}", lambda: idx.locate(*hr, u32=u32), lambda: idx.locate(*dr, u32=u32), (U64, P),
                   fields=csr, **kw)
        hfx, _ = chk(f"locate_fixed u32={u32}", lambda: idx.locate_fixed(hf, M, u32=u32),
                     lambda: idx.locate_fixed(df, M, u32=u32), (U64, P), fields=csr, **kw)
        lo, hi = idx.search_range(*dr)
        if h is not None:
            chk(f"locate_ranges u32={u32}", lambda: h, lambda: idx.locate_ranges(lo, hi, u32=u32), (U64, P),
                fields=csr, **kw)
        if h is not None and not empty:
            cap = len(h[1]) + 5
            chk(f"locate capacity u32={u32}", lambda: h, lambda: idx.locate(*dr, u32=u32, capacity=cap), (U64, P),
                cut=(1,), total=cap)
            chk(f"locate_fixed capacity u32={u32}", lambda: hfx,
                lambda: idx.locate_fixed(df, M, u32=u32, capacity=len(hfx[1]) + 5), (U64, P), cut=(1,),
                total=len(hfx[1]) + 5)
            chk(f"locate_ranges capacity u32={u32}", lambda: h,
                lambda: idx.locate_ranges(lo, hi, u32=u32, capacity=cap), (U64, P), cut=(1,), total=cap)
            buf = c.torch.empty(cap + 2, dtype=c.torch.int32 if u32 else c.torch.int64, device="cuda")
            chk(f"locate out= u32={u32}", lambda: h, lambda: idx.locate(*dr, u32=u32, out=buf), (U64, P), cut=(1,),
                total=cap + 2)
        found = ("off", "pos", "dist", "qflags")
        for fam in ("locate_mismatch", "locate_edit"):
            rag, fix = getattr(idx, fam), getattr(idx, fam + "_fixed")
            for dist in (True, False):
                kinds = (U64, P, U8 if dist else None, U8)
                tag = f"u32={u32} dist={dist}"
                h, d = chk(f"{fam} {tag}", lambda: rag(*hr, K, u32=u32, dist=dist),
                           lambda: rag(*dr, K, u32=u32, dist=dist), kinds, fields=found, **kw)
                hx, _ = chk(f"{fam}_fixed {tag}", lambda: fix(hf, M, K, u32=u32, dist=dist),
                            lambda: fix(df, M, K, u32=u32, dist=dist), kinds, fields=found, **kw)
                if h is not None and hx is not None and not empty:
                    cap, capx = len(h[1]) + 3, len(hx[1]) + 3
                    chk(f"{fam} capacity {tag}", lambda: h, lambda: rag(*dr, K, u32=u32, dist=dist, capacity=cap),
                        kinds, cut=(1, 2), total=cap)
                    chk(f"{fam}_fixed capacity {tag}", lambda: hx,
                        lambda: fix(df, M, K, u32=u32, dist=dist, capacity=capx), kinds, cut=(1, 2), total=capx)
        # the ends of locate_edit, aligned
        try:
            ho, he, _, _ = idx.locate_edit(*hr, K, u32=u32)
            hof, hef, _, _ = idx.locate_edit_fixed(hf, M, K, u32=u32)
        except Exception as e:  # noqa: BLE001
            chk.bad.append(f"align_edit u32={u32}: no ends to align ({e})")
            continue
        al = (P, U8, U8, U16)
        h, _ = chk(f"align_edit u32={u32}", lambda: idx.align_edit(*hr, K, ho, he, u32=u32),
                   lambda: idx.align_edit(*dr, K, c.dev(ho), c.dev(he), u32=u32), al, **kw)
        chk(f"align_edit_fixed u32={u32}", lambda: idx.align_edit_fixed(hf, M, K, hof, hef, u32=u32),
            lambda: idx.align_edit_fixed(df, M, K, c.dev(hof), c.dev(hef), u32=u32), al, **kw)
        if h is not None:
            assert h[3].shape == (len(he), 2 * K + 1)

        # -- read mapping: records
        rec = (P, P, U8, U8, U32, U32, U8, U16, U8)
        per_pair = (U8, U32, U32)
        h, _ = chk(f"map_edit u32={u32}", lambda: idx.map_edit(*hr, K, u32=u32), lambda: idx.map_edit(*dr, K, u32=u32),
                   rec, fields=MAPPED, **kw)
        chk(f"map_edit_fixed u32={u32}", lambda: idx.map_edit_fixed(hf, M, K, u32=u32),
            lambda: idx.map_edit_fixed(df, M, K, u32=u32), rec, fields=MAPPED, **kw)
        if h is not None:
            assert h.runs.shape == (nq, 2 * K + 1) and type(h).__name__ == "Mapped"
        h, _ = chk(f"map_pairs u32={u32}", lambda: idx.map_pairs(*hp, K, *FRAG, u32=u32),
                   lambda: idx.map_pairs(*dp, K, *FRAG, u32=u32), rec + per_pair, fields=PAIRS, **kw)
        chk(f"map_pairs_fixed u32={u32}", lambda: idx.map_pairs_fixed(hpf, M, K, *FRAG, u32=u32),
            lambda: idx.map_pairs_fixed(dpf, M, K, *FRAG, u32=u32), rec + per_pair, fields=PAIRS, **kw)
        if h is not None:
            assert h.runs.shape == (len(hp[1]), 2 * K + 1) and len(h.pflags) == len(hp[1]) // 2
            assert type(h).__name__ == "MappedPairs"
        h, _ = chk(f"map_pairs_rescue u32={u32}",
                   lambda: idx.map_pairs_rescue(*hp, K, K_RESCUE, *FRAG, MAX_ANCHORS, u32=u32),
                   lambda: idx.map_pairs_rescue(*dp, K, K_RESCUE, *FRAG, MAX_ANCHORS, u32=u32), rec + per_pair + (U32,),
                   fields=RESCUE, **kw)
        chk(f"map_pairs_rescue_fixed u32={u32}",
            lambda: idx.map_pairs_rescue_fixed(hpf, M, K, K_RESCUE, *FRAG, MAX_ANCHORS, u32=u32),
            lambda: idx.map_pairs_rescue_fixed(dpf, M, K, K_RESCUE, *FRAG, MAX_ANCHORS, u32=u32),
            rec + per_pair + (U32,), fields=RESCUE, **kw)
        if h is not None:
            assert h.runs.shape == (len(hp[1]), 2 * K_RESCUE + 1) and len(h.n_rescue) == len(hp[1]) // 2
            assert type(h).__name__ == "MappedPairsRescue"
            if not empty and not u32:  # a pair that joins, one that is rescued, a read that maps nowhere
                assert (h.pflags & _lib.SAS_PAIR_PROPER).sum() >= 6 and (h.pflags & _lib.SAS_PAIR_RESCUED).any()
                assert (h.end == N).any() and (h.end < N).sum() >= 14

        # -- positions back to (sequence, offset): two sequences of one segment each
        idx.set_layout([0, N // 2, N], [0, N // 2], [N // 2, N])
        try:
            pos = (np.append(np.arange(0, N, 257), N // 2 - 10) if not empty else np.zeros(0)).astype(P)
            span = np.full(len(pos), 40, U32)
            chk(f"translate u32={u32}", lambda: idx.translate(pos, u32=u32), lambda: idx.translate(c.dev(pos), u32=u32),
                (U32, P), **kw)
            h, _ = chk(f"translate span u32={u32}", lambda: idx.translate(pos, span, u32=u32),
                       lambda: idx.translate(c.dev(pos), c.dev(span), u32=u32), (U32, P), **kw)
            if h is not None and not empty:
                assert (h[0] == _lib.SAS_SEQ_NONE).any() and set(h[0].tolist()) >= {0, 1}
        finally:
            idx.set_layout(None)


def test_host_and_device_agree_on_every_call(case):
    """Each call on numpy arrays and on CUDA tensors: same tuple shape and field names, the documented
    dtypes on each side, equal lengths, the same bits; with u32 positions too, and the CUDA side of
    the sized calls with and without a capacity."""
    chk = Checker(case.torch)
    run_all(case, chk, "ragged", "fixed", "pairs", "pairs_fixed", empty=False)
    assert len(chk.seen) >= 80
    assert not chk.bad, "\n".join(chk.bad)


def test_empty_batches(case):
    """Each call with no query (the paired calls: no pair) returns without error on both sides, every
    output of length 0 in its documented dtype, an `off` of one entry holding 0."""
    case.h["empty_fixed"], case.d["empty_fixed"] = case.h["empty"][0], case.d["empty"][0]
    chk = Checker(case.torch)
    run_all(case, chk, "empty", "empty_fixed", "empty", "empty_fixed", empty=True)
    assert len(chk.seen) >= 60
    assert not chk.bad, "\n".join(chk.bad)
