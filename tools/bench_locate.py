#!/usr/bin/env python3
"""Batched locate on one MI355X: sas_locate_fill alone and sas_locate whole (range search +
offsets + fill), in elements/s and GB/s, on the quad + prefix index of a generated text.

Shapes (n = 2^30: occurrences ~ n / 4^len):
  A  10^7 len-32 slices of the text      ~1 occurrence each (one random request per element)
  B  10^6 len-12 slices                  ~64 each
  C  10^3 len-6 slices                   ~2.6 x 10^5 each (streamed)
  D  A plus one len-4 query              bounded work per tile: D against A + the len-4 alone
Beside them: the plain copy the fill is held against (the device-pointer sas_copy_sa64 kernel,
k_widen_sa<4>, over one contiguous range of C's element count; both bracketed the same way,
a device synchronise inside the events, because sas_copy_sa64 synchronises itself), the fill
without the partition pre-pass (SAS_LOCATE_NO_PARTITION, alternating with the default), and
the present workaround timed once: a host loop of sas_copy_sa_range over 10^4 of B's queries.

Timing: HIP events on the current stream, `--warmup` untimed calls, the median of `--reps`
(>= 20) timed ones.  A sample of every shape's output is checked against the text.
The result goes to --out as JSON tagged with the library's source hash.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "suffix-array-searching_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

REQ_CEILING = 5.08e10  # random requests/s, DESIGN.md's randbench figure


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--prefix-inline", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts (rehearsals)")
    ap.add_argument("--only-c", action="store_true", help="shape C and its bar only (counter runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be >= 20")
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_locate: needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    n = args.n
    t0 = time.perf_counter()
    text = sas_amd.random_string(n, seed=args.seed, device=dev)
    idx = sas_amd.SaNaive.build(text, lcp=False, stree=False, sector=False, llcp=False, prefix=args.prefix_chars,
                                prefix_inline=args.prefix_inline)
    torch.cuda.synchronize()
    stats = idx.stats()
    W = stats["sa_width"]
    print(f"index built in {time.perf_counter() - t0:.1f} s (sa_width {W})", file=sys.stderr)
    st = torch.cuda.current_stream(dev).cuda_stream
    DEV = _lib.SAS_DEVICE_PTRS

    def cut(nq, m, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        off = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        ar = torch.arange(m, device=dev)
        q = torch.empty(nq * m, dtype=torch.uint8, device=dev)
        for s in range(0, nq, 1 << 18):
            e = min(nq, s + (1 << 18))
            q[s * m:e * m] = text[(off[s:e, None] + ar[None, :]).reshape(-1)]
        return q

    def timed(fn, sync_inside=False):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            if sync_inside:
                torch.cuda.synchronize()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def rate(total, ms, out_bytes=8):
        return {"ms": ms[0], "ms_min": ms[1], "ms_max": ms[2], "elements_per_s": total / (ms[0] * 1e-3),
                "GB_per_s": total * (W + out_bytes) / (ms[0] * 1e-3) / 1e9}

    def check_sample(qb, qoff, qlen, off, pos, total):
        """1000 output elements: the text at the position starts with the element's query."""
        if total == 0:
            return True
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        j = torch.randint(0, total, (1000,), generator=g, device=dev)
        k = torch.searchsorted(off, j, right=True) - 1
        ok = True
        for jj, kk in zip(j.tolist(), k.tolist()):
            p, m, o = int(pos[jj]), int(qlen[kk]), int(qoff[kk])
            ok &= p + m <= n and bool(torch.equal(text[p:p + m], qb[o:o + m]))
        return ok

    def shape(name, qb, qoff, qlen, fixed_m=None):
        nq = int(qoff.numel())
        lo, hi = idx.search_range(qb, qoff, qlen)
        off, _ = idx.locate_ranges(lo, hi, capacity=0)
        total = int(off[nq].item())
        out = torch.empty(total + 64, dtype=torch.int64, device=dev)
        out32 = torch.empty(total + 64, dtype=torch.int32, device=dev)

        def fill(fl=0, o=out):
            _lib.check(L.sas_locate_fill(idx._h, lo.data_ptr(), off.data_ptr(), nq, o.data_ptr(), total, st, DEV | fl))

        def whole():
            if fixed_m:
                idx.locate_fixed(qb, fixed_m, out=out)
            else:
                idx.locate(qb, qoff, qlen, out=out)

        rec = {"nq": nq, "total": total, "mean_occurrences": total / nq}
        ab = [], []
        for _ in range(3):  # the pre-pass against the in-block search, alternating
            ab[0].append(timed(fill)[0])
            ab[1].append(timed(lambda: fill(_lib.SAS_LOCATE_NO_PARTITION))[0])
        rec["fill_u64"] = rate(total, timed(fill))
        rec["fill_u32"] = rate(total, timed(lambda: fill(_lib.SAS_LOCATE_U32, out32)), 4)
        rec["fill_u64_partition_ms"] = ab[0]
        rec["fill_u64_no_partition_ms"] = ab[1]
        rec["locate_u64"] = rate(total, timed(whole))
        rec["range_search_ms"] = timed(lambda: idx.search_range(qb, qoff, qlen))[0]
        whole()
        torch.cuda.synchronize()
        rec["verified_sample"] = check_sample(qb, qoff, qlen, off, out, total)
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec, (lo, hi, off, out, total)

    def fixed(nq, m, seed):
        qb = cut(nq, m, seed)
        return qb, torch.arange(nq, device=dev, dtype=torch.int64) * m, torch.full((nq,), m, dtype=torch.int32, device=dev)

    sc = args.scale
    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": W, "prefix_chars": stats["prefix_chars"],
           "reps": args.reps, "warmup": args.warmup, "tile": 2048, "shapes": {}}
    blo = bhi = None
    if not args.only_c:
        qa = fixed(max(int(10_000_000 * sc), 1), 32, 11)
        res["shapes"]["A"], _ = shape("A", *qa, fixed_m=32)
        res["shapes"]["A"]["fill_vs_request_ceiling"] = res["shapes"]["A"]["fill_u64"]["elements_per_s"] / REQ_CEILING
        qbq = fixed(max(int(1_000_000 * sc), 1), 12, 12)
        res["shapes"]["B"], (blo, bhi, _, _, _) = shape("B", *qbq, fixed_m=12)
        q4 = fixed(1, 4, 14)
        res["shapes"]["len4_alone"], _ = shape("len4_alone", *q4)
        qd = (torch.cat([qa[0], q4[0]]), torch.cat([qa[1], qa[1][-1:] + 32]), torch.cat([qa[2], q4[2]]))
        res["shapes"]["D"], _ = shape("D", *qd)
        res["shapes"]["D"]["A_plus_len4_fill_ms"] = (res["shapes"]["A"]["fill_u64"]["ms"] +
                                                     res["shapes"]["len4_alone"]["fill_u64"]["ms"])
        del qa, qd
    qc = fixed(max(int(1000 * sc), 1), 6, 13)
    res["shapes"]["C"], (_, _, _, cout, ctotal) = shape("C", *qc, fixed_m=6)

    # the bar for C: the plain widening copy over one contiguous range of the same length
    cnt = min(ctotal, n)

    def copy64():
        _lib.check(L.sas_copy_sa64(idx._h, 0, cnt, cout.data_ptr(), DEV))

    def fill_c():
        lo, hi, off, out, total = c_state
        _lib.check(L.sas_locate_fill(idx._h, lo.data_ptr(), off.data_ptr(), int(lo.numel()), out.data_ptr(), total, st,
                                     DEV))

    lo_c, hi_c = idx.search_range(*qc)
    off_c, _ = idx.locate_ranges(lo_c, hi_c, capacity=0)
    c_state = (lo_c, hi_c, off_c, cout, ctotal)
    base, mine = [], []
    for _ in range(3):  # alternating, both with the synchronise inside the events
        base.append(timed(copy64, sync_inside=True))
        mine.append(timed(fill_c, sync_inside=True))
    b = sorted(base)[1]
    f = sorted(mine)[1]
    res["C_bar"] = {"elements_copy": cnt, "elements_fill": ctotal, "copy_sa64": rate(cnt, b), "fill_u64": rate(ctotal, f),
                    "ratio_fill_over_copy": (ctotal / f[0]) / (cnt / b[0]), "bar": 0.9,
                    "copy_ms_runs": [x[0] for x in base], "fill_ms_runs": [x[0] for x in mine]}
    res["C_bar"]["met"] = res["C_bar"]["ratio_fill_over_copy"] >= 0.9
    print("C bar: " + json.dumps(res["C_bar"]), file=sys.stderr)

    # the workaround locate replaces: one synchronous sas_copy_sa_range per query
    if W == 4 and blo is not None:
        k = min(10_000, int(blo.numel()))
        hlo, hhi = blo[:k].cpu().numpy(), bhi[:k].cpu().numpy()
        buf = np.zeros(int((hhi - hlo).max()) + 1, np.uint32)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for a, c in zip(hlo.tolist(), hhi.tolist()):
            _lib.check(L.sas_copy_sa_range(idx._h, a, c - a, buf.ctypes.data, 0))
        dt = time.perf_counter() - t1
        tot = int((hhi - hlo).sum())
        res["host_loop_copy_sa_range"] = {"queries": k, "elements": tot, "seconds": dt, "elements_per_s": tot / dt,
                                          "queries_per_s": k / dt}
        res["host_loop_copy_sa_range"]["locate_speedup_elements"] = (
            res["shapes"]["B"]["locate_u64"]["elements_per_s"] / (tot / dt))
    out = args.out or os.path.join(REPO, "profiles", "locate", f"locate_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "C_bar_ratio": res["C_bar"]["ratio_fill_over_copy"]}))


if __name__ == "__main__":
    main()
