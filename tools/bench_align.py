#!/usr/bin/env python3
"""Alignment start and edit script (sas_align_edit) on one MI355X, on the quad + two-suffix p = 16
prefix table index of a generated text (n = 2^30), against the sas_locate_edit call that produced
the ends.

Queries are made on the device as in tools/bench_edit.py: text slices with edits drawn uniformly
from substitution, insertion and deletion at random places:
  S  10^7 of 32 chars, k = 1, one edit        L  10^7 of 100 chars, k = 3, 1..3 edits
Per shape the ends come from locate_edit_fixed in the same process; then two legs run
round-robin `--rounds` times (each figure the median over rounds of the median of `--reps`
event-timed calls):
  align     sas_align_edit_fixed on device pointers into preallocated buffers (one kernel, no
            host read)
  locate    locate_edit_fixed into a preallocated buffer: the call that produced the ends, on the
            same library.  It is the yardstick because an alignment pass per reported end is the
            same kind of work as its verify pass per candidate
Before timing, every alignment is checked on the device: dist equals locate_edit's D(e), the run
lengths add up to m and to e - start, the chars that are not = number dist.  JSON to --out,
tagged with the source hash.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "suffix-array-searching_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {  # name: (record key, queries, m, k, fewest edits, most edits, seed)
    "S": ("S_1e7_len32_k1", 10_000_000, 32, 1, 1, 1, 11),
    "L": ("L_1e7_len100_k3", 10_000_000, 100, 3, 1, 3, 12),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts (rehearsals)")
    ap.add_argument("--shapes", default="S,L")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_align: needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.n
    t0 = time.perf_counter()
    idx = sas_amd.SaNaive.build_gen(n, seed=args.seed, lcp=False, stree=False, sector=False, llcp=False,
                                    prefix=args.prefix_chars, prefix_inline=2)
    torch.cuda.synchronize()
    stats = idx.stats()
    print(f"index built in {time.perf_counter() - t0:.1f} s (p = {stats['prefix_chars']})", file=sys.stderr)
    L = _lib.lib()

    def cut_edited(nq, m, e_lo, e_hi, seed, chunk=1 << 20):
        """nq queries of m chars: text slices after e_lo..e_hi edits each, of uniformly drawn kinds."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        w = m + e_hi  # spare chars behind the slice: a deletion pulls one in
        q = torch.zeros(nq * m + 64, dtype=torch.uint8, device=dev)
        col = torch.arange(w, device=dev)[None, :]
        for c0 in range(0, nq, chunk):
            cq = min(nq, c0 + chunk) - c0
            off = torch.randint(0, n - w, (cq,), generator=g, device=dev)
            buf = torch.zeros(cq * w, dtype=torch.uint8, device=dev)
            idx.extract(off, torch.full((cq,), w, dtype=torch.int32, device=dev),
                        torch.arange(cq, device=dev, dtype=torch.int64) * w, buf)
            buf = buf.view(cq, w)
            count = torch.randint(e_lo, e_hi + 1, (cq,), generator=g, device=dev)
            for e in range(e_hi):
                live = (count > e)[:, None]
                kind = torch.randint(0, 3, (cq,), generator=g, device=dev)[:, None]  # sub, ins, del
                at = torch.randint(0, m, (cq,), generator=g, device=dev)[:, None]
                other = torch.randint(1, 4, (cq,), generator=g, device=dev).to(torch.uint8)[:, None]
                fresh = torch.randint(0, 4, (cq,), generator=g, device=dev).to(torch.uint8)[:, None]
                src = col - ((kind == 1) & (col > at)).long() + ((kind == 2) & (col >= at)).long()
                moved = torch.gather(buf, 1, src.clamp(0, w - 1))
                moved = torch.where((kind == 0) & (col == at), (moved + other) & 3, moved)
                moved = torch.where((kind == 1) & (col == at), fresh, moved)
                buf = torch.where(live, moved, buf)
            q[c0 * m:(c0 + cq) * m] = buf[:, :m].reshape(-1)
        return q

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def shape(name):
        _, nq, m, k, e_lo, e_hi, seed = SHAPES[name]
        nq = max(int(nq * args.scale), 1)
        stride = 2 * k + 1
        qb = cut_edited(nq, m, e_lo, e_hi, seed)[:nq * m]
        off, end, dist, _ = idx.locate_edit_fixed(qb, m, k)  # the ends: a sizing call, then the real one
        na = int(off[nq])
        end = end[:na].contiguous()
        lout = torch.empty(max(na, 1), dtype=torch.int64, device=dev)
        start = torch.empty(max(na, 1), dtype=torch.int64, device=dev)
        adist = torch.empty(max(na, 1), dtype=torch.uint8, device=dev)
        nruns = torch.empty(max(na, 1), dtype=torch.uint8, device=dev)
        runs = torch.empty((max(na, 1), stride), dtype=torch.int16, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def align():
            _lib.check(L.sas_align_edit_fixed(idx._h, qb.data_ptr(), m, nq, k, off.data_ptr(), end.data_ptr(), na,
                                              start.data_ptr(), adist.data_ptr(), nruns.data_ptr(), runs.data_ptr(),
                                              st, _lib.SAS_DEVICE_PTRS))

        legs = {"align": align, "locate": lambda: idx.locate_edit_fixed(qb, m, k, out=lout)}
        # every alignment, before timing: the distance and the lengths of the script
        align()
        ok = True
        for a0 in range(0, na, 1 << 24):
            sl = slice(a0, min(na, a0 + (1 << 24)))
            r = runs[sl].to(torch.int32)
            ops, lens = r & 3, r >> 2
            ok = ok and bool(torch.equal(adist[sl], dist[sl]))
            ok = ok and bool(((lens * (ops != _lib.SAS_AL_DEL)).sum(1) == m).all())
            ok = ok and bool(((lens * (ops != _lib.SAS_AL_INS)).sum(1) == end[sl] - start[sl]).all())
            ok = ok and bool(((lens * (ops != _lib.SAS_AL_EQ)).sum(1) == adist[sl]).all())
        rec = {"nq": nq, "m": m, "k": k, "edits": [e_lo, e_hi], "ends": na, "ends_per_query": na / nq,
               "scripts_consistent": ok, "mean_runs": float(nruns[:na].float().mean()) if na else 0.0,
               "first_cigar": sas_amd.cigar(runs[0], nruns[0]) if na else ""}
        res = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                res[x].append(timed(fn, args.reps))
        ms = {x: float(np.median(v)) for x, v in res.items()}
        rec.update(ms=ms, ms_runs=res, alignments_per_s=na / (ms["align"] * 1e-3),
                   align_over_locate_same_library=ms["align"] / ms["locate"])
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    out = args.out or os.path.join(REPO, "profiles", "align", f"align_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in args.shapes.split(","):
        res["shapes"][SHAPES[name][0]] = shape(name)
        with open(out, "w") as fh:  # after every shape: a cut-short run keeps what it measured
            json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "ms": {x: v["ms"] for x, v in res["shapes"].items()},
                      "align_over_locate": {x: v["align_over_locate_same_library"] for x, v in res["shapes"].items()},
                      "consistent": {x: v["scripts_consistent"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
