#!/usr/bin/env python3
"""A/B of the sequence layout's cost on one GPU: the approximate calls on the 2^30-char generated
text without a layout, with a synthetic one (25 sequences, 1,000 segments laid over the text), and
sas_translate's rate.  It times whole calls on device pointers, as tools/bench_mismatch.py,
bench_edit.py, bench_pairs.py and bench_rescue.py time their "new" legs (median of --reps calls per
round, every round kept), without their baselines and checks, so that one process covers the four
calls in seconds.  --pkg points at another checkout's suffix-array-searching_amd directory: with
--legs none it uses nothing that checkout lacks, which gives the parent's figures for the no-layout
comparison on the same card in the same session.

Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "suffix-array-searching_amd"))
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads per call (pairs: half as many pairs)")
    ap.add_argument("--legs", default="none,layout,translate", help="none: no layout; layout: the synthetic one")
    ap.add_argument("--sequences", type=int, default=25)
    ap.add_argument("--segments", type=int, default=1000)
    ap.add_argument("--positions", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import torch
    import sas_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_layout: needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n, legs = args.n, args.legs.split(",")
    t0 = time.perf_counter()
    idx = sas_amd.SaNaive.build_gen(n, seed=args.seed, lcp=False, stree=False, sector=False, llcp=False,
                                    prefix=args.prefix_chars, prefix_inline=2)
    torch.cuda.synchronize()
    print(f"index built in {time.perf_counter() - t0:.1f} s", file=sys.stderr)

    def slices(off, m):
        nq = int(off.numel())
        q = torch.zeros(nq * m + 64, dtype=torch.uint8, device=dev)
        idx.extract(off, torch.full((nq,), m, dtype=torch.int32, device=dev),
                    torch.arange(nq, device=dev, dtype=torch.int64) * m, q)
        return q

    def substitute(q, nq, m, nsub, g):
        for _ in range(nsub):
            at = torch.arange(nq, device=dev) * m + torch.randint(0, m, (nq,), generator=g, device=dev)
            q[at] = (q[at] + torch.randint(1, 4, (nq,), generator=g, device=dev).to(torch.uint8)) & 3
        return q

    def reads(nq, m, nsub, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return substitute(slices(torch.randint(0, n - m, (nq,), generator=g, device=dev), m), nq, m, nsub, g)

    def pairs(npairs, m, nsub, heavy, seed):
        """interleaved mates: the forward slice and the reverse complement of the slice 300..500 on;
        a share `heavy` of the second mates carries nsub + 2 substitutions (the rescue's work)"""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        off = torch.randint(0, n - 600 - m, (npairs,), generator=g, device=dev)
        frag = torch.randint(300, 500, (npairs,), generator=g, device=dev)
        a = substitute(slices(off, m), npairs, m, nsub, g)[:npairs * m].view(npairs, m)
        b = substitute(slices(off + frag - m, m), npairs, m, nsub, g)[:npairs * m].view(npairs, m)
        nh = int(npairs * heavy)
        if nh:
            hb = substitute(b[:nh].reshape(-1).clone(), nh, m, 2, g)
            b = torch.cat([hb.view(nh, m), b[nh:]])
        b = b.flip(1) ^ 3
        q = torch.stack([a, b], 1).reshape(-1)
        return torch.cat([q, torch.zeros(64, dtype=torch.uint8, device=dev)])

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(args.rounds):
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            rounds.append(round(float(np.median(ms)), 4))
        return rounds

    nq = args.reads
    calls = {}
    for name, m, k in (("S", 32, 1), ("L", 100, 3)):
        q = reads(nq, m, 1 if name == "S" else 2, 7 + m)
        p = pairs(nq // 2, m, 1, 0.02, 11 + m)
        cap_mm = int(idx.locate_mismatch_fixed(q[:nq * m], m, k, capacity=0, dist=False)[0][nq]) + nq
        cap_ed = int(idx.locate_edit_fixed(q[:nq * m], m, k, capacity=0, dist=False)[0][nq]) + nq
        out_mm = torch.empty(cap_mm, dtype=torch.int64, device=dev)
        out_ed = torch.empty(cap_ed, dtype=torch.int64, device=dev)
        calls[f"mismatch_{name}"] = lambda q=q, m=m, k=k, o=out_mm: idx.locate_mismatch_fixed(q[:nq * m], m, k, out=o)
        calls[f"edit_{name}"] = lambda q=q, m=m, k=k, o=out_ed: idx.locate_edit_fixed(q[:nq * m], m, k, out=o)
        calls[f"map_{name}"] = lambda q=q, m=m, k=k: idx.map_edit_fixed(q[:nq * m], m, k)
        calls[f"pairs_{name}"] = lambda p=p, m=m, k=k: idx.map_pairs_fixed(p[:nq * m], m, k, 200, 600)
        calls[f"rescue_{name}"] = lambda p=p, m=m, k=k: idx.map_pairs_rescue_fixed(p[:nq * m], m, k, k + 2, 200, 600, 4)
    res = {"n": n, "source_hash": sas_amd.source_hash(), "reads": nq, "reps": args.reps, "rounds": args.rounds,
           "ms_rounds": {}}
    if "none" in legs:
        res["ms_rounds"]["none"] = {name: timed(fn) for name, fn in calls.items()}
    if "layout" in legs or "translate" in legs:
        per = n // args.sequences
        starts = [i * per for i in range(args.sequences)] + [n]
        each = args.segments // args.sequences
        lo, hi = [], []
        for i in range(args.sequences):
            slot = (starts[i + 1] - starts[i]) // each
            for j in range(each):
                lo.append(starts[i] + j * slot + slot // 40)  # a gap of 2.5 % in front of every segment
                hi.append(starts[i] + (j + 1) * slot)
        idx.set_layout(starts, lo, hi)
        res["layout"] = {"sequences": args.sequences, "segments": len(lo)}
        if "layout" in legs:
            res["ms_rounds"]["layout"] = {name: timed(fn) for name, fn in calls.items()}
            if "none" in legs:
                res["layout_over_none"] = {name: round(float(np.median(res["ms_rounds"]["layout"][name]) /
                                                             np.median(res["ms_rounds"]["none"][name])), 4)
                                           for name in calls}
        if "translate" in legs:
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            pos = torch.randint(0, n, (args.positions,), generator=g, device=dev)
            span = torch.full((args.positions,), 32, dtype=torch.int32, device=dev)
            tr = timed(lambda: idx.translate(pos, span))
            res["translate"] = {"positions": args.positions, "ms_rounds": tr,
                                "positions_per_s": args.positions / (float(np.median(tr)) * 1e-3)}
        idx.set_layout(None)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
