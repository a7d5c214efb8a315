#!/usr/bin/env python3
"""Read mapping (sas_map_edit) on one MI355X, on the quad + two-suffix p = 16 prefix table index of
a generated text (n = 2^30), against the calls a user composes today.

Reads are made on the device as in tools/bench_align.py (text slices with edits drawn uniformly
from substitution, insertion and deletion at random places); every second read is then
reverse-complemented on the device (sas_revcomp_fixed), so half of them map on each strand:
  S  10^7 of 32 chars, k = 1, one edit        L  10^7 of 100 chars, k = 3, 1..3 edits
Per shape five legs run round-robin `--rounds` times (each figure the median over rounds of the
median of `--reps` event-timed calls):
  map            sas_map_edit_fixed on device pointers into preallocated buffers
  locate2        locate_edit_fixed on the reads plus on a pre-made reverse-complement batch, into
                 preallocated buffers: the floor, as map contains both passes
  align_all      align_edit_fixed over every end of both strands
  align_winners  sas_align_edit over map's request: one alignment per read (the alignment stage
                 inside map)
  workaround     locate2 + align_all + the per-read reduction in torch (scatter_reduce amin on the
                 packed key, interval starts by comparing with the shifted array, bincount), what
                 a user writes today; its records are checked to equal map's
Before timing, every record is checked on the device: dist is the least distance of the two
locate_edit answers, the run lengths add up to m and to end - start, n_best >= 1 exactly where
mapped.  JSON to --out, tagged with the source hash.
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
        raise SystemExit("bench_map: needs the GPU (no CPU fallback)")
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
    NONE = torch.iinfo(torch.int64).max

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
        st = torch.cuda.current_stream().cuda_stream
        qb = cut_edited(nq, m, e_lo, e_hi, seed)[:nq * m]
        # every second read from the other strand
        flip = sas_amd.revcomp(qb, m=m).view(nq, m)
        qv = qb.view(nq, m)
        qv[1::2] = flip[1::2]
        del flip
        rq = sas_amd.revcomp(qb, m=m)  # the pre-made reverse batch of locate2
        both = torch.cat([qb, rq, torch.zeros(64, dtype=torch.uint8, device=dev)])
        ar = torch.arange(nq, device=dev)

        # sizes and buffers of the composed path
        sized = [idx.locate_edit_fixed(b, m, k) for b in (qb, rq)]
        na = [int(s[0][nq]) for s in sized]
        del sized
        lend = [torch.empty(max(a, 1), dtype=torch.int64, device=dev) for a in na]
        astart = [torch.empty(max(a, 1), dtype=torch.int64, device=dev) for a in na]
        anr = [torch.empty(max(a, 1), dtype=torch.uint8, device=dev) for a in na]
        aruns = [torch.empty((max(a, 1), stride), dtype=torch.int16, device=dev) for a in na]
        loc = [None, None]

        def locate2():
            for s, b in enumerate((qb, rq)):
                loc[s] = idx.locate_edit_fixed(b, m, k, out=lend[s])

        def align_all():
            for s, b in enumerate((qb, rq)):
                off, end = loc[s][0], loc[s][1]
                _lib.check(L.sas_align_edit_fixed(idx._h, b.data_ptr(), m, nq, k, off.data_ptr(), end.data_ptr(),
                                                  na[s], astart[s].data_ptr(), None, anr[s].data_ptr(),
                                                  aruns[s].data_ptr(), st, _lib.SAS_DEVICE_PTRS))

        def reduce():
            """One record per read from the CSR answers of both strands."""
            best = torch.full((nq,), NONE, dtype=torch.int64, device=dev)
            n_loci = torch.zeros(nq, dtype=torch.int64, device=dev)
            n_best = torch.zeros(nq, dtype=torch.int64, device=dev)
            per = []
            for s in (0, 1):
                off, end, dist = loc[s][0], loc[s][1][:na[s]], loc[s][2][:na[s]].long()
                rid = torch.repeat_interleave(ar, off[1:] - off[:-1], output_size=na[s])
                key = (dist << 56) | (s << 55) | end
                best.scatter_reduce_(0, rid, key, "amin")
                follows = torch.zeros(na[s], dtype=torch.bool, device=dev)
                if na[s] > 1:
                    follows[1:] = (rid[1:] == rid[:-1]) & (end[1:] == end[:-1] + 1)
                n_loci += torch.bincount(rid[~follows], minlength=nq)
                per.append((rid, key, dist, follows))
            d = best >> 56
            pick = []
            for s in (0, 1):
                rid, key, dist, follows = per[s]
                same = follows.clone()
                if na[s] > 1:
                    same[1:] &= dist[1:] == dist[:-1]
                n_best += torch.bincount(rid[(dist == d[rid]) & ~same], minlength=nq)
                pick.append(torch.nonzero(key == best[rid]).squeeze(1))
            mapped = best != NONE
            end = torch.where(mapped, best & ((1 << 55) - 1), n)
            strand = torch.where(mapped, (best >> 55) & 1, 0)
            start = torch.full((nq,), n, dtype=torch.int64, device=dev)
            nruns = torch.zeros(nq, dtype=torch.uint8, device=dev)
            runs = torch.zeros((nq, stride), dtype=torch.int16, device=dev)
            for s in (0, 1):
                r = per[s][0][pick[s]]
                start[r], nruns[r], runs[r] = astart[s][pick[s]], anr[s][pick[s]], aruns[s][pick[s]]
            return end, start, torch.where(mapped, d, 255), strand, n_best, n_loci, nruns, runs

        def workaround():
            locate2()
            align_all()
            return reduce()

        # map into preallocated buffers
        out = dict(end=torch.empty(nq, dtype=torch.int64, device=dev),
                   start=torch.empty(nq, dtype=torch.int64, device=dev),
                   dist=torch.empty(nq, dtype=torch.uint8, device=dev),
                   strand=torch.empty(nq, dtype=torch.uint8, device=dev),
                   n_best=torch.empty(nq, dtype=torch.int32, device=dev),
                   n_loci=torch.empty(nq, dtype=torch.int32, device=dev),
                   nruns=torch.empty(nq, dtype=torch.uint8, device=dev),
                   runs=torch.empty((nq, stride), dtype=torch.int16, device=dev),
                   qflags=torch.empty(nq, dtype=torch.uint8, device=dev))

        def do_map():
            _lib.check(L.sas_map_edit_fixed(idx._h, qb.data_ptr(), m, nq, k, 0, 3, *(v.data_ptr() for v in out.values()),
                                            st, _lib.SAS_DEVICE_PTRS))

        do_map()
        got = workaround()
        torch.cuda.synchronize()
        mapped = out["dist"] != 255
        names = ("end", "start", "dist", "strand", "n_best", "n_loci", "nruns", "runs")
        equal = {f: bool(torch.equal(out[f].long(), g.long())) for f, g in zip(names, got)}
        r = out["runs"].to(torch.int32) & 0xFFFF
        ops, lens = r & 3, r >> 2
        checks = {
            "dist_is_least_of_both_answers": equal["dist"],
            "query_chars": bool(((lens * (ops != _lib.SAS_AL_DEL)).sum(1) == m * mapped).all()),
            "text_chars": bool(((lens * (ops != _lib.SAS_AL_INS)).sum(1) == out["end"] - out["start"]).all()),
            "edits": bool(((lens * (ops != _lib.SAS_AL_EQ)).sum(1) == out["dist"] * mapped).all()),
            "n_best_where_mapped": bool(torch.equal(out["n_best"] >= 1, mapped)),
            "workaround_equals_map": all(equal.values()),
        }
        # the alignment stage inside map: its own request, one alignment per read
        aoff = torch.arange(nq + 1, device=dev)
        aqoff = (out["strand"].long() * nq + ar) * m
        aqlen = torch.where(mapped, m, 0).to(torch.int32)
        wstart = torch.empty(nq, dtype=torch.int64, device=dev)

        def align_winners():
            _lib.check(L.sas_align_edit(idx._h, both.data_ptr(), aqoff.data_ptr(), aqlen.data_ptr(), nq, k,
                                        aoff.data_ptr(), out["end"].data_ptr(), nq, wstart.data_ptr(), None,
                                        out["nruns"].data_ptr(), out["runs"].data_ptr(), st, _lib.SAS_DEVICE_PTRS))

        legs = {"map": do_map, "locate2": locate2, "align_all": align_all, "align_winners": align_winners,
                "workaround": workaround}
        rec = {"nq": nq, "m": m, "k": k, "edits": [e_lo, e_hi], "ends": na, "ends_per_read": sum(na) / nq,
               "mapped": int(mapped.sum()), "reverse_winners": int(out["strand"].sum()),
               "unique": int(((out["n_best"] == 1) & (out["n_loci"] == 1)).sum()),
               "multi_best": int((out["n_best"] > 1).sum()), "checks": checks,
               "first_cigar": sas_amd.cigar(out["runs"][0], out["nruns"][0])}
        res = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                res[x].append(timed(fn, args.reps))
        ms = {x: float(np.median(v)) for x, v in res.items()}
        rec.update(ms=ms, ms_runs=res, reads_per_s=nq / (ms["map"] * 1e-3),
                   map_over_locate2=ms["map"] / ms["locate2"],
                   align_winners_over_align_all=ms["align_winners"] / ms["align_all"],
                   map_over_workaround=ms["map"] / ms["workaround"])
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    out = args.out or os.path.join(REPO, "profiles", "map", f"map_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in args.shapes.split(","):
        res["shapes"][SHAPES[name][0]] = shape(name)
        with open(out, "w") as fh:  # after every shape: a cut-short run keeps what it measured
            json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "ms": {x: v["ms"] for x, v in res["shapes"].items()},
                      "map_over_locate2": {x: v["map_over_locate2"] for x, v in res["shapes"].items()},
                      "checks": {x: v["checks"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
