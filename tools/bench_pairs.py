#!/usr/bin/env python3
"""Paired-end mapping (sas_map_pairs) on one MI355X, on the quad + two-suffix p = 16 prefix table
index of a generated text (n = 2^30), against sas_map_edit over the same reads.

Pairs are cut on the device: a fragment t[s .. s + L) with L uniform in [200, 500], mate 1 = the
first m chars, mate 2 = the reverse complement (sas_revcomp_fixed) of the last m chars, both with
the edits of tools/bench_map.py (drawn uniformly from substitution, insertion and deletion at
random places); every second pair has its mates swapped.  The window is (150, 550).
  S  5 x 10^6 pairs of 32-char mates, k = 1, one edit
  L  5 x 10^6 pairs of 100-char mates, k = 3, 1..3 edits
Per shape two legs run round-robin `--rounds` times (each figure the median over rounds of the
median of `--reps` event-timed calls), both on device pointers into preallocated buffers:
  pairs  sas_map_pairs_fixed
  map    sas_map_edit_fixed over the same 2 np interleaved reads: the same seeds, verify, sort and
         one alignment per read, so the difference is the loci compaction, the join and the finalize
Before timing, the records are checked on the device: in every proper pair one mate is on each
strand and F = e_rev - e_fwd + m lies in the window; the run lengths add up to m and to
end - start and the edits to dist; n_best, n_loci and qflags equal map's; the reads of a pair that
is not proper carry map's record.  JSON to --out, tagged with the source hash.
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

SHAPES = {  # name: (record key, pairs, m, k, fewest edits, most edits, seed)
    "S": ("S_5e6_pairs_len32_k1", 5_000_000, 32, 1, 1, 1, 21),
    "L": ("L_5e6_pairs_len100_k3", 5_000_000, 100, 3, 1, 3, 22),
}
FRAG = (200, 500)
WINDOW = (150, 550)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the pair counts (rehearsals)")
    ap.add_argument("--shapes", default="S,L")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairs: needs the GPU (no CPU fallback)")
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

    def edited_at(off, m, e_lo, e_hi, g, chunk=1 << 20):
        """One read of m chars per offset: the text slice there after e_lo..e_hi edits, of uniformly
        drawn kinds (tools/bench_map.py: cut_edited)."""
        nq = off.numel()
        w = m + e_hi  # spare chars behind the slice: a deletion pulls one in
        q = torch.zeros(nq * m, dtype=torch.uint8, device=dev)
        col = torch.arange(w, device=dev)[None, :]
        for c0 in range(0, nq, chunk):
            cq = min(nq, c0 + chunk) - c0
            buf = torch.zeros(cq * w, dtype=torch.uint8, device=dev)
            idx.extract(off[c0:c0 + cq].contiguous(), torch.full((cq,), w, dtype=torch.int32, device=dev),
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
        _, npairs, m, k, e_lo, e_hi, seed = SHAPES[name]
        npairs = max(int(npairs * args.scale), 1)
        nq, stride = 2 * npairs, 2 * k + 1
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        frag = torch.randint(FRAG[0], FRAG[1] + 1, (npairs,), generator=g, device=dev)
        s = torch.randint(0, n - FRAG[1] - e_hi - 1, (npairs,), generator=g, device=dev)
        mate1 = edited_at(s, m, e_lo, e_hi, g).view(npairs, m)
        mate2 = sas_amd.revcomp(edited_at(s + frag - m, m, e_lo, e_hi, g), m=m).view(npairs, m)
        swap = (torch.arange(npairs, device=dev) % 2 == 1)[:, None]
        qb = torch.cat([torch.stack([torch.where(swap, mate2, mate1), torch.where(swap, mate1, mate2)], 1).reshape(-1),
                        torch.zeros(64, dtype=torch.uint8, device=dev)])
        del mate1, mate2

        def buffers():
            return dict(end=torch.empty(nq, dtype=torch.int64, device=dev),
                        start=torch.empty(nq, dtype=torch.int64, device=dev),
                        dist=torch.empty(nq, dtype=torch.uint8, device=dev),
                        strand=torch.empty(nq, dtype=torch.uint8, device=dev),
                        n_best=torch.empty(nq, dtype=torch.int32, device=dev),
                        n_loci=torch.empty(nq, dtype=torch.int32, device=dev),
                        nruns=torch.empty(nq, dtype=torch.uint8, device=dev),
                        runs=torch.empty((nq, stride), dtype=torch.int16, device=dev),
                        qflags=torch.empty(nq, dtype=torch.uint8, device=dev))
        one = buffers()
        out = buffers()
        out.update(pflags=torch.empty(npairs, dtype=torch.uint8, device=dev),
                   n_pairs=torch.empty(npairs, dtype=torch.int32, device=dev),
                   n_best_pairs=torch.empty(npairs, dtype=torch.int32, device=dev))

        def do_map():
            _lib.check(L.sas_map_edit_fixed(idx._h, qb.data_ptr(), m, nq, k, 0, 3, *(v.data_ptr() for v in one.values()),
                                            st, _lib.SAS_DEVICE_PTRS))

        def do_pairs():
            _lib.check(L.sas_map_pairs_fixed(idx._h, qb.data_ptr(), m, npairs, k, 0, WINDOW[0], WINDOW[1],
                                             *(v.data_ptr() for v in out.values()), st, _lib.SAS_DEVICE_PTRS))

        do_map()
        do_pairs()
        torch.cuda.synchronize()
        proper = out["pflags"] == 1
        per_read = proper.repeat_interleave(2)
        mapped = out["dist"] != 255
        s1, s2 = out["strand"][0::2].long(), out["strand"][1::2].long()
        e1, e2 = out["end"][0::2], out["end"][1::2]
        F = torch.where(s1 == 0, e2 - e1, e1 - e2) + m  # the forward mate is the one on strand 0
        r = out["runs"].to(torch.int32) & 0xFFFF
        ops, lens = r & 3, r >> 2
        differs = ((out["end"] != one["end"]) | (out["strand"] != one["strand"])).view(npairs, 2).any(1)
        checks = {
            "one_mate_per_strand": bool(((s1 + s2 == 1) | ~proper).all()),
            "fragment_in_window": bool((((WINDOW[0] <= F) & (F <= WINDOW[1])) | ~proper).all()),
            "proper_reads_mapped": bool((mapped | ~per_read).all()),
            "flags_and_counts": bool(torch.equal(proper, out["n_pairs"] > 0) and
                                     torch.equal(out["n_pairs"] > 0, out["n_best_pairs"] > 0) and
                                     bool((out["n_best_pairs"].long() <= out["n_pairs"].long()).all())),
            "query_chars": bool(((lens * (ops != _lib.SAS_AL_DEL)).sum(1) == m * mapped).all()),
            "text_chars": bool(((lens * (ops != _lib.SAS_AL_INS)).sum(1) == out["end"] - out["start"]).all()),
            "edits": bool(((lens * (ops != _lib.SAS_AL_EQ)).sum(1) == out["dist"] * mapped).all()),
            "single_read_counts": all(bool(torch.equal(out[f], one[f])) for f in ("n_best", "n_loci", "qflags")),
            "not_proper_is_map": all(bool(torch.equal(out[f][~per_read], one[f][~per_read])) for f in one),
            "moved_only_if_proper": bool((proper | ~differs).all()),
        }
        legs = {"pairs": do_pairs, "map": do_map}
        rec = {"pairs": npairs, "m": m, "k": k, "edits": [e_lo, e_hi], "fragment": list(FRAG), "window": list(WINDOW),
               "proper": int(proper.sum()), "proper_share": float(proper.float().mean()),
               "moved": int(differs.sum()), "moved_share": float(differs.float().mean()),
               "multi_best_pairs": int((out["n_best_pairs"] > 1).sum()),
               "max_n_pairs": int(out["n_pairs"].max()), "mapped_reads": int(mapped.sum()),
               "mapped_reads_single": int((one["dist"] != 255).sum()), "checks": checks}
        res = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                res[x].append(timed(fn, args.reps))
        ms = {x: float(np.median(v)) for x, v in res.items()}
        rec.update(ms=ms, ms_runs=res, pairs_per_s=npairs / (ms["pairs"] * 1e-3), pairs_over_map=ms["pairs"] / ms["map"],
                   pairs_minus_map_ms=ms["pairs"] - ms["map"])
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    out = args.out or os.path.join(REPO, "profiles", "pairs", f"pairs_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in args.shapes.split(","):
        res["shapes"][SHAPES[name][0]] = shape(name)
        with open(out, "w") as fh:  # after every shape: a cut-short run keeps what it measured
            json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "ms": {x: v["ms"] for x, v in res["shapes"].items()},
                      "pairs_over_map": {x: v["pairs_over_map"] for x, v in res["shapes"].items()},
                      "checks": {x: v["checks"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
