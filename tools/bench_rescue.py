#!/usr/bin/env python3
"""Paired-end mapping with mate rescue (sas_map_pairs_rescue) on one MI355X, on the quad +
two-suffix p = 16 prefix table index of a generated text (n = 2^30).

Pairs are those of tools/bench_pairs.py (shapes S and L, fragments of 200..500 chars, window
(150, 550)); in `--heavy` (2 %) of them one mate, the second of an even pair and the first of an odd
one, carries k_rescue = k + 2 edits instead, more than the seeds bear.  max_anchors is 16.  Per shape
the legs run round-robin `--rounds` times (each figure the median over rounds of the median of
`--reps` event-timed calls), all on device pointers into preallocated buffers:
  pairs  sas_map_pairs_fixed(k)
  off    sas_map_pairs_rescue_fixed(k, k_rescue = k, max_anchors = 0): the same path, byte for byte
  on     sas_map_pairs_rescue_fixed(k, k + 2, max_anchors = 16)
  wide   sas_map_pairs_rescue_fixed(k, k + 2, max_anchors = 0): no scan, but every read aligned with
         k + 2 as in `on`, so on - wide is the rescue itself (anchors, scan, the wider finalize) and
         wide - off the price of the wider alignment band
  route  what a caller of the calls before this one has to do for the same records: `pairs`,
         the pairs without a proper candidate picked in torch (a host read), sas_extract of every
         window with its lead-in, Sellers' rows in torch, the least (D, e) per window, and
         sas_align_edit_fixed of both mates with k + 2.  It serves the pairs with exactly one locus
         (the single-read record is then the anchor); their share is recorded
  cNN    `on` through a library built with -DRS_CHUNK=NN (--chunk-libs NN=path/libsas_amd.so,...),
         on the same index and buffers: the sweep of the chunk length
Before timing, the records are checked on the device: `off` equals `pairs` in every output; in every
rescued pair one mate is on each strand, F lies in the window, exactly one read carries
SAS_MAP_RESCUED and its distance is within k + 2; the run lengths add up to m and to end - start
and the edits to dist; proper pairs and the counts are those of `pairs`; `route` and every cNN give
`on`'s records.  The scan's work is reported in Myers columns: per anchor spread + 1 ends and, per
chunk, m + k_rescue + 1 columns of lead-in (nominal: the cut-off and the text's ends take some
away).  JSON to --out, tagged with the source hash.
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

SHAPES = {  # name: (record key, pairs, m, k, fewest edits, most edits, seed): tools/bench_pairs.py's
    "S": ("S_5e6_pairs_len32_k1", 5_000_000, 32, 1, 1, 1, 21),
    "L": ("L_5e6_pairs_len100_k3", 5_000_000, 100, 3, 1, 3, 22),
}
FRAG = (200, 500)
WINDOW = (150, 550)
MAX_ANCHORS = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the pair counts (rehearsals)")
    ap.add_argument("--heavy", type=float, default=0.02, help="share of the pairs with a mate of k + 2 edits")
    ap.add_argument("--shapes", default="S,L")
    ap.add_argument("--chunk-libs", default="", help="NN=path,...: libraries built with -DRS_CHUNK=NN")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_rescue: needs the GPU (no CPU fallback)")
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
    chunk_libs = {}
    for item in filter(None, args.chunk_libs.split(",")):
        tag, path = item.split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        lib.sas_map_pairs_rescue_fixed.argtypes = L.sas_map_pairs_rescue_fixed.argtypes
        lib.sas_source_hash.restype = C.c_char_p
        chunk_libs[int(tag)] = (lib, lib.sas_source_hash().decode())

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
        kr = k + 2
        nq = 2 * npairs
        spread = WINDOW[1] - WINDOW[0]
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        frag = torch.randint(FRAG[0], FRAG[1] + 1, (npairs,), generator=g, device=dev)
        s = torch.randint(0, n - FRAG[1] - kr - 1, (npairs,), generator=g, device=dev)
        mate1 = edited_at(s, m, e_lo, e_hi, g).view(npairs, m)
        mate2 = edited_at(s + frag - m, m, e_lo, e_hi, g).view(npairs, m)
        # the heavy mates: the second of an even pair, the first of an odd one
        hv = torch.nonzero(torch.rand(npairs, generator=g, device=dev) < args.heavy).flatten()
        odd = hv % 2 == 1
        h1, h2 = hv[odd], hv[~odd]
        if h1.numel():
            mate1[h1] = edited_at(s[h1], m, kr, kr, g).view(-1, m)
        if h2.numel():
            mate2[h2] = edited_at((s + frag - m)[h2], m, kr, kr, g).view(-1, m)
        mate2 = sas_amd.revcomp(mate2.reshape(-1), m=m).view(npairs, m)
        swap = (torch.arange(npairs, device=dev) % 2 == 1)[:, None]
        qb = torch.cat([torch.stack([torch.where(swap, mate2, mate1), torch.where(swap, mate1, mate2)], 1).reshape(-1),
                        torch.zeros(64, dtype=torch.uint8, device=dev)])
        del mate1, mate2
        rcb = sas_amd.revcomp(qb[:nq * m], m=m)

        def buffers(stride, rescue):
            b = dict(end=torch.empty(nq, dtype=torch.int64, device=dev),
                     start=torch.empty(nq, dtype=torch.int64, device=dev),
                     dist=torch.empty(nq, dtype=torch.uint8, device=dev),
                     strand=torch.empty(nq, dtype=torch.uint8, device=dev),
                     n_best=torch.empty(nq, dtype=torch.int32, device=dev),
                     n_loci=torch.empty(nq, dtype=torch.int32, device=dev),
                     nruns=torch.empty(nq, dtype=torch.uint8, device=dev),
                     runs=torch.zeros((nq, stride), dtype=torch.int16, device=dev),
                     qflags=torch.empty(nq, dtype=torch.uint8, device=dev),
                     pflags=torch.empty(npairs, dtype=torch.uint8, device=dev),
                     n_pairs=torch.empty(npairs, dtype=torch.int32, device=dev),
                     n_best_pairs=torch.empty(npairs, dtype=torch.int32, device=dev))
            if rescue:
                b["n_rescue"] = torch.empty(npairs, dtype=torch.int32, device=dev)
            return b
        plain, off, on = buffers(2 * k + 1, False), buffers(2 * k + 1, True), buffers(2 * kr + 1, True)
        rt = buffers(2 * kr + 1, True)     # the route's records
        var = buffers(2 * kr + 1, True)    # a chunk variant's

        def do_pairs(b=plain):
            _lib.check(L.sas_map_pairs_fixed(idx._h, qb.data_ptr(), m, npairs, k, 0, WINDOW[0], WINDOW[1],
                                             *(b[f].data_ptr() for f in list(plain)), st, _lib.SAS_DEVICE_PTRS))

        def rescue(lib, b, k_r, anchors):
            rc = lib.sas_map_pairs_rescue_fixed(idx._h, qb.data_ptr(), m, npairs, k, k_r, 0, WINDOW[0], WINDOW[1],
                                                anchors, *(v.data_ptr() for v in b.values()), st,
                                                _lib.SAS_DEVICE_PTRS)
            if rc:
                raise SystemExit(f"bench_rescue: sas_map_pairs_rescue_fixed returned {rc}")

        def do_off():
            rescue(L, off, k, 0)

        def do_on():
            rescue(L, on, kr, MAX_ANCHORS)

        def do_wide():
            rescue(L, var, kr, 0)

        route_info = {}

        def do_route():
            """The records of `on` from the calls before it.  Pairs with one locus only."""
            W = spread + 1 + m + kr + 1                  # the window's ends and the lead-in columns
            do_pairs(rt)                                 # the records of k (the runs of the rescued reads follow)
            improper = rt["pflags"] == 0
            loci = rt["n_loci"][0::2].long() + rt["n_loci"][1::2].long()
            pi = torch.nonzero(improper & (loci == 1)).flatten()   # a host read: the route synchronises here
            a = 2 * pi + (rt["dist"][2 * pi] == 255).long()        # the mapped read is the anchor
            b = a ^ 1
            sa_, ea = rt["strand"][a].long(), rt["end"][a]
            lo = torch.where(sa_ == 0, ea - m + WINDOW[0], ea + m - WINDOW[1])
            w0 = lo - m - kr - 1
            ok = (w0 >= 0) & (lo + spread <= n)          # windows inside the text (the others are left out)
            pi, a, b, sa_, ea, lo, w0 = pi[ok], a[ok], b[ok], sa_[ok], ea[ok], lo[ok], w0[ok]
            na = pi.numel()
            route_info.update(served=na, one_locus=int(ok.numel()), pairs=pi)
            rt["n_rescue"].zero_()
            if na == 0:
                return
            tx = torch.empty(na * (W - 1), dtype=torch.uint8, device=dev)
            idx.extract(w0.contiguous(), torch.full((na,), W - 1, dtype=torch.int32, device=dev),
                        torch.arange(na, device=dev, dtype=torch.int64) * (W - 1), tx)
            tx = tx.view(na, W - 1)
            # the partner on the other strand: q_b for a reverse anchor, rc(q_b) for a forward one
            q = torch.where((sa_ == 1)[:, None], qb[:nq * m].view(nq, m)[b], rcb.view(nq, m)[b])
            ar = torch.arange(W, device=dev, dtype=torch.int32)[None, :]
            P = -ar.repeat(na, 1)                        # Sellers' rows as row - arange (EBrute.rows)
            S = torch.empty_like(P)
            for i in range(m):
                eq = (tx == q[:, i:i + 1]).to(torch.int32)
                S[:, 1:] = torch.minimum(P[:, 1:] + 1, P[:, :-1] - eq)
                S[:, 0] = i + 1
                P = torch.cummin(S, 1).values
            D = (P + ar)[:, m + kr + 1:].long()          # the ends lo .. lo + spread
            cand = D <= kr
            prev = torch.cat([torch.zeros(na, 1, dtype=torch.bool, device=dev), cand[:, :-1]], 1)
            rt["n_rescue"][pi] = (cand & ~prev).sum(1).to(torch.int32)
            key = torch.where(cand, D * (spread + 1) + torch.arange(spread + 1, device=dev)[None, :], 1 << 40).min(1).values
            hit = key < (1 << 40)
            pi, a, b, sa_ = pi[hit], a[hit], b[hit], sa_[hit]
            eb, db = lo[hit] + key[hit] % (spread + 1), key[hit] // (spread + 1)
            rt["end"][b], rt["dist"][b], rt["strand"][b] = eb, db.to(torch.uint8), (1 - sa_).to(torch.uint8)
            rt["qflags"][b] |= _lib.SAS_MAP_RESCUED
            rt["pflags"][pi] |= _lib.SAS_PAIR_RESCUED
            # both mates on their strands, aligned with k + 2
            r = torch.cat([a, b])
            chosen = torch.where((rt["strand"][r] == 1)[:, None], rcb.view(nq, m)[r], qb[:nq * m].view(nq, m)[r])
            al = idx.align_edit_fixed(chosen.reshape(-1).contiguous(), m, kr,
                                      torch.arange(r.numel() + 1, device=dev, dtype=torch.int64), rt["end"][r].contiguous())
            rt["start"][r], rt["nruns"][r], rt["runs"][r] = al[0], al[2], al[3]

        do_pairs()
        do_off()
        do_on()
        do_route()
        torch.cuda.synchronize()
        proper = (on["pflags"] & _lib.SAS_PAIR_PROPER) != 0
        resc = (on["pflags"] & _lib.SAS_PAIR_RESCUED) != 0
        skipped = (on["pflags"] & _lib.SAS_PAIR_RESCUE_SKIPPED) != 0
        got = (on["qflags"] & _lib.SAS_MAP_RESCUED) != 0
        placed = proper | resc
        mapped = on["dist"] != 255
        s1, s2 = on["strand"][0::2].long(), on["strand"][1::2].long()
        e1, e2 = on["end"][0::2], on["end"][1::2]
        F = torch.where(s1 == 0, e2 - e1, e1 - e2) + m
        r = on["runs"].to(torch.int32) & 0xFFFF
        ops, lens = r & 3, r >> 2
        loci = on["n_loci"][0::2].long() + on["n_loci"][1::2].long()
        eligible = ~proper & ~skipped & (loci > 0)
        heavy_pair = torch.zeros(npairs, dtype=torch.bool, device=dev)
        heavy_pair[hv] = True
        pr = torch.nonzero((rt["pflags"] & _lib.SAS_PAIR_RESCUED) != 0).flatten()   # the pairs the route rescued
        rr = torch.stack([2 * pr, 2 * pr + 1], 1).reshape(-1)
        served = route_info.get("pairs", torch.zeros(0, dtype=torch.int64, device=dev))
        checks = {
            "off_is_pairs": all(bool(torch.equal(off[f], plain[f])) for f in plain) and not bool(off["n_rescue"].any()),
            "proper_unchanged": bool(torch.equal(proper, plain["pflags"] == 1)) and
            all(bool(torch.equal(on[f], plain[f])) for f in ("n_pairs", "n_best_pairs", "n_best", "n_loci")) and
            all(bool(torch.equal(on[f][proper.repeat_interleave(2)], plain[f][proper.repeat_interleave(2)]))
                for f in ("end", "start", "dist", "strand", "nruns")),
            "rescued_not_proper": not bool((resc & proper).any()) and bool((resc <= eligible).all()),
            "one_rescued_read": bool(torch.equal(got[0::2].long() + got[1::2].long(), resc.long())),
            "one_mate_per_strand": bool(((s1 + s2 == 1) | ~placed).all()),
            "fragment_in_window": bool((((WINDOW[0] <= F) & (F <= WINDOW[1])) | ~placed).all()),
            "rescued_within_k_rescue": bool((on["dist"][got] <= kr).all()) and
            bool((on["dist"][resc.repeat_interleave(2) & ~got] <= k).all()),
            "n_rescue_only_if_eligible": bool(((on["n_rescue"] == 0) | eligible).all()) and
            bool(((on["n_rescue"] > 0) == resc).all()),
            "query_chars": bool(((lens * (ops != _lib.SAS_AL_DEL)).sum(1) == m * mapped).all()),
            "text_chars": bool(((lens * (ops != _lib.SAS_AL_INS)).sum(1) == on["end"] - on["start"]).all()),
            "edits": bool(((lens * (ops != _lib.SAS_AL_EQ)).sum(1) == on["dist"] * mapped).all()),
            "route_is_on": all(bool(torch.equal(rt[f][rr], on[f][rr])) for f in
                               ("end", "start", "dist", "strand", "nruns", "runs", "qflags")) and
            bool(torch.equal(rt["pflags"][served] & 3, on["pflags"][served] & 3)) and
            bool(torch.equal(rt["n_rescue"][served], on["n_rescue"][served])),
        }
        legs = {"pairs": do_pairs, "off": do_off, "on": do_on, "wide": do_wide, "route": do_route}
        for tag, (lib, _) in sorted(chunk_libs.items()):
            rescue(lib, var, kr, MAX_ANCHORS)
            torch.cuda.synchronize()
            checks[f"c{tag}_is_on"] = all(bool(torch.equal(var[f], on[f])) for f in on)
            legs[f"c{tag}"] = (lambda lb: lambda: rescue(lb, var, kr, MAX_ANCHORS))(lib)
        anchors = int(loci[eligible].sum())
        cpa = spread // _lib.SAS_RESCUE_CHUNK + 1
        columns = anchors * (spread + 1 + cpa * (m + kr + 1))
        rec = {"pairs": npairs, "m": m, "k": k, "k_rescue": kr, "max_anchors": MAX_ANCHORS, "edits": [e_lo, e_hi],
               "heavy_share_asked": args.heavy, "heavy_pairs": int(hv.numel()), "heavy_share": hv.numel() / npairs,
               "fragment": list(FRAG), "window": list(WINDOW), "proper": int(proper.sum()),
               "rescued": int(resc.sum()), "rescued_heavy": int((resc & heavy_pair).sum()),
               "skipped": int(skipped.sum()), "eligible": int(eligible.sum()), "anchors": anchors,
               "rescued_beyond_k": int((on["dist"][got] > k).sum()),
               "chunk": _lib.SAS_RESCUE_CHUNK, "chunks_per_anchor": cpa, "columns_nominal": columns,
               "route_one_locus_pairs": route_info.get("one_locus", 0), "route_served": route_info.get("served", 0),
               "route_rescued": int(pr.numel()), "checks": checks,
               "chunk_lib_hashes": {str(t): h for t, (_, h) in chunk_libs.items()}}
        res = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                res[x].append(timed(fn, args.reps))
        ms = {x: float(np.median(v)) for x, v in res.items()}
        extra = ms["on"] - ms["off"]
        scan = ms["on"] - ms["wide"]
        rec.update(ms=ms, ms_runs=res, off_minus_pairs_ms=ms["off"] - ms["pairs"],
                   pairs_round_spread_ms=max(res["pairs"]) - min(res["pairs"]),
                   on_minus_off_ms=extra, columns_per_s=columns / (extra * 1e-3) if extra > 0 else None,
                   on_minus_wide_ms=scan, wide_minus_off_ms=ms["wide"] - ms["off"],
                   columns_per_s_of_on_minus_wide=columns / (scan * 1e-3) if scan > 0 else None,
                   on_over_route=ms["on"] / ms["route"], route_over_on=ms["route"] / ms["on"],
                   chunk_sweep_ms={str(t): ms[f"c{t}"] for t in chunk_libs} | {str(_lib.SAS_RESCUE_CHUNK): ms["on"]},
                   chunk_sweep_extra_ms={str(t): ms[f"c{t}"] - ms["off"] for t in chunk_libs} |
                   {str(_lib.SAS_RESCUE_CHUNK): extra},
                   chunk_sweep_minus_wide_ms={str(t): ms[f"c{t}"] - ms["wide"] for t in chunk_libs} |
                   {str(_lib.SAS_RESCUE_CHUNK): scan})
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    out = args.out or os.path.join(REPO, "profiles", "rescue", f"rescue_n{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in args.shapes.split(","):
        res["shapes"][SHAPES[name][0]] = shape(name)
        with open(out, "w") as fh:  # after every shape: a cut-short run keeps what it measured
            json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "ms": {x: v["ms"] for x, v in res["shapes"].items()},
                      "checks": {x: v["checks"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
