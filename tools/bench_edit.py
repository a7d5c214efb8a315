#!/usr/bin/env python3
"""k-difference locate (edit distance) on one MI355X, on the quad + two-suffix p = 16 prefix table
index of a generated text (n = 2^30), against what a user could do on the device without it.

Queries are made on the device: text slices with edits drawn uniformly from substitution,
insertion and deletion at random places (the slice is cut longer and the first m chars kept):
  S  10^7 of 32 chars, k = 1, one edit        L  10^7 of 100 chars, k = 3, 1..3 edits
  T  10^6 of 32 chars, k = 2, 1..2 edits, max_seed_hits = 1024 (the 10-char seeds occur ~1024
     times each)
Per shape, legs run round-robin `--rounds` times (each figure the median over rounds of the
median of `--reps` event-timed calls):
  new       locate_edit_fixed into a preallocated buffer (one call, two read-backs inside)
  mismatch  locate_mismatch_fixed at the same m and k on the same queries: context only, it
            answers a different, smaller question (with --legs mismatch alone the tool needs
            nothing of the k-difference call, so it also runs on a library without it)
  base      the workaround: piece offsets with torch, search_range + the seed gate, one
            locate_ranges over all pieces, extract of the (m + 3k)-char windows, a batched
            free-start Sellers dynamic program in torch (one row per query char, the horizontal
            term through cummin of row - arange) and torch.unique of (query, end); in chunks of
            queries so that the windows fit, timed over --base-queries queries (a sixteenth of
            them on T, whose queries have ~10^3 candidates each) and scaled to the shape's count
The verify kernel and the de-duplication alone are timed by the library (SAS_ED_TIMING=1, HIP
events) in a separate pass.  The answers of `new` and `base` must be identical on the first
--check-queries queries.  JSON to --out, tagged with the source hash.
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

SHAPES = {  # name: (record key, queries, m, k, max_seed_hits, fewest edits, most edits, seed)
    "S": ("S_1e7_len32_k1", 10_000_000, 32, 1, 0, 1, 1, 11),
    "L": ("L_1e7_len100_k3", 10_000_000, 100, 3, 0, 1, 3, 12),
    "T": ("T_1e6_len32_k2_cap1024", 1_000_000, 32, 2, 1024, 1, 2, 13),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts (rehearsals)")
    ap.add_argument("--shapes", default="S,L,T")
    ap.add_argument("--legs", default="new,mismatch,base")
    ap.add_argument("--base-queries", type=int, default=1 << 20)
    ap.add_argument("--check-queries", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit: needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.n
    want_legs = args.legs.split(",")
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
                # an insertion at `at` shifts the chars from there one to the right, a deletion
                # pulls the chars behind it one to the left
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

    def baseline(qb, nq, m, k, mh, chunk):
        """(keys, dist): sorted unique query * (n + 1) + end of every end within k, without
        locate_edit; chunked over the queries."""
        b = torch.tensor([j * m // (k + 1) for j in range(k + 2)], device=dev, dtype=torch.int64)
        wd = m + 3 * k
        ar = torch.arange(wd + 1, device=dev, dtype=torch.int16)[None, :]
        keys, dists = [], []
        for c0 in range(0, nq, chunk):
            c1 = min(nq, c0 + chunk)
            cq = c1 - c0
            qoff = (torch.arange(c0, c1, device=dev, dtype=torch.int64) * m)[:, None] + b[None, :-1]
            plen = (b[1:] - b[:-1]).to(torch.int32)[None, :].expand(cq, k + 1).contiguous()
            lo, hi = idx.search_range(qb, qoff.reshape(-1).contiguous(), plen.reshape(-1))
            if mh:
                hi = torch.where(hi - lo > mh, lo, hi)
            off, pos = idx.locate_ranges(lo, hi)
            piece = torch.repeat_interleave(torch.arange(cq * (k + 1), device=dev), off[1:] - off[:-1])
            query = piece // (k + 1)
            s0 = pos - b[piece % (k + 1)]
            w0 = (s0 - 2 * k).clamp(min=0)
            w1 = (s0 + m + k).clamp(max=n)
            nc = int(s0.numel())
            win = torch.full((max(nc * wd, 1),), 4, dtype=torch.uint8, device=dev)  # 4: behind the window
            idx.extract(w0, (w1 - w0).to(torch.int32), torch.arange(nc, device=dev, dtype=torch.int64) * wd, win)
            win = win[:nc * wd].view(nc, wd)
            qv = qb[c0 * m:c1 * m].view(cq, m)[query]
            # Sellers' rows minus arange: P[e] = D(e) - e; free start, so row 0 is 0
            P = (torch.zeros((nc, wd + 1), dtype=torch.int16, device=dev) - ar).contiguous()
            for i in range(m):
                S = torch.empty_like(P)
                S[:, 0] = i + 1
                S[:, 1:] = torch.minimum(P[:, 1:] + 1, P[:, :-1] - (win == qv[:, i:i + 1]).to(torch.int16))
                P = torch.cummin(S, dim=1).values
            D = P + ar
            e = w0[:, None] + ar.long()
            ok = (D <= k) & (e <= w1[:, None]) & ((e - (s0 + m)[:, None]).abs() <= k)
            key = ((query + c0)[:, None] * (n + 1) + e)[ok]
            uk, inv = torch.unique(key, return_inverse=True)
            ud = torch.empty_like(uk)
            ud[inv] = D[ok].long()
            keys.append(uk)
            dists.append(ud)
        return torch.cat(keys), torch.cat(dists)

    def as_keys(res, nq):
        off, end, dist, _ = res
        total = int(off[nq])
        query = torch.repeat_interleave(torch.arange(nq, device=dev), off[1:] - off[:-1])
        return query * (n + 1) + end[:total], dist[:total].to(torch.int64)  # already ascending

    def shape(name):
        _, nq, m, k, mh, e_lo, e_hi, seed = SHAPES[name]
        nq = max(int(nq * args.scale), 1)
        qb = cut_edited(nq, m, e_lo, e_hi, seed)
        chunk = 1 << (14 if name == "T" else 20)
        nb = min(nq, max(int(args.base_queries * args.scale) >> (4 if name == "T" else 0), 1))
        legs, rec = {}, {"nq": nq, "m": m, "k": k, "max_seed_hits": mh, "edits": [e_lo, e_hi], "base_queries": nb}
        if "new" in want_legs:
            # size the output once (the sizing call), then every timed call is one pipeline
            total = int(idx.locate_edit_fixed(qb[:nq * m], m, k, max_seed_hits=mh, capacity=0, dist=False)[0][nq])
            out = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            legs["new"] = lambda: idx.locate_edit_fixed(qb[:nq * m], m, k, max_seed_hits=mh, out=out)
            rec["ends"] = total
        if "mismatch" in want_legs:
            mtotal = int(idx.locate_mismatch_fixed(qb[:nq * m], m, k, max_seed_hits=mh, capacity=0,
                                                   dist=False)[0][nq])
            mout = torch.empty(max(mtotal, 1), dtype=torch.int64, device=dev)
            legs["mismatch"] = lambda: idx.locate_mismatch_fixed(qb[:nq * m], m, k, max_seed_hits=mh, out=mout)
            rec["mismatch_alignments"] = mtotal
        if "base" in want_legs:
            legs["base"] = lambda: baseline(qb, nb, m, k, mh, chunk)
        runs = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                runs[x].append(timed(fn, args.base_reps if x == "base" else args.reps))
        ms = {x: float(np.median(v)) for x, v in runs.items()}
        if "base" in ms:
            ms["base_scaled"] = ms["base"] * nq / nb
        rec.update(ms=ms, ms_runs=runs)
        if "new" in legs:
            rec["queries_per_s"] = nq / (ms["new"] * 1e-3)
            # the verify kernel and the de-duplication alone (the library's HIP events; synchronises)
            os.environ["SAS_ED_TIMING"] = "1"
            ver, ded, cand, prop = [], [], C.c_uint64(0), C.c_uint64(0)
            for _ in range(args.reps):
                legs["new"]()
                ver.append(L.sas_locate_edit_verify_ms(C.byref(cand)))
                ded.append(L.sas_locate_edit_dedup_ms(C.byref(prop)))
            os.environ["SAS_ED_TIMING"] = "0"
            qfl = legs["new"]()[3]
            torch.cuda.synchronize()
            rec.update(candidates=cand.value, candidates_per_query=cand.value / nq, proposals=prop.value,
                       verify_ms=float(np.median(ver)), dedup_ms=float(np.median(ded)),
                       verify_share=float(np.median(ver)) / ms["new"], dedup_share=float(np.median(ded)) / ms["new"],
                       candidates_per_s=cand.value / (float(np.median(ver)) * 1e-3),
                       truncated_queries=int((qfl & _lib.SAS_ED_TRUNCATED != 0).sum()))
            if "mismatch" in ms:
                rec["new_over_mismatch_same_library"] = ms["new"] / ms["mismatch"]
        if "new" in legs and "base" in legs:
            rec.update(new_over_base=ms["new"] / ms["base_scaled"],
                       new_faster=max(runs["new"]) < min(runs["base"]) * nq / nb)
            # identical answers on a subsample
            nc = min(nq, args.check_queries)
            bk, bd = baseline(qb, nc, m, k, mh, chunk)
            gk, gd = as_keys(idx.locate_edit_fixed(qb[:nc * m], m, k, max_seed_hits=mh), nc)
            rec.update(identical_to_base=bool(torch.equal(gk, bk)) and bool(torch.equal(gd, bd)), check_queries=nc,
                       check_ends=int(bk.numel()))
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "base_reps": args.base_reps,
           "rounds": args.rounds, "warmup": args.warmup, "legs": want_legs, "shapes": {}}
    out = args.out or os.path.join(REPO, "profiles", "edit", f"edit_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in args.shapes.split(","):
        res["shapes"][SHAPES[name][0]] = shape(name)
        with open(out, "w") as fh:  # after every shape: a cut-short run keeps what it measured
            json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "ms": {x: v["ms"] for x, v in res["shapes"].items()},
                      "new_over_base": {x: v.get("new_over_base") for x, v in res["shapes"].items()},
                      "identical": {x: v.get("identical_to_base") for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
