#!/usr/bin/env python3
"""k-mismatch locate on one MI355X, on the quad + two-suffix p = 16 prefix table index of a
generated text (n = 2^30), against what a user could do on the device without it.

Queries: text slices (cut from the index with extract) with one char (S, L) or two (T)
substituted at random places:
  S  10^7 of 32 chars, k = 1       L  10^7 of 100 chars, k = 3
  T  10^6 of 32 chars, k = 2, max_seed_hits = 1024 (the 10-char seeds occur ~1024 times each)
Per shape, legs run round-robin `--rounds` times (each figure the median over rounds of the
median of `--reps` event-timed calls):
  new       locate_mismatch_fixed into a preallocated buffer (one call, one read-back inside;
            query words packed from the bytes per candidate, the default)
  new_packed the same with SAS_MM_QWORDS=packed (every query packed once into scratch)
  base      the workaround: piece offsets with torch, search_range + the seed gate, one
            locate_ranges over all pieces, extract of the m-char windows, a torch compare and
            count, torch.unique of (query, position) for the de-duplication; in chunks of
            queries so that the windows fit (2^20 queries; 2^16 on T, whose queries have ~10^3
            candidates each), timed over --base-queries queries and scaled to the shape's count
The verify kernel alone is timed by the library (SAS_MM_TIMING=1, HIP events) in a separate
pass and set against the random-request rate of --rand-rate (requests per second; DESIGN.md's
tools/randbench.hip calibration): one SA request plus the 32-B sectors an unaligned m-char
window of the 2-bit text touches per candidate.  The answers of `new`, `new_packed` and `base`
must be identical on the first --check-queries queries.  JSON to --out, tagged with the source
hash.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts (rehearsals)")
    ap.add_argument("--shapes", default="S,L,T")
    ap.add_argument("--base-queries", type=int, default=1 << 20)
    ap.add_argument("--check-queries", type=int, default=100_000)
    ap.add_argument("--rand-rate", type=float, default=0.0, help="random 32-B requests per second of the chip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_mismatch: needs the GPU (no CPU fallback)")
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

    def cut_subst(nq, m, nsub, seed):
        """nq text slices of m chars, nsub chars of each replaced by another code."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        off = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        q = torch.zeros(nq * m + 64, dtype=torch.uint8, device=dev)
        idx.extract(off, torch.full((nq,), m, dtype=torch.int32, device=dev),
                    torch.arange(nq, device=dev, dtype=torch.int64) * m, q)
        for _ in range(nsub):
            at = torch.arange(nq, device=dev) * m + torch.randint(0, m, (nq,), generator=g, device=dev)
            q[at] = (q[at] + torch.randint(1, 4, (nq,), generator=g, device=dev).to(torch.uint8)) & 3
        return q

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def baseline(qb, nq, m, k, mh, chunk):
        """(keys, dist): sorted unique query * n + position of every alignment within k, without
        locate_mismatch; chunked over the queries."""
        b = torch.tensor([j * m // (k + 1) for j in range(k + 2)], device=dev, dtype=torch.int64)
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
            s = pos - b[piece % (k + 1)]
            keep = (s >= 0) & (s + m <= n)
            s, query = s[keep], query[keep]
            nc = int(s.numel())
            win = torch.empty(max(nc * m, 1), dtype=torch.uint8, device=dev)
            idx.extract(s, torch.full((nc,), m, dtype=torch.int32, device=dev),
                        torch.arange(nc, device=dev, dtype=torch.int64) * m, win)
            qv = qb[c0 * m:c1 * m].view(cq, m)
            d = (win[:nc * m].view(nc, m) != qv[query]).sum(1)
            ok = d <= k
            key = (query[ok] + c0) * n + s[ok]
            uk, inv = torch.unique(key, return_inverse=True)
            ud = torch.empty_like(uk)
            ud[inv] = d[ok]
            keys.append(uk)
            dists.append(ud)
        return torch.cat(keys), torch.cat(dists)

    def new_call(qb, nq, m, k, mh, out, variant="bytes", dist=True):
        os.environ["SAS_MM_QWORDS"] = variant
        return idx.locate_mismatch_fixed(qb[:nq * m], m, k, max_seed_hits=mh, out=out, dist=dist)

    def as_keys(res, nq):
        off, pos, dist, _ = res
        total = int(off[nq])
        query = torch.repeat_interleave(torch.arange(nq, device=dev), off[1:] - off[:-1])
        key = query * n + pos[:total]
        order = torch.argsort(key)
        return key[order], dist[:total][order].to(torch.int64)

    def shape(name, nq, m, k, mh, seed):
        qb = cut_subst(nq, m, 2 if name == "T" else 1, seed)
        chunk = 1 << (16 if name == "T" else 20)
        # size the output once (the sizing call), then every timed call is one pipeline
        off = idx.locate_mismatch_fixed(qb[:nq * m], m, k, max_seed_hits=mh, capacity=0, dist=False)[0]
        total = int(off[nq])
        out = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        nb = min(nq, max(int(args.base_queries * args.scale), 1))
        legs = {
            "new": lambda: new_call(qb, nq, m, k, mh, out),
            "new_packed": lambda: new_call(qb, nq, m, k, mh, out, "packed"),
            "base": lambda: baseline(qb, nb, m, k, mh, chunk),
        }
        runs = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                runs[x].append(timed(fn))
        ms = {x: float(np.median(v)) for x, v in runs.items()}
        ms["base_scaled"] = ms["base"] * nq / nb
        # the verify kernel alone, both variants (the library's HIP events; synchronises)
        os.environ["SAS_MM_TIMING"] = "1"
        verify, cand = {}, C.c_uint64(0)
        for variant in ("bytes", "packed"):
            v = []
            for _ in range(args.reps):
                new_call(qb, nq, m, k, mh, out, variant)
                v.append(L.sas_locate_mismatch_verify_ms(C.byref(cand)))
            verify[variant] = float(np.median(v))
        os.environ["SAS_MM_TIMING"] = "0"
        # identical answers on a subsample
        nc = min(nq, args.check_queries)
        bk, bd = baseline(qb, nc, m, k, mh, chunk)
        ok = True
        for variant in ("bytes", "packed"):
            gk, gd = as_keys(new_call(qb, nc, m, k, mh, None, variant), nc)
            ok &= bool(torch.equal(gk, bk)) and bool(torch.equal(gd, bd))
        qfl = new_call(qb, nq, m, k, mh, out)[3]
        torch.cuda.synchronize()
        # an unaligned m-char window of the 2-bit text: m / 4 bytes at a random 2-bit offset
        sectors = (m / 4 - 1 / 4) / 32 + 1
        req = cand.value * (1 + sectors)
        rec = {"nq": nq, "m": m, "k": k, "max_seed_hits": mh, "ms": ms, "ms_runs": runs,
               "base_queries": nb, "new_over_base": ms["new"] / ms["base_scaled"],
               "new_faster": ms["new"] < ms["base_scaled"], "queries_per_s": nq / (ms["new"] * 1e-3),
               "alignments": total, "candidates": cand.value, "candidates_per_query": cand.value / nq,
               "truncated_queries": int((qfl & _lib.SAS_MM_TRUNCATED != 0).sum()),
               "verify_ms": verify, "candidates_per_s": cand.value / (verify["bytes"] * 1e-3),
               "model_requests_per_candidate": 1 + sectors,
               "model_requests_per_s": req / (verify["bytes"] * 1e-3),
               "fraction_of_rand_rate": (req / (verify["bytes"] * 1e-3) / args.rand_rate) if args.rand_rate else None,
               "identical_to_base": ok, "check_queries": nc}
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    import ctypes as C
    sc = args.scale
    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "rand_rate": args.rand_rate, "shapes": {}}
    want = args.shapes.split(",")
    if "S" in want:
        res["shapes"]["S_1e7_len32_k1"] = shape("S", max(int(10_000_000 * sc), 1), 32, 1, 0, 11)
    if "L" in want:
        res["shapes"]["L_1e7_len100_k3"] = shape("L", max(int(10_000_000 * sc), 1), 100, 3, 0, 12)
    if "T" in want:
        res["shapes"]["T_1e6_len32_k2_cap1024"] = shape("T", max(int(1_000_000 * sc), 1), 32, 2, 1024, 13)
    out = args.out or os.path.join(REPO, "profiles", "mismatch", f"mismatch_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "new_over_base": {x: v["new_over_base"] for x, v in res["shapes"].items()},
                      "identical": {x: v["identical_to_base"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
