#!/usr/bin/env python3
"""Longest-prefix match on one MI355X, on the quad + default prefix table index of a generated
text (n = 2^30), against what it is made of and what it replaces.

Queries: text slices with ONE substituted char at a random offset (the read with a mismatch):
  S  10^7 of 32 chars      L  10^6 of 100 chars
Per shape, in one process, the five legs run round-robin `--rounds` times (each leg's figure is
the median over rounds of the median of `--reps` event-timed calls), so slow drift hits all alike:
  a  match_fixed, ranges=False                 the match kernel alone
  b  match_fixed, ranges=True                  + one range search on (q, len)
  c  search_fixed(algo="lcp", SAS_PREFIX_RANGE)  the same probes without the neighbour step
  d  one search_range_fixed call on the full queries
  e  ceil(log2(m + 1)) search_range calls over truncated lengths: bisection on the length, the
     only way to get `len` without sas_match (device-side length updates, no host round trip:
     a lower bound on what that workaround costs)
Ratios a/c, b/(c + d), b/e go to the record.  One matching-statistics figure: a 10^6-char
pattern (slices with substitutions), max_len = 64.  A sample of every shape's answers is
checked against the text.  The result goes to --out as JSON tagged with the source hash.
"""
import argparse
import json
import math
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
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_match: needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.n
    t0 = time.perf_counter()
    text = sas_amd.random_string(n, seed=args.seed, device=dev)
    idx = sas_amd.SaNaive.build(text, lcp=False, stree=False, sector=False, llcp=False)
    torch.cuda.synchronize()
    stats = idx.stats()
    print(f"index built in {time.perf_counter() - t0:.1f} s (p = {stats['prefix_chars']})", file=sys.stderr)

    def cut_subst(nq, m, seed):
        """nq slices of m chars, one char of each replaced by another code."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        off = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        ar = torch.arange(m, device=dev)
        q = torch.empty(nq * m + 64, dtype=torch.uint8, device=dev)
        q[nq * m:] = 0
        for s in range(0, nq, 1 << 18):
            e = min(nq, s + (1 << 18))
            q[s * m:e * m] = text[(off[s:e, None] + ar[None, :]).reshape(-1)]
        j = torch.randint(0, m, (nq,), generator=g, device=dev)
        at = torch.arange(nq, device=dev) * m + j
        q[at] = (q[at] + torch.randint(1, 4, (nq,), generator=g, device=dev).to(torch.uint8)) & 3
        return q, j

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

    def shape(name, nq, m, seed):
        q, j = cut_subst(nq, m, seed)
        qb = q[:nq * m]
        qoff = torch.arange(nq, device=dev, dtype=torch.int64) * m
        steps = math.ceil(math.log2(m + 1))
        lo_k = torch.empty(nq, dtype=torch.int32, device=dev)
        hi_k = torch.empty(nq, dtype=torch.int32, device=dev)

        def bisect_len():
            """len by bisection on the prefix length: `steps` range searches."""
            lo_k.zero_()
            hi_k.fill_(m)
            for _ in range(steps):
                mid = (lo_k + hi_k + 1) >> 1
                lo, hi = idx.search_range(q, qoff, mid)
                occ = hi > lo
                lo_k.copy_(torch.where(occ, mid, lo_k))
                hi_k.copy_(torch.where(occ, hi_k, mid - 1))
            return lo_k

        legs = {
            "a_match": lambda: idx.match_fixed(qb, m, ranges=False),
            "b_match_ranges": lambda: idx.match_fixed(qb, m, ranges=True),
            "c_search_lcp_prefix_range": lambda: idx.search_fixed(qb, m, algo="lcp", flags=_lib.SAS_PREFIX_RANGE),
            "d_search_range": lambda: idx.search_range_fixed(qb, m),
            "e_bisect_ranges": bisect_len,
        }
        runs = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                runs[k].append(timed(fn))
        ms = {k: float(np.median(v)) for k, v in runs.items()}
        # the answers: against the text, against the bisection, and the no-table path
        ln, pos, lo, hi = idx.match_fixed(qb, m, ranges=True)
        ln2, pos2 = idx.match_fixed(qb, m, ranges=False, flags=_lib.SAS_NO_PREFIX_TABLE)
        blen = bisect_len().clone()
        torch.cuda.synchronize()
        ok = bool(torch.equal(ln, blen)) and bool(torch.equal(ln, ln2)) and bool((ln >= j).all()) and bool((hi > lo).all())
        for k in torch.randint(0, nq, (500,)).tolist():
            p, c = int(pos[k]), int(ln[k])
            ok &= bool(torch.equal(text[p:p + c], qb[k * m:k * m + c]))
        rec = {"nq": nq, "m": m, "range_calls_in_e": steps, "ms": ms, "ms_runs": runs,
               "queries_per_s_a": nq / (ms["a_match"] * 1e-3), "queries_per_s_b": nq / (ms["b_match_ranges"] * 1e-3),
               "a_over_c": ms["a_match"] / ms["c_search_lcp_prefix_range"],
               "b_over_c_plus_d": ms["b_match_ranges"] / (ms["c_search_lcp_prefix_range"] + ms["d_search_range"]),
               "b_over_e": ms["b_match_ranges"] / ms["e_bisect_ranges"],
               "b_below_e": ms["b_match_ranges"] < ms["e_bisect_ranges"],
               "mean_len": float(ln.float().mean()), "full_matches": int((ln == m).sum()), "verified": ok}
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    sc = args.scale
    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    res["shapes"]["S_1e7_len32"] = shape("S", max(int(10_000_000 * sc), 1), 32, 11)
    res["shapes"]["L_1e6_len100"] = shape("L", max(int(1_000_000 * sc), 1), 100, 12)
    # matching statistics: a pattern of slices with substitutions, every start position
    plen, max_len = max(int(1_000_000 * sc), 64), 64
    pat, _ = cut_subst(plen // 50 + 1, 50, 13)
    pat = pat[:plen]
    runs = [timed(lambda: idx.match_stats(pat, max_len, ranges=False)) for _ in range(args.rounds)]
    runs_r = [timed(lambda: idx.match_stats(pat, max_len, ranges=True)) for _ in range(args.rounds)]
    ln, pos = idx.match_stats(pat, max_len, ranges=False)
    torch.cuda.synchronize()
    ok = bool((ln[1:] >= ln[:-1] - 1).all())
    for k in torch.randint(0, plen, (500,)).tolist():
        p, c = int(pos[k]), int(ln[k])
        ok &= bool(torch.equal(text[p:p + c], pat[k:k + c]))
    res["stats_1e6_maxlen64"] = {"plen": plen, "max_len": max_len, "ms": float(np.median(runs)), "ms_runs": runs,
                                 "ms_with_ranges": float(np.median(runs_r)), "ms_with_ranges_runs": runs_r,
                                 "positions_per_s": plen / (float(np.median(runs)) * 1e-3),
                                 "mean_len": float(ln.float().mean()), "verified": ok}
    print("stats: " + json.dumps(res["stats_1e6_maxlen64"]), file=sys.stderr)
    out = args.out or os.path.join(REPO, "profiles", "match", f"match_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "b_over_e": {k: v["b_over_e"] for k, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
