#!/usr/bin/env python3
"""Maximal exact matches (sas_mems) on one MI355X, on the quad + two-suffix p = 16 prefix table
index of a generated text (n = 2^30), against what a user could do on the device without it.

Shapes (queries cut from the index with extract, chars substituted at random places):
  R  10^6 reads of 150 chars, 3 substituted chars each, L = 20
  G  one slice of 10^7 chars with a substitution every ~1,000 chars, L = 32
  H  10^5 reads of 150 chars, 3 substituted chars each, L = 12, max_hits = 1024
Per shape, legs run round-robin `--rounds` times (each figure the median over rounds of the median
of `--reps` event-timed calls):
  new   mems_fixed (R, H) / mems (G) into a preallocated buffer (one call)
  base  the workaround: window offsets with torch, search_range, the gate, one locate_ranges over all
        windows, extract of the left char, extract of 64-char chunks and a torch compare repeated
        while matches go on, a mask; in chunks of windows so that the chunks fit, timed over
        --base-windows windows and scaled to the shape's count
The verify kernel alone is timed by the library (SAS_MEM_TIMING=1, HIP events) in a separate pass;
its candidate rate is written next to k_mm_verify's on the same index in the same process
(SAS_MM_TIMING=1, 10^7 reads of 32 chars, one substituted char, k = 1: shape S of
tools/bench_mismatch.py).  The answers of `new` and `base` must be identical, element for element
and in order, on the first --check-windows windows.  JSON to --out, tagged with the source hash.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=31415)
    ap.add_argument("--prefix-chars", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the query counts and G's length (rehearsals)")
    ap.add_argument("--shapes", default="R,G,H")
    ap.add_argument("--base-windows", type=int, default=1 << 22)
    ap.add_argument("--check-windows", type=int, default=1 << 21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sas_amd
    from sas_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_mems: needs the GPU (no CPU fallback)")
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
    i64, i32 = torch.int64, torch.int32

    def cut_subst(nq, m, nsub, seed):
        """nq text slices of m chars, nsub chars of each replaced by another code (64 spare bytes)."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        off = torch.randint(0, n - m, (nq,), generator=g, device=dev)
        q = torch.zeros(nq * m + 64, dtype=torch.uint8, device=dev)
        idx.extract(off, torch.full((nq,), m, dtype=i32, device=dev), torch.arange(nq, device=dev, dtype=i64) * m, q)
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

    def baseline(qb, nq, m, Lm, mh, nwin, chunk):
        """(query, qpos, tpos, len) of the MEMs of the first nwin windows (window w = query w // per,
        offset w % per), in the call's order, without sas_mems; chunked over the windows."""
        per = m - Lm + 1
        outs = []
        qpad = torch.cat([qb[:nq * m], torch.full((64,), 4, dtype=torch.uint8, device=dev)])
        for w0 in range(0, nwin, chunk):
            w1 = min(nwin, w0 + chunk)
            w = torch.arange(w0, w1, device=dev, dtype=i64)
            qoff = (w // per) * m + w % per
            lo, hi = idx.search_range(qb, qoff, torch.full((w1 - w0,), Lm, dtype=i32, device=dev))
            if mh:
                hi = torch.where(hi - lo > mh, lo, hi)
            off, j = idx.locate_ranges(lo, hi)
            cw = torch.repeat_interleave(w, off[1:] - off[:-1])
            q, i = cw // per, cw % per
            keep = j + Lm <= n
            q, i, j = q[keep], i[keep], j[keep]
            nc = int(j.numel())
            # the left char: one extract of one char per candidate
            left = torch.full((max(nc, 1),), 5, dtype=torch.uint8, device=dev)
            has = (i > 0) & (j > 0)
            idx.extract(torch.where(has, j - 1, j), has.to(i32), torch.arange(nc, device=dev, dtype=i64), left)
            ql = qpad[q * m + torch.clamp(i - 1, min=0)]
            keep = ~(has & (left[:nc] == ql))
            q, i, j = q[keep], i[keep], j[keep]
            nc = int(j.numel())
            ln = torch.full((nc,), Lm, dtype=i64, device=dev)
            act = torch.arange(nc, device=dev, dtype=i64)
            ar = torch.arange(64, device=dev, dtype=i64)
            while act.numel():
                na = int(act.numel())
                s = j[act] + ln[act]
                room = torch.clamp(torch.minimum(n - s, m - i[act] - ln[act]), min=0, max=64)
                win = torch.full((na * 64,), 5, dtype=torch.uint8, device=dev)
                idx.extract(torch.clamp(s, max=n - 1), room.to(i32), torch.arange(na, device=dev, dtype=i64) * 64, win)
                qi = torch.clamp((q[act] * m + i[act] + ln[act])[:, None] + ar[None, :], max=nq * m + 63)
                eq = (win.view(na, 64) == qpad[qi]) & (ar[None, :] < room[:, None])
                run = torch.cumprod(eq.to(torch.int8), 1).sum(1)
                ln[act] += run
                act = act[run == 64]
            outs.append((q, i, j, ln))
        return tuple(torch.cat([o[k] for o in outs]) for k in range(4))

    def shape(name, nq, m, Lm, mh, qb):
        per = m - Lm + 1
        nwin = nq * per
        ragged = nq == 1
        qoff = torch.zeros(1, dtype=i64, device=dev)
        qlen = torch.full((1,), m, dtype=i32, device=dev)

        def new_call(cnt, out=None, capacity=None):
            if ragged:
                return idx.mems(qb[:m + 64], qoff, qlen, Lm, max_hits=mh, out=out, capacity=capacity)
            return idx.mems_fixed(qb[:cnt * m], m, Lm, max_hits=mh, out=out, capacity=capacity)
        # size the output once (the sizing call), then every timed call is one pipeline
        total = int(new_call(nq, capacity=0)[0][nq])
        out = torch.empty(max(total, 1), dtype=i64, device=dev)
        nb = min(nwin, max(int(args.base_windows * args.scale), per))
        nb -= nb % per if not ragged else 0
        chunk = 1 << (17 if mh else 20)  # H: ~64 candidates per window, each a 64-char chunk and its indices
        legs = {"new": lambda: new_call(nq, out=out), "base": lambda: baseline(qb, nq, m, Lm, mh, nb, chunk)}
        runs = {x: [] for x in legs}
        for _ in range(args.rounds):
            for x, fn in legs.items():
                runs[x].append(timed(fn))
        ms = {x: float(np.median(v)) for x, v in runs.items()}
        ms["base_scaled"] = ms["base"] * nwin / nb
        os.environ["SAS_MEM_TIMING"] = "1"
        verify, cand = [], C.c_uint64(0)
        for _ in range(args.reps):
            new_call(nq, out=out)
            verify.append(L.sas_mems_verify_ms(C.byref(cand)))
        os.environ["SAS_MEM_TIMING"] = "0"
        vms = float(np.median(verify))
        # identical answers, element for element and in order, on the first windows
        nc = min(nwin, max(int(args.check_windows * args.scale), per))
        nc -= nc % per if not ragged else 0
        bq, bi, bj, bl = baseline(qb, nq, m, Lm, mh, nc, chunk)
        off, qpos, tpos, ln, qfl = new_call(nq, out=out)
        torch.cuda.synchronize()
        if ragged:  # the matches of the first nc windows: those with qpos < nc
            sel = qpos[:total] < nc
            g = (qpos[:total][sel].to(i64), tpos[:total][sel], ln[:total][sel].to(i64))
        else:
            cut = int(off[nc // per])
            g = (qpos[:cut].to(i64), tpos[:cut], ln[:cut].to(i64))
        ok = all(a.shape == b.shape and bool(torch.equal(a, b)) for a, b in zip(g, (bi, bj, bl)))
        rec = {"nq": nq, "m": m, "min_len": Lm, "max_hits": mh, "windows": nwin, "ms": ms, "ms_runs": runs,
               "base_windows": nb, "new_over_base": ms["new"] / ms["base_scaled"],
               "new_faster": ms["new"] < ms["base_scaled"], "query_chars_per_s": nq * m / (ms["new"] * 1e-3),
               "mems": total, "candidates": cand.value, "candidates_per_window": cand.value / nwin,
               "truncated_queries": int((qfl & _lib.SAS_MEM_TRUNCATED != 0).sum()),
               "verify_ms": vms, "candidates_per_s": cand.value / (vms * 1e-3) if vms > 0 else None,
               "identical_to_base": ok, "check_windows": nc}
        print(f"{name}: {json.dumps(rec)}", file=sys.stderr)
        return rec

    def mm_verify_rate(nq):
        """k_mm_verify on this index: candidates per second on shape S of tools/bench_mismatch.py."""
        qb = cut_subst(nq, 32, 1, 11)
        off = idx.locate_mismatch_fixed(qb[:nq * 32], 32, 1, capacity=0, dist=False)[0]
        out = torch.empty(max(int(off[nq]), 1), dtype=i64, device=dev)
        os.environ["SAS_MM_TIMING"] = "1"
        v, cand = [], C.c_uint64(0)
        for _ in range(args.reps + 1):
            idx.locate_mismatch_fixed(qb[:nq * 32], 32, 1, out=out)
            v.append(L.sas_locate_mismatch_verify_ms(C.byref(cand)))
        os.environ["SAS_MM_TIMING"] = "0"
        vms = float(np.median(v[1:]))
        return {"nq": nq, "m": 32, "k": 1, "candidates": cand.value, "verify_ms": vms,
                "candidates_per_s": cand.value / (vms * 1e-3)}

    sc = args.scale
    res = {"n": n, "source_hash": sas_amd.source_hash(), "sa_width": stats["sa_width"],
           "prefix_chars": stats["prefix_chars"], "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "shapes": {}}
    want = args.shapes.split(",")
    if "R" in want:
        nq = max(int(1_000_000 * sc), 1)
        res["shapes"]["R_1e6_len150_L20"] = shape("R", nq, 150, 20, 0, cut_subst(nq, 150, 3, 21))
    if "G" in want:
        m = max(int(10_000_000 * sc), 1000)
        res["shapes"]["G_1x1e7_L32"] = shape("G", 1, m, 32, 0, cut_subst(1, m, m // 1000, 22))
    if "H" in want:
        nq = max(int(100_000 * sc), 1)
        res["shapes"]["H_1e5_len150_L12_cap1024"] = shape("H", nq, 150, 12, 1024, cut_subst(nq, 150, 3, 23))
    res["k_mm_verify"] = mm_verify_rate(max(int(10_000_000 * sc), 1))
    for v in res["shapes"].values():
        if v["candidates_per_s"]:
            v["verify_rate_over_k_mm_verify"] = v["candidates_per_s"] / res["k_mm_verify"]["candidates_per_s"]
    out = args.out or os.path.join(REPO, "profiles", "mems", f"mems_n{n}_{sas_amd.source_hash()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": out, "new_over_base": {x: v["new_over_base"] for x, v in res["shapes"].items()},
                      "identical": {x: v["identical_to_base"] for x, v in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
