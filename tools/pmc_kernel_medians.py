#!/usr/bin/env python3
"""Median-dispatch counters per kernel from one rocprofv3 --pmc counter_collection CSV.

Usage:
  rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_HIT_sum TCC_MISS_sum \
      --output-format csv -d OUT -o run -- python tools/bench_locate.py --only-c --out OUT/under_pmc.json
  python tools/pmc_kernel_medians.py OUT/**/run_counter_collection.csv \
      --kernels k_locate_fill k_locate_tiles k_widen_sa --out profiles/locate/pmc_c_summary.json

Every counter is summed over a dispatch's rows (one row per counter instance), then the median
over the kernel's dispatches is taken: warm-up and timed calls launch the same grid, and a median
is not skewed by the one dispatch that finds cold caches.  Kernels are keyed by their name up to
the parameter list (template arguments kept).  tools/pmc_to_json.py writes the per-lookup records
bench.py reads; this one is for side-by-side kernels of one run.
"""
import argparse
import collections
import csv
import json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--kernels", nargs="+", required=True, help="substrings of the kernel names to keep")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    with open(a.csv) as f:
        for row in csv.DictReader(f):
            k = row["Kernel_Name"]
            if any(s in k for s in a.kernels):
                per[(k.split("(")[0][:60], row["Dispatch_Id"])][row["Counter_Name"]] += float(row["Counter_Value"])
    by = collections.defaultdict(lambda: collections.defaultdict(list))
    for (k, _), c in per.items():
        for name, v in c.items():
            by[k][name].append(v)
    out = {}
    for k, c in by.items():
        out[k] = {name: sorted(v)[len(v) // 2] for name, v in c.items()}
        out[k]["dispatches"] = len(next(iter(c.values())))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
