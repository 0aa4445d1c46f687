"""Per-launch means of the instruction-fetch counters that scripts/probes/pmc_ifetch.sh collected, for the k_step dispatches
of whole episodes.  The counters are sums over the chip: 256 CUs = 128 instruction caches (one per CU pair), 1024 waves per
launch at 65 536 envs.  A miss is one 64-byte line.   usage: python scripts/probes/pmc_ifetch_summary.py <outdir>"""
import csv
import glob
import os
import sys
from collections import defaultdict

CU_PAIRS, LINE = 128, 64


def counters(pass_dir):
    hits = glob.glob(os.path.join(pass_dir, "**", "*counter_collection.csv"), recursive=True)
    if not hits:
        raise SystemExit("no counter_collection.csv under " + pass_dir)
    vals = defaultdict(lambda: defaultdict(dict))
    with open(hits[0]) as f:
        for r in csv.DictReader(f):
            d = vals[r["Counter_Name"]][r["Kernel_Name"]]
            i = int(r["Dispatch_Id"])
            d[i] = d.get(i, 0.0) + float(r["Counter_Value"])          # (a counter may come as one row per dimension)
    return vals


def step_kernel(table):
    ks = [k for k in table if "k_step<" in k]
    if not ks:
        raise SystemExit("no k_step dispatches")
    return max(ks, key=lambda k: len(table[k]))


def main(out):
    for name in ("sq", "sqc"):
        v = counters(os.path.join(out, name))
        k = step_kernel(next(iter(v.values())))
        n = len(next(iter(v.values()))[k])
        print("%s pass: %s, %d launches" % (name, k.split("(")[0], n))
        means = {}
        for c in sorted(v):
            x = sorted(v[c][k].values())
            means[c] = sum(x) / len(x)
            print("  %-28s mean %14.1f  median %14.1f  min %14.1f  max %14.1f" % (c, means[c], x[len(x) // 2], x[0], x[-1]))
        if "SQC_ICACHE_MISSES" in means:
            m, dup, req = means["SQC_ICACHE_MISSES"], means.get("SQC_ICACHE_MISSES_DUPLICATE", 0.0), means.get("SQC_ICACHE_REQ", 0.0)
            print("  misses per launch and CU pair: %.1f lines = %.0f bytes (+ %.1f duplicate misses); requests per CU pair %.1f; "
                  "miss rate %.4f" % (m / CU_PAIRS, m / CU_PAIRS * LINE, dup / CU_PAIRS, req / CU_PAIRS, (m / req) if req else 0.0))
        if "SQ_WAIT_INST_ANY" in means and "SQ_WAVE_CYCLES" in means:
            print("  SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES = %.4f" % (means["SQ_WAIT_INST_ANY"] / means["SQ_WAVE_CYCLES"]))
        if "SQ_IFETCH" in means and "SQ_WAVES" in means and means["SQ_WAVES"]:
            print("  SQ_IFETCH per wave = %.1f" % (means["SQ_IFETCH"] / means["SQ_WAVES"]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "build/pmc_ifetch")
