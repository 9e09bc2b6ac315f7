"""kernel_trace.csv files of rocprofv3 (one or more runs of the same library) -> per kernel of an LM iteration, in launch order:
mean, min, max and standard deviation of its duration over the steady iterations of all runs, in µs.  Iterations are cut and
chosen as in timeline_summary.py.   usage: kernel_spread.py OUT.json TRACE.csv [TRACE.csv ...]"""
import csv
import json
import statistics
import sys
from collections import Counter

from timeline_summary import short


def main():
    pooled, iterations = None, 0
    for path in sys.argv[2:]:
        rows = []
        with open(path) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
        rows.sort()
        starts = [i for i, r in enumerate(rows) if r[2].startswith("cam_pass_kernel") and ", 0>" in r[2]]
        its = [rows[a:b] for a, b in zip(starts[:-1], starts[1:])]
        sig = Counter(tuple(r[2] for r in it) for it in its).most_common(1)[0][0]
        its = [it for it in its if tuple(r[2] for r in it) == sig][2:]
        if pooled is None:
            pooled = [(name, []) for name in sig]
        assert tuple(p[0] for p in pooled) == sig, "the runs' iterations differ in their launches"
        for it in its:
            for k, r in enumerate(it):
                pooled[k][1].append((r[1] - r[0]) / 1e3)
        iterations += len(its)
    out = dict(iterations=iterations, runs=len(sys.argv) - 2, launches_per_iteration=len(pooled),
               kernels=[dict(kernel=name, mean=round(statistics.mean(v), 2), min=round(min(v), 2), max=round(max(v), 2),
                             stdev=round(statistics.stdev(v), 2)) for name, v in pooled])
    json.dump(out, open(sys.argv[1], "w"), indent=1)
    for k in out["kernels"]:
        print(f"{k['kernel'][:60]:60s} {k['mean']:8.2f} [{k['min']:.2f} .. {k['max']:.2f}] sd {k['stdev']:.2f}")
    print("kernel time", round(sum(k["mean"] for k in out["kernels"]), 1))


if __name__ == "__main__":
    main()
