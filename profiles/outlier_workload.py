"""The workload behind DESIGN.md 4, "Outlier removal".

On c4_surface(1M), one warmed context: the statistical filter at k = 8, 16, 20, 50, 64 (k_knn_mean_dist: the LDS candidate list), the
k-NN read-back of the normals pre-step at k = 8, 16 (k_normals_knn<true>: the register list, the yardstick at equal k), and the
radius filter at 4 median spacings (k_radius<false>: the count pass of the radius search).  Every case runs 1 + REPS calls in a row,
in the order of CASES below.  Host wall times per whole call (index build, kernel, read-back, host statistics) are printed as one
JSON line; kernel times come from the profiler's per-dispatch trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/outlier_workload.py --reps 11
    python profiles/outlier_workload.py --reps 11 --trace OUT/trace > profiles/outlier_kernel_times.csv

The second form reads the kernel-trace CSV under OUT/trace, assigns the dispatches of the three kernels to the cases in call order
(every call launches its kernel exactly once), drops each case's first (warm-up) call and writes case, kernel, call, duration_ns."""
import argparse
import csv
import glob
import json
import os
import sys
import time

CASES = [("sor", 8), ("sor", 16), ("sor", 20), ("sor", 50), ("sor", 64), ("knn", 8), ("knn", 16), ("ror", 0)]
KERNEL = {"sor": "k_knn_mean_dist", "knn": "k_normals_knn<true>", "ror": "k_radius<false>"}

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

if a.trace:
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if k in r["Kernel_Name"]] for k in set(KERNEL.values())}
    w = csv.writer(sys.stdout)
    w.writerow(["case", "kernel", "call", "duration_ns"])
    for kind, k in CASES:
        name = KERNEL[kind]
        mine, per[name] = per[name][:a.reps + 1], per[name][a.reps + 1:]
        assert len(mine) == a.reps + 1, (kind, k, len(mine))
        for c, ns in enumerate(mine[1:]):
            w.writerow(["%s k=%d" % (kind, k) if k else kind, name, c, ns])
    assert not any(per.values()), {k: len(v) for k, v in per.items()}
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import symmicp
from symmicp import synth
import _fpfh_ref as R

xyz = synth.c4_surface(a.n)["src"]
sp = R.median_spacing(xyz, np.sort(np.random.default_rng(5).choice(a.n, min(4096, a.n), replace=False)))
radius = 4 * sp
out = dict(n=a.n, spacing=sp, radius=float(radius), reps=a.reps, cases=[])
with symmicp.Engine() as e:
    e.estimate_normals(xyz, 10)                       # the context warmed: arenas sized, code objects loaded
    for kind, k in CASES:
        fn = {"sor": lambda: e.remove_statistical_outlier_raw(xyz, k, 2.0, cap=a.n),
              "knn": lambda: e.knn(xyz, k),
              "ror": lambda: e.remove_radius_outlier_raw(xyz, radius, 3, cap=a.n)}[kind]
        walls = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            res = fn()
            walls.append(1e3 * (time.perf_counter() - t0))
        rec = dict(case=kind, k=k, wall_ms_median=float(np.median(walls[1:])), wall_ms_min=float(min(walls[1:])))
        if kind != "knn":
            assert res[0] == 0
            rec["kept"] = int(res[2])
        if kind == "ror":
            rec["median_neighbours"] = float(np.median(res[3]))
        out["cases"].append(rec)
print(json.dumps(out))
