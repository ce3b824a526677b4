"""The workload behind DESIGN.md 4, "Clustering".

On c4_surface(1M), one warmed context: symmicp_ctx_cluster at eps = 2 and 4 median spacings and min_points = 1 and 10, each case
1 + REPS calls in a row, in the order of CASES below.  Every call launches k_radius<false> (the count pass of the radius search: the
same walk WITHOUT the unions, the yardstick), k_cluster_init, k_cluster_union, k_cluster_flatten and, for min_points > 1,
k_cluster_border exactly once.  Host wall times per whole call (index build, kernels, read-back, host numbering) are printed as one JSON
line; with --sklearn N the whole call at N points is also timed against scikit-learn's DBSCAN on the host CPU, as context only.
Kernel times come from the profiler's per-dispatch trace of the same run:

    python profiles/cluster_workload.py --reps 5 --sklearn 100000 > profiles/cluster_workload.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/cluster_workload.py --reps 5
    python profiles/cluster_workload.py --reps 5 --trace OUT/trace > profiles/cluster_kernel_times.csv
    SYMMICP_DEBUG_COUNTERS=1 python profiles/cluster_workload.py --reps 0 2> profiles/cluster_counters.txt

The third form reads the kernel-trace CSV under OUT/trace, assigns the dispatches to the cases in call order, drops each case's first
(warm-up) call and writes case, kernel, call, duration_ns.  The fourth prints, per call, the number of unite() calls of the union kernel
and of compare-and-swaps that lost (the library's debug counter)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

CASES = [(2, 1), (2, 10), (4, 1), (4, 10)]                 # (eps in median spacings, min_points)
KERNELS = ["k_radius<false>", "k_cluster_init", "k_cluster_union", "k_cluster_flatten", "k_cluster_border"]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
ap.add_argument("--sklearn", type=int, default=0)
a = ap.parse_args()

if a.trace:
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    per["k_radius<false>"] = per["k_radius<false>"][1:]          # (the call that warms the context)
    w = csv.writer(sys.stdout)
    w.writerow(["case", "kernel", "call", "duration_ns"])
    for m, mp in CASES:
        for name in KERNELS:
            if name == "k_cluster_border" and mp == 1:
                continue
            mine, per[name] = per[name][:a.reps + 1], per[name][a.reps + 1:]
            assert len(mine) == a.reps + 1, (m, mp, name, len(mine))
            for c, ns in enumerate(mine[1:]):
                w.writerow(["eps=%gsp min_points=%d" % (m, mp), name, c, ns])
    assert not any(per.values()), {k: len(v) for k, v in per.items()}
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import symmicp
from symmicp import synth
import _fpfh_ref as R


def spacing(x):
    return R.median_spacing(x, np.sort(np.random.default_rng(5).choice(len(x), min(4096, len(x)), replace=False)))


xyz = synth.c4_surface(a.n)["src"]
sp = spacing(xyz)
out = dict(n=a.n, spacing=sp, reps=a.reps, cases=[])
with symmicp.Engine() as e:
    e.remove_radius_outlier_raw(xyz[:4096], 4 * sp, 3)          # the context warmed: arenas sized, code objects loaded (no cluster kernel runs)
    for m, mp in CASES:
        cfg = symmicp.cluster_config(m * sp, mp)
        walls = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            st, labels, clusters, sizes, core, nb = e.cluster_dbscan_raw(xyz, cfg, cap=a.n)
            walls.append(1e3 * (time.perf_counter() - t0))
            assert st == 0
        timed = walls[1:] or walls
        out["cases"].append(dict(eps_spacings=m, min_points=mp, wall_ms_median=float(np.median(timed)), wall_ms_min=float(min(timed)),
                                 clusters=int(clusters), largest=int(sizes[:clusters].max()) if clusters else 0, core=int(core.sum()),
                                 noise=int((labels < 0).sum()), median_neighbours=float(np.median(nb)), edges=int(nb.astype(np.int64).sum() // 2)))
    if a.sklearn:
        from sklearn.cluster import DBSCAN
        y = synth.c4_surface(a.sklearn)["src"]
        spy = spacing(y)
        e.cluster_dbscan(y, 4 * spy, 10)
        t0 = time.perf_counter()
        dev = e.cluster_dbscan(y, 4 * spy, 10, return_info=True)
        t_dev = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        fit = DBSCAN(eps=float(np.float32(4 * spy)), min_samples=10, n_jobs=-1).fit(y.astype(np.float64))
        t_sk = 1e3 * (time.perf_counter() - t0)
        core = np.zeros(len(y), bool)
        core[fit.core_sample_indices_] = True
        out["sklearn"] = dict(n=a.sklearn, eps_spacings=4, min_points=10, device_wall_ms=t_dev, sklearn_wall_ms=t_sk, clusters=dev["clusters"],
                              core_sets_equal=bool(np.array_equal(core, dev["core"])), core_labels_equal=bool(np.array_equal(fit.labels_[core], dev["labels"][core])),
                              noise_sets_equal=bool(np.array_equal(fit.labels_ < 0, dev["labels"] < 0)))
print(json.dumps(out))
