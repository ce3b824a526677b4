"""The workload behind DESIGN.md 4, "Region growing".

On c4_surface(1M) with k = 10 normals and curvature from estimate_normals, one warmed context, each entry of PLAN 1 + REPS calls in a
row, in the order of PLAN:

  * cluster   symmicp_ctx_cluster at min_points = 1 and eps = 2 and 4 median spacings: k_radius<false> (the count pass of the radius
              search: the walk WITHOUT unions or normals) and k_cluster_union, the two yardsticks, in the same session;
  * region    symmicp_ctx_region_growing without seed_out / smooth_out at eps = 2 and 4 spacings, 15 and 30 degrees, the curvature
              threshold at 0.05 and off (curv = NULL): k_region_seeds, k_cluster_init, k_region_union, k_cluster_flatten and, with a
              curvature, k_region_border, each exactly once per call;
  * smooth    the same call WITH smooth_out at (eps, 30 degrees, 0.05): k_region_smooth once more per call.

Host wall times per whole call (index build, kernels, read-back, host numbering) are printed as one JSON line.  Kernel times come from
the profiler's per-dispatch trace of the same run:

    python profiles/region_workload.py --reps 5 > profiles/region_workload.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/region_workload.py --reps 5
    python profiles/region_workload.py --reps 5 --trace OUT/trace > profiles/region_kernel_times.csv
    SYMMICP_DEBUG_COUNTERS=1 python profiles/region_workload.py --reps 0 2> profiles/region_counters.txt

The third form reads the kernel-trace CSV under OUT/trace, assigns the dispatches to the entries in call order, drops each entry's first
(warm-up) call and writes case, kernel, call, duration_ns.  The fourth prints, per call, the unite() calls, the lost compare-and-swaps,
the edges the union kernel examined and the normal loads among them (the library's debug counter)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

SPACINGS = [2, 4]
REGION = ["k_region_seeds", "k_cluster_init", "k_region_union", "k_cluster_flatten"]
PLAN = []                                                      # (case, kind, (eps in spacings, degrees, threshold or None), kernels per call)
for m in SPACINGS:
    PLAN.append(("cluster eps=%gsp" % m, "cluster", (m, None, None), ["k_radius<false>", "k_cluster_init", "k_cluster_union", "k_cluster_flatten"]))
    for deg in (15, 30):
        for thr in (0.05, None):
            PLAN.append(("region eps=%gsp %gdeg %s" % (m, deg, "curv<=0.05" if thr else "no-curv"), "region", (m, deg, thr),
                         REGION + (["k_region_border"] if thr else [])))
    PLAN.append(("smooth eps=%gsp 30deg curv<=0.05" % m, "smooth", (m, 30, 0.05), REGION + ["k_region_border", "k_region_smooth"]))
KERNELS = sorted({k for p in PLAN for k in p[3]})

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

if a.trace:
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    per["k_radius<false>"] = per["k_radius<false>"][1:]          # (the call that warms the context)
    w = csv.writer(sys.stdout)
    w.writerow(["case", "kernel", "call", "duration_ns"])
    for case, kind, _, kernels in PLAN:
        for name in kernels:
            mine, per[name] = per[name][:a.reps + 1], per[name][a.reps + 1:]
            assert len(mine) == a.reps + 1, (case, name, len(mine))
            for c, ns in enumerate(mine[1:]):
                w.writerow([case, name, c, ns])
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
    nrm, curv = e.estimate_normals(xyz, 10)
    out["seeds_at_0.05"] = int((curv <= np.float32(0.05)).sum())
    e.remove_radius_outlier_raw(xyz[:4096], 4 * sp, 3)          # the context warmed: arenas sized, code objects loaded (no region kernel runs)
    for case, kind, (m, deg, thr), _ in PLAN:
        walls = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            if kind == "cluster":
                st, labels, parts, sizes, _, _ = e.cluster_dbscan_raw(xyz, symmicp.cluster_config(m * sp, 1), cap=a.n)
            else:
                cfg = symmicp.region_config(m * sp, deg, 0.05 if thr is None else thr)
                st, labels, parts, sizes, seed, smooth = e.region_growing_raw(xyz, nrm, None if thr is None else curv, cfg, cap=a.n, want=kind == "smooth")
            walls.append(1e3 * (time.perf_counter() - t0))
            assert st == 0
        timed = walls[1:] or walls
        row = dict(case=case, wall_ms_median=float(np.median(timed)), wall_ms_min=float(min(timed)), parts=int(parts),
                   largest=int(sizes[:parts].max()) if parts else 0, unlabelled=int((labels < 0).sum()))
        if kind == "smooth":
            row.update(border=int(((seed == 0) & (labels >= 0)).sum()), median_smooth=float(np.median(smooth)),
                       smooth_edges=int(smooth.astype(np.int64).sum() // 2))
        out["cases"].append(row)
print(json.dumps(out))
