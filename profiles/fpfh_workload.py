"""The workload behind DESIGN.md 4, "FPFH features and radius search": c4_surface(1M) at the two radii of tests/test_gpu_fpfh.py
(about 30 and about 100 neighbours), the radius search (count pass, scan, fill pass) and the FPFH features (k_spfh, k_fpfh), and
the k = 10 normals pre-step as the yardstick.  Run it under the profiler, kernel times and counters in runs of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/fpfh_workload.py --reps 5
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT/pmc -- python profiles/fpfh_workload.py --reps 1

Prints one JSON line: the radii, the pairs per call (sum of the neighbour counts) and host wall times of the calls (upload, index
build and read-back included; the kernel times are the profiler's)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

import symmicp
from symmicp import synth
import _fpfh_ref as R

d = synth.c4_surface(a.n)
xyz, nrm = d["src"], d["src_n"]
rows = np.sort(np.random.default_rng(5).choice(a.n, min(4096, a.n), replace=False))
sp = R.median_spacing(xyz, rows)
out = dict(n=a.n, spacing=sp, reps=a.reps, cases=[])
with symmicp.Engine() as e:
    e.estimate_normals(xyz, 10)                                     # warm-up of the context, and the yardstick kernel
    t0 = time.perf_counter()
    for _ in range(a.reps):
        e.estimate_normals(xyz, 10)
    out["normals_k10_wall_ms"] = 1e3 * (time.perf_counter() - t0) / a.reps
    for r in (R.SPACINGS_30 * sp, R.SPACINGS_100 * sp):
        st, count, _, _, _, total = e.radius_search_raw(xyz, r)      # count pass only
        assert st == 0
        t0 = time.perf_counter()
        for _ in range(a.reps):
            st = e.radius_search_raw(xyz, r, cap=total)[0]           # count pass + scan + fill pass
            assert st == 0
        t_rad = 1e3 * (time.perf_counter() - t0) / a.reps
        e.fpfh(xyz, nrm, r)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            e.fpfh(xyz, nrm, r)
        t_fp = 1e3 * (time.perf_counter() - t0) / a.reps
        out["cases"].append(dict(radius=float(r), pairs=int(total), median_neighbours=float(np.median(count)),
                                 radius_search_wall_ms=t_rad, fpfh_wall_ms=t_fp))
print(json.dumps(out))
