"""The workload behind DESIGN.md 4, "NDT".

On c4_surface(1M) at resolution 0.02, for the neighbourhoods 7 and 1: symmicp_set_target (the map build), symmicp_set_source, one
warm-up alignment of 30 fixed iterations, the same alignment timed, one more pass at its end for the item count.  For context only,
PLANE over the exact tree search on the same pair, run the same way (its kernels are not touched by NDT).  Host wall times are printed
as one JSON line; kernel times come from the profiler's per-dispatch trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/ndt_workload.py
    python profiles/ndt_workload.py --trace OUT/trace > profiles/ndt_kernel_times.csv

The second form reads the kernel-trace CSV under OUT/trace, splits the dispatches of k_pass_ndt between the two neighbourhoods in
call order (per neighbourhood 31 warm-up passes, 31 timed ones, 1 more) and writes the median and the extremes of the timed passes
and of every map-build kernel."""
import argparse
import csv
import glob
import json
import os
import sys
import time

NEIGHBORS = (7, 1)
ITERS = 30
BUILD_KERNELS = ("k_bbox", "k_deinterleave3", "k_voxel_keys", "k_rs_hist", "k_rs_scan", "k_rs_scatter", "k_voxel_heads", "k_scan_tiles", "k_scan_add", "k_voxel_first", "k_voxel_keep", "k_voxel_compact", "k_gather_soa", "k_ndt_voxels",
                 "k_ndt_compact", "k_ndt_insert", "k_morton")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--resolution", type=float, default=0.02)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

if a.trace:
    import statistics
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    w = csv.writer(sys.stdout)
    w.writerow(["what", "kernel", "dispatches", "median_ns", "min_ns", "max_ns"])
    ndt = [dur(r) for r in rows if "k_pass_ndt" in r["Kernel_Name"]]
    per = 2 * (ITERS + 1) + 1
    assert len(ndt) == per * len(NEIGHBORS), len(ndt)
    for k, nb in enumerate(NEIGHBORS):
        timed = ndt[k * per + ITERS + 1: k * per + 2 * (ITERS + 1)]
        w.writerow(["pass, neighbors %d, first (identity guess)" % nb, "k_pass_ndt", 1, timed[0], timed[0], timed[0]])
        w.writerow(["pass, neighbors %d, steps" % nb, "k_pass_ndt", len(timed) - 1, int(statistics.median(timed[1:])), min(timed[1:]), max(timed[1:])])
    # the map build: every kernel between the start of the run and the first NDT pass belongs to set_target / set_source of neighbours 7
    first_pass = next(i for i, r in enumerate(rows) if "k_pass_ndt" in r["Kernel_Name"])
    for name in BUILD_KERNELS:
        d = [dur(r) for r in rows[:first_pass] if name in r["Kernel_Name"]]
        if d:
            w.writerow(["set_target + set_source, neighbors 7", name, len(d), int(statistics.median(d)), min(d), max(d)])
    for name in ("k_search", "k_accumulate", "k_pass_fused", "k_pass_certified", "k_reduce_solve", "k_final_reduce"):
        d = [dur(r) for r in rows if name in r["Kernel_Name"]]
        if d:
            w.writerow(["whole run", name, len(d), int(statistics.median(d)), min(d), max(d)])
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))

import symmicp
from symmicp import synth

d = synth.c4_surface(a.n)
out = dict(n=a.n, resolution=a.resolution, iters=ITERS, ndt=[], plane_tree=None)


def pose_error(X, truth):
    E = np.asarray(X, np.float64) @ np.linalg.inv(truth)
    tr = (np.trace(E[:3, :3]) - 1.0) * 0.5
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, tr))))), float(np.linalg.norm(np.asarray(X, np.float64)[:3, 3] - truth[:3, 3]))


for nb in NEIGHBORS:
    with symmicp.Engine(mode=symmicp.MODE_NDT, max_iters=ITERS, fixed_iters=1) as e:
        e.set_ndt(resolution=a.resolution, neighbors=nb)
        t0 = time.perf_counter()
        e.set_target(d["tgt"], None)
        t_target = time.perf_counter() - t0
        t0 = time.perf_counter()
        e.set_source(d["src"], None)
        t_source = time.perf_counter() - t0
        e.align(None, check=True)
        t0 = time.perf_counter()
        r = e.align(None, check=True)
        wall = time.perf_counter() - t0
        it = e.begin(r["transform"])
        _, _, m = symmicp._ndt_map_call(e._L.symmicp_get_ndt_map, (e._h,), 0, want=False)      # (the count alone: ERR_SIZE at cap 0)
        rot, tr = pose_error(r["transform"], d["truth"])
        out["ndt"].append(dict(neighbors=nb, voxels=m, set_target_ms=1e3 * t_target, set_source_ms=1e3 * t_source, align_ms=1e3 * wall,
                               iter_per_s=ITERS / wall, items_last=int(it["sums"][37]), sum_w_last=float(it["sums"][34]), end_rot_deg=rot, end_trans=tr))
with symmicp.Engine(mode=symmicp.MODE_PLANE, corr=symmicp.CORR_TREE, max_iters=ITERS, fixed_iters=1) as e:
    e.set_target(d["tgt"], d["tgt_n"])
    e.set_source(d["src"], None)
    e.align(None, check=True)
    t0 = time.perf_counter()
    r = e.align(None, check=True)
    wall = time.perf_counter() - t0
    rot, tr = pose_error(r["transform"], d["truth"])
    out["plane_tree"] = dict(align_ms=1e3 * wall, iter_per_s=ITERS / wall, end_rot_deg=rot, end_trans=tr)
print(json.dumps(out))
