"""The workload behind DESIGN.md 4, "Normal orientation".

On c4_surface(1M) with the k = 10 normals of the normals pre-step, one warmed context: for k = 10 and 16, first 1 + REPS calls of
symmicp_ctx_knn at that k (the yardstick: symmicp_ctx_orient_normals contains that walk, so it cannot be faster), then 1 + REPS calls
of symmicp_ctx_orient_normals.  Every orientation call launches k_normals_knn<true>, k_orient_edges and k_orient_init once, then per
round k_orient_min_key, k_orient_min_hi and k_orient_hook (one round more than the rounds that join something: the last one finds no
edge) and k_orient_flatten (once per joining round), then k_orient_seed_key, k_orient_root_flip and k_orient_apply once.  Host wall
times per whole call (index build, kernels, the one word read per round, read-back, host counts) are printed as one JSON line.  Kernel
times come from the profiler's per-dispatch trace of the same run:

    python profiles/orient_workload.py --reps 5 > profiles/orient_workload.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/orient_workload.py --reps 5
    python profiles/orient_workload.py --reps 5 --trace OUT/trace > profiles/orient_kernel_times.csv

The third form reads the kernel-trace CSV under OUT/trace, cuts it into calls at every k_normals_knn<true> dispatch (a call without
k_orient kernels is a yardstick call), drops each case's first (warm-up) call and writes case, call, kernel, round, duration_ns: one row
per dispatch, `round` counting a kernel's dispatches within its call."""
import argparse
import csv
import glob
import json
import os
import sys
import time

KS = [10, 16]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

if a.trace:
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    calls = []                                                 # [(kernel, ns), ...] per call
    for r in rows:
        name = r["Kernel_Name"]
        if "k_normals_knn<true>" in name:
            calls.append([])
        if calls and ("k_orient_" in name or "k_normals_knn<true>" in name):
            short = "k_normals_knn<true>" if "k_normals_knn" in name else name[name.index("k_orient_"):].split("(")[0]
            calls[-1].append((short, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    assert len(calls) == 2 * len(KS) * (a.reps + 1), len(calls)
    w = csv.writer(sys.stdout)
    w.writerow(["case", "call", "kernel", "round", "duration_ns"])
    for k in KS:
        for what in ("knn", "orient"):
            mine, calls = calls[:a.reps + 1], calls[a.reps + 1:]
            for c, call in enumerate(mine[1:]):
                assert (len(call) == 1) == (what == "knn"), (k, what, len(call))
                seen = {}
                for name, ns in call:
                    w.writerow(["%s k=%d" % (what, k), c, name, seen.get(name, 0), ns])
                    seen[name] = seen.get(name, 0) + 1
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))

import symmicp
from symmicp import synth

xyz = synth.c4_surface(a.n)["src"]
out = dict(n=a.n, reps=a.reps, cases=[])
with symmicp.Engine() as e:
    nrm, _ = e.estimate_normals(xyz, 10)                      # (k_normals_knn<false>: not a call of the trace's cut)
    e.remove_radius_outlier_raw(xyz[:4096], 1.0, 3)            # the context warmed: arenas sized, code objects loaded
    for k in KS:
        walls_knn, walls = [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            e.knn(xyz, k)
            walls_knn.append(1e3 * (time.perf_counter() - t0))
        cfg = symmicp.orient_config(k)
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            st, on, flip, comp, tree, res = e.orient_normals_raw(xyz, nrm, cfg)
            walls.append(1e3 * (time.perf_counter() - t0))
            assert st == 0
        timed, timed_knn = walls[1:] or walls, walls_knn[1:] or walls_knn
        out["cases"].append(dict(k=k, wall_ms_median=float(np.median(timed)), wall_ms_min=float(min(timed)),
                                 knn_wall_ms_median=float(np.median(timed_knn)), knn_wall_ms_min=float(min(timed_knn)),
                                 rounds=int(res.rounds), graph_edges=int(res.graph_edges), tree_edges=int(res.tree_edges),
                                 components=int(res.components), largest_component=int(res.largest_component), flipped=int(res.flipped)))
print(json.dumps(out))
