"""The workload behind DESIGN.md 4, "Plane segmentation".

The cloud is synth.c4_surface(--surface) plus a noisy plane of --plane points under it, rows shuffled.  For each scoring shape
(SYMMICP_PLANE_SCORE = 0: hypotheses in lanes, two per lane, the points staged in LDS -- the kernel in use; 1 and 4: the same with one and
four per lane; 3: one per lane on wave-uniform global loads; 2: points in registers and a ballot per hypothesis) a context is created and warmed by one small call, then every case of CASES runs 1 + REPS
segment_plane calls in a row.  Every call launches k_plane_hyp, the shape's scoring kernel, k_ransac_argmax and k_plane_mask exactly
once.  Host wall times per whole call (pivot, upload, kernels, read-back, one host refit) and the refit-free call are printed as one
JSON line; all shapes must return equal bytes.  Kernel times come from the profiler's per-dispatch trace of a run of its own:

    python profiles/plane_workload.py --reps 5 > profiles/plane_workload.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/plane_workload.py --reps 5
    python profiles/plane_workload.py --reps 5 --trace OUT/trace > profiles/plane_kernel_times.csv

The third form reads the kernel-trace CSV under OUT/trace, assigns the dispatches to the shapes and cases in call order, drops the warming
call and each case's first call, and writes shape, case, kernel, call, duration_ns."""
import argparse
import csv
import glob
import json
import os
import sys
import time

SHAPES = [(0, "k_plane_score<true, 2>"), (1, "k_plane_score<true, 1>"), (4, "k_plane_score<true, 4>"), (3, "k_plane_score<false, 1>"),
          (2, "k_plane_score_pts")]
COMMON = ["k_plane_hyp", "k_ransac_argmax", "k_plane_mask"]

ap = argparse.ArgumentParser()
ap.add_argument("--surface", type=int, default=500_000)
ap.add_argument("--plane", type=int, default=500_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
a = ap.parse_args()
N = a.surface + a.plane
CASES = [(N, 1024), (N, 4096), (2 * N, 1024)]           # (points, hypotheses); the last is c4_surface(2 * surface) + 2 * plane points

if a.trace:
    files = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    w = csv.writer(sys.stdout)
    w.writerow(["shape", "points", "hypotheses", "kernel", "call", "duration_ns"])
    per = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if k + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(k)]
           for k in [s for _, s in SHAPES] + COMMON}
    for shape, score in SHAPES:
        for name in [score] + COMMON:
            per[name] = per[name][1:]                     # the warming call
        for n, H in CASES:
            for name in [score] + COMMON:
                mine, per[name] = per[name][:2 * (a.reps + 1)], per[name][2 * (a.reps + 1):]      # (with and without the refit)
                assert len(mine) == 2 * (a.reps + 1), (shape, n, H, name, len(mine))
                for c, ns in enumerate(mine[1:a.reps + 1]):
                    w.writerow([shape, n, H, name, c, ns])
    assert not any(per.values()), {k: len(v) for k, v in per.items()}
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-symm_amd", "py"))

import symmicp
from symmicp import synth


def cloud(surface, plane):
    s = synth.c4_surface(surface)["src"].astype(np.float64)
    lo, hi = s.min(axis=0), s.max(axis=0)
    side = int(np.ceil(np.sqrt(plane)))
    g = np.stack(np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[1], hi[1], side), indexing="ij"), -1).reshape(-1, 2)[:plane]
    sp = (hi[0] - lo[0]) / side
    z = lo[2] - 4 * sp + (synth.uniform01(21, plane) - 0.5) * 0.6 * sp
    x = np.concatenate([s, np.concatenate([g, z[:, None]], 1)]).astype(np.float32)
    return np.ascontiguousarray(x[np.random.default_rng(7).permutation(len(x))]), float(sp)


clouds = {}
for n, _ in CASES:
    if n not in clouds:
        clouds[n] = cloud(a.surface * n // N, a.plane * n // N)
out = dict(surface=a.surface, plane=a.plane, reps=a.reps, cases=[])
first = {}
for shape, score in SHAPES:
    os.environ["SYMMICP_PLANE_SCORE"] = str(shape)        # read when the context is created
    with symmicp.Engine() as e:
        e.segment_plane(clouds[N][0][:4096], clouds[N][1], 64)      # the context warmed: code objects loaded
        for n, H in CASES:
            xyz, sp = clouds[n]
            for refits in (1, 0):
                cfg = symmicp.plane_config(0.5 * sp, H, 0, refits)
                walls = []
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    st, r = e.segment_plane_raw(xyz, cfg, cap=n, want=True)      # (returns after the stream is synchronised)
                    walls.append(1e3 * (time.perf_counter() - t0))
                    assert st == 0, st
                timed = walls[1:] or walls
                key = (n, H, refits)
                blob = b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("plane", "rows", "hyp_inliers", "hyp_status", "distance"))
                same = first.setdefault(key, blob) == blob
                out["cases"].append(dict(shape=shape, kernel=score, points=n, hypotheses=H, refits=refits, wall_ms_median=float(np.median(timed)),
                                         wall_ms_min=float(min(timed)), evaluated=r["evaluated"], inliers_ransac=r["inliers_ransac"],
                                         inliers_final=r["inliers_final"], plane=r["plane"].tolist(), equal_to_shape_0=bool(same)))
                assert same, key
print(json.dumps(out))
