"""The workloads behind DESIGN.md 4, "ISS keypoints".

Default: c4_surface(1M) at the two radii of the FPFH table (6.4 and 11.7 median spacings), the count pass of the radius search
(k_radius<false>: the walk alone, the yardstick) and the keypoints with rn = rs (k_iss_saliency, k_iss_nms).  Run it under the
profiler, kernel times and counters in runs of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/iss_workload.py --reps 3
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT/pmc -- python profiles/iss_workload.py --reps 1

--global N: the steps of the global initialisation on a c4_surface(N) pair, with and without the keypoint stage (host wall times,
uploads and read-backs included; no profiler).

Prints one JSON line."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--global", dest="global_n", type=int, default=0)
a = ap.parse_args()

import symmicp
from symmicp import synth
import _fpfh_ref as R


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return 1e3 * (time.perf_counter() - t0) / reps, out


if a.global_n:
    d = synth.c4_surface(a.global_n)
    rows = np.sort(np.random.default_rng(5).choice(a.global_n, min(4096, a.global_n), replace=False))
    sp = R.median_spacing(d["src"], rows)
    r = R.SPACINGS_30 * sp
    out = dict(n=a.global_n, spacing=sp, radius=float(r), reps=a.reps)
    with symmicp.Engine() as e:
        t, fs = wall(lambda: e.fpfh(d["src"], d["src_n"], r), 1)
        t2, ft = wall(lambda: e.fpfh(d["tgt"], d["tgt_n"], r), 1)
        out["fpfh_both_wall_ms"] = t + t2
        t, ks = wall(lambda: e.iss_keypoints(d["src"], r, r), a.reps)
        t2, kt = wall(lambda: e.iss_keypoints(d["tgt"], r, r), a.reps)
        out.update(iss_both_wall_ms=t + t2, source_keypoints=len(ks), target_keypoints=len(kt))
        t, (pairs, _) = wall(lambda: e.feature_correspondences(fs, ft), a.reps)
        out.update(matching_full_wall_ms=t, pairs_full=len(pairs))
        t, (kpairs, _) = wall(lambda: e.feature_correspondences(fs[ks], ft[kt]), a.reps)
        out.update(matching_keypoints_wall_ms=t, pairs_keypoints=len(kpairs))
        kpairs = np.stack([ks[kpairs[:, 0]], kt[kpairs[:, 1]]], 1).astype(np.int32)
        for name, p in (("full", pairs), ("keypoints", kpairs)):
            t, g = wall(lambda: e.ransac(d["src"], d["tgt"], p, 2 * sp, hypotheses=100000, seed=1, check=False), a.reps)
            out["ransac_%s_wall_ms" % name] = t
            out["ransac_%s_status" % name] = int(g["status"])
            out["ransac_%s_inliers" % name] = int(g["inliers_final"])
    print(json.dumps(out))
    sys.exit(0)

d = synth.c4_surface(a.n)
xyz = d["src"]
rows = np.sort(np.random.default_rng(5).choice(a.n, min(4096, a.n), replace=False))
sp = R.median_spacing(xyz, rows)
out = dict(n=a.n, spacing=sp, reps=a.reps, cases=[])
with symmicp.Engine() as e:
    for r in (R.SPACINGS_30 * sp, R.SPACINGS_100 * sp):
        t_rad, res = wall(lambda: e.radius_search_raw(xyz, r), a.reps)                     # count pass only
        assert res[0] == 0
        t_iss, k = wall(lambda: e.iss_keypoints(xyz, r, r, return_saliency=True), a.reps)
        out["cases"].append(dict(radius=float(r), pairs=int(res[5]), median_neighbours=float(np.median(res[1])), keypoints=len(k["rows"]),
                                 salient=int((k["saliency"] > 0).sum()), radius_count_wall_ms=t_rad, iss_wall_ms=t_iss))
print(json.dumps(out))
