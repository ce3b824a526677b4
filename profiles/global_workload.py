"""The workload behind DESIGN.md 4, "Feature matching and RANSAC".

  --what nn       symmicp_ctx_feature_nn on FPFH rows of c4_surface(n) (source rows against target rows, radius 6.4 median
                  spacings) for every n of --sizes; --queries 1|2 and --splits S force the kernel's shape (default: its own choice)
  --what ransac   symmicp_ctx_ransac on the two test inputs (cat, H = 4 000; bumps, H = 262 144) and on m = 100 000 synthetic
                  correspondences with 50 % and 5 % inliers at H = 2^20
  --what scipy    the outside yardstick for the matching: cKDTree(fb).query(fa, workers=16) on the same rows (no GPU work timed)

Run it under the profiler, kernel times and counters in runs of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/global_workload.py --what nn --reps 5
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT/pmc -- python profiles/global_workload.py --what nn --reps 1
    rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS --output-format csv -d OUT/pmc2 -- python ... --reps 1

Prints one JSON line per case: sizes, pairs per call and the host wall time of the call (upload and read-back included; the kernel
times are the profiler's).  Every timed call follows a warm-up call of the same shape."""
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
ap.add_argument("--what", choices=["nn", "ransac", "scipy"], default="nn")
ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 65536, 262144])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries", type=int, default=0)
ap.add_argument("--splits", type=int, default=0)
a = ap.parse_args()
if a.queries:
    os.environ["SYMMICP_FEATURE_NN_QUERIES"] = str(a.queries)
if a.splits:
    os.environ["SYMMICP_FEATURE_NN_SPLITS"] = str(a.splits)

import symmicp
from symmicp import synth
import _fpfh_ref as R
import _global_ref as G


def surface_features(e, n):
    d = synth.c4_surface(n)
    rows = np.sort(np.random.default_rng(5).choice(n, min(4096, n), replace=False))
    r = R.SPACINGS_30 * R.median_spacing(d["src"], rows)
    return e.fpfh(d["src"], d["src_n"], r), e.fpfh(d["tgt"], d["tgt_n"], r)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(wall_ms_mean=float(np.mean(t)), wall_ms_min=float(np.min(t)), wall_ms_max=float(np.max(t)))


def synthetic_pairs(m, inlier_share):
    """m correspondences (k, k): points of the unit cube, the target the source turned by 140 degrees, moved, with noise of a
    tenth of max_dist on the inliers and unrelated points on the rest; max_dist = 0.01"""
    src = np.stack([synth.uniform01(21, m, k) for k in range(3)], 1)
    Rm, t = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([0.7, -0.4, 1.1])
    tgt = src @ Rm.T + t + 1e-3 * (2.0 * np.stack([synth.uniform01(22, m, k) for k in range(3)], 1) - 1.0)
    out = synth.uniform01(23, m, 0) >= inlier_share
    tgt[out] = np.stack([synth.uniform01(24, m, k) for k in range(3)], 1)[out] @ Rm.T + t
    return src.astype(np.float32), tgt.astype(np.float32), np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32), 0.01


with symmicp.Engine() as e:
    if a.what in ("nn", "scipy"):
        for n in a.sizes:
            fa, fb = surface_features(e, n)
            if a.what == "nn":
                out = dict(case="feature_nn", na=n, nb=n, pairs=n * n, queries=a.queries, splits=a.splits, reps=a.reps)
                out.update(timed(lambda: e.feature_nn(fa, fb), a.reps))
            else:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                tree = cKDTree(fb)
                t1 = time.perf_counter()
                j = tree.query(fa, 1, workers=16)[1]
                t2 = time.perf_counter()
                nn = e.feature_nn(fa, fb)[0]
                # where the two pick different rows, the fp64 distances of both picks: near-ties that fp32 and fp64 order differently
                a64, b64 = fa.astype(np.float64), fb.astype(np.float64)
                d_dev, d_tree = ((a64 - b64[nn]) ** 2).sum(1), ((a64 - b64[j]) ** 2).sum(1)
                out = dict(case="scipy_ckdtree", na=n, nb=n, build_ms=1e3 * (t1 - t0), query_ms=1e3 * (t2 - t1), workers=16,
                           same_row_as_device=float((j == nn).mean()),
                           device_within_1e6_of_tree=float((d_dev <= d_tree * (1 + 1e-6) + 1e-30).mean()),
                           worst_relative_excess=float(((d_dev - d_tree) / np.maximum(d_tree, 1e-30)).max()))
            print(json.dumps(out), flush=True)
    else:
        from oracle import oracle as O
        g = os.path.join(ROOT, "tests", "golden")
        cs, _ = O.pcd_read(os.path.join(g, "cat.pcd"))
        ct, _ = O.pcd_read(os.path.join(g, "cat_out.pcd"))
        gold = np.load(os.path.join(g, "cat_golden.npz"))
        cases = []
        pairs, _ = e.feature_correspondences(e.fpfh(cs, gold["src_n"], 11.05), e.fpfh(ct, gold["tgt_n"], 11.05))
        cases.append(("cat", cs, ct, pairs, 11.05 / 4, 4000))
        b = G.bumps_pair()
        pairs, _ = e.feature_correspondences(e.fpfh(b["src"], b["src_n"], b["radius"]), e.fpfh(b["tgt"], b["tgt_n"], b["radius"]))
        cases.append(("bumps", b["src"], b["tgt"], pairs, b["max_dist"], 262144))
        for share in (0.5, 0.05):
            s, t, p, md = synthetic_pairs(100_000, share)
            cases.append(("synthetic_%g" % share, s, t, p, md, 1 << 20))
        for name, s, t, p, md, H in cases:
            r = e.ransac(s, t, p, md, hypotheses=H, seed=1, check=False)
            out = dict(case="ransac_" + name, m=len(p), hypotheses=H, evaluated=r["evaluated"], inliers=r["inliers_final"], status=r["status"],
                       reps=a.reps)
            out.update(timed(lambda: e.ransac(s, t, p, md, hypotheses=H, seed=1, check=False), a.reps))
            print(json.dumps(out), flush=True)
