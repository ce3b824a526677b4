"""The workload behind DESIGN.md 4, "Fast Global Registration": symmicp_ctx_fgr on the cat pair, the bumps pair and 100 000 synthetic
correspondences with 50 % inliers, with the tuple test on and off, next to symmicp_ctx_ransac at its defaults on the same inputs.

Run it under the profiler for the kernel times, in a run of its own (never combined with --pmc):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fgr -- python profiles/fgr_workload.py

Prints one line per case with the host wall time of the call (upload, the tuple test's read-back and the result's included; the least of
five calls after a warm-up call); the kernel times are the profiler's."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "icp-symm_amd", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)
import numpy as np
import symmicp as sym
import _global_ref as G
from symmicp import synth
from oracle import oracle as O
F = np.float32
O.lib()
src, _ = O.pcd_read(os.path.join(ROOT, "tests", "golden", "cat.pcd")); tgt, _ = O.pcd_read(os.path.join(ROOT, "tests", "golden", "cat_out.pcd"))
g = np.load(os.path.join(ROOT, "tests", "golden", "cat_golden.npz"))

def wall(f, n=5):
    f()
    t = []
    for _ in range(n):
        t0 = time.perf_counter(); r = f(); t.append(time.perf_counter() - t0)
    return min(t) * 1e3, r

with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
    fs, ft = e.fpfh(src, g["src_n"], 11.05), e.fpfh(tgt, g["tgt_n"], 11.05)
    cp, _ = e.feature_correspondences(fs, ft)
    b = G.bumps_pair()
    bp, _ = e.feature_correspondences(e.fpfh(b["src"], b["src_n"], b["radius"]), e.fpfh(b["tgt"], b["tgt_n"], b["radius"]))
    n = 100000
    rng = np.random.default_rng(1)
    S = rng.random((n, 3)).astype(F)
    T4 = synth.rigid4(synth.rotation(75.0, (0.2, 0.9, 0.4)), np.array([0.5, -1.0, 2.0]))
    Tt = (S.astype(np.float64) @ T4[:3, :3].T + T4[:3, 3]).astype(F)
    pairs = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    bad = rng.random(n) < 0.5
    pairs[bad, 1] = rng.integers(0, n, int(bad.sum()))
    for name, a in (("cat", (src, tgt, cp, 11.05 / 4)), ("bumps", (b["src"], b["tgt"], bp, b["max_dist"])), ("synth100k", (S, Tt, pairs, 0.01))):
        truth = dict(cat=None, bumps=b["truth"], synth100k=T4)[name]
        for label, kw in (("fgr", dict()), ("fgr, tuple test off", dict(max_tuples=0))):
            ms, r = wall(lambda: e.fgr(*a, seed=1, check=False, **kw))
            rms = G.rms_to_truth(r["transform"], truth, a[0]) if truth is not None else float("nan")
            print("%-10s %-20s m %6d  M %6d  accepted %8d  status %d  inliers %6d  wall %8.3f ms  rms to truth %.3e" % (
                name, label, len(a[2]), r["set_size"], r["tuples_accepted"], r["status"], r["inliers"], ms, rms), flush=True)
        ms, r = wall(lambda: e.ransac(*a, seed=1, check=False))
        rms = G.rms_to_truth(r["transform"], truth, a[0]) if truth is not None else float("nan")
        print("%-10s %-20s m %6d  evaluated %d  status %d  inliers %6d  wall %8.3f ms  rms to truth %.3e" % (
            name, "ransac (defaults)", len(a[2]), r["evaluated"], r["status"], r["inliers_final"], ms, rms), flush=True)
