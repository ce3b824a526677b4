"""The workload behind DESIGN.md 4, "Batched alignment": many multi-start problems on one pair, PAPER, 10 fixed iterations,

  cat      1 024 problems on the cat pair (3 400 x 3 400 points)
  p512       256 problems on a 512-point pair (the cat's first 512 rows)
  p4096       64 problems on a 4 096-point pair (the cat and a jittered copy of its first 696 rows)

each run two ways on the same machine, warm, --reps times:

  batch        one Engine.align_multistart call (host wall time: upload, the one launch, read-back)
  sequential   the same alignments one after another on one Engine(corr=BRUTE, fixed_iters=1) whose clouds are set once

and compared: the largest difference between the two routes' transforms is printed with the times.  The kernel's own time comes from
the profiler in a run of its own (the host wall times are taken with the profiler off):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python profiles/batch_workload.py --what batch --reps 5

Prints one JSON line per case and route.  evals = B x 11 passes x src_count x tgt_count distance evaluations; the VALU issue limit
they are held against is 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz / 11 vector instructions per evaluation = 7.15e12 evaluations/s."""
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
ap.add_argument("--what", choices=["batch", "sequential", "both"], default="both")
ap.add_argument("--cases", nargs="+", default=["cat", "p512", "p4096"])
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

import symmicp
import _batch_ref as B

ITERS = 10
VALU_LIMIT = 256 * 4 * 32 * 2.4e9 / 11.0
f32 = np.float32


def pair(name):
    g = os.path.join(ROOT, "tests", "golden")
    src, _ = symmicp.pcd_read(os.path.join(g, "cat.pcd"))
    tgt, _ = symmicp.pcd_read(os.path.join(g, "cat_out.pcd"))
    gold = np.load(os.path.join(g, "cat_golden.npz"))
    sn, tn = gold["src_n"], gold["tgt_n"]
    if name == "cat":
        return src, sn, tgt, tn, 1024
    if name == "p512":
        return src[:512], sn[:512], tgt[:512], tn[:512], 256
    rng = np.random.default_rng(20261019)
    jit = lambda x: np.concatenate([x, x[:696] + rng.normal(0, 0.3, (696, 3)).astype(f32)]).astype(f32)
    return jit(src), np.concatenate([sn, sn[:696]]), jit(tgt), np.concatenate([tn, tn[:696]]), 64


def guesses(tgt, n):
    """the known answer perturbed by up to 4 degrees and 2 % of the extent, seeded"""
    rng = np.random.default_rng(7)
    t = tgt.astype(np.float64)
    centre, extent = t.mean(0), float(np.linalg.norm(t.max(0) - t.min(0)))
    return np.stack([B.perturbed(B.CAT_TRUTH, rng.normal(size=3), rng.uniform(-4, 4), extent * 0.02 * rng.uniform(-1, 1, 3), centre) for _ in range(n)])


def timed(fn, reps):
    out = fn()                                   # warm-up: code objects, arenas
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return out, t


for name in a.cases:
    src, sn, tgt, tn, nb = pair(name)
    g = guesses(tgt, nb)
    evals = float(nb) * (ITERS + 1) * len(src) * len(tgt)
    rec = dict(case=name, problems=nb, src=len(src), tgt=len(tgt), iters=ITERS, evals=evals)
    Xb = Xs = None
    if a.what in ("batch", "both"):
        with symmicp.Engine() as e:
            res, t = timed(lambda: e.align_multistart(src, sn, tgt, tn, g, mode=symmicp.MODE_PAPER, max_iters=ITERS, fixed_iters=1), a.reps)
        assert all(r["status"] == 0 and r["iters"] == ITERS for r in res)
        Xb = np.stack([r["transform"] for r in res])
        print(json.dumps(dict(rec, route="batch", wall_ms=[round(x, 3) for x in t], wall_ms_median=round(float(np.median(t)), 3),
                              evals_per_s_wall=evals / (1e-3 * float(np.median(t))), valu_limit_evals_per_s=VALU_LIMIT)), flush=True)
    if a.what in ("sequential", "both"):
        with symmicp.Engine(mode=symmicp.MODE_PAPER, corr=symmicp.CORR_BRUTE, max_iters=ITERS, fixed_iters=1) as e:
            e.set_target(tgt, tn)
            e.set_source(src, sn)
            res, t = timed(lambda: [e.align(x) for x in g], a.reps)
        assert all(r["status"] == 0 and r["iters"] == ITERS for r in res)
        Xs = np.stack([r["transform"] for r in res])
        print(json.dumps(dict(rec, route="sequential", wall_ms=[round(x, 3) for x in t], wall_ms_median=round(float(np.median(t)), 3),
                              us_per_iteration=1e3 * float(np.median(t)) / (nb * ITERS))), flush=True)
    if Xb is not None and Xs is not None:
        print(json.dumps(dict(case=name, max_abs_transform_difference=float(np.abs(Xb.astype(np.float64) - Xs).max()))), flush=True)
