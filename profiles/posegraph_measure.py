"""Wall time of the pose-graph optimiser ("Pose-graph optimisation"; output: profiles/posegraph_measure.json).

  python profiles/posegraph_measure.py [OUT_DIR]

The graphs are those of tests/_posegraph_ref.py: the pass probe at the caps (n = 1024, m = 16384) and at n = 100, and the optimiser on the
noisy ring of 8 with and without the false closure.  Host clock around calls that end in a stream synchronise (upload, launches and
read-back included); two warm-up calls before every timed series.  There is no parent-commit number to compare with: the feature is new.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "icp-symm_amd", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
REPS = 9


def timed(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return dict(min_ms=min(out), median_ms=sorted(out)[len(out) // 2], max_ms=max(out))


def main(out_dir):
    import symmicp
    import _posegraph_ref as R
    res = {}
    with symmicp.Engine() as e:
        graphs = R.pass_graphs(with_cap=True)
        for name in ("n100", "cap"):
            poses, edges, ref = graphs[name]
            E = symmicp.pose_edges(edges)                   # (the conversion of 16384 tuples is Python's time, not the call's)
            a = R.assemble(poses, edges, ref, R.PASS_MU)
            lam = R.PASS_LAMBDA_REL * max(a["hdiag"][i][k, k] for i in range(len(poses)) for k in range(6))
            r = e.posegraph_pass(poses, E, ref, R.PASS_MU, lam)
            res["pass_" + name] = dict(n=len(poses), m=len(edges), lam=lam, cg_iterations=r["cg_iterations"], cg_residual=r["cg_residual"],
                                       **timed(lambda: e.posegraph_pass(poses, E, ref, R.PASS_MU, lam)))
        for name in ("noisy", "false"):
            start, edges, _ = R.ring_cases()[name]
            E = symmicp.pose_edges(edges)
            r = e.posegraph_optimize(start, E, R.RING_MAX_DIST)
            res["optimize_" + name] = dict(n=len(start), m=len(edges), iterations=r["iterations"], cg_iterations=r["cg_iterations"],
                                           **timed(lambda: e.posegraph_optimize(start, E, R.RING_MAX_DIST)))
    print(json.dumps(res, indent=1))
    with open(os.path.join(out_dir, "posegraph_measure.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.getcwd())
