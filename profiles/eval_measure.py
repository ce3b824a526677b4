"""Measurement of the registration evaluation against its comparators on the 1M / 1M surface pair of the benchmark
("Registration evaluation"; output: profiles/eval_measure.json).

  SYMMICP_PARENT_LIB=<libsymmicp.so of the parent commit> SYMMICP_PARENT_PY=<its icp-symm_amd/py> python profiles/eval_measure.py [OUT_DIR]
        driver: alternates comparator children (the parent commit's build and package: set_target + set_source + begin, begin alone)
        and evaluation children (this build), three of each, and writes OUT_DIR/eval_measure.json (default: the working directory)
  python profiles/eval_measure.py ROLE OUT.json      one child: ROLE = comparator | evaluation
Host clock around calls that end in a stream synchronise; two warm-up calls before every timed series.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the comparator children run the parent commit's build through the parent commit's package
sys.path.insert(0, os.environ["SYMMICP_PARENT_PY"] if os.environ.get("SYMMICP_LIB") else os.path.join(ROOT, "icp-symm_amd", "py"))
N = 1_000_000
REPS = 7


def timed(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def child(role, out_path):
    import numpy as np
    import symmicp
    from symmicp import synth
    d = synth.c4_surface(N)
    src, sn, tgt, tn = d["src"], d["src_n"], d["tgt"], d["tgt_n"]
    res = dict(role=role, lib=symmicp.LIB_PATH, n=N)
    I = np.eye(4, dtype=np.float32)

    def fresh():
        return symmicp.Engine(mode=symmicp.MODE_PAPER, corr=symmicp.CORR_TREE, max_iters=10)

    if role == "comparator":
        def sets_and_begin():
            with fresh() as e:
                e.set_target(tgt, tn)
                e.set_source(src, sn)
                e.begin()
        res["create_set_target_set_source_begin_ms"] = timed(sets_and_begin)
        with fresh() as e:
            def sets_begin_ctx():
                e.set_target(tgt, tn)
                e.set_source(src, sn)
                e.begin()
            res["set_target_set_source_begin_ms"] = timed(sets_begin_ctx)
            res["begin_ms"] = timed(lambda: e.begin())
    else:
        rng = np.random.default_rng(1)
        import math
        def small(k):
            a = math.radians(0.05 * (k + 1))
            X = np.eye(4, dtype=np.float32)
            X[0, 0], X[0, 1], X[1, 0], X[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
            X[:3, 3] = 1e-3 * rng.normal(size=3)
            return X
        Xs = np.stack([small(k) for k in range(64)])
        spacing = float(np.sqrt(1.0 / N))
        res["free_function_ms"] = timed(lambda: symmicp.evaluate_registration(src, tgt, I, 0.0))
        with fresh() as e:
            res["host_arrays_ms"] = timed(lambda: e.evaluate_registration(src, tgt, I, 0.0))
            res["host_arrays_gated_2_spacings_ms"] = timed(lambda: e.evaluate_registration(src, tgt, I, 2 * spacing))
            e.set_target(tgt, tn)
            e.set_source(src, sn)
            res["context_ms"] = timed(lambda: e.evaluate(I, 0.0))
            res["context_gated_2_spacings_ms"] = timed(lambda: e.evaluate(I, 2 * spacing))
            res["context_pairs_ms"] = timed(lambda: e.evaluate(I, 0.0, want_pairs=True))
            res["begin_ms"] = timed(lambda: e.begin())
            res["context_k64_ms"] = timed(lambda: e.evaluate(Xs, 0.0), reps=3, warm=1)
            res["context_64_x_k1_ms"] = timed(lambda: [e.evaluate(Xs[k], 0.0) for k in range(64)], reps=3, warm=1)
            r = e.evaluate(I, 2 * spacing)
            res["fitness_identity_2_spacings"] = r["fitness"]
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    out_dir = sys.argv[1] if len(sys.argv) == 2 else os.getcwd()
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for rep in range(3):
        for role in ("comparator", "evaluation"):
            env = dict(os.environ)
            if role == "comparator":
                env["SYMMICP_LIB"] = os.environ["SYMMICP_PARENT_LIB"]
            path = os.path.join(out_dir, "eval_measure_%s_%d.json" % (role, rep))
            r = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), role, path], env=env)
            print("[measure] %s %d -> rc %d" % (role, rep, r.returncode), flush=True)
            if r.returncode != 0:
                sys.exit(r.returncode)
            runs.append(json.load(open(path)))
    with open(os.path.join(out_dir, "eval_measure.json"), "w") as f:
        json.dump(runs, f, indent=1)
    for r in runs:
        print(r["role"], {k: (round(min(v), 3), round(sorted(v)[len(v) // 2], 3), round(max(v), 3)) for k, v in r.items() if isinstance(v, list)})


if __name__ == "__main__":
    if len(sys.argv) == 3:
        child(sys.argv[1], sys.argv[2])
    else:
        main()
