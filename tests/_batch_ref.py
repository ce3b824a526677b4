"""The loop of one problem of the batched alignment (include/symmicp.h, "batched alignment"), restated in numpy: symmicp_align's host
loop with exact brute-force pairs and cumulative apply.  The pass is _record_ref's (moved, nn_ref, record: the kernels' fp32 row
expressions, summed in fp64), the solve is symmicp.solve (a host function: the code the device compiles, with the exact
conditioning), the composition is _solve_ref.mat4_mul (fp32, k sequential) and the stop rule is written out below.

Shared by tests/test_batch_ref.py (which checks this restatement on its own, on the CPU) and tests/test_gpu_batch.py."""
import numpy as np

import _record_ref as RR
import _solve_ref as SR

f32 = np.float32
OK, ERR_DEGENERATE = 0, 3

# the known answer of the cat pair (tests/golden/cat.pcd -> cat_out.pcd): Rz(45 deg), then (2.5, 0, 0)
_c, _s = np.cos(np.pi / 4), np.sin(np.pi / 4)
CAT_TRUTH = np.array([[_c, -_s, 0, 2.5], [_s, _c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def pivot_ref(tgt):
    """the mean of the target rows in fp64, rounded to fp32"""
    return np.asarray(tgt, np.float64).mean(0).astype(f32)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def perturbed(truth, axis, deg, shift, centre):
    """truth followed by a rotation of deg degrees about `axis` through `centre` and a translation `shift` -> 4x4 f32"""
    D = np.eye(4)
    D[:3, :3] = rot(axis, deg)
    D[:3, 3] = np.asarray(centre, np.float64) - D[:3, :3] @ np.asarray(centre, np.float64) + np.asarray(shift, np.float64)
    return (D @ truth).astype(f32)


def cat_guesses(cat):
    """The multi-start guesses of the known-answer tests: the cat pair's answer perturbed by 2 .. 6 degrees about six axes through the
    target's centroid and by 1 .. 3 % of the cloud's extent.  test_batch_ref.py asserts that the reference converges from every one
    of them in PAPER, P2P and PLANE; test_gpu_batch.py runs exactly these."""
    tgt = cat["tgt"].astype(np.float64)
    centre, extent = tgt.mean(0), float(np.linalg.norm(tgt.max(0) - tgt.min(0)))
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, -1, 1), (1, 1, 1)]
    out = []
    for k, ax in enumerate(axes):
        deg = 2.0 + 0.8 * k
        frac = 0.01 + 0.004 * k
        shift = extent * frac * np.roll(np.array([1.0, -0.5, 0.25]), k) / np.linalg.norm([1.0, -0.5, 0.25])
        out.append(perturbed(CAT_TRUTH, ax, deg if k % 2 == 0 else -deg, shift, centre))
    return np.stack(out)


def truth_error(X, cat):
    """rms distance, over the source, between the points moved by X and by the known answer"""
    x = cat["src"].astype(np.float64)
    X = np.asarray(X, np.float64).reshape(4, 4)
    d = (x @ X[:3, :3].T + X[:3, 3]) - (x @ CAT_TRUTH[:3, :3].T + CAT_TRUTH[:3, 3])
    return float(np.sqrt((d ** 2).sum(1).mean()))


def one_pass(mode, X, src, src_n, tgt, tgt_n, pivot, max_corr_dist=0.0, min_normal_dot=-2.0):
    """pass k of a problem: the original source moved by X, exact pairs, the gates, the mode's record about pivot
    -> (record [40], sum of |terms| [40], pairs kept)"""
    if src_n is None:
        src_n = np.zeros_like(np.asarray(src, f32))
    p, pn = RR.moved(X, src, src_n, mode)
    idx, _ = RR.nn_ref(p, tgt)
    return RR.record(mode, p, pn, tgt, tgt_n, idx, pivot, max_d2=RR.f32_max_d2(max_corr_dist), min_ndot=min_normal_dot)


def small_increment(Xi, eps_rotation, eps_translation):
    """the eps rule on an increment (engine_loop.cpp, symmicp_align): fp64 from the fp32 entries, compared with the fp32 bounds"""
    Xi = np.asarray(Xi, f32).reshape(16).astype(np.float64)
    tr = (Xi[0] + Xi[5] + Xi[10] - 1.0) * 0.5
    ang = np.arccos(min(1.0, max(-1.0, tr)))
    tn = np.sqrt(Xi[3] * Xi[3] + Xi[7] * Xi[7] + Xi[11] * Xi[11])
    return bool(ang < float(f32(eps_rotation)) and tn < float(f32(eps_translation)))


def stop_rule(records, solve, cfg, X0=None):
    """symmicp_align's loop, line for line, over a way to get records: records(k, X) -> the record of pass k run with X (a traced
    record, or a pass computed here); solve(record) -> (status, increment 4x4, rcond).  -> dict(status, iters, diff_initial,
    diff_final, diffs, rcond, X = [X_0 .. X_last], passes = number of passes run)"""
    X = np.eye(4, dtype=f32) if X0 is None else np.asarray(X0, f32).reshape(4, 4)
    Xs = [X]
    S = records(0, X)
    diff = f32(S[33])
    out = dict(status=OK, diff_initial=diff, diffs=[], rcond=f32(0))
    iters = 0
    fixed = bool(cfg.get("fixed_iters", 0))
    er, et = cfg.get("eps_rotation", 0.0), cfg.get("eps_translation", 0.0)
    while (fixed or diff > f32(cfg.get("diff_threshold", 1.0))) and iters < cfg.get("max_iters", 10):
        iters += 1
        out["diffs"].append(diff)
        st, Xi, rc = solve(S)
        out["rcond"] = f32(rc)
        if st != OK:
            iters -= 1
            out["status"] = ERR_DEGENERATE
            break
        X = SR.mat4_mul(Xi, X)
        Xs.append(X)
        S = records(iters, X)
        diff = f32(S[33])
        if er > 0 and et > 0 and not fixed and small_increment(Xi, er, et):
            break
    out.update(iters=iters, diff_final=diff, X=Xs, passes=len(Xs), last=S)
    return out


def run(sym, mode, src, src_n, tgt, tgt_n, guess=None, pivot=None, **cfg):
    """one problem from start to end on the CPU -> stop_rule's dict plus records (one per pass) and pivot"""
    pivot = pivot_ref(tgt) if pivot is None else np.asarray(pivot, f32)
    recs = []

    def records(k, X):
        S, _, _ = one_pass(mode, X, src, src_n, tgt, tgt_n, pivot, cfg.get("max_corr_dist", 0.0), cfg.get("min_normal_dot", -2.0))
        recs.append(S)
        return S

    def solve(S):
        r = sym.solve(mode, S, pivot)
        return r[0], np.asarray(r[6], f32).reshape(4, 4), r[5]

    out = stop_rule(records, solve, cfg, guess)
    out.update(records=recs, pivot=pivot)
    return out
