"""Plain numpy references for feature matching and RANSAC (kernels_global.hip; include/symmicp.h defines the arithmetic).

feature_nn()        the header's D(i, j) in np.float32, one operation at a time in ascending bin order (numpy's float32 ufuncs round
                    every operation and fuse nothing), then nn = the lowest row of the minimum and second = the minimum over the
                    other rows: what the device must reproduce bit for bit.
correspondences()   the mutual and ratio filters on top of it.
draws()             the three SplitMix64 draws of every hypothesis (integers: exact).
hypotheses()        status, R and t of every hypothesis in fp64 from the SAME fp32 inputs (the pivoted points), with every check
                    evaluated whether it is reached or not, and `clear`: every compared quantity is more than a relative CLEAR = 1e-4
                    away from its threshold (a hypothesis with a repeated draw is never clear: its triangle has a zero edge).
inlier_counts()     |R p + t - q| <= dist over the correspondences, fp64.
kabsch()            the least-squares rigid fit by SVD, fp64.
ransac()            the whole method in fp64: what the table of numbers in tests/test_global_ref.py pins.
bumps_pair()        the hard synthetic pair: a height field of 24 Gaussian bumps, 75 % overlap, 140 degrees apart.

DELTA.  A device inlier count is compared with the fp64 counts at max_dist * (1 -+ DELTA).  DELTA is four times the largest
displacement between the device's fp32 transform and the fp64 transform of the same hypothesis, over every correspondence point and
every evaluated hypothesis of the inputs of tests/test_gpu_global.py, as a fraction of max_dist (rounding differs between
libraries; four leaves room without hiding a wrong transform, which shows as a displacement of order 1).
tests/test_gpu_global.py::test_hypotheses_against_fp64 measures it again, prints it and asserts that it stays below half of DELTA
(twice the recorded value).  Measured on an MI355X:

    input (max_dist)                                 evaluated      largest displacement / max_dist
    cat, H = 4 000, seeds 1-3 (2.7625)               3 966-3 974    7.74e-5
    the same shifted by 1e4 in every coordinate      3 966-3 974    1.17e-4
    bumps, H = 262 144, seeds 1-8 (0.01183)          494-575        1.40e-4   (seed 8)

    MEASURED_DISPLACEMENT = 1.41e-4, DELTA = 4 x 1.41e-4 = 5.64e-4
(a CPU fp32 prototype of the same arithmetic gave 1.2e-4 to 1.9e-4.)
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "icp-symm_amd", "py")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CLEAR = 1e-4
MEASURED_DISPLACEMENT = 1.41e-4
DELTA = 4 * MEASURED_DISPLACEMENT

EVALUATED, REPEATED, EDGE, DEGENERATE, FAR = range(5)
F = np.float32


# ---- feature matching -----------------------------------------------------------------------------------------------------------
def feature_d2(fa, fb):
    """D(i, j) of the header for every row of fa against every row of fb -> [na, nb] float32"""
    fa, fb = np.ascontiguousarray(fa, F), np.ascontiguousarray(fb, F)
    acc = np.zeros((fa.shape[0], fb.shape[0]), F)
    with np.errstate(over="ignore"):
        for b in range(33):
            t = fa[:, b][:, None] - fb[:, b][None, :]
            acc = acc + t * t
    return acc


def feature_nn(fa, fb, budget=1 << 24):
    """-> (nn [na] int32, d2 [na] f32, second [na] f32); queries in chunks of about `budget` pairs"""
    fa, fb = np.ascontiguousarray(fa, F), np.ascontiguousarray(fb, F)
    na, nb = fa.shape[0], fb.shape[0]
    nn = np.zeros(na, np.int32)
    d2 = np.zeros(na, F)
    second = np.full(na, np.inf, F)
    step = max(1, budget // nb)
    for a in range(0, na, step):
        D = feature_d2(fa[a:a + step], fb)
        j = D.argmin(1)                                   # the first, i.e. lowest, row of the minimum
        rows = np.arange(D.shape[0])
        nn[a:a + step] = j
        d2[a:a + step] = D[rows, j]
        if nb > 1:
            D[rows, j] = np.inf
            second[a:a + step] = D.min(1)
    return nn, d2, second


def correspondences(fa, fb, mutual=True, max_ratio=0.0):
    """-> (pairs [count, 2] int32 in ascending i, d2 [count] f32)"""
    nn, d2, second = feature_nn(fa, fb)
    keep = np.ones(len(nn), bool)
    if mutual:
        back = feature_nn(fb, fa)[0]
        keep &= back[nn] == np.arange(len(nn))
    if max_ratio > 0:
        r2 = F(max_ratio) * F(max_ratio)
        with np.errstate(invalid="ignore", over="ignore"):
            keep &= d2 <= r2 * second
    i = np.nonzero(keep)[0]
    return np.stack([i, nn[i]], 1).astype(np.int32), d2[i]


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------------
def draws(seed, H, m):
    """c [H, 3] int64: c_k = ((u(3h + k) >> 32) * m) >> 32"""
    from symmicp import synth
    u = synth.splitmix64(seed, 3 * H, 0)
    return (((u >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64).reshape(H, 3)


def pivoted(src, tgt, pairs, pivots=None):
    """the fp32 points the device works on: p = src[pairs[:, 0]] - cs, q = tgt[pairs[:, 1]] - ct, cs / ct the fp64 means rounded
    to fp32 (or the given pivots [2, 3]) -> (p [m, 3] f32, q [m, 3] f32, cs, ct)"""
    x, y = np.asarray(src, F)[pairs[:, 0]], np.asarray(tgt, F)[pairs[:, 1]]
    if pivots is None:
        cs, ct = x.astype(np.float64).mean(0).astype(F), y.astype(np.float64).mean(0).astype(F)
    else:
        cs, ct = np.asarray(pivots[0], F), np.asarray(pivots[1], F)
    return x - cs, y - ct, cs, ct


def _far(a, b, rel):
    """a and b differ by more than `rel`, relatively"""
    return np.abs(a - b) > rel * np.maximum(np.abs(a), np.abs(b))


def _frame(u, v):
    e1 = u / np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(e1, v)
    e3 = w / np.linalg.norm(w, axis=1, keepdims=True)
    return e1, np.cross(e3, e1), e3


def hypotheses(p, q, c, max_dist, edge_ratio=0.9):
    """p, q: the pivoted fp32 points; c: draws [H, 3] -> dict(status [H], Rt [H, 12] f64 (R row-major, then t), clear [H] bool)"""
    P, Q = p.astype(np.float64)[c], q.astype(np.float64)[c]          # [H, 3 samples, 3]
    H = len(c)
    md2 = float(F(max_dist)) ** 2
    e2 = float(F(edge_ratio)) ** 2 if edge_ratio > 0 else 0.0
    rep = (c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 0] == c[:, 2])
    clear = ~rep
    with np.errstate(all="ignore"):
        edge = np.zeros(H, bool)
        if e2 > 0:
            for a, b in ((0, 1), (1, 2), (2, 0)):
                lp, lq = ((P[:, a] - P[:, b]) ** 2).sum(1), ((Q[:, a] - Q[:, b]) ** 2).sum(1)
                edge |= (lp < e2 * lq) | (lq < e2 * lp)
                clear &= _far(lp, e2 * lq, CLEAR) & _far(lq, e2 * lp, CLEAR)
        up, vp, uq, vq = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0]
        deg = np.zeros(H, bool)
        for u, v in ((up, vp), (uq, vq)):
            prod = (u * u).sum(1) * (v * v).sum(1)
            w2 = (np.cross(u, v) ** 2).sum(1)
            deg |= ~(prod > 0) | (w2 < 1e-4 * prod)
            clear &= _far(w2, 1e-4 * prod, CLEAR)
        fp, fq = _frame(up, vp), _frame(uq, vq)
        R = sum(fq[k][:, :, None] * fp[k][:, None, :] for k in range(3))
        t = Q.mean(1) - np.einsum("hij,hj->hi", R, P.mean(1))
        r2 = ((np.einsum("hij,hkj->hki", R, P) + t[:, None, :] - Q) ** 2).sum(2)          # [H, 3]
        far = ~(r2 <= md2).all(1)
        clear &= _far(r2, md2, CLEAR).all(1) & np.isfinite(r2).all(1)
    status = np.where(rep, REPEATED, np.where(edge, EDGE, np.where(deg, DEGENERATE, np.where(far, FAR, EVALUATED)))).astype(np.uint8)
    Rt = np.concatenate([R.reshape(H, 9), t], 1)
    return dict(status=status, Rt=Rt, clear=clear)


def residuals(Rt, p, q):
    """|R p_k + t - q_k| for the transforms Rt [h, 12] over all correspondences -> [h, m] f64"""
    R, t = Rt[:, :9].reshape(-1, 3, 3), Rt[:, 9:]
    d = np.einsum("hij,kj->hki", R, p.astype(np.float64)) + t[:, None, :] - q.astype(np.float64)[None]
    return np.sqrt((d * d).sum(2))


def inlier_counts(Rt, p, q, dist, chunk=512):
    out = np.zeros(len(Rt), np.int64)
    for a in range(0, len(Rt), chunk):
        out[a:a + chunk] = (residuals(Rt[a:a + chunk], p, q) <= dist).sum(1)
    return out


def kabsch(X, Y):
    """the proper rotation R and translation t minimising sum |R x + t - y|^2 -> 4x4 f64"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    cx, cy = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((X - cx).T @ (Y - cy))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = cy - R @ cx
    return T


def inlier_mask64(T, X, Y, max_dist):
    d = np.asarray(X, np.float64) @ T[:3, :3].T + T[:3, 3] - np.asarray(Y, np.float64)
    return (d * d).sum(1) <= float(F(max_dist)) ** 2


def ransac(src, tgt, pairs, max_dist, H, seed, edge_ratio=0.9, refits=1):
    """the method in fp64 -> dict(status [H], inliers [H], best, runner_up, T [4, 4] (caller's coordinates), T_ransac, mask, evaluated)
    or None when there is no consensus"""
    p, q, cs, ct = pivoted(src, tgt, pairs)
    c = draws(seed, H, len(pairs))
    hy = hypotheses(p, q, c, max_dist, edge_ratio)
    ev = np.nonzero(hy["status"] == EVALUATED)[0]
    inl = np.zeros(H, np.int64)
    inl[ev] = inlier_counts(hy["Rt"][ev], p, q, float(F(max_dist)))
    if len(ev) == 0 or inl.max() < 3:
        return None
    best = int(np.argmax(inl))                                         # the lowest h of the maximum
    R, t = hy["Rt"][best, :9].reshape(3, 3), hy["Rt"][best, 9:]
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t + ct.astype(np.float64) - R @ cs.astype(np.float64)
    X, Y = np.asarray(src, F)[pairs[:, 0]].astype(np.float64), np.asarray(tgt, F)[pairs[:, 1]].astype(np.float64)
    mask = residuals(hy["Rt"][best:best + 1], p, q)[0] <= float(F(max_dist))
    T0 = T.copy()
    for _ in range(refits):
        T = kabsch(X[mask], Y[mask])
        mask = inlier_mask64(T, X, Y, max_dist)
    others = np.delete(inl, best)
    return dict(status=hy["status"], clear=hy["clear"], inliers=inl, best=best, runner_up=int(others.max()) if len(others) else 0,
                T=T, T_ransac=T0, mask=mask, evaluated=len(ev))


# ---- errors against a known truth ----------------------------------------------------------------------------------------------------
def rotation_error_deg(T, truth):
    R = np.asarray(T, np.float64)[:3, :3] @ np.asarray(truth, np.float64)[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


def rms_to_truth(T, truth, src):
    x = np.asarray(src, np.float64)
    T, truth = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    d = (x @ T[:3, :3].T + T[:3, 3]) - (x @ truth[:3, :3].T + truth[:3, 3])
    return float(np.sqrt((d * d).sum(1).mean()))


# ---- the hard pair -------------------------------------------------------------------------------------------------------------------
def _bumps(u, v):
    """a height field of 24 Gaussian bumps over the unit square and its analytic normals"""
    from symmicp import synth
    cen = synth.uniform01(0xB0, 48, 0).reshape(24, 2)
    wid = 0.04 + 0.10 * synth.uniform01(0xB0, 24, 1)
    hgt = 0.3 * (synth.uniform01(0xB0, 24, 2) - 0.5)
    du, dv = u[:, None] - cen[None, :, 0], v[:, None] - cen[None, :, 1]
    g = hgt * np.exp(-(du * du + dv * dv) / (2.0 * wid * wid))
    z = g.sum(1)
    zu, zv = (-g * du / (wid * wid)).sum(1), (-g * dv / (wid * wid)).sum(1)
    n = np.stack([-zu, -zv, np.ones_like(u)], 1)
    return np.stack([u, v, z], 1), n / np.linalg.norm(n, axis=1, keepdims=True)


BUMPS_ROTATION = (140.0, (0.3, 0.5, 0.8))
BUMPS_TRANSLATION = (0.7, -0.4, 1.1)


def bumps_pair(n=6000, shift=None):
    """source: n points of the surface over u in [0, 0.8]; target: n DIFFERENT points over u in [0.2, 1] (75 % overlap), jittered
    by a quarter of the spacing per axis, then moved by 140 degrees about (0.3, 0.5, 0.8) and (0.7, -0.4, 1.1).  shift: added to
    both clouds before the motion is composed (the truth is conjugated accordingly).
    -> dict(src, src_n, tgt, tgt_n (f32), truth [4, 4], spacing, radius = 12 spacings, max_dist = 2 spacings)"""
    from scipy.spatial import cKDTree
    from symmicp import synth
    ps, ns = _bumps(0.8 * synth.uniform01(11, n, 0), synth.uniform01(11, n, 1))
    pt, nt = _bumps(0.2 + 0.8 * synth.uniform01(12, n, 0), synth.uniform01(12, n, 1))
    spacing = float(np.median(cKDTree(ps).query(ps, 2)[0][:, 1]))
    pt = pt + 0.25 * spacing * (2.0 * np.stack([synth.uniform01(13, n, k) for k in range(3)], 1) - 1.0)
    R = synth.rotation(*BUMPS_ROTATION)
    t = np.array(BUMPS_TRANSLATION)
    tgt, tn = pt @ R.T + t, nt @ R.T
    truth = synth.rigid4(R, t)
    if shift is not None:
        s = np.asarray(shift, np.float64)
        ps, tgt = ps + s, tgt + s
        truth = synth.rigid4(R, t + s - R @ s)
    return dict(src=ps.astype(F), src_n=ns.astype(F), tgt=tgt.astype(F), tgt_n=tn.astype(F), truth=truth, spacing=spacing,
                radius=12.0 * spacing, max_dist=2.0 * spacing)


def reference_fpfh(xyz, nrm, r):
    """the fp64 FPFH of tests/_fpfh_ref.py for a whole cloud"""
    import _fpfh_ref as R
    count, offs, rows, d2 = R.radius_sets(xyz, r)
    c, k = R.spfh_counts(xyz, nrm, np.arange(len(xyz)), offs, rows, np.float64)
    return R.fpfh_from_spfh(np.where(k[:, None] > 0, 100.0 * c / np.maximum(k, 1)[:, None], 0.0), offs, rows, d2)


def mutual_matches_kdtree(fs, ft):
    """mutual nearest neighbours in feature space by SciPy's k-d tree (fp64): the independent matching of the reference pipeline"""
    from scipy.spatial import cKDTree
    ab = cKDTree(ft).query(fs, 1)[1]
    ba = cKDTree(fs).query(ft, 1)[1]
    i = np.nonzero(ba[ab] == np.arange(len(fs)))[0]
    return np.stack([i, ab[i]], 1).astype(np.int32)
