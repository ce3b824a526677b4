"""Numpy references of the point-to-plane mode (SYMMICP_MODE_PLANE, include/symmicp.h), shared by test_plane.py and
test_gpu_plane.py.

plane_terms repeats the kernels' fp32 expressions (acc_plane in icp-symm_amd/csrc/kernels_pass.hip) element by element, so an fp64
sum of its terms is the record the pass must give up to summation order.  plane_solve is an independent restatement of the solve:
it centres the rows directly from the points (m~ = (p - pbar) x n_q) in fp64, solves the 6 x 6 normal equations with
np.linalg.solve and composes T(pbar + t) R(a) T(-pbar) in fp64."""
import numpy as np

NSUM = 40


def np_weight(loss, scale, r):
    """robust_loss.h in fp32 (0 = none)"""
    r = np.asarray(r, np.float32)
    one = np.float32(1)
    with np.errstate(divide="ignore", over="ignore"):
        u = r / np.float32(scale)
        au = np.abs(u)
        u2 = u * u
        if loss == 1:
            return np.where(au <= one, one, one / au).astype(np.float32)
        if loss == 2:
            t = one - u2
            return np.where(au < one, t * t, np.float32(0)).astype(np.float32)
        if loss == 3:
            return (one / (one + u2)).astype(np.float32)
        if loss == 4:
            t = one + u2
            return (one / (t * t)).astype(np.float32)
    return np.ones_like(r)


def plane_terms(p, q, nq, pivot, loss=0, scale=1.0, dtype=np.float32):
    """per-pair terms [n, 38] of the PLANE record and the residuals r = c.  dtype float32: the kernels' rows (fp32, unfused, their
    association); float64: the same rows in fp64 (an exact-as-possible record for the solve tests)."""
    f = dtype
    pv = np.asarray(pivot, f)
    R = np.asarray(p, np.float32) - np.asarray(q, np.float32)          # (the pair's distance is taken before the pivot comes off)
    d2 = (R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]) + R[:, 2] * R[:, 2]
    P = np.asarray(p, f) - pv
    Q = np.asarray(q, f) - pv
    N = np.asarray(nq, f)
    D = P - Q
    m0 = P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1]
    m1 = P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2]
    m2 = P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]
    c = (D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]
    n = len(P)
    w = np_weight(loss, scale, c).astype(np.float64) if loss else np.ones(n)
    V = np.stack([m0, m1, m2, N[:, 0], N[:, 1], N[:, 2]], 1).astype(np.float64)
    T = np.zeros((n, 38))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            T[:, k] = w * V[:, a] * V[:, b]
            k += 1
    cd = c.astype(np.float64)
    T[:, 21:27] = V * (w * cd)[:, None]
    T[:, 27:30] = w[:, None] * P.astype(np.float64)
    T[:, 30:33] = w[:, None] * Q.astype(np.float64)
    T[:, 33] = np.sqrt(d2)
    T[:, 34] = w
    T[:, 35] = w * cd * cd
    T[:, 36] = d2
    T[:, 37] = 1.0 if loss else 0.0
    return T, c


def plane_record(p, q, nq, pivot, loss=0, scale=1.0, dtype=np.float32):
    """-> (record [40], sum of |terms| [40]: the scale a slot is compared at)"""
    T, _ = plane_terms(p, q, nq, pivot, loss, scale, dtype)
    S = np.zeros(NSUM)
    M = np.zeros(NSUM)
    S[:38] = T.sum(0)
    M[:38] = np.abs(T).sum(0)
    return S, M


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def angle_axis(a):
    a = np.asarray(a, np.float64)
    th = np.linalg.norm(a)
    if th == 0.0:
        return np.eye(3)
    k = skew(a / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def plane_solve(p, q, nq, pivot, w=None):
    """fp64 restatement: the rows centred at the (weighted) source centroid, the normal equations solved directly.
    -> dict(a, t, pbar (caller's frame), qbar, X 4x4)"""
    pv = np.asarray(pivot, np.float64)
    P = np.asarray(p, np.float64) - pv
    Q = np.asarray(q, np.float64) - pv
    N = np.asarray(nq, np.float64)
    w = np.ones(len(P)) if w is None else np.asarray(w, np.float64)
    pbar = (w[:, None] * P).sum(0) / w.sum()
    qbar = (w[:, None] * Q).sum(0) / w.sum()
    V = np.concatenate([np.cross(P - pbar, N), N], 1)
    c = ((P - Q) * N).sum(1)
    A = (V * w[:, None]).T @ V
    b = (V * (w * c)[:, None]).sum(0)
    x = np.linalg.solve(A, -b)
    a, t = x[:3], x[3:]
    pa = pbar + pv
    R = angle_axis(a)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = pa + t - R @ pa
    return dict(a=a, t=t, pbar=pa, qbar=qbar + pv, X=X)


def rot_err(X, truth):
    """rotation angle of X R_truth^T (stable near 0) and the largest translation error"""
    Rd = np.asarray(X, np.float64)[:3, :3] @ np.asarray(truth, np.float64)[:3, :3].T
    s = np.linalg.norm(Rd - Rd.T) / (2.0 * np.sqrt(2.0))
    c = (np.trace(Rd) - 1.0) / 2.0
    return float(np.arctan2(s, c)), float(np.abs(np.asarray(X, np.float64)[:3, 3] - np.asarray(truth, np.float64)[:3, 3]).max())
