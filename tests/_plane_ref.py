"""Numpy references of the point-to-plane mode (SYMMICP_MODE_PLANE, include/symmicp.h), shared by test_plane.py and
test_gpu_plane.py.

plane_terms repeats the kernels' fp32 expressions (acc_plane in icp-symm_amd/csrc/kernels_pass.hip) element by element, so an fp64
sum of its terms is the record the pass must give up to summation order.  plane_solve is an independent restatement of the solve:
it centres the rows directly from the points (m~ = (p - pbar) x n_q) in fp64, solves the 6 x 6 normal equations with
np.linalg.solve and composes T(pbar + t) R(a) T(-pbar) in fp64."""
import numpy as np

from _record_ref import NSUM, np_weight, plane_terms      # noqa: F401  (the terms live with the other modes' terms)


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
