"""Trimmed ICP (include/symmicp.h, symmicp_set_trim_fraction) restated in numpy, on top of _record_ref.py.

A trimmed pass keeps the closest fraction rho of its candidate pairs:
  candidates  the pairs that exist (target row >= 0) and pass the two gates (_record_ref.gate); n_c of them
  d2          _record_ref.dist2 at the moved position (fp32, the kernels' expression)
  k           ceil(double(fp32 rho) * double(n_c)) clamped to [1, n_c]
  tau         the k-th smallest candidate d2; the kept set is the candidates with d2 <= tau (ties kept)
and its record is _record_ref.record over the kept pairs.  Also here: the partial-overlap surface pair the feature is for, and
an fp64 point-to-plane loop (exact nearest neighbours) with and without trimming."""
import math

import numpy as np

import _record_ref as R

f32 = np.float32


def trim_k(rho, n_c):
    """the rank of the threshold: rho is rounded to fp32 first, the product and the ceiling are taken in double"""
    n_c = int(n_c)
    if n_c == 0:
        return 0
    k = int(math.ceil(float(f32(rho)) * float(n_c)))
    return min(max(k, 1), n_c)


def trim_select(d2_cand, rho):
    """-> (k, tau as fp32, kept mask over the candidates); no candidates: (0, fp32 0, empty mask)"""
    d2 = np.asarray(d2_cand, f32)
    k = trim_k(rho, len(d2))
    if k == 0:
        return 0, f32(0), np.zeros(0, bool)
    tau = np.partition(d2, k - 1)[k - 1]
    return k, f32(tau), d2 <= tau


def trim_pass(p, pn, q, qn, idx, rho, max_d2=0.0, min_ndot=-2.0):
    """the trimmed pass over the moved source (p, pn), target (q, qn) and pairs idx (-1: none; None: identity pairing)
    -> dict(cand = candidate mask over the source rows, n_c, k, tau (fp32), kept = kept mask over the source rows, d2 = fp32 d2 of
    every existing pair, 0 elsewhere)"""
    p, pn = np.asarray(p, f32), np.asarray(pn, f32)
    q, qn = np.asarray(q, f32), np.asarray(qn, f32)
    n = len(p)
    idx = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    has = idx >= 0
    rows = np.flatnonzero(has)
    j = idx[rows]
    d2 = np.zeros(n, f32)
    d2[rows] = R.dist2(p[rows], q[j])
    cand = np.zeros(n, bool)
    cand[rows] = R.gate(p[rows], pn[rows], q[j], qn[j], max_d2, min_ndot)
    k, tau, keep_c = trim_select(d2[cand], rho)
    kept = np.zeros(n, bool)
    kept[np.flatnonzero(cand)] = keep_c
    return dict(cand=cand, n_c=int(cand.sum()), k=k, tau=tau, kept=kept, d2=d2)


def trimmed_record(mode, p, pn, q, qn, idx, kept, pivot, loss=0, scale=1.0, eps=1e-3):
    """_record_ref.record over the kept pairs only (they passed the gates already: none is applied again)"""
    n = len(p)
    idx = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    return R.record(mode, p, pn, q, qn, np.where(kept, idx, -1), pivot, loss, scale, 0.0, -2.0, eps)


# ---- the partial-overlap pair ---------------------------------------------------------------------------------------------------
def partial_overlap(n=20000, seed=0xC4):
    """two scans of the C4 height field that share 4/7 of the source: the source covers u in [0, 0.7], the target u in [0.3, 1]
    (another sampling) moved by c4_surface's motion (3 degrees about (2, -1, 4), t = (0.004, 0.003, -0.002)).  spacing =
    sqrt(0.7 / n), the mean sample spacing of either cloud."""
    from symmicp import synth
    ps, ns = synth._surface(0.7 * synth.uniform01(seed, n, 0), synth.uniform01(seed, n, 1))
    pt, nt = synth._surface(0.3 + 0.7 * synth.uniform01(seed + 1, n, 0), synth.uniform01(seed + 1, n, 1))
    Rm = synth.rotation(3.0, (2, -1, 4))
    t = np.array([0.004, 0.003, -0.002])
    return dict(src=ps.astype(f32), src_n=ns.astype(f32), tgt=(pt @ Rm.T + t).astype(f32), tgt_n=(nt @ Rm.T).astype(f32),
                truth=synth.rigid4(Rm, t), spacing=math.sqrt(0.7 / n))


def rms_spacings(T, d):
    """rms distance, in sample spacings, between the source under T and under the true transform"""
    x = d["src"].astype(np.float64)
    T = np.asarray(T, np.float64)
    a = x @ T[:3, :3].T + T[:3, 3]
    b = x @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1).mean())) / d["spacing"]


def _rodrigues(a):
    th = float(np.linalg.norm(a))
    if th < 1e-300:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def plane_icp_fp64(d, rho=1.0, iters=30):
    """point-to-plane ICP in fp64 with exact nearest neighbours: each iteration pairs every source point with its nearest target
    point, keeps the closest fraction rho of the pairs (trim_k's rank, ties kept), solves the linearised 6x6 system about the kept
    source centroid and composes the increment -> the 4x4"""
    from scipy.spatial import cKDTree
    src = d["src"].astype(np.float64)
    tgt = d["tgt"].astype(np.float64)
    tn = d["tgt_n"].astype(np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4)
    for _ in range(iters):
        p = src @ T[:3, :3].T + T[:3, 3]
        dist, j = tree.query(p)
        d2 = dist * dist
        keep = np.ones(len(p), bool)
        if rho < 1.0:
            k = trim_k(rho, len(p))
            keep = d2 <= np.partition(d2, k - 1)[k - 1]
        P, Q, N = p[keep], tgt[j[keep]], tn[j[keep]]
        c0 = P.mean(0)
        Pc = P - c0
        V = np.concatenate([np.cross(Pc, N), N], 1)
        c = ((P - Q) * N).sum(1)
        x = np.linalg.solve(V.T @ V, -(V.T @ c))
        Rm = _rodrigues(x[:3])
        inc = np.eye(4)
        inc[:3, :3] = Rm
        inc[:3, 3] = c0 + x[3:] - Rm @ c0
        T = inc @ T
    return T
