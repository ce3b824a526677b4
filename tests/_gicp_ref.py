"""Numpy references of the plane-to-plane mode (SYMMICP_MODE_GICP, include/symmicp.h), shared by test_gicp.py and test_gpu_gicp.py.

gicp_terms repeats the kernels' expressions (acc_gicp in icp-symm_amd/csrc/kernels_pass.hip) term by term: the u and v rows, their
weights gu and gv and the robust-loss residual in fp32, unfused and in the kernel's association; the axis rows (1/2 J^T J and
1/2 J^T d) in fp64 from the fp32 p and d.  So an fp64 sum of its terms is the record the pass must give, up to summation order.

gicp_direct and gicp_solve are an independent fp64 restatement: the covariances C = I - (1 - eps) n n^T built explicitly, M the
np.linalg.inv of C_p + C_q, H = sum w J^T M J and g = sum w J^T M d with J = [-[p]x, I]; the solve centres at the (weighted) source
centroid, solves H x = -g with np.linalg.solve and composes T(pbar + t) R(a) T(-pbar) in fp64, as _plane_ref.plane_solve does."""
import numpy as np

from _plane_ref import angle_axis, skew
from _record_ref import NSUM, dist2, np_weight

f32 = np.float32
EPS_DEFAULT = 1e-3


def gicp_k(eps, dtype=f32):
    """1 - eps as the engine forms it (fp32: 1.0f - eps, engine_loop.cpp fill_pass_args)"""
    return dtype(1) - dtype(eps)


def gicp_terms(p, pn, q, qn, pivot, eps=EPS_DEFAULT, loss=0, scale=1.0, dtype=f32):
    """per-pair terms [n, 38] of the GICP record and the residuals r = sqrt(d^T M d).  p, pn: the moved source and its (rotated)
    normals; q, qn: the paired target rows.  dtype float32: the kernel's rows; float64: the same expressions in fp64 (a record
    as exact as the closed form allows, for the solve tests)."""
    f = dtype
    pv = np.asarray(pivot, f)
    d2 = dist2(p, q)                                              # (taken before the pivot comes off, as every mode's)
    P = np.asarray(p, f) - pv
    Q = np.asarray(q, f) - pv
    A = np.asarray(pn, f)
    B = np.asarray(qn, f)
    D = P - Q
    k = gicp_k(eps, f)
    cs = np.clip((A[:, 0] * B[:, 0] + A[:, 1] * B[:, 1]) + A[:, 2] * B[:, 2], f(-1), f(1))
    gu = k / (f(4) * (f(2) - k * (f(1) + cs)))
    gv = k / (f(4) * (f(2) - k * (f(1) - cs)))
    U = A + B
    V = A - B
    cu = (D[:, 0] * U[:, 0] + D[:, 1] * U[:, 1]) + D[:, 2] * U[:, 2]
    cv = (D[:, 0] * V[:, 0] + D[:, 1] * V[:, 1]) + D[:, 2] * V[:, 2]
    dd = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    r = np.sqrt((f(0.5) * dd + (gu * cu) * cu) + (gv * cv) * cv)
    n = len(P)
    w = np_weight(loss, scale, r).astype(np.float64) if loss else np.ones(n)
    T = np.zeros((n, 38))
    for L, g, c in ((U, gu, cu), (V, gv, cv)):
        m0 = P[:, 1] * L[:, 2] - P[:, 2] * L[:, 1]
        m1 = P[:, 2] * L[:, 0] - P[:, 0] * L[:, 2]
        m2 = P[:, 0] * L[:, 1] - P[:, 1] * L[:, 0]
        R = np.stack([m0, m1, m2, L[:, 0], L[:, 1], L[:, 2]], 1).astype(np.float64)
        wg = w * g.astype(np.float64)
        kk = 0
        for a in range(6):
            for b in range(a, 6):
                T[:, kk] += wg * R[:, a] * R[:, b]
                kk += 1
        wc = wg * c.astype(np.float64)
        T[:, 21:27] += R * wc[:, None]
        T[:, 35] += wc * c.astype(np.float64)
    # the three axis rows at weight 1/2: 1/2 J^T J and 1/2 J^T d
    P64, D64 = P.astype(np.float64), D.astype(np.float64)
    px, py, pz = P64.T
    h = 0.5 * w
    T[:, 0] += h * (py * py + pz * pz)
    T[:, 1] -= h * px * py
    T[:, 2] -= h * px * pz
    T[:, 4] -= h * pz
    T[:, 5] += h * py
    T[:, 6] += h * (px * px + pz * pz)
    T[:, 7] -= h * py * pz
    T[:, 8] += h * pz
    T[:, 10] -= h * px
    T[:, 11] += h * (px * px + py * py)
    T[:, 12] -= h * py
    T[:, 13] += h * px
    T[:, 15] += h
    T[:, 18] += h
    T[:, 20] += h
    T[:, 21:24] += h[:, None] * np.cross(P64, D64)
    T[:, 24:27] += h[:, None] * D64
    T[:, 35] += h * (D64 * D64).sum(1)
    T[:, 27:30] = w[:, None] * P64
    T[:, 30:33] = w[:, None] * Q.astype(np.float64)
    T[:, 33] = np.sqrt(d2)
    T[:, 34] = w
    T[:, 36] = d2
    T[:, 37] = 1.0 if loss else 0.0
    return T, r


def gicp_record(p, pn, q, qn, pivot, eps=EPS_DEFAULT, loss=0, scale=1.0, dtype=f32):
    """-> (record [40], sum of |terms| [40]: the scale a slot is compared at)"""
    T, _ = gicp_terms(p, pn, q, qn, pivot, eps, loss, scale, dtype)
    S = np.zeros(NSUM)
    M = np.zeros(NSUM)
    S[:38] = T.sum(0)
    M[:38] = np.abs(T).sum(0)
    return S, M


def gicp_pass_record(p, pn, q, qn, idx=None, pivot=(0.0, 0.0, 0.0), eps=EPS_DEFAULT, loss=0, scale=1.0, max_d2=0.0, min_ndot=-2.0):
    """_record_ref.record for GICP: the pass whose moved source is (p, pn), target (q, qn), pairs idx (-1: none; None: identity),
    gated as the kernels gate -> (record, magnitudes, pairs kept)"""
    from _record_ref import gate
    p, pn = np.asarray(p, f32), np.asarray(pn, f32)
    q, qn = np.asarray(q, f32), np.asarray(qn, f32)
    idx = np.arange(len(p)) if idx is None else np.asarray(idx, np.int64)
    has = idx >= 0
    p, pn, j = p[has], pn[has], idx[has]
    keep = gate(p, pn, q[j], qn[j], max_d2, min_ndot)
    S, M = gicp_record(p[keep], pn[keep], q[j[keep]], qn[j[keep]], pivot, eps, loss, scale)
    return S, M, int(keep.sum())


# ---- the independent fp64 restatement ----------------------------------------------------------------------------------------
def gicp_matrices(pn, qn, eps=EPS_DEFAULT):
    """M_i = (C_p + C_q)^-1 per pair [n, 3, 3], C_x = I - (1 - eps) x x^T, by np.linalg.inv"""
    A = np.asarray(pn, np.float64)
    B = np.asarray(qn, np.float64)
    k = 1.0 - float(eps)
    Cp = np.eye(3)[None] - k * A[:, :, None] * A[:, None, :]
    Cq = np.eye(3)[None] - k * B[:, :, None] * B[:, None, :]
    return np.linalg.inv(Cp + Cq)


def gicp_direct(p, pn, q, qn, pivot, eps=EPS_DEFAULT, w=None, centre=None, M=None):
    """-> (H [6, 6], g [6], sum w d^T M d) about the pivot; centre: rotations about this point (about the pivot) instead; M: the
    per-pair [n, 3, 3] to use instead of gicp_matrices (a test's mutant)"""
    pv = np.asarray(pivot, np.float64)
    P = np.asarray(p, np.float64) - pv
    Q = np.asarray(q, np.float64) - pv
    D = P - Q
    w = np.ones(len(P)) if w is None else np.asarray(w, np.float64)
    Pc = P if centre is None else P - np.asarray(centre, np.float64)
    M = gicp_matrices(pn, qn, eps) if M is None else np.asarray(M, np.float64)
    J = np.zeros((len(P), 3, 6))                                 # d(p + a x p + t) / d(a, t) = [-[p]x, I]
    J[:, :, :3] = -np.stack([skew(v) for v in Pc]) if len(P) else 0.0
    J[:, :, 3:] = np.eye(3)
    JM = np.einsum("nij,nik->njk", J, M)
    H = np.einsum("n,njk,nkl->jl", w, JM, J)
    g = np.einsum("n,njk,nk->j", w, JM, D)
    e = float(np.einsum("n,ni,nij,nj->", w, D, M, D))
    return H, g, e


def direct_record(p, pn, q, qn, pivot, eps=EPS_DEFAULT, M=None):
    """gicp_direct in the record's slots: 0..20 = H (upper triangle, row by row), 21..26 = g, 35 = sum d^T M d"""
    H, g, e = gicp_direct(p, pn, q, qn, pivot, eps, M=M)
    D = np.zeros(NSUM)
    D[:21] = H[np.triu_indices(6)]
    D[21:27] = g
    D[35] = e
    return D


# The bar of a record against the fp64 definition.  The kernels' cs is an fp32 dot product of fp32-rounded normals, so gamma_u and
# gamma_v carry a relative error of ~2^-24 / eps whatever the kernel does (d gamma_u / gamma_u ~ d cs / (2 eps) near cs = 1), and
# non-unit normals move the closed form off the inverse by as much.  Slot k is held to FP64_C x 2^-24 / eps x (the sum of its terms'
# magnitudes).  Measured at eps = 1e-3 on the fp32 restatement: 0.08 on the cat pair's first passes, 1.4 on the 200k surface pair
# at its true pose (synth normals, |n|^2 - 1 up to ~1e-7); a record with gamma_u and gamma_v swapped, or the axis rows at weight 1,
# misses it by 100x and more.
FP64_C = 4.0
FP64_SLOTS = list(range(27)) + [35]


def fp64_excess(S, M, D, eps):
    """max over the slots of FP64_SLOTS of |S - D| / (2^-24 / eps x M): <= FP64_C passes; a slot of no magnitude must be 0"""
    S, M, D = (np.asarray(x, np.float64)[FP64_SLOTS] for x in (S, M, D))
    err = np.abs(S - D)
    bar = 2.0 ** -24 / float(eps) * M
    assert not (err[bar == 0] > 1e-300).any()
    return float((err[bar > 0] / bar[bar > 0]).max())


def swapped_matrices(pn, qn, eps=EPS_DEFAULT):
    """a mutant of the closed form in fp64: gamma_u on v v^T and gamma_v on u u^T"""
    A = np.asarray(pn, np.float64)
    B = np.asarray(qn, np.float64)
    k = 1.0 - float(eps)
    cs = np.clip((A * B).sum(1), -1.0, 1.0)
    gu = k / (4 * (2 - k * (1 + cs)))
    gv = k / (4 * (2 - k * (1 - cs)))
    U, V = A + B, A - B
    return 0.5 * np.eye(3)[None] + gv[:, None, None] * U[:, :, None] * U[:, None, :] + gu[:, None, None] * V[:, :, None] * V[:, None, :]


def unpack_upper(S):
    """slots 0..20 -> the symmetric 6 x 6"""
    H = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = S[k]
            k += 1
    return H


def gicp_solve(p, pn, q, qn, pivot, eps=EPS_DEFAULT, w=None):
    """fp64 restatement of one GICP step: H x = -g about the (weighted) source centroid -> dict(a, t, pbar, qbar (caller's frame), X)"""
    pv = np.asarray(pivot, np.float64)
    P = np.asarray(p, np.float64) - pv
    Q = np.asarray(q, np.float64) - pv
    w = np.ones(len(P)) if w is None else np.asarray(w, np.float64)
    pbar = (w[:, None] * P).sum(0) / w.sum()
    qbar = (w[:, None] * Q).sum(0) / w.sum()
    H, g, _ = gicp_direct(p, pn, q, qn, pivot, eps, w, centre=pbar)
    x = np.linalg.solve(H, -g)
    a, t = x[:3], x[3:]
    pa = pbar + pv
    R = angle_axis(a)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = pa + t - R @ pa
    return dict(a=a, t=t, pbar=pa, qbar=qbar + pv, X=X)
