"""Colored ICP (SYMMICP_MODE_COLOR, include/symmicp.h) restated in numpy, on top of _record_ref.py: the intensity gradient on the
tangent plane (fp64, every step in the order the header writes it), the COLOR record (fp32 rows as acc_color forms them in
icp-symm_amd/csrc/kernels_pass.hip, fp64 sums; gates, robust loss and trimming as the other modes' records), and an fp64 colored-ICP
loop with exact nearest neighbours."""
import math

import numpy as np

import _record_ref as R
import _trim_ref as TR

f32 = np.float32
MODE_COLOR = 7
LAMBDA_DEFAULT = 0.968


# ---- the gradient ------------------------------------------------------------------------------------------------------------
def gradient(xyz, nrm, intensity, rows, want_cond=False):
    """symmicp_ctx_intensity_gradient in fp64.  rows [n, k]: every point's k-NN set in ascending (d2, row) order, the point itself
    included (symmicp_ctx_knn's output, or knn_rows below); row i itself is left out BY ROW.
    -> (g [n, 3] fp64 -- exactly 0 on degenerate rows --, degenerate mask [, condition number of A on the others])"""
    x = np.asarray(xyz, f32).astype(np.float64)
    nn = np.asarray(nrm, f32).astype(np.float64)
    it = np.asarray(intensity, f32).astype(np.float64)
    rows = np.asarray(rows, np.int64)
    n, k = rows.shape
    me = np.arange(n)
    nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
    z = np.zeros(n)
    m00, m01, m02, m11, m12, m22, r0, r1, r2 = (z.copy() for _ in range(9))
    for c in range(k):
        j = rows[:, c]
        use = (j != me) & (j >= 0)
        jj = np.where(use, j, 0)
        dx, dy, dz = x[jj, 0] - x[:, 0], x[jj, 1] - x[:, 1], x[jj, 2] - x[:, 2]
        s = (dx * nx + dy * ny) + dz * nz
        ex, ey, ez = dx - s * nx, dy - s * ny, dz - s * nz
        di = it[jj] - it
        u = use.astype(np.float64)                      # (a skipped neighbour adds an exact 0)
        m00 = m00 + u * (ex * ex); m01 = m01 + u * (ex * ey); m02 = m02 + u * (ex * ez)
        m11 = m11 + u * (ey * ey); m12 = m12 + u * (ey * ez); m22 = m22 + u * (ez * ez)
        r0 = r0 + u * (ex * di); r1 = r1 + u * (ey * di); r2 = r2 + u * (ez * di)
    mu = ((m00 + m11) + m22) / 2.0
    a00, a01, a02 = m00 + (mu * nx) * nx, m01 + (mu * nx) * ny, m02 + (mu * nx) * nz
    a11, a12, a22 = m11 + (mu * ny) * ny, m12 + (mu * ny) * nz, m22 + (mu * nz) * nz
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    t = ((a00 + a11) + a22) / 3.0
    ok = det > 1e-12 * ((t * t) * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
    g[~ok] = 0.0
    if not want_cond:
        return g, ~ok
    A = np.stack([np.stack([a00, a01, a02], 1), np.stack([a01, a11, a12], 1), np.stack([a02, a12, a22], 1)], 1)
    return g, ~ok, np.linalg.cond(A[ok])


def knn_rows(xyz, k):
    """the k-NN sets of symmicp_ctx_knn for a cloud WITHOUT exact ties (the synthetic pairs): rows in ascending fp32 (d2, row)"""
    from scipy.spatial import cKDTree
    x = np.asarray(xyz, f32)
    kk = min(len(x), k + 6)
    _, cand = cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=kk)
    d2 = np.stack([R.dist2(x, x[cand[:, c]]) for c in range(kk)], 1)
    # (d2, row): sort by row first, then stably by d2
    byrow = np.argsort(cand, axis=1, kind="stable")
    cand_r = np.take_along_axis(cand, byrow, 1)
    d2_r = np.take_along_axis(d2, byrow, 1)
    order = np.argsort(d2_r, axis=1, kind="stable")
    return np.take_along_axis(cand_r, order, 1)[:, :k].astype(np.int32)


# ---- the record ----------------------------------------------------------------------------------------------------------------
def color_terms(p, q, nq, gq, iq, ip, pivot, lam=LAMBDA_DEFAULT, loss=0, scale=1.0):
    """per-pair terms [n, 38] of the COLOR record (acc_color), their magnitudes (|geometric row's term| + |photometric row's|: the
    kernels add the two rows one after the other) and the residuals r = sqrtf((lam c_G) c_G + (om c_C) c_C)"""
    pv = np.asarray(pivot, f32)
    lam = f32(lam)
    om = f32(f32(1.0) - lam)
    d2 = R.dist2(p, q)
    P = np.asarray(p, f32) - pv
    Q = np.asarray(q, f32) - pv
    N = np.asarray(nq, f32)
    G = np.asarray(gq, f32)
    D = P - Q
    m0 = P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1]
    m1 = P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2]
    m2 = P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]
    cg = (D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]
    k0 = P[:, 1] * G[:, 2] - P[:, 2] * G[:, 1]
    k1 = P[:, 2] * G[:, 0] - P[:, 0] * G[:, 2]
    k2 = P[:, 0] * G[:, 1] - P[:, 1] * G[:, 0]
    cc = ((D[:, 0] * G[:, 0] + D[:, 1] * G[:, 1]) + D[:, 2] * G[:, 2]) + (np.asarray(iq, f32) - np.asarray(ip, f32))
    r = np.sqrt((lam * cg) * cg + (om * cc) * cc)
    n = len(P)
    w = R.np_weight(loss, scale, r).astype(np.float64) if loss else np.ones(n)
    T = np.zeros((n, 38))
    A = np.zeros((n, 38))
    for V, c, o in ((np.stack([m0, m1, m2, N[:, 0], N[:, 1], N[:, 2]], 1).astype(np.float64), cg.astype(np.float64), float(lam)),
                    (np.stack([k0, k1, k2, G[:, 0], G[:, 1], G[:, 2]], 1).astype(np.float64), cc.astype(np.float64), float(om))):
        wo = w * o
        s = 0
        for a in range(6):
            for b in range(a, 6):
                t = wo * V[:, a] * V[:, b]
                T[:, s] += t
                A[:, s] += np.abs(t)
                s += 1
        t = V * (wo * c)[:, None]
        T[:, 21:27] += t
        A[:, 21:27] += np.abs(t)
        T[:, 35] += wo * c * c
    T[:, 27:30] = w[:, None] * P.astype(np.float64)
    T[:, 30:33] = w[:, None] * Q.astype(np.float64)
    T[:, 33] = np.sqrt(d2)
    T[:, 34] = w
    T[:, 36] = d2
    T[:, 37] = 1.0 if loss else 0.0
    A[:, 27:] = np.abs(T[:, 27:])
    return T, A, r


def color_record(p, pn, ip, q, qn, gq, iq, idx=None, pivot=(0.0, 0.0, 0.0), lam=LAMBDA_DEFAULT, loss=0, scale=1.0, max_d2=0.0,
                 min_ndot=-2.0, rho=1.0):
    """-> (record [40], sum of |terms| [40], kept mask over the source rows) of the COLOR pass whose moved source is (p, pn) with
    intensities ip, target (q, qn, gq, iq) and pairs idx (-1: no pair; None: identity pairing); the gates, then the trim fraction
    rho, act on the pair before its rows, as in every mode."""
    p, pn = np.asarray(p, f32), np.asarray(pn, f32)
    q, qn = np.asarray(q, f32), np.asarray(qn, f32)
    n = len(p)
    idx = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    tp = TR.trim_pass(p, pn, q, qn, idx, rho, max_d2, min_ndot)
    kept = tp["kept"] if rho < 1.0 else tp["cand"]
    j = idx[kept]
    T, A, _ = color_terms(p[kept], q[j], qn[j], np.asarray(gq, f32)[j], np.asarray(iq, f32)[j], np.asarray(ip, f32)[kept], pivot, lam, loss, scale)
    S = np.zeros(R.NSUM)
    M = np.zeros(R.NSUM)
    S[:38] = T.sum(0)
    M[:38] = A.sum(0)
    return S, M, kept


# ---- the fp64 loop ---------------------------------------------------------------------------------------------------------------
def rms_spacings(T, d):
    return TR.rms_spacings(T, d)


def _system(p, Q, N, G, dI, lam):
    """the 6x6 normal matrix and right-hand side about the source centroid; lam = 1: the geometric rows alone"""
    c0 = p.mean(0)
    Pc = p - c0
    Vg = np.concatenate([np.cross(Pc, N), N], 1)
    cg = ((p - Q) * N).sum(1)
    A = lam * (Vg.T @ Vg)
    r = lam * (Vg.T @ cg)
    if lam < 1:
        Vc = np.concatenate([np.cross(Pc, G), G], 1)
        cc = ((p - Q) * G).sum(1) + dI
        A = A + (1 - lam) * (Vc.T @ Vc)
        r = r + (1 - lam) * (Vc.T @ cc)
    return A, r, c0


def rcond6(A):
    w = np.linalg.eigvalsh(A)
    return float(w[0] / w[-1])


def geometric_rcond(d):
    """smallest / largest eigenvalue of the geometric-only normal matrix of the pair at the identity, exact neighbours"""
    from scipy.spatial import cKDTree
    src, tgt, tn = (d[k].astype(np.float64) for k in ("src", "tgt", "tgt_n"))
    _, j = cKDTree(tgt).query(src)
    A, _, _ = _system(src, tgt[j], tn[j], None, None, 1.0)
    return rcond6(A)


def color_icp_fp64(d, grad, lam=LAMBDA_DEFAULT, iters=30, tgt_n=None, src_i=None, tgt_i=None):
    """colored ICP in fp64 with exact nearest neighbours: both rows per pair, the 6x6 system about the source centroid, the
    increment T(c0 + t) R(a) T(-c0) composed each iteration -> (4x4, smallest rcond of the systems solved)"""
    from scipy.spatial import cKDTree
    src, tgt = d["src"].astype(np.float64), d["tgt"].astype(np.float64)
    tn = (d["tgt_n"] if tgt_n is None else tgt_n).astype(np.float64)
    Is = (d["src_i"] if src_i is None else src_i).astype(np.float64)
    It = (d["tgt_i"] if tgt_i is None else tgt_i).astype(np.float64)
    g = np.asarray(grad, np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4)
    rc = []
    for _ in range(iters):
        p = src @ T[:3, :3].T + T[:3, 3]
        _, j = tree.query(p)
        A, r, c0 = _system(p, tgt[j], tn[j], g[j], It[j] - Is, lam)
        rc.append(rcond6(A))
        x = np.linalg.solve(A, -r)
        Rm = TR._rodrigues(x[:3])
        inc = np.eye(4)
        inc[:3, :3] = Rm
        inc[:3, 3] = c0 + x[3:] - Rm @ c0
        T = inc @ T
    return T, min(rc)


def rgb_pack(intensity):
    """an intensity in [0, 1] as a grey 0x00RRGGBB word (r = g = b = round(255 I)): what a PCD `rgb` field carries -> uint32"""
    v = np.clip(np.rint(np.asarray(intensity, np.float64) * 255.0), 0, 255).astype(np.uint32)
    return (v << np.uint32(16)) | (v << np.uint32(8)) | v


def rgb_intensity(words):
    """symmicp_pcd_read_intensity's rule: (float)(r + g + b) / 765.0f"""
    w = np.asarray(words, np.uint32)
    s = ((w >> np.uint32(16)) & np.uint32(255)) + ((w >> np.uint32(8)) & np.uint32(255)) + (w & np.uint32(255))
    return s.astype(f32) / f32(765.0)
