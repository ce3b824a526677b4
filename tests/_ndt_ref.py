"""numpy restatement of SYMMICP_MODE_NDT (include/symmicp.h, "NDT registration"; DESIGN.md 4, "NDT") with the library's arithmetic:

the map     the voxel grid of _voxel_ref, plus the 2^23 rule; per kept voxel the fp64 mean and covariance summed one member at a time in
            ascending caller row (np.add.accumulate: sequential by definition, never np.sum, which is pairwise); numpy.linalg.eigh for the
            eigen-decomposition (the device runs a cyclic Jacobi: the two agree in M = sum o l l^T to rounding, not in the vectors' bits)
the weight  symmicp_ndt_weight in fp32 ops numpy has too (np.rint, np.ldexp): bit for bit
the Gauss constants, in fp64
a pass      the items of every source point (own cell, or own cell and six face neighbours) and their terms, formed as k_pass_ndt forms
            them in fp32 and carried to fp64; record() returns (S, M, count) in the shape of _record_ref.record, for assert_record."""
import numpy as np

import _voxel_ref
from _record_ref import NSUM, f32, f32_max_d2, xf_rows

F = np.float32


class NdtError(ValueError):
    """the cases the library answers with SYMMICP_ERR_ARG"""


# ---- constants and the weight ----------------------------------------------------------------------------------------------------
def gauss(outlier_ratio=0.55):
    """symmicp_ndt_gauss in fp64 (the engine calls it with the configuration's fp32 ratio widened: gauss(float(F(ratio))))"""
    po = float(outlier_ratio)
    if not (0.0 < po < 1.0):
        raise NdtError("outlier_ratio outside (0, 1)")
    c1, c2 = 10.0 * (1.0 - po), po
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return float(d1), float(d2)


def pass_h(outlier_ratio=0.55):
    """the pass's constant h = (float)(0.5 * d2)"""
    return F(0.5 * gauss(float(F(outlier_ratio)))[1])


def weight(x):
    """symmicp_ndt_weight on an array, fp32 op for fp32 op"""
    x = np.asarray(x, F)
    live = x > F(-64.0)                                   # (NaN: False)
    with np.errstate(invalid="ignore"):
        xx = np.where(live, np.where(x > F(0), F(0), x), F(0)).astype(F)
    k = np.rint(xx * F(1.44269504))
    r = (xx - k * F(0.693359375)) - k * F(-2.12194440e-4)
    p = np.full_like(r, F(1.9875691500e-4))
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * r + F(c)
    y = (p * (r * r) + r) + F(1.0)
    out = np.ldexp(y, k.astype(np.int32)).astype(F)
    return np.where(live, out, F(0)).astype(F)


# ---- the map --------------------------------------------------------------------------------------------------------------------
def check_config(resolution, min_points=6, eig_ratio=0.01, outlier_ratio=0.55, neighbors=7):
    if not (np.isfinite(F(resolution)) and F(resolution) > 0):
        raise NdtError("resolution")
    if min_points < 3:
        raise NdtError("min_points")
    if not (F(eig_ratio) > 0 and F(eig_ratio) <= 1):
        raise NdtError("eig_ratio")
    if not (F(outlier_ratio) > 0 and F(outlier_ratio) < 1):
        raise NdtError("outlier_ratio")
    if neighbors not in (1, 7):
        raise NdtError("neighbors")


def grid(xyz, resolution):
    """-> (inv f32, lo [3] int64, dims [3] int64): _voxel_ref's grid, refused as well when a |lo| or |hi| reaches 2^23"""
    xyz = np.asarray(xyz, F)
    try:
        inv, lo, dims = _voxel_ref.grid(xyz, resolution)
    except _voxel_ref.GridError as e:
        raise NdtError(str(e))
    hi = lo + dims - 1
    if np.any(np.abs(lo) >= 2 ** 23) or np.any(np.abs(hi) >= 2 ** 23):
        raise NdtError("a cell coordinate reaches 2^23")
    return inv, lo, dims


def _seq_sum(a):
    """the rows of a [c, k] added one at a time from zero, in fp64"""
    return np.add.accumulate(np.asarray(a, np.float64), axis=0)[-1]


def build_map(xyz, resolution, min_points=6, eig_ratio=0.01):
    """-> dict(key [m] uint32, count [m] int32, mean [m,3] f32, cov [m,6] f64, M [m,3,3] f64 (the inverse covariance sum 1/lambda' v v^T),
    lam [m,3] f64 (lambda', ascending), grid [6] int32 = lo xyz, n xyz, inv f32)"""
    xyz = np.asarray(xyz, F)
    check_config(resolution, min_points, eig_ratio)
    inv, lo, dims = grid(xyz, resolution)
    cell = np.floor(xyz * inv).astype(np.int64) - lo
    k = cell[:, 0] + dims[0] * (cell[:, 1] + dims[1] * cell[:, 2])
    rows = np.argsort(k, kind="stable")
    ks = k[rows]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    first = np.flatnonzero(head)
    count = np.diff(np.append(first, len(ks)))
    er = float(F(eig_ratio))
    out = dict(key=[], count=[], mean=[], cov=[], M=[], lam=[])
    for f, c in zip(first, count):
        if c < min_points:
            continue
        mem = xyz[rows[f:f + c]].astype(np.float64)
        mu = _seq_sum(mem) / float(c)
        d = mem - mu
        prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        cv = _seq_sum(prods) / float(c - 1)
        Cm = np.array([[cv[0], cv[1], cv[2]], [cv[1], cv[3], cv[4]], [cv[2], cv[4], cv[5]]])
        lam, vec = np.linalg.eigh(Cm)
        lmax = lam[2]
        if not (np.isfinite(lmax) and lmax > 0):
            continue
        lam = np.maximum(lam, er * lmax)
        out["key"].append(ks[f]); out["count"].append(c); out["mean"].append(mu.astype(F)); out["cov"].append(cv)
        out["M"].append((vec / lam) @ vec.T); out["lam"].append(lam)
    m = len(out["key"])
    return dict(key=np.array(out["key"], np.uint32), count=np.array(out["count"], np.int32), mean=np.array(out["mean"], F).reshape(m, 3),
                cov=np.array(out["cov"], np.float64).reshape(m, 6), M=np.array(out["M"], np.float64).reshape(m, 3, 3),
                lam=np.array(out["lam"], np.float64).reshape(m, 3), grid=np.concatenate([lo, dims]).astype(np.int32), inv=inv)


def with_factors(ref):
    """a reference map with the factors the device keeps, from eigh: axes [m,3,3] f32 (axis r at [:, r]) and inv_eig [m,3] f32 -- what the
    restated loop of the CPU tests runs on (the GPU tests feed the pass the device's own factors)"""
    m = len(ref["key"])
    axes = np.zeros((m, 3, 3), F)
    inv_eig = np.zeros((m, 3), F)
    for v in range(m):
        # M = sum 1/lambda' v v^T: its own eigen-decomposition gives the factors back
        lam_inv, vec = np.linalg.eigh(ref["M"][v])
        order = np.argsort(-lam_inv, kind="stable")          # ascending lambda = descending 1 / lambda
        axes[v] = vec[:, order].T.astype(F)
        inv_eig[v] = lam_inv[order].astype(F)
    return dict(ref, axes=axes, inv_eig=inv_eig)


def M_of(axes, inv_eig):
    """sum_r o_r l_r l_r^T in fp64 from the fp32 factors -> [m,3,3]"""
    a = np.asarray(axes, np.float64)
    o = np.asarray(inv_eig, np.float64)
    return np.einsum("vr,vri,vrj->vij", o, a, a)


# ---- a pass ---------------------------------------------------------------------------------------------------------------------
_OFFS = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def items(nmap, y, neighbors):
    """the items of the moved points y [n,3] f32 -> (point [k] int64, map row [k] int64); also own-cell rows [n] (-1: no voxel)"""
    y = np.asarray(y, F)
    inv = F(nmap["inv"])
    lo = nmap["grid"][:3].astype(np.int64)
    dims = nmap["grid"][3:].astype(np.int64)
    flo, fhi = lo.astype(F), (lo + dims - 1).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.floor(y * inv).astype(F)
    keys = nmap["key"].astype(np.int64)
    pts, rws = [], []
    own = None
    for off in _OFFS[:neighbors]:
        c = (g + np.asarray(off, F)).astype(F)
        with np.errstate(invalid="ignore"):
            inb = np.all((c >= flo) & (c <= fhi), axis=1)
        ci = np.where(inb[:, None], c, flo).astype(np.int64) - lo
        k = ci[:, 0] + dims[0] * (ci[:, 1] + dims[1] * ci[:, 2])
        at = np.searchsorted(keys, k)
        hit = inb & (at < len(keys))
        hit[hit] = keys[at[hit]] == k[hit]
        row = np.where(hit, at, -1)
        if own is None:
            own = row.copy()
        sel = np.flatnonzero(hit)
        pts.append(sel); rws.append(row[sel])
    return np.concatenate(pts), np.concatenate(rws), own


def item_terms(nmap, y, pt, row, pivot, h, max_corr_dist=0.0):
    """-> (T [k,38] the items' terms, A [k,38] the sums of their parts' magnitudes, w [k] f32, d2 [k] f32, keep [k]) of the items the
    distance gate keeps; every fp32 expression as k_pass_ndt forms it"""
    pv = np.asarray(pivot, F)
    P = np.asarray(y, F)[pt] - pv
    MU = np.asarray(nmap["mean"], F)[row] - pv
    D = P - MU
    L = np.asarray(nmap["axes"], F)[row]                  # [k,3,3]
    O = np.asarray(nmap["inv_eig"], F)[row]               # [k,3]
    d2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    md2 = f32_max_d2(max_corr_dist)
    keep = ~(d2 > md2) if md2 > 0 else np.ones(len(d2), bool)
    P, MU, D, L, O, d2 = P[keep], MU[keep], D[keep], L[keep], O[keep], d2[keep]
    c = [(D[:, 0] * L[:, r, 0] + D[:, 1] * L[:, r, 1]) + D[:, 2] * L[:, r, 2] for r in range(3)]
    mm = ((O[:, 0] * c[0]) * c[0] + (O[:, 1] * c[1]) * c[1]) + (O[:, 2] * c[2]) * c[2]
    w = weight(-(F(h) * mm))
    n = len(P)
    T = np.zeros((n, 38))
    A = np.zeros((n, 38))
    w64 = w.astype(np.float64)
    for r in range(3):
        l = L[:, r]
        m0 = P[:, 1] * l[:, 2] - P[:, 2] * l[:, 1]
        m1 = P[:, 2] * l[:, 0] - P[:, 0] * l[:, 2]
        m2 = P[:, 0] * l[:, 1] - P[:, 1] * l[:, 0]
        V = np.stack([m0, m1, m2, l[:, 0], l[:, 1], l[:, 2]], 1).astype(np.float64)
        ww = w64 * O[:, r].astype(np.float64)
        cd = c[r].astype(np.float64)
        k = 0
        for a in range(6):
            for b in range(a, 6):
                t = ww * V[:, a] * V[:, b]
                T[:, k] += t; A[:, k] += np.abs(t)
                k += 1
        t = V * (ww * cd)[:, None]
        T[:, 21:27] += t; A[:, 21:27] += np.abs(t)
        t = ww * cd * cd
        T[:, 35] += t; A[:, 35] += np.abs(t)
    T[:, 27:30] = w64[:, None] * P.astype(np.float64)
    T[:, 30:33] = w64[:, None] * MU.astype(np.float64)
    T[:, 33] = np.sqrt(d2)
    T[:, 34] = w64
    T[:, 36] = d2
    T[:, 37] = 1.0
    for sl in (slice(27, 35), slice(36, 38)):
        A[:, sl] = np.abs(T[:, sl])
    return T, A, w, d2, keep


def record(nmap, X, src, pivot, neighbors=7, outlier_ratio=0.55, max_corr_dist=0.0):
    """-> (record [40], sum of |terms| [40], number of items) of the pass at the cumulative transform X over the source rows src"""
    y = xf_rows(X, src, 1.0)
    pt, row, _ = items(nmap, y, neighbors)
    T, A, _, _, keep = item_terms(nmap, y, pt, row, pivot, pass_h(outlier_ratio), max_corr_dist)
    S = np.zeros(NSUM)
    M = np.zeros(NSUM)
    S[:38] = T.sum(0)
    M[:38] = A.sum(0)
    return S, M, int(keep.sum())


def correspondences(nmap, X, src, pivot):
    """symmicp_get_correspondences of an NDT context: (own-cell map row or -1, the pass's d2 to that voxel's mean or 0) per row"""
    y = xf_rows(X, src, 1.0)
    _, _, own = items(nmap, y, 1)
    pv = np.asarray(pivot, F)
    has = own >= 0
    D = (y[has] - pv) - (np.asarray(nmap["mean"], F)[own[has]] - pv)
    d2 = np.zeros(len(y), F)
    d2[has] = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    return own.astype(np.int32), d2


# ---- the restated loop (fp64 Gauss-Newton on the record: what PLANE's solve does, without its fp32 roundings) -------------------------
def gn_increment(S, pivot):
    """the step of record S about the pivot -> 4x4 fp64: G x = -b, x = (a, t), R = the rotation by |a| about a"""
    G = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            G[a, b] = G[b, a] = S[k]
            k += 1
    x = np.linalg.solve(G, -np.asarray(S[21:27]))
    a, t = x[:3], x[3:]
    th = np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)
    pv = np.asarray(pivot, np.float64)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = pv + t - R @ pv
    return X


def loop(nmap, src, pivot, passes, neighbors=7, outlier_ratio=0.55, X0=None):
    """-> (X after `passes` steps, [(items, sum w)] of every pass run, the first included)"""
    X = np.eye(4) if X0 is None else np.asarray(X0, np.float64)
    log = []
    for _ in range(passes):
        S, _, cnt = record(nmap, X.astype(F), src, pivot, neighbors, outlier_ratio)
        log.append((cnt, S[34]))
        X = gn_increment(S, pivot) @ X
    S, _, cnt = record(nmap, X.astype(F), src, pivot, neighbors, outlier_ratio)
    log.append((cnt, S[34]))
    return X, log


def pose_error(X, truth):
    """-> (rotation error in degrees, translation error) of X against truth"""
    E = np.asarray(X, np.float64) @ np.linalg.inv(np.asarray(truth, np.float64))
    tr = (np.trace(E[:3, :3]) - 1.0) * 0.5
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, tr))))), float(np.linalg.norm(np.asarray(X)[:3, 3] - np.asarray(truth)[:3, 3]))
