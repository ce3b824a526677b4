"""Registration evaluation (include/symmicp.h, symmicp_evaluation) restated in numpy.

For a source, a target, a row-major 4x4 X and max_dist:
  moved point   y_i = the three top rows of X on source row i with w = 1: ((m0 x + m1 y) + m2 z) + m3 in fp32, unfused
  neighbour     nn(i) = the target row j that minimises (d2(i, j), j), d2 = (dx dx + dy dy) + dz dz in fp32: brute force in chunks,
                ties to the lowest row (argmin's first hit)
  inlier        r2 = max_dist * max_dist in fp32; row i is an inlier iff max_dist <= 0 or d2_i <= r2
  per point     nn_out / d2_out: nn(i) and d2_i for an inlier, -1 and +Inf otherwise
  sums          over the inliers, by math.fsum (correctly rounded): inliers, sum d2, sum q, the upper triangle of sum q q^T with q the
                caller's target point widened to fp64; next to each the sum of the terms' magnitudes, the scale of a tolerance
  information   the 6x6 matrix by its closed form (information_from_sums) and by summing explicit G^T G (information_explicit)"""
import math

import numpy as np

f32 = np.float32


def move(X, src):
    """xf_row of device_common.h on every row of src with w = 1, in fp32 and unfused; X's bottom row is ignored"""
    m = np.asarray(X, f32).reshape(4, 4)
    v = np.asarray(src, f32)
    out = np.empty_like(v)
    for r in range(3):
        out[:, r] = ((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3]
    return out


def nearest(y, tgt, chunk=None):
    """per row of y the target row that minimises (d2, row): fp32 brute force in chunks -> (rows int64 [n], d2 fp32 [n])"""
    y, tgt = np.asarray(y, f32), np.asarray(tgt, f32)
    if chunk is None:
        chunk = max(1, (1 << 22) // max(1, len(tgt)))
    rows = np.empty(len(y), np.int64)
    d2o = np.empty(len(y), f32)
    for a in range(0, len(y), chunk):
        yy = y[a:a + chunk]
        dx = yy[:, None, 0] - tgt[None, :, 0]
        dy = yy[:, None, 1] - tgt[None, :, 1]
        dz = yy[:, None, 2] - tgt[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        k = np.argmin(d2, axis=1)
        rows[a:a + chunk] = k
        d2o[a:a + chunk] = d2[np.arange(len(yy)), k]
    return rows, d2o


def inlier_mask(d2, max_dist):
    m = f32(max_dist)
    if not m > 0:
        return np.ones(len(d2), bool)
    return np.asarray(d2, f32) <= f32(m * m)


def information_from_sums(n, sum_q, sum_qq):
    """the closed form: rotation block tr(S) I - S, rotation-translation block [s]x, its transpose, translation block n I"""
    sx, sy, sz = (float(v) for v in sum_q)
    xx, xy, xz, yy, yz, zz = (float(v) for v in sum_qq)
    nd = float(n)
    return np.array([
        [yy + zz, -xy, -xz, 0.0, -sz, sy],
        [-xy, xx + zz, -yz, sz, 0.0, -sx],
        [-xz, -yz, xx + yy, -sy, sx, 0.0],
        [0.0, sz, -sy, nd, 0.0, 0.0],
        [-sz, 0.0, sx, 0.0, nd, 0.0],
        [sy, -sx, 0.0, 0.0, 0.0, nd]], np.float64)


def G_rows(q):
    """the three rows of G for q = (x, y, z): Open3D's GetInformationMatrixFromPointClouds"""
    x, y, z = (float(v) for v in q)
    return np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]], np.float64)


def information_explicit(q):
    """sum G^T G over the rows of q [n, 3], every entry by math.fsum of its per-point terms"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    terms = np.zeros((len(q), 6, 6))
    for i, p in enumerate(q):
        G = G_rows(p)
        terms[i] = G.T @ G
    out = np.zeros((6, 6))
    for a in range(6):
        for b in range(6):
            out[a, b] = math.fsum(terms[:, a, b])
    return out


def evaluate(src, tgt, X=None, max_dist=0.0, neighbours=None):
    """-> dict(nn int64 [ns], d2 fp32 [ns], inliers, fitness, rmse, mean_d2, sum_d2, sum_q [3], sum_qq [6], information [6, 6],
    mag = dict(sum_d2, sum_q [3], sum_qq [6]): the sums of the terms' magnitudes, nn_all / d2_all: the neighbour of every row).
    neighbours: (nn_all, d2_all) of an earlier call with the same clouds and X (the search does not depend on max_dist)"""
    src, tgt = np.asarray(src, f32), np.asarray(tgt, f32)
    X = np.eye(4, dtype=f32) if X is None else np.asarray(X, f32).reshape(4, 4)
    rows, d2 = nearest(move(X, src), tgt) if neighbours is None else neighbours
    keep = inlier_mask(d2, max_dist)
    q = tgt[rows[keep]].astype(np.float64)
    dd = d2[keep].astype(np.float64)
    n = int(keep.sum())
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    sum_d2 = math.fsum(dd)
    sum_q = np.array([math.fsum(q[:, a]) for a in range(3)])
    sum_qq = np.array([math.fsum(q[:, a] * q[:, b]) for a, b in pairs])
    mag = dict(sum_d2=math.fsum(np.abs(dd)), sum_q=np.array([math.fsum(np.abs(q[:, a])) for a in range(3)]),
               sum_qq=np.array([math.fsum(np.abs(q[:, a] * q[:, b])) for a, b in pairs]))
    return dict(nn=np.where(keep, rows, -1), d2=np.where(keep, d2, f32(np.inf)).astype(f32), inliers=n, fitness=n / len(src),
                rmse=math.sqrt(sum_d2 / n) if n else 0.0, mean_d2=sum_d2 / n if n else 0.0, sum_d2=sum_d2, sum_q=sum_q, sum_qq=sum_qq,
                information=information_from_sums(n, sum_q, sum_qq), mag=mag, nn_all=rows, d2_all=d2, q=q)


def random_rigid(rng, angle_deg=20.0, shift=0.3):
    """a rigid 4x4 (float32): a rotation of up to angle_deg about a random axis and a translation of up to shift per axis"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = math.radians(angle_deg) * rng.uniform(-1, 1)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    X = np.eye(4)
    X[:3, :3] = Rm
    X[:3, 3] = rng.uniform(-shift, shift, 3)
    return X.astype(f32)
