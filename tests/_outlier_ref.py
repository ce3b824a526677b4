"""Plain numpy references for the outlier filters (symmicp_statistical_outlier_removal, symmicp_radius_outlier_removal;
include/symmicp.h defines the arithmetic).

mean_dist()    m_i of the rows asked for: the exact (k + 1)-NN set of _knn_ref.knn (fp32 d2 in the kernels' association, (d2, row)
               order) with the point's own row dropped -- or, when more than k duplicates with a lower row push it out of the set,
               the last value -- then sqrt in float64 and a SEQUENTIAL sum (np.cumsum; np.sum adds pairwise and would not match).
statistics()   PCL's formula over all m_i, in a Python loop in row order -> (mu, sd, thr).
statistical()  both, and the kept rows.
radius()       the neighbour counts of _fpfh_ref.radius_sets and the kept rows.
noisy_cat()    the cat with stray points injected away from the surface, rows shuffled.
"""
import math

import numpy as np

import _fpfh_ref as R
import _knn_ref as K

CAT_SPACING = 1.3816


def mean_dist(xyz, k, queries=None):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    assert 1 <= k <= n - 1
    qi = np.arange(n) if queries is None else np.asarray(queries)
    with np.errstate(over="ignore"):
        rows, d2 = K.knn(xyz, k + 1, qi)
    own = rows == qi[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k)
    keep = np.ones(rows.shape, bool)
    keep[np.arange(len(qi)), drop] = False
    d = d2[keep].reshape(len(qi), k)                     # still ascending
    return np.cumsum(np.sqrt(d.astype(np.float64)), axis=1)[:, -1] / float(k)


def statistics(m, std_mul):
    s1 = s2 = 0.0
    for v in np.asarray(m, np.float64).tolist():
        s1 = s1 + v
        s2 = s2 + v * v
    n = float(len(m))
    mu = s1 / n
    var = (s2 - s1 * s1 / n) / (n - 1.0)
    sd = math.sqrt(0.0 if var < 0.0 else var)            # (a NaN variance stays NaN)
    return mu, sd, mu + float(np.float32(std_mul)) * sd


def kept(m, thr):
    return np.nonzero(np.asarray(m) <= thr)[0].astype(np.int32)


def statistical(xyz, k, std_mul):
    """-> dict(rows=, mean_dist=, mu=, sd=, thr=) as symmicp.remove_statistical_outlier(..., return_stats=True)"""
    m = mean_dist(xyz, k)
    mu, sd, thr = statistics(m, std_mul)
    return dict(rows=kept(m, thr), mean_dist=m, mu=mu, sd=sd, thr=thr)


def radius(xyz, r, min_neighbors):
    """-> dict(rows=, neighbors=) as symmicp.remove_radius_outlier(..., return_counts=True)"""
    count = R.radius_sets(xyz, r)[0]
    return dict(rows=np.nonzero(count >= min_neighbors)[0].astype(np.int32), neighbors=count)


def noisy_cat(cat_xyz, seed=7, draws=60, clearance=8 * CAT_SPACING):
    """the cat plus stray points: `draws` uniform points in the bounding box grown by half its extent on every side, of which those
    farther than `clearance` from every surface point stay; the rows of the union shuffled.
    -> (xyz [n,3] f32, injected [n] bool, origin [n]: the cat row of a surface point, -1 for an injected one)"""
    from scipy.spatial import cKDTree
    cat_xyz = np.ascontiguousarray(cat_xyz, np.float32)
    rng = np.random.default_rng(seed)
    lo, hi = cat_xyz.min(axis=0).astype(np.float64), cat_xyz.max(axis=0).astype(np.float64)
    ext = hi - lo
    p = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (draws, 3)).astype(np.float32)
    far = cKDTree(cat_xyz.astype(np.float64)).query(p.astype(np.float64))[0] > clearance
    p = p[far]
    xyz = np.concatenate([cat_xyz, p])
    origin = np.concatenate([np.arange(len(cat_xyz)), np.full(len(p), -1)])
    perm = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm]), origin[perm] < 0, origin[perm]
