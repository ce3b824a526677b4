"""Plain numpy references for the k-NN PCA normals (k_normals_knn, symmicp_ctx_knn).

knn()      the exact k-NN set of every point in its own cloud: the fp32 distance in the kernel's association
           (dx*dx + dy*dy) + dz*dz, ordered by (d2, row).  Chunked brute force up to BRUTE_MAX points; above it a
           cKDTree proposes k+8 candidates that are re-ranked in fp32, and a row whose (k+8)-th candidate is not clearly
           beyond its k-th neighbour goes back to brute force.
moments()  each point's fp64 mean and covariance over its set, summed in the set's order (the kernel's and the oracle's).
eig()      numpy eigh of those covariances: eigenvalues ascending, eigenvectors in columns.
emulate()  the kernel's arithmetic after the walk, step by step in fp64 (cyclic Jacobi with a sweep cap, flip, curvature).
           With sweeps=12 it is the device's rule, with sweeps=64 the oracle's (orc_normals_knn).
"""
import numpy as np

BRUTE_MAX = 8192


def _keys(d2, cols):
    # (d2, row) lexicographic as one int64: the bits of a non-negative fp32 are monotone in its value
    return (d2.view(np.uint32).astype(np.int64) << 32) | cols.astype(np.int64)


def _d2(q, p):
    """fp32 (dx*dx + dy*dy) + dz*dz of every query in q [m,3] against every point in p [n,3] -> [m,n]"""
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _brute(xyz, k, qi):
    n = xyz.shape[0]
    rows = np.empty((len(qi), k), np.int32)
    d2 = np.empty((len(qi), k), np.float32)
    m = max(1, (1 << 22) // n)
    cols = np.arange(n, dtype=np.int64)[None, :]
    for a in range(0, len(qi), m):
        key = _keys(_d2(xyz[qi[a:a + m]], xyz), cols)
        key = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
        rows[a:a + m] = (key & 0xFFFFFFFF).astype(np.int32)
        d2[a:a + m] = (key >> 32).astype(np.uint32).view(np.float32)
    return rows, d2


def knn(xyz, k, queries=None):
    """-> (rows [m,k] int32, d2 [m,k] f32) of the points `queries` (default: all), ascending (d2, row)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    qi = np.arange(n) if queries is None else np.asarray(queries)
    if n <= BRUTE_MAX:
        return _brute(xyz, k, qi)
    from scipy.spatial import cKDTree
    c = min(k + 8, n)
    x64 = xyz.astype(np.float64)
    dd, ii = cKDTree(x64).query(x64[qi], c)
    q = xyz[qi]
    dx = q[:, None, 0] - xyz[ii, 0]
    dy = q[:, None, 1] - xyz[ii, 1]
    dz = q[:, None, 2] - xyz[ii, 2]
    key = np.sort(_keys((dx * dx + dy * dy) + dz * dz, ii), axis=1)[:, :k]
    rows = (key & 0xFFFFFFFF).astype(np.int32)
    d2 = (key >> 32).astype(np.uint32).view(np.float32)
    # every point off the candidate list is at least as far as the last candidate (exact distance); the fp32 d2 is within a few
    # ulps of the exact square, so with this margin none of them can reach or tie the k-th
    bad = ~(dd[:, -1] ** 2 > d2[:, -1].astype(np.float64) * (1 + 1e-5)) if c < n else np.zeros(len(qi), bool)
    if bad.any():
        rows[bad], d2[bad] = _brute(xyz, k, qi[bad])
    return rows, d2


def moments(xyz, rows):
    """-> (mean [m,3], cov [m,3,3]) fp64 over each set, accumulated in the set's order as the kernel does"""
    pts = np.ascontiguousarray(xyz, np.float32)[rows].astype(np.float64)       # [m,k,3]
    k = rows.shape[1]
    mu = np.zeros((rows.shape[0], 3))
    for j in range(k):
        mu += pts[:, j]
    mu /= k
    C = np.zeros((rows.shape[0], 3, 3))
    for j in range(k):
        d = pts[:, j] - mu
        for r in range(3):
            for c in range(r, 3):
                C[:, r, c] += d[:, r] * d[:, c]
    C /= k
    for r in range(3):
        for c in range(r):
            C[:, r, c] = C[:, c, r]
    return mu, C


def eig(C):
    """-> (lam [m,3] ascending, vec [m,3,3] eigenvectors in columns)"""
    return np.linalg.eigh(C)


def emulate(xyz, rows, viewpoint=(0.0, 0.0, 0.0), sweeps=12, centres=None):
    """the kernel's normal and curvature of each set, rounded exactly as k_normals_knn rounds them -> (nrm [m,3] f32, curv [m] f32).
    `centres`: the rows of the query points when `rows` holds the sets of a subset (default: every point, in order)."""
    _, C = moments(xyz, rows)
    A = [[C[:, r, c].copy() for c in range(3)] for r in range(3)]
    m = rows.shape[0]
    one, zero = np.ones(m), np.zeros(m)
    V = [[one.copy() if r == c else zero.copy() for c in range(3)] for r in range(3)]
    live = np.ones(m, bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2]
            live &= ~(off < 1e-300)
            if not live.any():
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[p][q]
                rot = live & ~(np.abs(apq) < 1e-300)
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for M, cols in ((A, True), (A, False), (V, True)):
                    for kk in range(3):
                        if cols:
                            a, b = M[kk][p], M[kk][q]
                            M[kk][p], M[kk][q] = np.where(rot, c * a - s * b, a), np.where(rot, s * a + c * b, b)
                        else:
                            a, b = M[p][kk], M[q][kk]
                            M[p][kk], M[q][kk] = np.where(rot, c * a - s * b, a), np.where(rot, s * a + c * b, b)
    w0, w1, w2 = A[0][0], A[1][1], A[2][2]
    tr = (w0 + w1) + w2
    mi = np.zeros(m, int)
    lam = w0.copy()
    sel = w1 < lam
    lam[sel], mi[sel] = w1[sel], 1
    sel = w2 < lam
    lam[sel], mi[sel] = w2[sel], 2
    n = np.stack([np.choose(mi, V[r]) for r in range(3)], axis=1)
    nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    n = n / nn[:, None]
    p = np.ascontiguousarray(xyz, np.float32)[np.arange(m) if centres is None else centres].astype(np.float64)
    vp = np.asarray(viewpoint, np.float32).astype(np.float64)
    dot = ((vp[0] - p[:, 0]) * n[:, 0] + (vp[1] - p[:, 1]) * n[:, 1]) + (vp[2] - p[:, 2]) * n[:, 2]
    n[dot < 0] *= -1.0
    with np.errstate(all="ignore"):
        curv = np.where(tr > 0, np.abs(lam) / tr, 0.0).astype(np.float32)
    return n.astype(np.float32), curv
