"""Plain numpy reference for the RANSAC plane segmentation (symmicp_ctx_segment_plane; include/symmicp.h defines the result).

The device part in fp32 exactly as the header writes it -- elementwise products and ordered adds on float32 arrays, no `@`, no fused
operation: the pivot, the draws of (seed, stream 2), the status of every hypothesis, (n, d) and the inlier counts.  The host part in fp64:
sequential sums (numpy's cumulative sum adds in row order; its plain sum does not), the cyclic Jacobi of eig3.h restated on Python
floats, the recomputed inlier set, the orientation rule and the plane in the caller's coordinates.

hypotheses()      -> dict(pivot, p, draws, status, hyp): what symmicp_ctx_plane_hypotheses returns, and the fp32 cloud about the pivot
segment()         -> dict as symmicp.segment_plane(..., return_info=True); status 0, or 8 (NO_CONSENSUS) with plane = 0 and no rows
segment_planes()  -> (planes, labels) as symmicp.segment_planes
floor_scene(), floor_wall_scene()   the scenes of the tests: three objects standing on a noisy floor, and the same next to a wall
"""
import math

import numpy as np

import _cluster_ref as CR
from symmicp import synth

EVALUATED, REPEATED, DEGENERATE, OFF_AXIS = 0, 1, 2, 3
OK, NO_CONSENSUS = 0, 8

K_CHUNK = 512       # kPlaneChunk of symmicp_internal.h: points a workgroup of the scoring kernel stages at a time
K_BATCH = 512       # ... and the evaluated hypotheses it owns: 256 lanes x kPlaneLaneHyps

f32 = np.float32


def seq_sum(a):
    """the sum over axis 0 in ascending row order, fp64 (np.sum adds pairwise)"""
    a = np.asarray(a, np.float64)
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:])


def dot(a, b):
    """(a0 b0 + a1 b1) + a2 b2 over the last axis, in the arrays' own precision"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pivot(xyz):
    x = np.ascontiguousarray(xyz, f32)
    return (seq_sum(x) / float(len(x))).astype(f32)


def draws(n, H, seed):
    u = synth.splitmix64(seed, 3 * H, stream=2)
    return (((u >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64).reshape(H, 3)


def axis_terms(axis, max_angle_deg):
    """-> (a^ [3] f32, cos_min f32), or (None, None) without an axis"""
    if axis is None or not np.any(np.asarray(axis, f32) != 0):
        return None, None
    a = np.asarray(axis, f32).astype(np.float64)
    length = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    return (a / length).astype(f32), f32(math.cos(float(f32(max_angle_deg)) * math.pi / 180.0))


def hypotheses(xyz, H, seed=0, axis=None, max_angle_deg=0.0):
    x = np.ascontiguousarray(xyz, f32)
    c = pivot(x)
    p = x - c                                                      # fp32
    d3 = draws(len(x), H, seed)
    a, b, cc = p[d3[:, 0]], p[d3[:, 1]], p[d3[:, 2]]
    ahat, cos_min = axis_terms(axis, max_angle_deg)
    with np.errstate(all="ignore"):
        u, v = b - a, cc - a
        w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        prod = dot(u, u) * dot(v, v)
        ww = dot(w, w)
        lw = np.sqrt(ww)
        n = w / lw[:, None]
        d = -dot(n, a)
        repeated = (d3[:, 0] == d3[:, 1]) | (d3[:, 1] == d3[:, 2]) | (d3[:, 0] == d3[:, 2])
        degenerate = ~(prod > 0) | (ww < f32(1e-4) * prod)
        off = np.zeros(H, bool) if ahat is None else np.abs(dot(n, ahat[None, :])) < cos_min
    status = np.where(repeated, REPEATED, np.where(degenerate, DEGENERATE, np.where(off, OFF_AXIS, EVALUATED))).astype(np.uint8)
    hyp = np.concatenate([n, d[:, None]], 1).astype(f32)
    hyp[(status == REPEATED) | (status == DEGENERATE)] = 0
    assert hyp.dtype == f32 and p.dtype == f32
    return dict(pivot=c, p=p, draws=d3, status=status, hyp=hyp)


def offsets32(p, nd):
    """fp32 signed offsets of the rows of p from the plane nd"""
    return ((nd[0] * p[:, 0] + nd[1] * p[:, 1]) + nd[2] * p[:, 2]) + nd[3]


def score(p, hyp, status, max_dist):
    md = f32(max_dist)
    inl = np.zeros(len(hyp), np.int32)
    for h in np.nonzero(status == EVALUATED)[0].tolist():
        inl[h] = int(np.count_nonzero(np.abs(offsets32(p, hyp[h])) <= md))
    return inl


def winner(status, inl):
    """-> the evaluated hypothesis with the most inliers, the lowest h among equal ones; -1 when none is evaluated"""
    ev = np.nonzero(status == EVALUATED)[0]
    if len(ev) == 0:
        return -1
    return int(ev[np.argmax(inl[ev])])                             # (argmax returns the first maximum)


def jacobi3(A):
    """eig3.h's jacobi3<true> on Python floats -> (A diagonalised, V: column j the eigenvector of A[j][j])"""
    A = [[float(A[r][c]) for c in range(3)] for r in range(3)]
    V = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    for _ in range(12):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        if off < 1e-300:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if abs(apq) < 1e-300:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                kp, kq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * kp - s * kq, s * kp + c * kq
            for k in range(3):
                pk, qk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * pk - s * qk, s * pk + c * qk
            for k in range(3):
                kp, kq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * kp - s * kq, s * kp + c * kq
    return A, V


def refit(x64, mask, max_dist):
    """one refit over the rows of mask (x64 = the cloud about the pivot in fp64) -> (nd [4] f64, the recomputed mask)"""
    e = x64[mask]
    k = float(len(e))
    m = seq_sum(e) / k
    e = e - m
    S = seq_sum(np.stack([e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2], e[:, 2] * e[:, 2]], 1))
    A, V = jacobi3([[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]])
    j = 0
    if A[1][1] < A[j][j]:
        j = 1
    if A[2][2] < A[j][j]:
        j = 2
    v = np.array([V[0][j], V[1][j], V[2][j]])
    n = v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    nd = np.array([n[0], n[1], n[2], -((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2])])
    return nd, np.abs(offsets64(x64, nd)) <= float(f32(max_dist))


def offsets64(x64, nd):
    return ((nd[0] * x64[:, 0] + nd[1] * x64[:, 1]) + nd[2] * x64[:, 2]) + nd[3]


def segment(xyz, max_dist, hypotheses_=1000, seed=0, refits=1, min_inliers=3, axis=None, max_angle_deg=0.0):
    x = np.ascontiguousarray(xyz, f32)
    n = len(x)
    hy = hypotheses(x, hypotheses_, seed, axis, max_angle_deg)
    status, hyp, p, c = hy["status"], hy["hyp"], hy["p"], hy["pivot"]
    inl = score(p, hyp, status, max_dist)
    need = max(3, int(min_inliers))
    hb = winner(status, inl)
    r = dict(status=NO_CONSENSUS, plane=np.zeros(4), plane32=np.zeros(4, f32), rows=np.zeros(0, np.int32), count=0, best_hypothesis=hb,
             evaluated=int(np.count_nonzero(status == EVALUATED)), inliers_ransac=int(inl[hb]) if hb >= 0 else 0, inliers_final=0, rmse_final=0.0,
             distance=None, hyp_status=status, hyp_inliers=inl, hyp=hyp, pivot=c)
    if hb < 0 or inl[hb] < need:
        return r
    mask = np.abs(offsets32(p, hyp[hb])) <= f32(max_dist)
    nd = hyp[hb].astype(np.float64)
    x64 = x.astype(np.float64) - c.astype(np.float64)
    for _ in range(int(refits)):
        nd, mask = refit(x64, mask, max_dist)
        if np.count_nonzero(mask) < need:
            return r
    ahat, _ = axis_terms(axis, max_angle_deg)
    if ahat is not None:
        a = ahat.astype(np.float64)
        flip = (nd[0] * a[0] + nd[1] * a[1]) + nd[2] * a[2] < 0
    else:
        j = 0
        if abs(nd[1]) > abs(nd[j]):
            j = 1
        if abs(nd[2]) > abs(nd[j]):
            j = 2
        flip = nd[j] < 0
    if flip:
        nd = -nd
    dist = offsets64(x64, nd)
    c64 = c.astype(np.float64)
    plane = np.array([nd[0], nd[1], nd[2], nd[3] - ((nd[0] * c64[0] + nd[1] * c64[1]) + nd[2] * c64[2])])
    k = int(np.count_nonzero(mask))
    sse = seq_sum(dist[mask] * dist[mask])
    r.update(status=OK, plane=plane, plane32=plane.astype(f32), rows=np.nonzero(mask)[0].astype(np.int32), count=k, inliers_final=k,
             rmse_final=math.sqrt(float(sse) / k), distance=dist)
    return r


def segment_planes(xyz, max_dist, max_planes, min_inliers, hypotheses_=1000, seed=0, refits=1, axis=None, max_angle_deg=0.0):
    x = np.ascontiguousarray(xyz, f32)
    labels = np.full(len(x), -1, np.int32)
    planes = []
    for k in range(max_planes):
        left = np.nonzero(labels < 0)[0]
        if len(left) < max(3, min_inliers):
            break
        r = segment(np.ascontiguousarray(x[left]), max_dist, hypotheses_, seed + k, refits, min_inliers, axis, max_angle_deg)
        if r["status"] != OK:
            break
        labels[left[r["rows"]]] = k
        planes.append(r["plane"])
    return np.array(planes, np.float64).reshape(-1, 4), labels


def margin(r, max_dist):
    """how close the nearest row comes to the fp64 threshold of the final plane, as a fraction of max_dist"""
    md = float(f32(max_dist))
    return float(np.min(np.abs(np.abs(r["distance"]) - md))) / md


def angle_deg(n, truth):
    n, t = np.asarray(n, np.float64), np.asarray(truth, np.float64)
    cs = abs(float(n @ t)) / (np.linalg.norm(n) * np.linalg.norm(t))
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(n, t)) / (np.linalg.norm(n) * np.linalg.norm(t)), cs)))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
SP = CR.CAT_SPACING
FLOOR, WALL = 3, 4          # `kind` of a row: 0, 1, 2 the object of _cluster_ref.three_objects it belongs to
SCENE_R = synth.rotation(20, (1, 0.3, 0.1))
SCENE_T = np.array([100.0, -50.0, 25.0])
SCENE_UP = SCENE_R @ np.array([0.0, 0.0, 1.0])          # the floor's normal in the scene
SCENE_WALL_NORMAL = SCENE_R @ np.array([1.0, 0.0, 0.0])


def _scene(cat_xyz, wall):
    obj, owner = CR.three_objects(cat_xyz)
    obj = obj.astype(np.float64)
    lo, hi = obj.min(axis=0), obj.max(axis=0)
    s = 2 * SP
    gx, gy = np.meshgrid(np.arange(lo[0] - 4 * SP, hi[0] + 4 * SP, s), np.arange(lo[1] - 4 * SP, hi[1] + 4 * SP, s), indexing="ij")
    floor = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, lo[2])], 1)
    floor[:, 2] += (synth.uniform01(17, len(floor)) - 0.5) * 0.6 * SP
    parts, kinds = [obj, floor], [owner, np.full(len(floor), FLOOR)]
    if wall:
        s = 1.5 * SP
        gy, gz = np.meshgrid(np.arange(lo[1] - 4 * SP, hi[1] + 4 * SP, s), np.arange(lo[2], lo[2] + 60.0, s), indexing="ij")
        w = np.stack([np.full(gy.size, lo[0] - 4 * SP), gy.ravel(), gz.ravel()], 1)
        w[:, 0] += (synth.uniform01(18, len(w)) - 0.5) * 0.6 * SP
        parts.append(w)
        kinds.append(np.full(len(w), WALL))
    x = (np.concatenate(parts) @ SCENE_R.T + SCENE_T).astype(f32)
    kind = np.concatenate(kinds)
    perm = np.random.default_rng(5).permutation(len(x))
    return np.ascontiguousarray(x[perm]), kind[perm]


def floor_scene(cat_xyz):
    """three_objects standing on a sparse noisy floor, turned, moved and shuffled -> (xyz [11 492, 3] f32, kind [11 492]); 5 542 rows are floor"""
    return _scene(cat_xyz, False)


def floor_wall_scene(cat_xyz):
    """the floor scene next to a wall -> (xyz [17 785, 3] f32, kind); 6 293 rows are wall"""
    return _scene(cat_xyz, True)


MAX_DIST = 0.5 * SP         # the scenes' max_dist
