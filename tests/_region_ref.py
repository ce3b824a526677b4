"""Plain numpy reference for region-growing segmentation (symmicp_ctx_region_growing; include/symmicp.h defines the result).

Brute force over _fpfh_ref.radius_sets (the exact fp32 neighbourhoods N(i) as CSR lists with their d2), the dot product of the normals in
np.float32 in the header's association (numpy's float32 ufuncs round every operation and fuse nothing), a SEQUENTIAL union-find of its
own over the smooth seed-seed edges, then the key minimum of the border rule, the numbering and the size filter exactly as the header
states them.  It shares no code with the device and none with _cluster_ref's union.

cos_of()         the one conversion from degrees: symmicp.region_cos restated (np.float32(np.cos(np.deg2rad(np.float64(deg))))).
region_growing() -> dict(labels, regions, sizes, seed, smooth, root) as symmicp.region_growing(..., return_info=True), plus root [n]: the
                    representative (lowest seed row) of every row's region BEFORE the size filter, -1 for unlabelled.
corner(m, h)     three faces of a lattice cube of spacing h at the origin with analytic normals, every shared edge given to one face:
                 z = 0 with m x m points, y = 0 with m x (m - 1), x = 0 with (m - 1) x (m - 1) -> (xyz, nrm, face [n]: 0, 1, 2)
chain(n, step)   n points one unit apart along x whose normals turn by step[k] degrees about x from link to link -> (xyz, nrm)
"""
import numpy as np

import _fpfh_ref as R

F = np.float32


def cos_of(deg):
    return np.float32(np.cos(np.deg2rad(np.float64(deg))))


def smooth_dot(a, b):
    """|n_a . n_b| in fp32: fabsf((ax*bx + ay*by) + az*bz), rows of a against rows of b"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return np.abs((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def _root(up, x):
    """the root of x in the forest `up` (a list), every node on the path re-hung under it"""
    r = x
    while up[r] != r:
        r = up[r]
    while up[x] != r:
        up[x], x = r, up[x]
    return r


def region_growing(xyz, nrm, eps, smoothness_cos, curv=None, curvature_threshold=0.05, min_region_size=0, max_region_size=0):
    xyz, nrm = np.ascontiguousarray(xyz, F), np.ascontiguousarray(nrm, F)
    n = len(xyz)
    cs = F(smoothness_cos)
    count, offs, rows, d2 = R.radius_sets(xyz, eps)
    src = np.repeat(np.arange(n), count)
    ok = smooth_dot(nrm[src], nrm[rows]) >= cs                                   # per listed pair (i, j): smooth(i, j)
    smooth = np.bincount(src[ok], minlength=n).astype(np.int32)
    seed = np.ones(n, bool) if curv is None else (np.asarray(curv, F) <= F(curvature_threshold))
    up = list(range(n))
    edge = ok & seed[src] & seed[rows] & (src < rows)
    for a, b in zip(src[edge].tolist(), rows[edge].tolist()):
        ra, rb = _root(up, a), _root(up, b)
        if ra < rb:
            up[rb] = ra                                                           # the lowest row of a component ends as its root
        elif rb < ra:
            up[ra] = rb
    root = np.full(n, -1, np.int64)
    for i in np.nonzero(seed)[0].tolist():
        root[i] = _root(up, i)
    bits = d2.view(np.uint32).astype(np.uint64)
    for i in np.nonzero(~seed)[0].tolist():
        s = slice(offs[i], offs[i + 1])
        use = ok[s] & seed[rows[s]]
        if use.any():
            key = (bits[s][use] << np.uint64(32)) | root[rows[s][use]].astype(np.uint64)
            root[i] = int(key.min() & np.uint64(0xFFFFFFFF))
    reps = np.nonzero((root == np.arange(n)) & seed)[0]                           # ascending
    label_of = np.full(n, -1, np.int64)
    label_of[reps] = np.arange(len(reps))
    labels = np.where(root >= 0, label_of[np.maximum(root, 0)], -1)
    sizes = np.bincount(labels[labels >= 0], minlength=len(reps))
    keep = np.ones(len(reps), bool)
    if min_region_size > 0:
        keep &= sizes >= min_region_size
    if max_region_size > 0:
        keep &= sizes <= max_region_size
    renum = np.append(np.where(keep, np.cumsum(keep) - 1, -1), -1)               # (the last slot: unlabelled)
    return dict(labels=renum[labels].astype(np.int32), regions=int(keep.sum()), sizes=sizes[keep].astype(np.int32), seed=seed, smooth=smooth,
                root=root)


def partition(labels):
    labels = np.asarray(labels)
    return frozenset(frozenset(np.nonzero(labels == k)[0].tolist()) for k in np.unique(labels[labels >= 0]).tolist())


def numbering_is_by_lowest_seed_row(labels, seed):
    """region k's lowest seed row ascends with k, and every label 0 .. max is used"""
    labels, seed = np.asarray(labels), np.asarray(seed, bool)
    r = int(labels.max()) + 1 if len(labels) else 0
    reps = [int(np.nonzero((labels == k) & seed)[0].min()) for k in range(r)]      # (raises on a region without a seed row)
    return reps == sorted(reps)


def corner(m, h):
    g = np.arange(m, dtype=np.float64) * h
    a, b = np.meshgrid(g, g, indexing="ij")
    z0 = np.stack([a.ravel(), b.ravel(), np.zeros(m * m)], 1)                      # x, y in 0 .. m-1
    a, b = np.meshgrid(g, g[1:], indexing="ij")
    y0 = np.stack([a.ravel(), np.zeros(a.size), b.ravel()], 1)                     # x in 0 .. m-1, z in 1 .. m-1
    a, b = np.meshgrid(g[1:], g[1:], indexing="ij")
    x0 = np.stack([np.zeros(a.size), a.ravel(), b.ravel()], 1)                     # y, z in 1 .. m-1
    xyz = np.concatenate([z0, y0, x0]).astype(F)
    face = np.concatenate([np.full(len(z0), 0), np.full(len(y0), 1), np.full(len(x0), 2)])
    nrm = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], F)[face]
    return np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), face


def chain(n, step_deg):
    """step_deg: a number, or [n - 1] degrees from link to link; the normals are (0, cos a, sin a) of the running angle a"""
    step = np.broadcast_to(np.asarray(step_deg, np.float64), (n - 1,))
    ang = np.deg2rad(np.concatenate([[0.0], np.cumsum(step)]))
    xyz = np.zeros((n, 3), F)
    xyz[:, 0] = np.arange(n)
    nrm = np.stack([np.zeros(n), np.cos(ang), np.sin(ang)], 1).astype(F)
    return xyz, np.ascontiguousarray(nrm)


def interleaved(n):
    """n coincident points whose normals alternate between two orthogonal directions -> (xyz, nrm)"""
    xyz = np.tile(np.array([[1.0, 2.0, 3.0]], F), (n, 1))
    nrm = np.zeros((n, 3), F)
    nrm[0::2, 2] = 1
    nrm[1::2, 0] = 1
    return xyz, nrm


def lattice(m):
    """an m x m unit lattice in z = 0 with the normal +z -> (xyz, nrm)"""
    g = np.arange(m, dtype=F)
    xyz = np.zeros((m * m, 3), F)
    xyz[:, :2] = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    nrm = np.zeros((m * m, 3), F)
    nrm[:, 2] = 1
    return xyz, nrm


def edge_curvature(xyz, h):
    """a caller-made curvature for corner(): 0.1 on the rows within h / 2 of two of the coordinate planes (the cube's edges), 0 elsewhere"""
    on = (np.abs(np.asarray(xyz, np.float64)) < 0.5 * h).sum(1) >= 2
    return np.where(on, F(0.1), F(0.0)).astype(F)


def border_case(moved):
    """corner(12, 2^-4) with every row a seed but ONE, the row at (0, 0, 5 h) on the edge x = y = 0: it is a non-seed (curvature 1) and
    has the normal (1, 1, 0) / sqrt 2, 45 degrees from the faces y = 0 and x = 0 and 90 from z = 0.  At eps 1.5 h and 50 degrees it has
    smooth seed neighbours in both faces, and the nearest of each -- (h, 0, 5 h) of y = 0 and (0, h, 5 h) of x = 0 -- are at the bit-equal
    d2 = h * h (h is a power of two): it goes to the LOWER representative, which is the face y = 0 in this row order and the face x = 0
    when the rows are reversed.  `moved`: the row stands one lattice step along y instead, on the seed (0, h, 5 h) of the face x = 0
    (d2 = 0 against 2 h * h to the nearest seed of y = 0): it goes to the nearer seed, in either row order.
    -> (xyz, nrm, curv, face, the row)"""
    h = 2.0 ** -4
    xyz, nrm, face = corner(12, h)
    row = int(np.nonzero((xyz == np.array([0, 0, 5 * h], F)).all(1))[0][0])
    assert face[row] == 1
    if moved:
        xyz[row] = [0, h, 5 * h]
    nrm[row] = (np.array([1, 1, 0], np.float64) / np.sqrt(2.0)).astype(F)
    curv = np.zeros(len(xyz), F)
    curv[row] = 1
    return xyz, nrm, curv, face, row
