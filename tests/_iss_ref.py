"""Plain numpy reference for the ISS keypoints (kernels_keypoints.hip; include/symmicp.h defines the arithmetic).

Neighbourhoods are the exact fp32 sets of tests/_fpfh_ref.radius_sets (r2 = fl32(r * r), d2 the kernels' fp32 (dx*dx + dy*dy) + dz*dz,
the row itself left out by row).  Everything after them is fp64:

saliency()   per query row: k = |N_rs(i)|, the scatter matrix of e = x_j - x_i (the fp32 differences, widened: their products are
             exact in fp64) divided by k, its eigenvalues l1 >= l2 >= l3 by numpy.linalg.eigvalsh, the salient flag
             (l2 < g21 l1, l3 < g32 l2, fl32(l3) > 0 with g = the fp32 gammas widened) and s = fl32(l3) or 0.
             It also reports the MARGIN of each ratio test, |l2 - g21 l1| / l1 and |l3 - g32 l2| / l1: a point is CLEAR when both
             exceed CLEAR_MARGIN = 1e-9.  Two correct fp64 evaluations differ by about 1e-15 l1 in an eigenvalue (the header promises
             1e-13 l1 for the device), so a clear point's flag cannot depend on which of them decided.
nms()        the non-maximum suppression as a pure function of a GIVEN fp32 saliency array (the device's own, in the GPU tests) and
             the exact neighbourhoods at rn: s_i > 0, |N_rn(i)| >= min_neighbors, no neighbour with a larger s or an equal s and a
             lower row.
keypoints()  both stages.

Every function evaluates a subset of query rows, so that large clouds can be checked on a few thousand rows.
"""
import numpy as np

import _fpfh_ref as R

CLEAR_MARGIN = 1e-9


def scatter(xyz, queries, offs, rows):
    """-> (C [m,3,3] f64, k [m] int64): the scatter matrices S / k of the CSR lists (zeros where k == 0)"""
    x32 = np.ascontiguousarray(xyz, np.float32)
    q = np.asarray(queries)
    m = len(offs) - 1
    seg = np.repeat(np.arange(m), np.diff(offs))
    e = (x32[rows] - x32[q[seg]]).astype(np.float64)          # fp32 differences, widened
    S = np.zeros((m, 3, 3))
    np.add.at(S, seg, e[:, :, None] * e[:, None, :])
    k = np.diff(offs).astype(np.int64)
    with np.errstate(all="ignore"):
        C = np.where(k[:, None, None] > 0, S / np.maximum(k, 1)[:, None, None], 0.0)
    return C, k


def saliency(xyz, rs, gamma21=0.975, gamma32=0.975, min_neighbors=5, queries=None, brute=None):
    """-> dict(k [m] int64, lam [m,3] f64 descending, salient [m] bool, s [m] f32, margin21, margin32 [m] f64, clear [m] bool) of the
    rows `queries` (default: all).  Rows with k < min_neighbors are not salient and clear (an integer decides)."""
    q = np.arange(len(xyz)) if queries is None else np.asarray(queries)
    count, offs, rows, _ = R.radius_sets(xyz, rs, q, brute=brute)
    C, k = scatter(xyz, q, offs, rows)
    lam = np.linalg.eigvalsh(C)[:, ::-1]
    l1, l2, l3 = lam[:, 0], lam[:, 1], lam[:, 2]
    g21, g32 = float(np.float32(gamma21)), float(np.float32(gamma32))
    enough = k >= int(min_neighbors)
    with np.errstate(all="ignore"):
        l3f = l3.astype(np.float32)
        salient = enough & (l2 < g21 * l1) & (l3 < g32 * l2) & (l3f > 0)
        m21 = np.where(l1 > 0, np.abs(l2 - g21 * l1) / l1, 0.0)
        m32 = np.where(l1 > 0, np.abs(l3 - g32 * l2) / l1, 0.0)
    clear = ~enough | ((m21 > CLEAR_MARGIN) & (m32 > CLEAR_MARGIN))
    s = np.where(salient, l3f, np.float32(0)).astype(np.float32)
    return dict(k=k, lam=lam, salient=salient, s=s, margin21=m21, margin32=m32, clear=clear)


def nms(s, xyz, rn, min_neighbors=5, queries=None, brute=None):
    """-> the keypoint rows among `queries` (default: all rows), ascending, for the saliency array s [n] (fp32) of the WHOLE cloud"""
    s = np.asarray(s, np.float32)
    q = np.arange(len(xyz)) if queries is None else np.asarray(queries)
    count, offs, rows, _ = R.radius_sets(xyz, rn, q, brute=brute)
    seg = np.repeat(np.arange(len(q)), np.diff(offs))
    si, sj = s[q[seg]], s[rows]
    beats = (sj > si) | ((sj == si) & (rows < q[seg]))
    beaten = np.zeros(len(q), np.int64)
    np.add.at(beaten, seg[beats], 1)
    keep = (s[q] > 0) & (count >= int(min_neighbors)) & (beaten == 0)
    return np.sort(q[keep]).astype(np.int32)


# ---- hand-worked clouds: every coordinate is a small multiple of 0.25, so every product and every fp64 sum of the scatter is exact
# whatever the order, and translated neighbourhoods give bit-identical saliencies -------------------------------------------------
LATTICE_DX, LATTICE_DY, BUMP_H = 1.0, 1.25, 0.5     # unequal spacings: l1 != l2 at a lattice point (gamma21 < 1 needs that)
LATTICE_RS = 2.75                                   # 18 lattice neighbours inside the lattice


def lattice(nx, ny, raised=()):
    """nx x ny points (row = iy * nx + ix) at (ix * 1.0, iy * 1.25, 0), the points `raised` = [(ix, iy), ...] lifted to z = 0.5"""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    x = np.stack([ix.ravel() * LATTICE_DX, iy.ravel() * LATTICE_DY, np.zeros(nx * ny)], 1).astype(np.float32)
    for a, b in raised:
        x[b * nx + a, 2] = BUMP_H
    return x


def double_bump(seed=3):
    """a 17 x 9 lattice with two raised points, (4, 4) and (12, 4), whose neighbourhoods at LATTICE_RS are exact translates of each
    other and share no point, rows shuffled -> (xyz, row of the first bump, row of the second)"""
    x = lattice(17, 9, [(4, 4), (12, 4)])
    perm = np.random.default_rng(seed).permutation(len(x))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(x))
    return x[perm], int(inv[4 * 17 + 4]), int(inv[4 * 17 + 12])


def keypoints(xyz, rs, rn, gamma21=0.975, gamma32=0.975, min_neighbors=5, brute=None):
    """-> (rows [K] int32 ascending, the saliency() dict)"""
    sal = saliency(xyz, rs, gamma21, gamma32, min_neighbors, brute=brute)
    return nms(sal["s"], xyz, rn, min_neighbors, brute=brute), sal
