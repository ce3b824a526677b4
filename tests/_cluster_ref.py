"""Plain numpy reference for DBSCAN / Euclidean cluster extraction (symmicp_ctx_cluster; include/symmicp.h defines the result).

Brute force over _fpfh_ref.radius_sets (the exact fp32 neighbourhoods N(i), d2 in the kernels' association, CSR lists with their d2),
a SEQUENTIAL union-find over the core-core edges, then the border rule, the numbering and the size filter exactly as the header states
them.  Needs no scipy below _fpfh_ref.BRUTE_MAX points.

cluster()        -> dict(labels, clusters, sizes, core, neighbors, root) as symmicp.cluster_dbscan(..., return_info=True), plus root [n]:
                    the representative (lowest core row) of every row's cluster BEFORE the size filter, -1 for noise.
partition()      labels -> a frozenset of frozensets of rows (noise left out): what must not depend on the row order.
scene()          the shuffled multi-object scene of the tests: two cats, a half-scale quarter-sampled cat and 200 uniform stray points.
"""
import numpy as np

import _fpfh_ref as R

CAT_SPACING = 1.3816


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def cluster(xyz, eps, min_points=1, min_cluster_size=0, max_cluster_size=0):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    count, offs, rows, d2 = R.radius_sets(xyz, eps)
    core = count.astype(np.int64) + 1 >= min_points
    parent = list(range(n))
    src = np.repeat(np.arange(n), count)
    edge = core[src] & core[rows] & (src < rows)
    for a, b in zip(src[edge].tolist(), rows[edge].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)            # the lower row stays the root: a component's root is its lowest row
    root = np.full(n, -1, np.int64)
    for i in np.nonzero(core)[0].tolist():
        root[i] = _find(parent, i)
    bits = d2.view(np.uint32).astype(np.uint64)
    for i in np.nonzero(~core & (count > 0))[0].tolist():
        j = rows[offs[i]:offs[i + 1]]
        c = core[j]
        if c.any():
            key = (bits[offs[i]:offs[i + 1]][c] << np.uint64(32)) | root[j[c]].astype(np.uint64)
            root[i] = int(key.min() & np.uint64(0xFFFFFFFF))
    reps = np.nonzero((root == np.arange(n)) & core)[0]                  # ascending
    label_of = np.full(n, -1, np.int64)
    label_of[reps] = np.arange(len(reps))
    labels = np.where(root >= 0, label_of[np.maximum(root, 0)], -1)
    sizes = np.bincount(labels[labels >= 0], minlength=len(reps))
    keep = np.ones(len(reps), bool)
    if min_cluster_size > 0:
        keep &= sizes >= min_cluster_size
    if max_cluster_size > 0:
        keep &= sizes <= max_cluster_size
    renum = np.append(np.where(keep, np.cumsum(keep) - 1, -1), -1)      # (the last slot: noise)
    labels = renum[labels].astype(np.int32)
    return dict(labels=labels, clusters=int(keep.sum()), sizes=sizes[keep].astype(np.int32), core=core, neighbors=count.astype(np.int32), root=root)


def partition(labels):
    labels = np.asarray(labels)
    return frozenset(frozenset(np.nonzero(labels == k)[0].tolist()) for k in np.unique(labels[labels >= 0]).tolist())


def scene(cat_xyz, seed=3):
    """-> xyz [7 850, 3] f32 for the 3 400-point cat: the cat, a copy moved well clear of it, a half-scale copy of every fourth row, and
    200 uniform points in the bounding box of the three; rows permuted"""
    cat = np.ascontiguousarray(cat_xyz, np.float32).astype(np.float64)
    ext = cat.max(axis=0) - cat.min(axis=0)
    second = cat + np.array([1.5 * ext[0], 0.0, 0.0])
    small = 0.5 * cat[::4] + np.array([0.0, 1.5 * ext[1], 0.0])
    body = np.concatenate([cat, second, small])
    rng = np.random.default_rng(seed)
    stray = rng.uniform(body.min(axis=0), body.max(axis=0), (200, 3))
    x = np.concatenate([body, stray]).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(len(x))])


def numbering_is_by_lowest_core_row(labels, core):
    """the labels' own numbering: cluster k's lowest core row ascends with k, and every label 0 .. max is used"""
    labels, core = np.asarray(labels), np.asarray(core, bool)
    c = int(labels.max()) + 1 if len(labels) else 0
    reps = [int(np.nonzero((labels == k) & core)[0].min()) for k in range(c)]      # (raises on a cluster without a core row)
    return reps == sorted(reps)


def line(xs):
    p = np.zeros((len(xs), 3), np.float32)
    p[:, 0] = xs
    return p


K_LEAF = 8          # kLeaf of symmicp_internal.h: points per leaf of the box tree


def border_case(tie, b_first):
    """Two runs of five collinear points half a unit apart and a point P between them, eps 1, min_points 4: the three inner points of
    a run and the end that faces P are core, the far ends are border rows of their own run, and P (two neighbours) is a border row
    with one core neighbour in each cluster: the end of A at d2 = 1 and the end of B at d2 = 0.5625 (B nearer), or with `tie` at a
    bit-equal d2 = 1.  Every coordinate is a multiple of 0.25.  -> (xyz, labels)"""
    a = [-2.0, -1.5, -1.0, -0.5, 0.0]
    b = [2.0, 2.5, 3.0, 3.5, 4.0] if tie else [1.75, 2.25, 2.75, 3.25, 3.75]
    xs = (b + a if b_first else a + b) + [1.0]
    la, lb = (1, 0) if b_first else (0, 1)
    p = min(la, lb) if tie else lb
    return line(xs), np.array(([lb] * 5 + [la] * 5 if b_first else [la] * 5 + [lb] * 5) + [p], np.int32)


def small_cases():
    """[(name, xyz, eps, min_points, labels)]: the smallest shapes with their answers written down by hand"""
    z = np.zeros((1, 3), np.float32)
    two = line([0.0, 1.0])
    pyth = np.array([[0, 0, 0], [3, 4, 0]], np.float32)                 # d2 = 25 == r2 at eps 5: members
    same = np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (100, 1))
    cases = [("one point", z, 1.0, 1, [0]), ("one point, min_points 2", z, 1.0, 2, [-1]),
             ("two within eps", two, 1.5, 1, [0, 0]), ("two beyond eps", two, 0.5, 1, [0, 1]),
             ("two within eps, both core at 2", two, 1.5, 2, [0, 0]), ("two beyond eps, noise at 2", two, 0.5, 2, [-1, -1]),
             ("d2 == r2 exactly", pyth, 5.0, 2, [0, 0]), ("just below", pyth, np.nextafter(np.float32(5.0), np.float32(0)), 2, [-1, -1]),
             ("100 coincident, min_points 1", same, 0.1, 1, [0] * 100), ("100 coincident, min_points 100", same, 0.1, 100, [0] * 100),
             ("100 coincident, min_points 101", same, 0.1, 101, [-1] * 100),
             ("min_points above n", line(np.arange(20.0)), 1.5, 21, [-1] * 20)]
    for n in (K_LEAF - 1, K_LEAF, K_LEAF + 1):
        xs = np.arange(n, dtype=np.float64)
        xs[-1] = n + 10.0                                               # the last row stands apart
        cases.append(("n = %d" % n, line(xs), 1.5, 1, [0] * (n - 1) + [1]))
        cases.append(("n = %d, min_points 3" % n, line(xs), 1.5, 3, [0] * (n - 1) + [-1]))      # the chain's ends are border rows
    # two tight clusters 1e4 times their own size apart, rows interleaved
    rng = np.random.default_rng(1)
    tight = (rng.random((10, 3)) * 1e-3).astype(np.float32)
    tight[1::2, 0] += np.float32(10.0)
    cases.append(("two tight clusters far apart", tight, 2e-3, 1, [0, 1] * 5))
    cases.append(("two tight clusters far apart, min_points 5", tight, 2e-3, 5, [0, 1] * 5))
    for tie in (False, True):
        for b_first in (False, True):
            x, lab = border_case(tie, b_first)
            cases.append(("border point, %s, %s first" % ("tie" if tie else "B nearer", "B" if b_first else "A"), x, 1.0, 4, lab.tolist()))
    return [(name, np.ascontiguousarray(x, np.float32), float(eps), mp, np.array(lab, np.int32)) for name, x, eps, mp, lab in cases]


def stress_cases():
    """[(name, xyz, eps)]: shapes that stress the union (min_points 1); every one is a single cluster whose representative is row 0"""
    chain = line(np.arange(4096.0))
    g = np.arange(64, dtype=np.float32)
    lattice = np.zeros((64 * 64, 3), np.float32)
    lattice[:, :2] = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    rng = np.random.default_rng(4)
    return [("chain ascending", chain, 1.5), ("chain descending", np.ascontiguousarray(chain[::-1]), 1.5),
            ("chain shuffled", np.ascontiguousarray(chain[rng.permutation(4096)]), 1.5),
            ("2048 coincident", np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (2048, 1)), 0.5),
            ("lattice 64 x 64", lattice, 1.0)]


THREE_EPS = 8 * CAT_SPACING


def three_objects(cat_xyz, seed=6):
    """three separated objects for the batch test -- the cat, every second row of it and a half-scale copy of every fourth row, each a
    single cluster at THREE_EPS and at most 4 096 points -- with the rows permuted -> (xyz [5 950, 3] f32, owner [5 950]: 0, 1, 2)"""
    cat = np.ascontiguousarray(cat_xyz, np.float32).astype(np.float64)
    ext = cat.max(axis=0) - cat.min(axis=0)
    parts = [cat, cat[::2] + np.array([1.5 * ext[0], 0.0, 0.0]), 0.5 * cat[::4] + np.array([0.0, 1.5 * ext[1], 0.0])]
    x = np.concatenate(parts).astype(np.float32)
    owner = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    perm = np.random.default_rng(seed).permutation(len(x))
    return np.ascontiguousarray(x[perm]), owner[perm]
