"""Plain numpy / scipy restatement of symmicp_ctx_orient_normals (include/symmicp.h, "consistent normal orientation"): what
tests/test_gpu_orient.py holds the device to, bit for bit.

graph()    the symmetrised k-NN graph from the exact sets of _knn_ref.knn (row i itself left out by ROW), each edge once as (lo, hi),
           its fp32 weight bits and its sign bit, and its RANK in the total order (w bits, lo, hi).
forest()   the minimum spanning forest: scipy's minimum_spanning_tree with the rank (1 .. m, distinct, exact in fp64) as the weight.
kruskal()  the same forest by Kruskal over the edges in rank order with a plain union-find (the check of forest()).
rounds()   the Boruvka rounds of the device counted on the host: per round every component's minimum outgoing edge, all of them joined.
orient()   components, seeds, the walk from each seed, the sign-only write -> the dict symmicp.orient_normals(return_info=True) returns.
"""
import numpy as np
from scipy.sparse import coo_matrix, csr_matrix
from scipy.sparse.csgraph import breadth_first_order, connected_components, minimum_spanning_tree

import _knn_ref as K

F = np.float32


def graph(xyz, nrm, k, rows=None):
    """-> dict(lo=, hi= [m] int64 in rank order, wbits= [m] uint32, s= [m] bool); position in the arrays = rank"""
    xyz, nrm = np.ascontiguousarray(xyz, F), np.ascontiguousarray(nrm, F)
    n = len(xyz)
    if rows is None:
        rows = K.knn(xyz, k)[0]
    i = np.repeat(np.arange(n, dtype=np.int64), rows.shape[1])
    j = rows.astype(np.int64).ravel()
    keep = i != j
    i, j = i[keep], j[keep]
    code = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    lo, hi = code // n, code % n
    a, b = nrm[lo], nrm[hi]
    d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    w = np.maximum(F(1.0) - np.abs(d), F(0.0)).astype(F)
    wbits = w.view(np.uint32)
    o = np.lexsort((hi, lo, wbits))
    return dict(n=n, lo=lo[o], hi=hi[o], wbits=wbits[o], s=(d < 0)[o])


def forest(g):
    """-> the ranks (ascending) of the edges of the minimum spanning forest"""
    m, n = len(g["lo"]), g["n"]
    rank = np.arange(1, m + 1, dtype=np.float64)
    t = minimum_spanning_tree(coo_matrix((rank, (g["lo"], g["hi"])), shape=(n, n)).tocsr())
    return np.sort(t.data.astype(np.int64) - 1)


def kruskal(g):
    parent = list(range(g["n"]))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    for r, (a, b) in enumerate(zip(g["lo"].tolist(), g["hi"].tolist())):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.append(r)
    return np.array(kept, np.int64)


def rounds(g):
    """-> (the rounds that joined something, the ranks of all edges chosen on the way, ascending)"""
    n, lo, hi = g["n"], g["lo"], g["hi"]
    m = len(lo)
    comp = np.arange(n)
    chosen_all = []
    count = 0
    rank = np.arange(m)
    while True:
        ca, cb = comp[lo], comp[hi]
        out = ca != cb
        if not out.any():
            break
        best = np.full(n, m, np.int64)
        np.minimum.at(best, ca[out], rank[out])
        np.minimum.at(best, cb[out], rank[out])
        chosen = np.unique(best[best < m])
        chosen_all.append(chosen)
        count += 1
        _, lab = connected_components(csr_matrix((np.ones(len(chosen)), (comp[lo[chosen]], comp[hi[chosen]])), shape=(n, n)), directed=False)
        comp = lab[comp]
    return count, (np.sort(np.concatenate(chosen_all)) if chosen_all else np.zeros(0, np.int64))


def orient(xyz, nrm, k=16, viewpoint=None, direction=None, rows=None):
    xyz, nrm = np.ascontiguousarray(xyz, F), np.ascontiguousarray(nrm, F)
    n = len(xyz)
    g = graph(xyz, nrm, k, rows)
    t = forest(g)
    lo, hi, s = g["lo"][t], g["hi"][t], g["s"][t]
    sym = csr_matrix((np.concatenate([s, s]) + 1.0, (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n))
    ncomp, lab = connected_components(sym, directed=False)
    low = np.full(ncomp, n, np.int64)
    np.minimum.at(low, lab, np.arange(n))
    component = low[lab].astype(np.int32)
    # the seed of every component: an order-preserving key, ties to the lowest row
    with np.errstate(all="ignore"):
        if direction is None:
            ref = np.zeros(3, F) if viewpoint is None else np.asarray(viewpoint, F)
            dx, dy, dz = xyz[:, 0] - ref[0], xyz[:, 1] - ref[1], xyz[:, 2] - ref[2]
            key = ((dx * dx + dy * dy) + dz * dz).astype(F).view(np.uint32).astype(np.int64)
        else:
            ref = np.asarray(direction, F)
            p = (((xyz[:, 0] * ref[0] + xyz[:, 1] * ref[1]) + xyz[:, 2] * ref[2]) + F(0.0)).astype(F)
            p = np.where(np.isnan(p), F(-np.inf), p).astype(F)
            u = p.view(np.uint32).astype(np.int64)
            key = 0xFFFFFFFF - np.where(u >> 31, 0xFFFFFFFF - u, u | 0x80000000)
    o = np.lexsort((np.arange(n), key, lab))
    seeds = o[np.concatenate([[True], lab[o][1:] != lab[o][:-1]])]           # one per component, in label order
    flip = np.zeros(n, bool)
    x64, n64, r64 = xyz.astype(np.float64), nrm.astype(np.float64), ref.astype(np.float64)
    for seed in seeds.tolist():
        if direction is None:
            dot = ((r64[0] - x64[seed, 0]) * n64[seed, 0] + (r64[1] - x64[seed, 1]) * n64[seed, 1]) + (r64[2] - x64[seed, 2]) * n64[seed, 2]
            f0 = bool(dot < 0)
        else:
            with np.errstate(all="ignore"):
                f0 = bool(((nrm[seed, 0] * ref[0] + nrm[seed, 1] * ref[1]) + nrm[seed, 2] * ref[2]) < 0)
        order, pred = breadth_first_order(sym, seed, directed=False)
        flip[seed] = f0
        if len(order) > 1:
            rest = order[1:]
            odd = (np.asarray(sym[pred[rest], rest]).ravel() - 1.0).astype(bool)
            for v, p_, e in zip(rest.tolist(), pred[rest].tolist(), odd.tolist()):
                flip[v] = flip[p_] ^ e
    out = nrm.view(np.uint32) ^ np.where(flip, np.uint32(0x80000000), np.uint32(0))[:, None]
    tree = np.stack([lo, hi], 1).astype(np.int32)
    tree = tree[np.lexsort((tree[:, 1], tree[:, 0]))]
    return dict(normals=out.view(F), flip=flip, component=component, tree=tree, graph_edges=len(g["lo"]), tree_edges=len(t),
                components=int(ncomp), largest_component=int(np.bincount(lab).max()), flipped=int(flip.sum()), rounds=rounds(g)[0])


def disagreement(na, nb, R):
    """the share of rows on which the normals of two clouds of one surface (b = R a + t, row for row) point to different sides"""
    return float((((na.astype(np.float64) @ R.T) * nb).sum(1) < 0).mean())
