"""Reciprocal correspondences (include/symmicp.h, symmicp_set_reciprocal) restated in numpy, on top of _record_ref.py, _trim_ref.py and
_reject_ref.py.

A reciprocal pass, in this order:
  candidates  as for one-to-one: the pairs that exist and pass the two gates; n_c of them
  claim       the one-to-one claim (_reject_ref.winners): per target the candidate with the smallest (d2 bits, caller row); n_u winners
  inverse     inverse_rigid(X) of the pass's cumulative 4x4: rows (R_0r, R_1r, R_2r, -((R_0r t_0 + R_1r t_1) + R_2r t_2)), formed in fp64
              from the fp32 entries, each entry rounded to fp32
  back()      y_j = back_project(inverse, q_j) in fp32, unfused; back(j) = the ORIGINAL source row i that minimises
              (dist2(y_j, p_i), i) over all source rows
  rule        the winner i of target j survives iff back(j) == i; n_r survivors
  quantile    over the survivors: the median factor, a trim fraction, or neither (every survivor kept, tau = +Inf)
and its record is _record_ref.record over the kept pairs.  Also here: the fp64 point-to-plane loop of _reject_ref with the reciprocal
rule, the CPU check of what it is for."""
import numpy as np

import _record_ref as R
import _reject_ref as J
import _trim_ref as TR

f32 = np.float32


def inverse_rigid(X):
    """-> (3, 4) float32"""
    X = np.asarray(X, f32).reshape(4, 4)
    Xd = X.astype(np.float64)
    t = Xd[:3, 3]
    out = np.empty((3, 4), f32)
    for r in range(3):
        out[r, :3] = X[:3, r]
        out[r, 3] = f32(-((Xd[0, r] * t[0] + Xd[1, r] * t[1]) + Xd[2, r] * t[2]))
    return out


def back_project(inv, q):
    """xf_row of the three inverse rows on every row of q with w = 1: ((m0 x + m1 y) + m2 z) + m3 in fp32, unfused"""
    m = np.asarray(inv, f32).reshape(3, 4)
    q = np.asarray(q, f32)
    out = np.empty_like(q)
    for r in range(3):
        out[:, r] = ((m[r, 0] * q[:, 0] + m[r, 1] * q[:, 1]) + m[r, 2] * q[:, 2]) + m[r, 3]
    return out


def back(db, labels, y, chunk=None):
    """per row of y the db point that minimises (dist2(y, db_i), label_i): fp32 brute force in chunks -> (labels int64 [n_q], d2 fp32 [n_q])"""
    db = np.asarray(db, f32)
    y = np.asarray(y, f32)
    labels = np.arange(len(db), dtype=np.int64) if labels is None else np.asarray(labels, np.int64)
    order = np.argsort(labels, kind="stable")          # ascending labels: argmin's first hit is the lowest label
    dbs, labs = db[order], labels[order]
    if chunk is None:
        chunk = max(1, (1 << 22) // max(1, len(db)))
    lab_out = np.empty(len(y), np.int64)
    d2_out = np.empty(len(y), f32)
    for a in range(0, len(y), chunk):
        yy = y[a:a + chunk]
        dx = yy[:, None, 0] - dbs[None, :, 0]
        dy = yy[:, None, 1] - dbs[None, :, 1]
        dz = yy[:, None, 2] - dbs[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        k = np.argmin(d2, axis=1)
        lab_out[a:a + chunk] = labs[k]
        d2_out[a:a + chunk] = d2[np.arange(len(yy)), k]
    return lab_out, d2_out


def back_loop(db, labels, y):
    """the definition as a plain double loop: for the tests of back()"""
    db, y = np.asarray(db, f32), np.asarray(y, f32)
    labels = np.arange(len(db)) if labels is None else labels
    lab_out, d2_out = [], []
    for a in range(len(y)):
        best = None
        for i in range(len(db)):
            d = y[a] - db[i]
            d2 = f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            key = (d2, int(labels[i]))
            if best is None or key < best:
                best = key
        lab_out.append(best[1])
        d2_out.append(best[0])
    return np.array(lab_out, np.int64), np.array(d2_out, f32)


def recip_pass(p, pn, q, qn, idx, src0, X, factor=0.0, rho=1.0, max_d2=0.0, min_ndot=-2.0, brute=False):
    """the reciprocal pass over the moved source (p, pn), target (q, qn), pairs idx in the caller's numbering (-1: none), the ORIGINAL
    source src0 and the pass's cumulative transform X -> dict(cand, n_c, uniq = the claim's winners, n_u, recip = survivor mask, n_r,
    tau (fp32), kept = kept mask, n_kept, d2, back = back(j) per winner row (-1 elsewhere)).  back() runs through _record_ref.nn_ref --
    the same minimum of (dist2(y, p_i), i) by the oracle's compiled brute force -- unless brute: the numpy one above
    (tests/test_recip_ref.py holds the two together)."""
    assert not (rho < 1.0 and factor > 0.0)
    base = J.reject_pass(p, pn, q, qn, idx, one_to_one=True, max_d2=max_d2, min_ndot=min_ndot)
    cand, d2, uniq = base["cand"], base["d2"], base["uniq"]
    n = len(d2)
    idx = np.asarray(idx, np.int64)
    win = np.flatnonzero(uniq)
    bk = np.full(n, -1, np.int64)
    if len(win):
        y = back_project(inverse_rigid(X), np.asarray(q, f32)[idx[win]])
        bk[win] = back(src0, None, y)[0] if brute else R.nn_ref(y, src0)[0]
    recip = uniq & (bk == np.arange(n))
    pop = np.flatnonzero(recip)
    if factor > 0.0:
        tau = J.median_tau(d2[pop], factor)
        keep_p = J.bits(d2[pop]) <= J.bits(tau)[0] if len(pop) else np.zeros(0, bool)
    elif rho < 1.0:
        _, tau, keep_p = TR.trim_select(d2[pop], rho)
    else:
        tau, keep_p = f32(np.inf), np.ones(len(pop), bool)
    kept = np.zeros(n, bool)
    kept[pop] = keep_p
    return dict(cand=cand, n_c=int(cand.sum()), uniq=uniq, n_u=int(uniq.sum()), recip=recip, n_r=int(recip.sum()), tau=f32(tau), kept=kept,
                n_kept=int(kept.sum()), d2=d2, back=bk)


def recip_icp_fp64(d, reciprocal=True, factor=0.0, iters=30, counts=None):
    """_reject_ref.reject_icp_fp64 with the reciprocal rule: each iteration pairs every source point with its nearest target point, keeps per
    target the closest source point (ties: the lowest row), carries that target point through inverse_rigid of the transform (the
    definition: the fp32 entries of T, the translation formed in fp64) and keeps the pair iff the nearest ORIGINAL source point of the
    result is that source point; then the median rule over the survivors -> the 4x4.  counts receives the kept count of every iteration."""
    from scipy.spatial import cKDTree
    src = d["src"].astype(np.float64)
    tgt = d["tgt"].astype(np.float64)
    tn = d["tgt_n"].astype(np.float64)
    tree, stree = cKDTree(tgt), cKDTree(src)
    T = np.eye(4)
    for _ in range(iters):
        p = src @ T[:3, :3].T + T[:3, 3]
        dist, j = tree.query(p)
        d2 = dist * dist
        order = np.lexsort((np.arange(len(p)), d2, j))
        js = j[order]
        first = np.ones(len(js), bool)
        first[1:] = js[1:] != js[:-1]
        keep = np.zeros(len(p), bool)
        keep[order[first]] = True
        if reciprocal:
            win = np.flatnonzero(keep)
            inv = inverse_rigid(T.astype(f32)).astype(np.float64)
            y = tgt[j[win]] @ inv[:, :3].T + inv[:, 3]
            keep[win] = stree.query(y)[1] == win
        pop = np.flatnonzero(keep)
        if factor > 0.0:
            k = TR.trim_k(0.5, len(pop))
            med = np.partition(d2[pop], k - 1)[k - 1]
            keep[pop] = d2[pop] <= factor * factor * med
        if counts is not None:
            counts.append(int(keep.sum()))
        P, Q, N = p[keep], tgt[j[keep]], tn[j[keep]]
        c0 = P.mean(0)
        Pc = P - c0
        V = np.concatenate([np.cross(Pc, N), N], 1)
        c = ((P - Q) * N).sum(1)
        x = np.linalg.solve(V.T @ V, -(V.T @ c))
        Rm = TR._rodrigues(x[:3])
        inc = np.eye(4)
        inc[:3, :3] = Rm
        inc[:3, 3] = c0 + x[3:] - Rm @ c0
        T = inc @ T
    return T
