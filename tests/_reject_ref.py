"""The one-to-one and median-distance rejectors (include/symmicp.h, symmicp_set_one_to_one / symmicp_set_median_factor) restated in
numpy, on top of _record_ref.py and _trim_ref.py.

A rejecting pass, in this order:
  candidates  the pairs that exist (target row >= 0) and pass the two gates (_record_ref.gate); n_c of them
  d2          _record_ref.dist2 at the moved position (fp32, the kernels' expression)
  one-to-one  candidate i claims its target with K(i) = (bits(d2_i) << 32) | i, i the caller's row; the smallest K of a target wins;
              the survivors are the winners, n_u of them
  quantile    over the survivors (one-to-one on) or the candidates: a trim fraction rho (_trim_ref.trim_select), or the median factor:
              med = the ceil(n / 2)-th smallest d2, tau = fp32(fp32(factor * factor) * med), kept iff bits(d2) <= bits(tau);
              neither: every survivor is kept and tau = +Inf
and its record is _record_ref.record over the kept pairs.  Also here: an fp64 point-to-plane loop (exact nearest neighbours) with the
rejectors, the CPU check of what they are for."""
import numpy as np

import _trim_ref as TR

f32 = np.float32


def bits(x):
    return np.asarray(x, f32).reshape(-1).view(np.uint32)


def claim_keys(d2, rows):
    """K = (d2 bits << 32) | row"""
    return (bits(d2).astype(np.uint64) << np.uint64(32)) | np.asarray(rows, np.uint64)


def winners(idx, d2, cand):
    """mask over the rows: the candidates that hold the smallest key among the candidates of their target"""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    rows = np.flatnonzero(cand)
    win = np.zeros(n, bool)
    if len(rows) == 0:
        return win
    K = claim_keys(np.asarray(d2, f32)[rows], rows)
    j = idx[rows]
    order = np.lexsort((K, j))          # by target, then by key
    js = j[order]
    first = np.ones(len(js), bool)
    first[1:] = js[1:] != js[:-1]
    win[rows[order[first]]] = True
    return win


def median_tau(d2_pop, factor):
    """-> tau as fp32 over the population's d2; an empty population: fp32 0"""
    d2 = np.asarray(d2_pop, f32)
    k = TR.trim_k(0.5, len(d2))
    if k == 0:
        return f32(0)
    med = np.partition(d2, k - 1)[k - 1]
    with np.errstate(over="ignore", invalid="ignore"):
        f2 = f32(f32(factor) * f32(factor))
        tau = f32(f2 * f32(med))
    return f32(np.inf) if np.isnan(tau) else tau


def reject_pass(p, pn, q, qn, idx, one_to_one=False, factor=0.0, rho=1.0, max_d2=0.0, min_ndot=-2.0):
    """the rejecting pass over the moved source (p, pn), target (q, qn) and pairs idx in the caller's numbering (-1: none; None: identity
    pairing) -> dict(cand, n_c, uniq = survivor mask, n_u, tau (fp32), kept = kept mask, n_kept, d2)"""
    assert not (rho < 1.0 and factor > 0.0)
    base = TR.trim_pass(p, pn, q, qn, idx, 1.0, max_d2, min_ndot)
    cand, d2 = base["cand"], base["d2"]
    n = len(d2)
    ident = idx is None
    idx = np.arange(n) if ident else np.asarray(idx, np.int64)
    uniq = winners(idx, d2, cand) if (one_to_one and not ident) else cand.copy()
    pop = np.flatnonzero(uniq)
    if factor > 0.0:
        tau = median_tau(d2[pop], factor)
        keep_p = bits(d2[pop]) <= bits(tau)[0] if len(pop) else np.zeros(0, bool)
    elif rho < 1.0:
        _, tau, keep_p = TR.trim_select(d2[pop], rho)
    else:
        tau, keep_p = f32(np.inf), np.ones(len(pop), bool)
    kept = np.zeros(n, bool)
    kept[pop] = keep_p
    return dict(cand=cand, n_c=int(cand.sum()), uniq=uniq, n_u=int(uniq.sum()), tau=f32(tau), kept=kept, n_kept=int(kept.sum()), d2=d2)


def winners_loop(idx, d2_bits, cand):
    """the definition as a plain double loop (O(n m)): for the tests of winners()"""
    n = len(idx)
    win = np.zeros(n, bool)
    for i in range(n):
        if not cand[i]:
            continue
        ok = True
        for m in range(n):
            if m != i and cand[m] and idx[m] == idx[i] and (int(d2_bits[m]), m) < (int(d2_bits[i]), i):
                ok = False
                break
        win[i] = ok
    return win


def reject_icp_fp64(d, one_to_one=False, factor=0.0, rho=1.0, iters=30, counts=None):
    """_trim_ref.plane_icp_fp64 with the rejectors: each iteration pairs every source point with its nearest target point, keeps per target
    the closest source point (ties: the lowest row), then the pairs with d2 <= factor^2 x the median d2 of those (or the closest fraction
    rho of them) -> the 4x4.  counts: a list that receives the kept count of every iteration."""
    from scipy.spatial import cKDTree
    src = d["src"].astype(np.float64)
    tgt = d["tgt"].astype(np.float64)
    tn = d["tgt_n"].astype(np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4)
    for _ in range(iters):
        p = src @ T[:3, :3].T + T[:3, 3]
        dist, j = tree.query(p)
        d2 = dist * dist
        keep = np.ones(len(p), bool)
        if one_to_one:
            order = np.lexsort((np.arange(len(p)), d2, j))
            js = j[order]
            first = np.ones(len(js), bool)
            first[1:] = js[1:] != js[:-1]
            keep[:] = False
            keep[order[first]] = True
        pop = np.flatnonzero(keep)
        if factor > 0.0:
            k = TR.trim_k(0.5, len(pop))
            med = np.partition(d2[pop], k - 1)[k - 1]
            keep[pop] = d2[pop] <= factor * factor * med
        elif rho < 1.0:
            k = TR.trim_k(rho, len(pop))
            keep[pop] = d2[pop] <= np.partition(d2[pop], k - 1)[k - 1]
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
