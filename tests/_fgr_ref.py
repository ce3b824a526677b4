"""Plain numpy restatement of Fast Global Registration (kernels_fgr.hip; include/symmicp.h, "symmicp_ctx_fgr", defines the arithmetic).

tuple_draws()    the three SplitMix64 draws of (seed, stream 1) of every trial (integers: exact).
edge_fails32()   RANSAC's EDGE check in np.float32, one operation at a time in ransac_core.h's association.
tuple_set()      accepted trials and the optimisation set in trial order: what the device must reproduce bit for bit.
d2_max(), schedule()   D2 and the mu of every iteration, in np.float32: bit for bit as well.
pass_terms()     the per-element terms [M, 38] of one pass and the weights l: dtype float32 repeats the device's fp32 expressions
                 (xf_row, r2, t = mu / (mu + r2), l = t t) and carries them to fp64 as acc_row does; dtype float64 forms everything in fp64
                 from the same fp32 inputs.
pass_record()    their sums, with the sums of magnitudes _record_ref.assert_record wants.
mat4_mul32()     solve_core.h's mat4_mul in np.float32.
fgr32()          the whole method in the device's precision: fp32 terms, the library's host solve (symmicp_solve, MODE_PLANE), fp32 chain.
fgr64()          the whole method in fp64 from the same pivoted fp32 points: a 6 x 6 solve by numpy, the increment composed as
                 solve_plane composes it (T(pbar + t) R(a) T(-pbar)), the chain in fp64.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "icp-symm_amd", "py")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _global_ref as G          # noqa: E402
import _record_ref as RR         # noqa: E402

F = np.float32
MODE_PLANE = RR.MODE_PLANE
OK, ERR_DEGENERATE, ERR_NO_CONSENSUS = 0, 3, 8

# E: the largest displacement between the final transforms of fgr32() and fgr64() over the paired source points, as a fraction of
# max_dist, on the inputs of tests/test_fgr_ref.py (measured there: its table has 3.38e-5 as the worst value), rounded up to 4e-5 so that
# another BLAS or numpy build has room.  tests/test_gpu_fgr.py holds the device within 4 E of fgr64() on the same pairs: the margin covers
# libm and reduction-order differences; a wrong transform shows as order 1.
E = 4e-5


# ---- tuple test ------------------------------------------------------------------------------------------------------------------
def default_trials(m):
    return min(100 * m, 1 << 24)


def tuple_draws(seed, trials, m):
    """c [trials, 3] int64: c_j = ((u(3t + j) >> 32) * m) >> 32, u = the SplitMix64 sequence of (seed, stream 1)"""
    from symmicp import synth
    u = synth.splitmix64(seed, 3 * trials, 1)
    return (((u >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64).reshape(trials, 3)


def _dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def edge_fails32(P, Q, scale):
    """P, Q [T, 3 samples, 3] f32 -> bool [T]: an edge 0-1, 1-2, 2-0 with lp < e2 lq or lq < e2 lp, e2 = scale * scale in fp32"""
    P, Q = np.asarray(P, F), np.asarray(Q, F)
    e2 = F(scale) * F(scale)
    bad = np.zeros(len(P), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            dp, dq = P[:, a] - P[:, b], Q[:, a] - Q[:, b]
            lp, lq = _dot32(dp, dp), _dot32(dq, dq)
            bad |= (lp < e2 * lq) | (lq < e2 * lp)
    return bad


def tuple_set(p, q, seed=0, tuple_scale=0.95, max_tuples=1000, trials=0):
    """-> (set [M] int32, accepted): the draws of the first min(accepted, max_tuples) accepted trials in ascending t, three per tuple,
    duplicates kept.  max_tuples == 0: all pairs in order, accepted 0."""
    m = len(p)
    if max_tuples == 0:
        return np.arange(m, dtype=np.int32), 0
    trials = trials or default_trials(m)
    c = tuple_draws(seed, trials, m)
    ok = ~((c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 0] == c[:, 2]))
    idx = np.nonzero(ok)[0]
    ok[idx] = ~edge_fails32(np.asarray(p, F)[c[idx]], np.asarray(q, F)[c[idx]], tuple_scale)
    acc = np.nonzero(ok)[0]
    return c[acc[:max_tuples]].reshape(-1).astype(np.int32), int(len(acc))


# ---- schedule ----------------------------------------------------------------------------------------------------------------------
def _norm2_32(v):
    v = np.asarray(v, F)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def d2_max(p, q):
    return F(max(_norm2_32(p).max(), _norm2_32(q).max()))


def delta2(max_dist):
    return F(max_dist) * F(max_dist)


def schedule_step(k, mu, d2, decrease_every, division_factor):
    mu = F(mu)
    if k % decrease_every == 0 and mu > d2:
        mu = F(mu / F(division_factor))
        if mu < d2:
            mu = F(d2)
    return mu


def schedule(D2, max_dist, iterations=64, decrease_every=4, division_factor=1.4):
    """mu of every iteration [iterations] f32"""
    d2 = delta2(max_dist)
    mu, out = F(D2), np.zeros(iterations, F)
    for k in range(iterations):
        mu = schedule_step(k, mu, d2, decrease_every, division_factor)
        out[k] = mu
    return out


# ---- one pass ------------------------------------------------------------------------------------------------------------------------
def pass_terms(p, q, X, mu, dtype=np.float32, weights=None):
    """-> (terms [M, 38] f64, l [M] in dtype); weights: given l instead of the line process's (tests of the rows alone)"""
    f = dtype
    q = np.asarray(q, F).astype(f)
    if f == np.float32:
        pm = RR.xf_rows(X, p, 1.0)
    else:
        X4 = np.asarray(X, np.float64).reshape(4, 4)
        pm = np.asarray(p, F).astype(np.float64) @ X4[:3, :3].T + X4[:3, 3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = pm - q
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        mu = f(mu)
        t = mu / (mu + r2)
        l = t * t if weights is None else np.asarray(weights, f)
    n = len(pm)
    w = l.astype(np.float64)
    P, D = pm.astype(np.float64), d.astype(np.float64)
    z, one = np.zeros(n), np.ones(n)
    rows = ((np.stack([z, P[:, 2], -P[:, 1], one, z, z], 1), D[:, 0]),
            (np.stack([-P[:, 2], z, P[:, 0], z, one, z], 1), D[:, 1]),
            (np.stack([P[:, 1], -P[:, 0], z, z, z, one], 1), D[:, 2]))
    T = np.zeros((n, 38))
    for V, c in rows:
        k = 0
        for a in range(6):
            for b in range(a, 6):
                T[:, k] += w * V[:, a] * V[:, b]
                k += 1
        T[:, 21:27] += V * (w * c)[:, None]
        T[:, 35] += w * c * c
    T[:, 27:30] = w[:, None] * P
    T[:, 30:33] = w[:, None] * q.astype(np.float64)
    T[:, 34] = w
    T[:, 36] = r2.astype(np.float64)
    T[:, 37] = 1.0
    return T, l


def pass_record(p, q, X, mu, dtype=np.float32, weights=None):
    """-> (record [40], sums of |terms| [40], l [M])"""
    T, l = pass_terms(p, q, X, mu, dtype, weights)
    S, Mg = np.zeros(RR.NSUM), np.zeros(RR.NSUM)
    S[:38] = T.sum(0)
    Mg[:38] = np.abs(T).sum(0)
    return S, Mg, l


# ---- solve and chain -------------------------------------------------------------------------------------------------------------------
def mat4_mul32(A, B):
    """solve_core.h's mat4_mul: fp32, k sequential"""
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    out = np.zeros((4, 4), F)
    for r in range(4):
        for c in range(4):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            s = s + A[r, 3] * B[3, c]
            out[r, c] = s
    return out


def _rodrigues(a):
    th = float(np.linalg.norm(a))
    if th == 0.0:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def solve64(S):
    """the increment of a record in fp64, composed as solve_plane composes it -> 4x4, or None when the system is degenerate"""
    cnt = S[34]
    if not (cnt >= 6.0) or not np.isfinite(S[:38]).all():
        return None
    A = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = S[k]
            k += 1
    b = S[21:27]
    w = np.linalg.eigvalsh(A / np.sqrt(np.outer(np.diag(A), np.diag(A)))) if (np.diag(A) > 0).all() else np.zeros(6)
    if not (w.min() > 1e-12 * w.max()):
        return None
    x = np.linalg.solve(A, -b)
    a, t0 = x[:3], x[3:]
    pbar = S[27:30] / cnt
    t = t0 + np.cross(a, pbar)
    R = _rodrigues(a)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = pbar + t - R @ pbar
    return T


def compose(X, cs, ct):
    """T = T(ct) X T(-cs) in fp64"""
    X = np.asarray(X, np.float64).reshape(4, 4)
    T = np.eye(4)
    T[:3, :3] = X[:3, :3]
    T[:3, 3] = X[:3, 3] + np.asarray(ct, np.float64) - X[:3, :3] @ np.asarray(cs, np.float64)
    return T


def _loop(p, q, sel, mus, dtype):
    import symmicp as sym
    ps, qs = p[sel], q[sel]
    X = np.eye(4, dtype=dtype)
    Xs, recs = [X.copy()], []
    status, l = OK, None
    for mu in mus:
        S, _, l = pass_record(ps, qs, X, mu, dtype)
        recs.append(S)
        if dtype == np.float32:
            st, *_, Xi = sym.solve(MODE_PLANE, S)
            if st != OK:
                status = ERR_DEGENERATE
                break
            X = mat4_mul32(Xi, X)
        else:
            Xi = solve64(S)
            if Xi is None:
                status = ERR_DEGENERATE
                break
            X = Xi @ X
        Xs.append(X.copy())
    return dict(status=status, X=X, X_trace=np.array(Xs), sums_trace=np.array(recs), weights=l, iterations=len(Xs) - 1)


def fgr(src, tgt, pairs, max_dist, iterations=64, decrease_every=4, division_factor=1.4, tuple_scale=0.95, max_tuples=1000, tuple_trials=0,
        seed=0, dtype=np.float64):
    """the whole method -> dict(status, T [4, 4] f64 in the caller's coordinates, X, set, accepted, mu_trace, X_trace, sums_trace, weights,
    iterations, p, q, cs, ct)"""
    pairs = np.asarray(pairs, np.int32)
    p, q, cs, ct = G.pivoted(src, tgt, pairs)
    sel, accepted = tuple_set(p, q, seed, tuple_scale, max_tuples, tuple_trials)
    out = dict(set=sel, accepted=accepted, p=p, q=q, cs=cs, ct=ct)
    if max_tuples and accepted == 0:
        out.update(status=ERR_NO_CONSENSUS, T=np.eye(4), X=np.eye(4), iterations=0)
        return out
    mus = schedule(d2_max(p, q), max_dist, iterations, decrease_every, division_factor)
    out.update(_loop(p, q, sel, mus, dtype), mu_trace=mus)
    out["T"] = compose(out["X"], cs, ct)
    return out


def fgr32(*a, **kw):
    return fgr(*a, dtype=np.float32, **kw)


def fgr64(*a, **kw):
    return fgr(*a, dtype=np.float64, **kw)


def displacement(Ta, Tb, X):
    """the largest |Ta x - Tb x| over the points X (fp64)"""
    X = np.asarray(X, np.float64)
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    d = (X @ Ta[:3, :3].T + Ta[:3, 3]) - (X @ Tb[:3, :3].T + Tb[:3, 3])
    return float(np.sqrt((d * d).sum(1)).max())
